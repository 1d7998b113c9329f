"""A plain reference of the forwarder's flow classification (pipck_fwd_classify_ring /
pipck_fwd_classify_device, include/pipck.h "flow classification"), written from that
comment and from nothing else: no ctypes, nothing of pip_amd.  The upper layer is
located by tx_reference._upper, as fwd_reference.rewrite locates it, so "keyed" here
and "an address-and-port rule rewrites or finds expired" there are one statement.

A key is its 40 bytes (src[16], dst[16], sport[2], dport[2], proto, family, pad[2]); a
table is a list of n_slots entries, each None (empty) or (key bytes, rule, tag), and
table_bytes() gives the 48-byte entries as memory holds them.  All arithmetic is exact
Python integers reduced modulo 2^32 where the header says so."""
from tests.tx_reference import MIN_L4, _upper

TCP, UDP, ICMP, ICMP6 = 6, 17, 1, 58
MAX_PROBE = 64
NO_RULE = 0xFFFFFFFF
HIT, MISS, UNKEYED, PASSED = 1, 2, 4, 8  # d_class values; 0: malformed or refused
MALFORMED, NO_KEY = "malformed", "unkeyed"  # frame_class's other answers
EINVAL, ERANGE = 1, 2
M32 = 0xFFFFFFFF


def key(family, proto, src, dst, sport=0, dport=0) -> bytes:
    """The 40 key bytes.  src / dst: wire bytes (4 or 16); sport / dport: numbers or 2 wire bytes."""
    def port(p):
        return p.to_bytes(2, "big") if isinstance(p, int) else bytes(p)

    out = bytes(src).ljust(16, b"\0") + bytes(dst).ljust(16, b"\0") + port(sport) + port(dport) + bytes([proto, family, 0, 0])
    assert len(out) == 40
    return out


def _be16(b, i) -> int:
    return b[i] << 8 | b[i + 1]


def frame_class(frame):
    """MALFORMED, NO_KEY, or the frame's 40 key bytes."""
    f = bytes(frame)
    if len(f) < 20:
        return MALFORMED
    version = f[0] >> 4
    if version == 4:
        ihl, total = (f[0] & 15) * 4, _be16(f, 2)
        if ihl < 20 or total < ihl or total > len(f):
            return MALFORMED
        src, dst = f[12:16], f[16:20]
    elif version == 6:
        if len(f) < 40 or 40 + _be16(f, 4) > len(f):
            return MALFORMED
        src, dst = f[8:24], f[24:40]
    else:
        return MALFORMED
    up = _upper(f)
    if up is None:
        return NO_KEY
    proto, at, end = up
    if proto not in (TCP, UDP, ICMP if version == 4 else ICMP6):
        return NO_KEY
    if end - at < MIN_L4[proto]:
        return NO_KEY
    ports = f[at:at + 4] if proto in (TCP, UDP) else bytes(4)
    return key(version, proto, src, dst, ports[:2], ports[2:])


def key_hash(k: bytes) -> int:
    assert len(k) == 40
    x = 0
    for j in range(10):
        x ^= int.from_bytes(k[4 * j:4 * j + 4], "little")
        x = ((x << 13) | (x >> 19)) & M32
        x = x * 0x9E3779B1 & M32
    x ^= x >> 16
    x = x * 0x85EBCA6B & M32
    x ^= x >> 13
    return x


def key_valid(k: bytes) -> bool:
    src, dst, sport, dport, proto, family, pad = k[:16], k[16:32], k[32:34], k[34:36], k[36], k[37], k[38:40]
    if pad != b"\0\0" or family not in (4, 6):
        return False
    if family == 4 and (any(src[4:]) or any(dst[4:])):
        return False
    if proto not in (TCP, UDP, ICMP if family == 4 else ICMP6):
        return False
    return proto in (TCP, UDP) or sport + dport == bytes(4)


def slots_valid(n_slots: int) -> bool:
    return 0 < n_slots <= 1 << 31 and n_slots & (n_slots - 1) == 0


def build(keys, rules, n_slots):
    """(status, table): 0 and the table, or EINVAL / ERANGE and None."""
    if not slots_valid(n_slots):
        return EINVAL, None
    table = [None] * n_slots
    for k, rule in zip(keys, rules):
        k = bytes(k)
        if len(k) != 40 or not key_valid(k):
            return EINVAL, None
        h = key_hash(k)
        for p in range(MAX_PROBE):
            i = (h + p) & (n_slots - 1)
            if table[i] is None:
                table[i] = (k, rule & M32, h | 0x80000000)
                break
            if table[i][0] == k:
                return EINVAL, None  # a duplicate key
        else:
            return ERANGE, None
    return 0, table


def table_bytes(table) -> bytes:
    return b"".join(bytes(48) if e is None else e[0] + e[1].to_bytes(4, "little") + e[2].to_bytes(4, "little")
                    for e in table)


def table_from_bytes(raw: bytes):
    """The inverse of table_bytes, for hand-made tables: any 48-byte entries, a zero tag empty."""
    assert len(raw) % 48 == 0
    out = []
    for i in range(0, len(raw), 48):
        tag = int.from_bytes(raw[i + 44:i + 48], "little")
        out.append(None if tag == 0 else (raw[i:i + 40], int.from_bytes(raw[i + 40:i + 44], "little"), tag))
    return out


def lookup(table, k: bytes):
    """The entry's rule, or None for a miss: at most MAX_PROBE entries from the key's home slot,
    every index masked; an empty entry ends the search."""
    n_slots = len(table)
    assert slots_valid(n_slots)
    h = key_hash(k)
    for p in range(MAX_PROBE):
        e = table[(h + p) & (n_slots - 1)]
        if e is None:
            return None
        if e[2] == h | 0x80000000 and e[0] == k:
            return e[1]
    return None


def classify(frame, table, miss_rule, other_rule, ok=None, ok_mask=3):
    """(rule index, class) of one frame that the layout does not refuse; ok: its RX verdict or None."""
    if ok is not None and ok & ok_mask != ok_mask:
        return NO_RULE, PASSED
    c = frame_class(frame)
    if c == MALFORMED:
        return NO_RULE, 0
    if c == NO_KEY:
        return other_rule & M32, UNKEYED
    rule = lookup(table, c)
    return (miss_rule & M32, MISS) if rule is None else (rule, HIT)
