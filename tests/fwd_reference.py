"""A plain reference of the forwarder's header rewrite (pipck_fwd_rewrite_ring,
include/pipck.h "NAT and TTL rewrite of frames in a device ring"), written from
that comment and the RFCs behind it -- 1624 (incremental update of the Internet
checksum, eqn. 3), 1812 section 5.3.1 (TTL), 3022 section 4.1 (NAT header
manipulations, the UDP zero field) -- and from nothing else: no ctypes, no
oracle, nothing of pip_amd.  It covers what the call does to ONE frame under ONE
rule, steps 2 to 6 of the header's list; the refusals of step 1 (a length past
the slot, a rule index past the table, PIPCK_FWD_NO_RULE) concern the ring and
are the GPU tests' own.  The GPU tests compare whole rings with rewrite() byte
for byte.

Arithmetic: exact Python integers.  RFC 1624 eqn. 3, HC' = ~(~HC + ~m + m'),
over all the 16-bit big-endian words of the named fields at once:
    s   = (~HC & 0xFFFF) + sum(~old_k & 0xFFFF) + sum(new_k)
    HC' = ~fold(s) & 0xFFFF,   fold: end-around carry until s < 0x10000.
"""
from tests.rx_reference import wsum  # noqa: F401  (the tests sum ranges with it)
from tests.tx_reference import CSUM_AT, MIN_L4, _upper

SET_SRC, SET_DST, SET_SPORT, SET_DPORT, DEC_TTL = 1, 2, 4, 8, 16
ALL_OPS = 31
UDP_ZERO_AS_ONES = 1  # flags bit 0
DONE, EXPIRED, UNHANDLED = 1, 2, 4

TCP, UDP, ICMP, ICMP6 = 6, 17, 1, 58


def rule(ops, family=0, src=b"", dst=b"", sport=b"\0\0", dport=b"\0\0"):
    """A rule as the dict rewrite() takes: addresses and ports as wire bytes
    (IPv4 uses the first 4 bytes of a 16-byte address)."""
    return {"ops": ops, "family": family, "src": bytes(src).ljust(16, b"\0"), "dst": bytes(dst).ljust(16, b"\0"),
            "sport": bytes(sport), "dport": bytes(dport)}


def rule_valid(r) -> bool:
    if r["ops"] & ~ALL_OPS or r["family"] not in (0, 4, 6):
        return False
    return r["family"] != 0 or not r["ops"] & (SET_SRC | SET_DST)


def fold(s: int) -> int:
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def update(hc: int, old: bytes, new: bytes) -> int:
    """RFC 1624 eqn. 3: the field hc after the words of `old` became those of `new`."""
    assert len(old) == len(new) and len(old) % 2 == 0
    s = ~hc & 0xFFFF
    for k in range(0, len(old), 2):
        s += ~(old[k] << 8 | old[k + 1]) & 0xFFFF
        s += new[k] << 8 | new[k + 1]
    return ~fold(s) & 0xFFFF


def _be16(b, i) -> int:
    return b[i] << 8 | b[i + 1]


def rewrite(frame, rule, flags=0):
    """(the frame after the call, its done value).  An invalid rule (rule_valid) leaves the
    frame untouched with done 0; the call also sets 1 << PIPCK_EINVAL in d_err then."""
    f = bytearray(frame)
    same = bytes(f)
    ops = rule["ops"]
    if not rule_valid(rule):
        return same, 0
    # 3. malformed, by the rules of pipck_tx_fill_device
    if len(f) < 20:
        return same, 0
    version = f[0] >> 4
    if version == 4:
        ihl, total = (f[0] & 15) * 4, _be16(f, 2)
        if ihl < 20 or total < ihl or total > len(f):
            return same, 0
        ttl_at = 8
    elif version == 6:
        if len(f) < 40 or 40 + _be16(f, 4) > len(f):
            return same, 0
        ttl_at = 7
    else:
        return same, 0
    v4 = version == 4
    # 4. nothing left to decrement
    if ops & DEC_TTL and f[ttl_at] <= 1:
        return same, EXPIRED
    # 5. what the call does not handle
    if rule["family"] and rule["family"] != version:
        return same, UNHANDLED
    addr, port = ops & (SET_SRC | SET_DST), ops & (SET_SPORT | SET_DPORT)
    proto = at = None
    if addr or port:
        up = _upper(f)
        if up is None:
            return same, UNHANDLED
        proto, at, end = up
        if port and proto not in (TCP, UDP):
            return same, UNHANDLED
        if proto not in (TCP, UDP, ICMP if v4 else ICMP6):
            return same, UNHANDLED
        if end - at < MIN_L4[proto]:
            return same, UNHANDLED
    # 6. the named fields, old and new, and the checksum fields that cover them
    ip_old, ip_new, l4_old, l4_new = b"", b"", b"", b""
    if ops & DEC_TTL:
        if v4:
            ip_old += bytes(f[8:10])
        f[ttl_at] -= 1
        if v4:
            ip_new += bytes(f[8:10])
    alen = 4 if v4 else 16
    for bit, at_v4, at_v6, value in ((SET_SRC, 12, 8, rule["src"]), (SET_DST, 16, 24, rule["dst"])):
        if ops & bit:
            a = at_v4 if v4 else at_v6
            old, new = bytes(f[a:a + alen]), value[:alen]
            f[a:a + alen] = new
            if v4:
                ip_old, ip_new = ip_old + old, ip_new + new
            if proto != ICMP:  # ICMP over IPv4 has no pseudo-header
                l4_old, l4_new = l4_old + old, l4_new + new
    for bit, off, value in ((SET_SPORT, 0, rule["sport"]), (SET_DPORT, 2, rule["dport"])):
        if ops & bit:
            old = bytes(f[at + off:at + off + 2])
            f[at + off:at + off + 2] = value
            l4_old, l4_new = l4_old + old, l4_new + value
    if ip_old:
        f[10:12] = update(_be16(f, 10), ip_old, ip_new).to_bytes(2, "big")
    if l4_old:
        c = at + CSUM_AT[proto]
        hc = _be16(f, c)
        if not (proto == UDP and v4 and hc == 0):  # RFC 3022 section 4.1: no checksum was sent
            hc = update(hc, l4_old, l4_new)
            if proto == UDP and hc == 0 and flags & UDP_ZERO_AS_ONES:
                hc = 0xFFFF
            f[c:c + 2] = hc.to_bytes(2, "big")
    return bytes(f), DONE
