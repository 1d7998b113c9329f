"""A plain reference of the RX verdict (the PIPCK_RX_* bits of include/pipck.h,
"RX verification of received packets"), written from that comment and the RFCs
it cites -- 791 (IPv4), 768 (UDP), 793 (TCP), 792 (ICMP), 8200 section 4 (IPv6
extension headers), 4443 section 2.3 (ICMPv6) -- and from nothing else: no
ctypes, no oracle, nothing of pip_amd.  The GPU tests compare every verifying
path with verdict() bit for bit.

Arithmetic: a range is summed as exact Python integers, big-endian 16-bit
words, an odd last byte being the high byte of a zero-padded word.  A range
VERIFIES iff that sum is non-zero and divisible by 0xFFFF: the one's-complement
sum of the words is then 0xFFFF ("all ones", RFC 1071), and an all-zero range
(whose one's-complement sum is +0, not -0) does not verify.  No fold, no carry,
so every 0x0000 / 0xFFFF corner is decided by that one rule.
"""
import struct

IP_OK, L4_OK, L4_CHECKED = 1, 2, 4
VERIFIED, UNCHECKED = 7, 3

TCP, UDP, ICMP, ICMP6 = 6, 17, 1, 58
HOPOPTS, DSTOPTS, FRAGMENT, ROUTING = 0, 60, 44, 43
MAX_EXT = 8  # extension headers walked; a ninth leaves the payload unchecked
MIN_L4 = {TCP: 20, UDP: 8, ICMP: 8, ICMP6: 8}
CSUM_AT = {TCP: 16, UDP: 6, ICMP: 2, ICMP6: 2}  # offset of the checksum field in the message


def wsum(b) -> int:
    """Exact sum of the big-endian 16-bit words of b (odd last byte: high byte)."""
    n = len(b) & ~1
    s = sum(struct.unpack(">%dH" % (n // 2), bytes(b[:n])))
    if len(b) & 1:
        s += b[-1] << 8
    return s


def verifies(s: int) -> bool:
    return s != 0 and s % 0xFFFF == 0


def _be16(b, i) -> int:
    return b[i] << 8 | b[i + 1]


def _l4(ip_bits: int, proto: int, msg, pseudo: int, v4: bool) -> int:
    """The verdict once the upper layer is found: msg is the IP payload from the
    upper-layer offset, pseudo the sum of addresses + protocol + L4 length."""
    if proto not in MIN_L4 or (proto == ICMP and not v4) or (proto == ICMP6 and v4):
        return ip_bits | L4_OK  # another protocol: nothing to check
    if len(msg) < MIN_L4[proto]:
        return ip_bits  # truncated TCP / UDP / ICMP header: L4 bits clear
    if proto == UDP and v4 and _be16(msg, 6) == 0:
        return ip_bits | L4_OK  # RFC 768: no checksum was sent
    s = wsum(msg) + (0 if proto == ICMP else pseudo)
    return ip_bits | L4_CHECKED | (L4_OK if verifies(s) else 0)


def verdict(frame: bytes) -> int:
    f = bytes(frame)
    if len(f) < 20:
        return 0
    version = f[0] >> 4
    if version == 4:
        ihl = (f[0] & 15) * 4
        total = _be16(f, 2)
        if ihl < 20 or total < ihl or total > len(f):
            return 0
        bits = IP_OK if verifies(wsum(f[:ihl])) else 0
        if _be16(f, 6) & 0x3FFF:  # MF or an offset: a fragment
            return bits | L4_OK
        msg = f[ihl:total]
        return _l4(bits, f[9], msg, wsum(f[12:20]) + f[9] + len(msg), True)
    if version == 6:
        if len(f) < 40:
            return 0
        end = 40 + _be16(f, 4)
        if end > len(f):
            return 0
        nh, at, walked = f[6], 40, 0
        while nh in (HOPOPTS, DSTOPTS, FRAGMENT):
            if walked == MAX_EXT:
                return IP_OK | L4_OK  # a ninth extension header
            if at + 8 > end:
                return IP_OK  # does not fit in the payload
            size = 8 if nh == FRAGMENT else 8 * (f[at + 1] + 1)
            if at + size > end:
                return IP_OK
            if nh == FRAGMENT and _be16(f, at + 2) & 0xFFF9:  # an offset or M
                return IP_OK | L4_OK
            nh, at, walked = f[at], at + size, walked + 1
        if nh == ROUTING:
            return IP_OK | L4_OK
        msg = f[at:end]
        return _l4(IP_OK, nh, msg, wsum(f[8:40]) + nh + len(msg), False)
    return 0


# ---- frames with correct checksums, by the same arithmetic ---------------------


def csum_field(s: int) -> int:
    """The 16-bit value that, added to a range of exact sum s (field zeroed),
    makes it verify: the one's complement of s folded (RFC 1071)."""
    return 0xFFFF - s % 0xFFFF if s % 0xFFFF else (0xFFFF if s == 0 else 0)


def ext_chain(chain, upper):
    """IPv6 extension headers, chain = [(type, arg)] in order: arg is the
    fragment field (offset << 3 | M) of a fragment header (44), else the Hdr Ext
    Len (the header is 8 * (arg + 1) bytes, PadN-filled).  Returns (bytes, type
    of the first header) -- what build(ext=...) takes."""
    out = b""
    types = [t for t, _ in chain] + [upper]
    for i, (t, arg) in enumerate(chain):
        if t == FRAGMENT:
            out += struct.pack(">BBHI", types[i + 1], 0, arg, 0x1234)
        else:
            n = 8 * (arg + 1)
            body, left = b"", n - 2
            while left:  # PadN options of at most 257 bytes each; Pad1 for a last single byte
                k = min(left, 257)
                body += bytes([1, k - 2]) + bytes(k - 2) if k >= 2 else b"\0"
                left -= k
            out += bytes([types[i + 1], arg]) + body
    return out, types[0]


def build(rng, fam, proto, l4len, *, options=b"", ext=None, frag=0, no_udp_sum=False, l4=None, fill=True):
    """An IPv4 (fam 4) or IPv6 (fam 6) frame carrying an l4len-byte message of
    `proto` with every checksum correct: the IPv4 header's over the header with
    its options; TCP / UDP / ICMPv6 over message + addresses + protocol + L4
    length; ICMPv4 over the message.  options: IPv4 option bytes (a multiple of
    4, at most 40); ext: IPv6 extension headers as ext_chain() returns them;
    frag: the IPv4 ip_off field (default DF); no_udp_sum: UDP over IPv4 with a
    zero field; l4: the message itself instead of random bytes (l4len ignored) --
    its checksum field is still filled in unless fill is false."""
    msg = bytearray(rng.randbytes(l4len) if l4 is None else l4)
    alen = 4 if fam == 4 else 16
    src, dst = rng.randbytes(alen), rng.randbytes(alen)
    known = proto in (TCP, UDP) or proto == (ICMP if fam == 4 else ICMP6)
    if known and fill and len(msg) >= CSUM_AT[proto] + 2:
        at = CSUM_AT[proto]
        msg[at:at + 2] = b"\0\0"
        if not (proto == UDP and fam == 4 and no_udp_sum):
            s = wsum(msg)
            if proto != ICMP:
                s += wsum(src + dst) + proto + len(msg)
            c = csum_field(s)
            if proto == UDP and c == 0:
                c = 0xFFFF  # RFC 768: a computed zero is sent as all ones
            msg[at:at + 2] = struct.pack(">H", c)
    if fam == 4:
        assert len(options) % 4 == 0 and len(options) <= 40
        ihl = 20 + len(options)
        hdr = bytearray(struct.pack(">BBHHHBBH4s4s", 0x40 | ihl // 4, 0, ihl + len(msg), rng.randrange(1 << 16),
                                    frag or 0x4000, 64, proto, 0, src, dst) + bytes(options))
        hdr[10:12] = struct.pack(">H", csum_field(wsum(hdr)))
        return bytes(hdr) + bytes(msg)
    chain, first = ext if ext else (b"", proto)
    hdr = struct.pack(">IHBB16s16s", 0x60000000 | rng.randrange(1 << 20), len(chain) + len(msg), first, 64, src, dst)
    return hdr + chain + bytes(msg)


def l4_range(frame):
    """(start, end) of the upper-layer message of a frame that build() made and
    verdict() walks to an upper layer (IPv4 without fragmenting, IPv6 through
    hop-by-hop / destination-options / atomic fragment headers)."""
    f = bytes(frame)
    if f[0] >> 4 == 4:
        return (f[0] & 15) * 4, _be16(f, 2)
    nh, at = f[6], 40
    while nh in (HOPOPTS, DSTOPTS, FRAGMENT):
        nh, at = f[at], at + (8 if nh == FRAGMENT else 8 * (f[at + 1] + 1))
    return at, 40 + _be16(f, 4)
