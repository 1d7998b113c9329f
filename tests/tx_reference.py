"""A plain reference of the TX checksum fill (pipck_tx_fill_device, include/pipck.h
"TX checksum fill of frames already in DEVICE memory"), written from that comment
and the RFCs behind it -- 791 (IPv4), 768 (UDP), 793 (TCP), 792 (ICMP), 8200
sections 4 and 8.1 (IPv6 extension headers, upper-layer checksums), 4443 section
2.3 (ICMPv6), 1071 (the sum) -- and from nothing else: no ctypes, no oracle,
nothing of pip_amd.  The GPU tests compare whole arenas with fill() byte for byte.

Arithmetic: a range is summed as exact Python integers (rx_reference.wsum:
big-endian 16-bit words, an odd last byte the high byte of a zero-padded word).
The value stored is pip's: the sum folded to 16 bits by end-around carry, then
complemented (pip_checksum.cpp:29-30 and the final ~).  Folding an exact sum s
gives 0 for s == 0 and 1 + (s - 1) % 0xFFFF otherwise, so a sum that is a
non-zero multiple of 0xFFFF stores 0x0000 and a zero sum stores 0xFFFF; both
corners come out of the one loop below.
"""
from tests.rx_reference import wsum

IP_FILLED, L4_FILLED = 1, 2
UDP_ZERO_AS_ONES = 1  # flags bit 0

TCP, UDP, ICMP, ICMP6 = 6, 17, 1, 58
HOPOPTS, DSTOPTS, FRAGMENT, ROUTING = 0, 60, 44, 43
MAX_EXT = 8
MIN_L4 = {TCP: 20, UDP: 8, ICMP: 8, ICMP6: 8}
CSUM_AT = {TCP: 16, UDP: 6, ICMP: 2, ICMP6: 2}


def checksum(s: int) -> int:
    """pip's checksum of a range whose exact word sum is s: fold, complement."""
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return ~s & 0xFFFF


def _be16(b, i) -> int:
    return b[i] << 8 | b[i + 1]


def _upper(f):
    """(protocol, offset, end) of the upper-layer message, or None where nothing
    more than the IPv4 header field is written.  f is a well-formed IPv4 or IPv6 frame."""
    if f[0] >> 4 == 4:
        if _be16(f, 6) & 0x3FFF:  # MF or an offset: a fragment
            return None
        return f[9], (f[0] & 15) * 4, _be16(f, 2)
    end = 40 + _be16(f, 4)
    nh, at, walked = f[6], 40, 0
    while nh in (HOPOPTS, DSTOPTS, FRAGMENT):
        if walked == MAX_EXT:
            return None  # a ninth extension header
        if at + 8 > end:
            return None  # does not fit in the payload
        size = 8 if nh == FRAGMENT else 8 * (f[at + 1] + 1)
        if at + size > end:
            return None
        if nh == FRAGMENT and _be16(f, at + 2) & 0xFFF9:  # an offset or M
            return None
        nh, at, walked = f[at], at + size, walked + 1
    if nh == ROUTING:
        return None
    return nh, at, end


def fields(frame):
    """[(offset of a checksum field this call writes, which bit it sets)] -- for
    tests that overwrite the fields before filling."""
    f = bytes(frame)
    filled, done = fill(f)
    out = []
    if done & IP_FILLED:
        out.append((10, IP_FILLED))
    if done & L4_FILLED:
        proto, at, _ = _upper(f)
        out.append((at + CSUM_AT[proto], L4_FILLED))
    return out


def fill(frame, flags=0):
    """(the frame with its checksum fields filled, the PIPCK_TX_* bits)."""
    f = bytearray(frame)
    if len(f) < 20:
        return bytes(f), 0
    version = f[0] >> 4
    done = 0
    if version == 4:
        ihl, total = (f[0] & 15) * 4, _be16(f, 2)
        if ihl < 20 or total < ihl or total > len(f):
            return bytes(f), 0
        hdr = bytearray(f[:ihl])
        hdr[10:12] = b"\0\0"  # the field taken as zero
        f[10:12] = checksum(wsum(hdr)).to_bytes(2, "big")
        done |= IP_FILLED
        addresses = f[12:20]
    elif version == 6:
        if len(f) < 40 or 40 + _be16(f, 4) > len(f):
            return bytes(f), 0
        addresses = f[8:40]
    else:
        return bytes(f), 0
    up = _upper(f)
    if up is None:
        return bytes(f), done
    proto, at, end = up
    v4 = version == 4
    if proto not in MIN_L4 or (proto == ICMP and not v4) or (proto == ICMP6 and v4):
        return bytes(f), done  # another protocol
    msg = bytearray(f[at:end])  # link padding after `end` is not summed
    if len(msg) < MIN_L4[proto]:
        return bytes(f), done
    c = CSUM_AT[proto]
    msg[c:c + 2] = b"\0\0"  # the field taken as zero, whatever it held (UDP over IPv4 too)
    s = wsum(msg)
    if proto != ICMP:  # ICMP over IPv4 has no pseudo-header
        s += wsum(addresses) + proto + len(msg)
    value = checksum(s)
    if proto == UDP and value == 0 and flags & UDP_ZERO_AS_ONES:
        value = 0xFFFF
    f[at + c:at + c + 2] = value.to_bytes(2, "big")
    return bytes(f), done | L4_FILLED
