"""A plain reference of the batch RX-verify rule (include/pipck.h, "batch ABI"
and "RX verification"): d_ok[i] = 1 iff the one's-complement sum of packet i,
with its pseudo-header where the call has one, is 0xFFFF.  Written from that
header comment and RFC 1071 alone, in Python integers: no ctypes, no oracle,
nothing of pip_amd; numpy arrays are accepted only as byte containers.  The GPU
tests (tests/test_gpu_verify.py) hold every verify kernel to verdict() byte for
byte; tests/test_verify_reference.py holds this module to pip first.

The terms, as pipck.h states them for the batch ABI:

    fold(pseudo[flow] + hi16(len) + lo16(len) + sum16be(bytes))

sum16be: the big-endian 16-bit words of the packet, an odd last byte being the
high byte of a zero-padded word.  pseudo[flow]: the big-endian 16-bit words of
the source and destination address (two each for IPv4, eight each for IPv6)
plus the protocol number.  fold: end-around carry until 16 bits remain, so the
result is 0 only for an exact sum of 0 and 0xFFFF for every other multiple of
0xFFFF.
"""
import struct


def _words(b: bytes) -> int:
    """Exact sum of the big-endian 16-bit words of b (odd last byte: high byte)."""
    n = len(b) & ~1
    s = sum(struct.unpack(">%dH" % (n // 2), b[:n]))
    if len(b) & 1:
        s += b[-1] << 8
    return s


def ones_sum(data, pseudo=None) -> int:
    """The folded 16-bit one's-complement sum of `data` (bytes or a uint8 array).
    pseudo = (family, src_bytes, dst_bytes, proto) adds the pseudo-header terms:
    the address words, proto, and hi16(len) + lo16(len) of len(data)."""
    b = bytes(data)
    s = _words(b)
    if pseudo is not None:
        family, src, dst, proto = pseudo
        src, dst = bytes(src), bytes(dst)
        alen = {4: 4, 6: 16}[family]
        if len(src) != alen or len(dst) != alen:
            raise ValueError("address length does not match the family")
        s += _words(src) + _words(dst) + proto + (len(b) >> 16) + (len(b) & 0xFFFF)
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def verdict(data, pseudo=None) -> int:
    """1 iff the packet verifies (its sum is 0xFFFF, "all ones"), else 0."""
    return 1 if ones_sum(data, pseudo) == 0xFFFF else 0
