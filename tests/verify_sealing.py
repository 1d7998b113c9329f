"""Host-side inputs for the batch RX-verify tests: flow tables, packets that
carry a correct checksum field ("sealed"), deliberate damage, and the expected
verdict of every packet from tests/verify_reference.py.  numpy only; the
checksum stored into a field comes from the CPU oracle (oracle/oracle.py),
never from a GPU kernel.
"""
import numpy as np

from tests import verify_reference as vr


def flow_table(rng, family: int, n_flows: int, proto: int):
    """(records, pseudo): n_flows pipck_flow4 / pipck_flow6 records (include/pipck.h)
    as bytes, and per flow the reference's (family, src, dst, proto).  Flow 0 is
    all zero (addresses and protocol), flow 1 all 0xFF, the rest random."""
    alen = 4 if family == 4 else 16
    rec, pseudo = bytearray(), []
    for f in range(n_flows):
        if f == 0:
            src, dst, p = bytes(alen), bytes(alen), 0
        elif f == 1:
            src, dst, p = b"\xff" * alen, b"\xff" * alen, 0xFF
        else:
            src, dst, p = rng.integers(0, 256, alen, dtype=np.uint8).tobytes(), \
                rng.integers(0, 256, alen, dtype=np.uint8).tobytes(), proto
        rec += src + dst + bytes([p, 0, 0, 0])
        pseudo.append((family, src, dst, p))
    return bytes(rec), pseudo


def _field(i: int, length: int, rng) -> int:
    """The even offset of packet i's checksum field, rotating over: the first
    word, the last whole word, 14 and 16 where they fit (at a misaligned packet
    start the field then straddles a 16-byte chunk in memory), a random one."""
    last = (length - 2) & ~1
    k = i % 5
    if k == 0:
        return 0
    if k == 1:
        return last
    if k == 2 and 14 <= last:
        return 14
    if k == 3 and 16 <= last:
        return 16
    return 2 * int(rng.integers(0, last // 2 + 1))


def seal(host: np.ndarray, offs, lens, pseudo_of, oracle, rng, rotate: int = 0) -> np.ndarray:
    """Give every packet of at least 2 bytes a correct checksum field, in place:
    the field is zeroed, the packet checksummed by the CPU oracle (ip_checksum
    without a pseudo-header, inet_checksum / inet6_checksum with pseudo_of(i) =
    (family, src, dst, proto)) and the result stored big-endian.  Packets of 0 or
    1 bytes and every byte outside the packets are left as they are.  `rotate`
    shifts the rotation of the field positions (packet i takes position i + rotate).
    Returns the field offsets (-1: not sealed)."""
    fields = np.full(len(lens), -1, dtype=np.int64)
    for i, (o, length) in enumerate(zip(offs, lens)):
        o, length = int(o), int(length)
        if length < 2:
            continue
        at = _field(i + rotate, length, rng)
        host[o + at:o + at + 2] = 0
        data = host[o:o + length].tobytes()
        ps = pseudo_of(i)
        if ps is None:
            c = oracle.ip_checksum(data)
        elif ps[0] == 4:
            c = oracle.inet_checksum(data, ps[3], ps[1], ps[2])
        else:
            c = oracle.inet6_checksum(data, ps[3], ps[1], ps[2])
        host[o + at], host[o + at + 1] = c >> 8, c & 0xFF
        fields[i] = at
    return fields


def damage(host: np.ndarray, offs, lens, rng) -> None:
    """Damage packets by index class i % 8, in place.  0: one flipped bit; 1: two
    16-bit words at even offsets swapped (sum-neutral: must still verify);
    2: the adjacent bytes at offsets 2k+1 and 2k+2 swapped; 3..7: untouched.
    In a batch of fewer than 64 packets, packet 0 stays untouched as well: it is
    the packet check_mix() requires to verify there."""
    for i, (o, length) in enumerate(zip(offs, lens)):
        o, length, k = int(o), int(length), i % 8
        if i == 0 and len(lens) < 64:
            continue
        if k == 0 and length >= 1:
            host[o + int(rng.integers(0, length))] ^= 1 << int(rng.integers(0, 8))
        elif k == 1 and length >= 4:
            a, b = (2 * int(x) for x in rng.choice(length // 2, 2, replace=False))
            wa = host[o + a:o + a + 2].copy()
            host[o + a:o + a + 2] = host[o + b:o + b + 2]
            host[o + b:o + b + 2] = wa
        elif k == 2 and length >= 3:
            a = 2 * int(rng.integers(0, (length - 1) // 2)) + 1
            host[o + a], host[o + a + 1] = host[o + a + 1], host[o + a]


def expected(host: np.ndarray, offs, lens, pseudo_of) -> np.ndarray:
    """verify_reference.verdict of every packet's bytes as they are now (uint8)."""
    return np.array([vr.verdict(host[int(o):int(o) + int(length)].tobytes(), pseudo_of(i))
                     for i, (o, length) in enumerate(zip(offs, lens))], dtype=np.uint8)


def check_mix(want: np.ndarray, lens, fields) -> None:
    """The condition every case's inputs meet, so that no case can go back to
    comparing all zeros: from 64 packets on, the reference gives at least two
    fifths of them 1 and at least one sixteenth 0; below that, packet 0 is a
    sealed packet of at least 2 bytes that the reference accepts."""
    n = len(want)
    if n >= 64:
        ones = int(want.sum())
        assert 5 * ones >= 2 * n, (ones, n)
        assert 16 * (n - ones) >= n, (ones, n)
    else:
        assert int(lens[0]) >= 2 and fields[0] >= 0 and want[0] == 1
