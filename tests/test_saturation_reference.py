"""tests/saturation_cases.py held to pip on the CPU: its single-packet and chain
values equal the oracle's (and pip's own compiled code where oracle/_ref holds
it) on everything those can express, the `dented` fill keeps a tile's results
apart, and the arithmetic behind the chosen segment counts and flow origins is
written out on plain integers."""
import ctypes as C

import numpy as np
import pytest

from tests import saturation_cases as sc
from tests import verify_reference as vr

SINGLE_LENGTHS = (65534, 65535)


def _impls(oracle):
    from oracle.oracle import Reference

    return [("oracle", oracle)] + ([("pip", Reference())] if Reference.available() else [])


def _single(impl, data, ps):
    if ps is None:
        return impl.ip_checksum(data)
    fam, src, dst, proto = ps
    return (impl.inet_checksum if fam == 4 else impl.inet6_checksum)(data, proto, src, dst)


def _same_segment_chain(impl, fam, seg, n, ps):
    """pip_inet{,6}_checksum_buf of n segments that all point at one buffer (70,001 buffers of
    their own cost the binding a second per call)."""
    buf = C.create_string_buffer(seg, len(seg))
    ptrs = (C.c_void_p * n)(*([C.cast(buf, C.c_void_p).value] * n))
    lens = (C.c_uint32 * n)(*([len(seg)] * n))
    _, src, dst, proto = ps
    if fam == 4:
        return impl._fn("inet_checksum_chain")(ptrs, lens, n, proto, int.from_bytes(src, "little"),
                                               int.from_bytes(dst, "little"))
    return impl._fn("inet6_checksum_chain")(ptrs, lens, n, proto, bytes(src), bytes(dst))


def _flow_picks(fam):
    """No pseudo-header for family 0; else the all-zero flow, the all-0xFF flow and two random ones."""
    return [None] if not fam else [sc.flows(fam)[1][f] for f in (0, 1, 2, 96)]


@pytest.mark.parametrize("fill", sc.FILLS)
@pytest.mark.parametrize("length", SINGLE_LENGTHS)
def test_single_packets_equal_pip(oracle, fill, length):
    """Odd and even starts of a saturated arena, all three families."""
    host = sc.arena(fill, length + 64, length)
    for name, impl in _impls(oracle):
        for start in (0, 1, 16, 33):
            data = host[start:start + length].tobytes()
            assert sc.words(data) == vr._words(data)
            for fam in (0, 4, 6):
                for ps in _flow_picks(fam):
                    want = _single(impl, data, ps)
                    assert sc.checksum(data, ps) == want, (name, fill, length, start, fam)
                    assert 0xFFFF ^ vr.ones_sum(data, ps) == want


def test_fill_covers_every_byte():
    ff = sc.arena("ff", 1000)
    assert (ff == 0xFF).all()
    d = sc.arena("dented", 1 << 20, 7)
    dents = int((d != 0xFF).sum())
    # one candidate per 64-byte block, 1/256 of which draw 0xFF again
    assert (1 << 14) * 0.98 < dents <= 1 << 14
    assert all((d[64 * b:64 * b + 64] != 0xFF).sum() <= 1 for b in range(0, 1 << 14, 97))
    assert np.array_equal(d, sc.arena("dented", 1 << 20, 7)) and not np.array_equal(d, sc.arena("dented", 1 << 20, 8))


@pytest.mark.parametrize("fam", [0, 4, 6])
@pytest.mark.parametrize("length", SINGLE_LENGTHS)
def test_dented_tiles_take_many_values(fam, length):
    """The condition on `dented`: the reference results of every 64-packet tile take at least 32
    distinct values (an all-0xFF tile takes one per flow), so a kernel that mixes up two packets
    of a tile, or returns one packet's value for all, cannot pass."""
    _, _, want = sc.fixed_batch("dented", 65536, length, 64 * 2 + 6, fam)
    assert sc.distinct_per_tile(want) >= 32
    _, _, flat = sc.fixed_batch("ff", 65536, length, 70, fam)
    assert len(set(flat.tolist())) <= (sc.NF if fam else 1)


def test_dented_short_packets():
    """Under 64 bytes a packet holds a dent only now and then (24-byte items: three in eight), so
    the 32-value condition cannot hold without a pseudo-header; with one the flows keep the
    results apart, and packets of 128 bytes or more always hold two dents."""
    _, _, w = sc.fixed_batch("dented", 128, 128, 64 * 3, 0)
    assert sc.distinct_per_tile(w) >= 32
    _, _, w = sc.fixed_batch("dented", 24, 20, 64 * 3, 4)
    assert sc.distinct_per_tile(w) >= 32
    _, _, w = sc.fixed_batch("dented", 24, 20, 64 * 3, 0)
    assert sc.distinct_per_tile(w) >= 8


def test_sealed_batches_verify_and_fail():
    for fill in sc.FILLS:
        for fam in (0, 4, 6):
            _, _, want = sc.sealed_fixed_batch(fill, 1008, 1007, 70, fam)
            assert want[0] == 1 and want[1] == 0 and 40 <= int(want.sum()) <= 50, (fill, fam, want)


@pytest.mark.parametrize("fam", [4, 6])
def test_chain_replay_equals_pip(oracle, fam):
    """65,536 to 70,001 two-byte FF FF segments, and six saturated 65,535-byte segments at odd
    and even starts: the replay equals pip_inet{,6}_checksum_buf."""
    ff = sc.arena("ff", 2)
    for name, impl in _impls(oracle):
        fn = impl.inet_checksum_chain if fam == 4 else impl.inet6_checksum_chain
        for ps in _flow_picks(fam)[1::2]:  # the all-0xFF flow and a random one
            for n in sc.CHAIN_COUNTS:
                got = sc.chain_checksum(ff, [0] * n, [2] * n, ps)
                assert got == _same_segment_chain(impl, fam, b"\xff\xff", n, ps), (name, n)
            for fill in sc.FILLS:
                host = sc.arena(fill, 6 * 65536 + 64, fam)
                offs = [k * 65536 + (k % 3) for k in range(6)]
                segs = [host[o:o + 65535].tobytes() for o in offs]
                assert sc.chain_checksum(host, offs, [65535] * 6, ps) == fn(segs, ps[3], ps[1], ps[2]), (name, fill)


def test_aliased_chain_total_len_wraps(oracle):
    """65,538 descriptors of one 65,535-byte region: total_len = 65,538 x 65,535 mod 2^32 = 65,534."""
    n = 65538
    assert (n * 65535) & sc.MASK32 == 65534
    host = sc.arena("dented", 65535 + 32, 9)
    ps = sc.flows(4)[1][5]
    w = sc.words(host[1:1 + 65535])
    want = sc.chain_replay([w] * n, [65535] * n, ps)
    assert want == sc.chain_checksum(host, [1] * n, [65535] * n, ps)
    # the same sum stated without the loop: the segments' total, the pseudo-header with the wrapped length
    assert want == 0xFFFF ^ sc.fold16(n * w + sc.pseudo_terms(ps, 65534))


def test_a_wrapping_u32_chain_sum_differs_from_65538_segments():
    """The finding the segment counts are chosen for.  A finish step that adds the segments'
    folded sums (0xFFFF each) into a u32 and folds once at the end equals pip's loop while
    n x 0xFFFF + P stays below 2^32.  65,537 x 0xFFFF = 2^32 - 1: without a pseudo-header the sum
    first wraps at 65,538 segments; with one, whose terms P are at least hi16 + lo16 of the
    length (>= 1), at 65,537.  Losing 2^32 = 1 (mod 0xFFFF) always changes the result."""
    assert 65537 * 0xFFFF == (1 << 32) - 1
    ff = sc.arena("ff", 2)
    zero4, ones4 = sc.flows(4)[1][0], sc.flows(4)[1][1]
    for n in (1, 2, 40, 65536, 65537, 65538, 70001):
        pip_bare = sc.chain_checksum(ff, [0] * n, [2] * n, None)
        pip_zero = sc.chain_checksum(ff, [0] * n, [2] * n, zero4)
        assert pip_bare == 0x0000  # n x 0xFFFF folds to 0xFFFF
        p_zero = sc.pseudo_terms(zero4, 2 * n)
        assert 1 <= p_zero < 0x10000
        assert (sc.u32_model(n, 0xFFFF, 0) != pip_bare) == (n >= 65538), n
        assert (sc.u32_model(n, 0xFFFF, p_zero) != pip_zero) == (n >= 65537), n
    assert sc.u32_model(65538, 0xFFFF, 0) == 0x0001
    # the all-0xFF flow's unfolded terms pass 0x10000, so for that flow the model already fails at 65,536
    p_ones = sc.pseudo_terms(ones4, 2 * 65536)
    assert p_ones >= 0x10000
    assert sc.u32_model(65536, 0xFFFF, p_ones) != sc.chain_checksum(ff, [0] * 65536, [2] * 65536, ones4)
    assert sc.u32_model(65000, 0xFFFF, sc.pseudo_terms(ones4, 2 * 65000)) == \
        sc.chain_checksum(ff, [0] * 65000, [2] * 65000, ones4)


def test_a_32_bit_remainder_differs_past_2_to_the_64():
    """The second finding.  A test "(flow_origin + p0 + 64) >> 32 == 0" for taking the remainder in
    32 bits passes when that sum wraps past 2^64, while flow_origin + p0 + lane has not wrapped:
    the flow is then the low 32 bits' remainder.  A power-of-two table hides it."""
    origin, nf = (1 << 64) - 32, 97
    assert ((origin + 0 + 64) & sc.MASK64) >> 32 == 0          # the test passes for the first task
    assert sc.implicit_flow(origin, 0, nf) == 29
    assert (origin & sc.MASK32) % nf == 3                       # what the 32-bit remainder gives
    for n_flows in (64, 1024):
        assert all(sc.implicit_flow(origin, i, n_flows) == ((origin + i) & sc.MASK32) % n_flows for i in range(64))
    # past the wrap both agree again: packets 32.. have small indices
    assert all(sc.implicit_flow(origin, i, nf) == (i - 32) % nf for i in range(32, 300))
    # every origin of the GPU cases disagrees with the 32-bit remainder somewhere, or never reaches 2^32
    for o in sc.FLOW_ORIGINS:
        wide = [i for i in range(300) if sc.implicit_flow(o, i, nf) != ((o + i) & sc.MASK32) % nf]
        assert bool(wide) == (o + 299 >= 1 << 32 and o != 0), o


def test_implicit_flows_use_the_whole_table():
    for o in sc.FLOW_ORIGINS:
        for nf in sc.FLOW_COUNTS:
            f = sc.flow_indices(o, 300, nf)
            assert f.min() == 0 and f.max() == nf - 1 and len(set(f.tolist())) == nf
