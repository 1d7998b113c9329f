"""tests/host_sum_reference.py held to pip, on the CPU, before pipck_host_sum is
held to it: chain_sum against the oracle restatement of pip_standard_checksum
on every table case and against every known answer of tests/golden/kat.json
(pip's compiled results), and the conditions on the table that keep the GPU
tests (tests/test_gpu_host_sum.py) from passing with nothing to find."""
import pytest

from pip_amd import checksum as pc
from tests import host_sum_reference as hr
from tests.golden.make_golden import pattern_bytes, run_case


def _oracle_chain(oracle, segs, init: int) -> int:
    s = init & 0xFFFFFFFF
    for seg in (segs if len(segs) else [b""]):
        s = oracle.standard_checksum(seg, None, s)
    return s


@pytest.mark.parametrize("cls", hr.CLASSES)
def test_reference_equals_the_oracle_on_every_table_case(oracle, cls):
    cases = hr.by_class(cls)
    assert cases
    want = hr.expected()
    for c in cases:
        assert want[c.name] == _oracle_chain(oracle, c.segs, c.init), c.name
        assert want[c.name] <= 0xFFFF, c.name


def test_reference_equals_the_oracle_on_the_stale_sequence(oracle):
    for c in hr.stale_sequence():
        assert hr.chain_sum(c.segs, c.init) == _oracle_chain(oracle, c.segs, c.init), c.name


def test_reference_small_known_values():
    assert hr.chain_sum([], 0) == 0 and hr.chain_sum([b""], 0) == 0
    assert hr.chain_sum([], 0xFFFFFFFF) == 0xFFFF  # fold(fold()) of the initial sum alone
    assert hr.chain_sum([b"\xff\xff"], 0) == 0xFFFF
    assert hr.chain_sum([b"\x01"], 0) == 0x0100  # an odd byte is a high byte
    assert hr.chain_sum([b"\x01", b"\x02"], 0) == 0x0300  # padded per segment, not joined
    assert hr.chain_sum([b"\x01\x02"], 0) == 0x0102
    assert hr.chain_sum([b"\x00\x01"], 0xFFFFFFFF) == 0  # 2^32 wraps to 0: the carry is lost
    assert hr.chain_sum_nowrap([b"\x00\x01"], 0xFFFFFFFF) == 1
    assert hr.wraps([b"\x00\x01"], 0xFFFFFFFF) and not hr.wraps([b"\x00\x00"], 0xFFFFFFFF)
    assert hr.chain_sum([bytearray(b"\x12\x34\x56")], 1) == 0x1234 + 0x5600 + 1


class _ChainSumAdapter:
    """run_case() adapter: pip_amd.checksum's own pseudo-header arithmetic with
    its device call replaced by chain_sum (see the monkeypatch below)."""

    standard_checksum = staticmethod(lambda d, n, s: pc.pip_standard_checksum(d, n, s))
    ip_checksum = staticmethod(lambda d, n=None: pc.pip_ip_checksum(d, n))
    fold_uint32 = staticmethod(pc.pip_fold_uint32)
    inet_checksum = staticmethod(lambda d, p, s, t, n=None: pc.pip_inet_checksum(d, p, s, t, n))
    inet6_checksum = staticmethod(lambda d, p, s, t, n=None: pc.pip_inet6_checksum(d, p, s, t, n))
    inet_checksum_chain = staticmethod(pc.pip_inet_checksum_buf)
    inet6_checksum_chain = staticmethod(pc.pip_inet6_checksum_buf)


def test_reference_equals_pips_known_answers(kat, monkeypatch):
    """Every kat.json case.  standard and ip straight through chain_sum; inet,
    inet6 and the two chain functions through pip_amd.checksum with _device_sum
    replaced by chain_sum, which pins checksum.py's pseudo-header terms as well."""
    seen = {}
    for c in kat:
        if c["fn"] == "standard":
            got = hr.chain_sum([pattern_bytes(c["data"])], c["sum"])
        elif c["fn"] == "ip":
            got = ~hr.chain_sum([pattern_bytes(c["data"])], 0) & 0xFFFF
        else:
            continue
        assert got == c["expect"], c
        seen[c["fn"]] = seen.get(c["fn"], 0) + 1
    calls = []

    def device_sum(segments, init):
        calls.append(len(segments))
        return hr.chain_sum([bytes(s) for s in segments], init)

    monkeypatch.setattr(pc, "_device_sum", device_sum)
    for c in kat:
        assert run_case(_ChainSumAdapter, c) == c["expect"], c
        seen[c["fn"]] = seen.get(c["fn"], 0) + 1
    assert len(calls) == sum(1 for c in kat if c["fn"] != "fold")
    assert all(seen.get(fn, 0) >= 10 for fn in ("standard", "ip", "inet", "inet6", "inet_chain", "inet6_chain")), seen


# ----------------------------------------------------------------------------
# conditions on the table
# ----------------------------------------------------------------------------
def _wrap_class(c) -> str:
    if hr.case_need(c) > hr.ZERO_COPY_MAX:
        return "over"
    return "inline" if 1 <= len(c.segs) <= hr.INLINE_SEGS else "long"


def test_table_wrap_cases_matter_in_every_loop():
    """At least eight wrapping cases for the resident block's one-pass loop
    (1..5 segments), eight for its long loop (6 or more) and eight that are
    staged in modes 2-4 (need > 68 KiB); each of them separates a u32
    accumulator from a wider one."""
    seen = {"inline": 0, "long": 0, "over": 0}
    for c in hr.table():
        if not hr.wraps(c.segs, c.init):
            continue
        assert hr.expected()[c.name] != hr.chain_sum_nowrap(c.segs, c.init), c.name
        seen[_wrap_class(c)] += 1
    assert all(v >= 8 for v in seen.values()), seen


def test_table_covers_every_segment_count():
    counts = {len(c.segs) for c in hr.table()}
    assert set(hr.COUNTS) <= counts
    for n in hr.COUNTS:
        inits = {c.init for c in hr.by_class("counts") if len(c.segs) == n}
        assert {0, 0xFFFF, 0x10000, 0xFFFF0000, 0xFFFFFFFF} < inits, n  # and one random u32
    # all of the counts class is served zero-copy (mode 2) or by the resident block (3, 4)
    assert max(hr.case_need(c) for c in hr.by_class("counts")) < hr.ZERO_COPY_MAX // 2
    assert {len(s) for c in hr.by_class("counts") for s in c.segs} == set(hr.LENGTH_CYCLE)


def test_table_paths_of_the_tiny_and_wrap_classes():
    need = {c.name: hr.case_need(c) for c in hr.table()}
    assert need["tiny_2000x1"] == 64000 and need["tiny_4000x0"] == 64000
    assert need["tiny_2200x1"] == 70400 > hr.ZERO_COPY_MAX
    later = [c for c in hr.by_class("wrap") if c.name.startswith("wrap_later_")]
    assert len(later) == 3
    for c in later:
        # the first segment does not wrap, the second does
        assert not hr.wraps(c.segs[:1], c.init) and hr.wraps(c.segs[:2], c.init), c.name
        assert need[c.name] > hr.ZERO_COPY_MAX


def test_table_threshold_lengths():
    """need = roundup16(16 * nseg) + sum(roundup16(len)) (pipck_host_sum): exactly
    68 KiB and one 16-byte chunk more, with a 16-byte and a 32-byte table."""
    assert hr.ZERO_COPY_MAX == 69632
    assert hr.threshold_lengths(1, False) == [69616] and hr.threshold_lengths(1, True) == [69617]
    assert hr.need([69616]) == 16 + 69616 == 69632 and hr.need([69617]) == 69648
    for nseg in (1, 2):
        at, over = hr.threshold_lengths(nseg, False), hr.threshold_lengths(nseg, True)
        assert len(at) == len(over) == nseg
        assert hr.need(at) == hr.ZERO_COPY_MAX and hr.need(over) == hr.ZERO_COPY_MAX + 16
        assert sum(over) == sum(at) + 1
    got = sorted(hr.case_need(c) for c in hr.by_class("threshold"))
    assert got == [69632, 69632, 69648, 69648]
    assert sorted(len(c.segs) for c in hr.by_class("threshold")) == [1, 1, 2, 2]


def test_table_inline_class_shapes():
    shapes = {tuple(len(s) for s in c.segs) for c in hr.by_class("inline")}
    for n in (32767, 32768, 32769, 32784, 65535):
        assert (n,) in shapes
    for want in ((0, 13000, 1, 0, 20001), (16, 0, 16), (0, 0, 0, 0, 7), (7, 0, 0, 0, 0), (6553,) * 5):
        assert want in shapes
    for n in (2, 3, 5):
        for pos in (0, n // 2, n - 1):
            assert any(len(s) == n and s[pos] == 0 and sum(1 for x in s if x == 0) == 1 for s in shapes), (n, pos)
    assert all(1 <= len(s) <= hr.INLINE_SEGS for s in shapes)
    assert all(hr.case_need(c) <= hr.ZERO_COPY_MAX for c in hr.by_class("inline"))


def test_stale_sequence_expects_zero_after_ff():
    seq = hr.stale_sequence()
    names = [c.name for c in seq]
    assert names[0] == "stale_fill_4096ff" and seq[0].segs == [b"\xff" * 4096]
    grow = names.index("stale_grow_1572864ff")
    assert hr.need([len(seq[grow].segs[0])]) > 1 << 20  # past the staging buffer's first allocation
    for part in (seq[1:grow], seq[grow + 1:]):
        assert [len(c.segs[0]) for c in part[:49]] == list(range(49))
        assert [len(s) for s in part[49].segs] == [1, 17, 33]
        assert [len(s) for s in part[50].segs] == [1, 17, 33, 1, 17, 33]
        assert len(part) == 51
        for c in part:
            assert c.init == 0 and not any(any(s) for s in c.segs), c.name
            assert hr.chain_sum(c.segs, c.init) == 0, c.name
    assert hr.chain_sum(seq[0].segs, 0) == 0xFFFF
    assert hr.wraps(seq[grow].segs, 0) and hr.chain_sum(seq[grow].segs, 0) == 0xFFF4  # 786,432 * 0xFFFF mod 2^32
