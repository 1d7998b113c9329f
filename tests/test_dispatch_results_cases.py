"""CPU: what tests/test_gpu_dispatch_results.py rests on (tests/dispatch_results.py).

The census: from tests/golden/dispatch.json and the rule "every knob of a
general or ring group whose flags lack bits 21-23 and whose probes word is 0",
today 5,847 checked launches of the table's 6,216, reaching 193 of its 196
kernel names -- all but the three k_flat_probe / k_flat_coop_probe
instantiations.  The inputs: every batch meets its condition, from the
reference alone, and the references agree with the CPU oracle on the batches as
built."""
import json

import numpy as np
import pytest

from tests import dispatch_cases as dc
from tests import dispatch_results as dr
from tests import rx_reference as R
from tests.conftest import GOLDEN


@pytest.fixture(scope="module")
def golden():
    return json.loads((GOLDEN / "dispatch.json").read_text())


def test_census_covers_every_result_kernel(golden):
    c = dr.census(golden)
    print(f"{sum(c.checked.values())} checked launches of {c.table}, "
          f"{len(c.checked)} of {len(golden['names'])} kernels")
    assert None not in c.checked  # every checked launch launched something
    names = set(golden["names"])
    assert set(c.checked) <= names
    # 1. every kernel but the probe kernels is reached by a checked launch
    assert names - set(c.checked) == {n for n in names if dr.is_probe_kernel(n)}
    assert not any(dr.is_probe_kernel(n) for n in c.checked)
    # 2. no excluded launch is the only route to a kernel that computes results
    assert {n for n in c.excluded if not dr.is_probe_kernel(n)} <= set(c.checked)
    # 3. the checked launches are the table minus the exclusions, counted from the rule alone
    excluded = sum(len(dc.knobs_of(g)) for g in dc.groups() if g not in dr.census_groups())
    excluded += sum(1 for g in dr.census_groups() for k in dc.knobs_of(g).values() if not dr.computes_results(k))
    assert c.table == sum(len(v) for v in golden["cases"].values()) == sum(len(dc.knobs_of(g)) for g in dc.groups())
    assert sum(c.checked.values()) == c.table - excluded == sum(len(dr.checked_knobs(g)) for g in dr.census_groups())
    assert sum(c.excluded.values()) == excluded


def test_the_rule_excludes_by_fields():
    """The knobs left out are those with a probe bit or a probes word, whatever they are called;
    the groups left out are the default-only ones."""
    for s, knobs in dc.KNOB_SETS.items():
        out = {n for n, k in knobs.items() if not dr.computes_results(k)}
        want = {n for n, k in knobs.items() if k["flags"] >> 21 & 7 or k["probes"]}
        assert out == want
        assert (len(out) == 5) == (s != "default_only")
    assert dr.PROBE_FLAGS == 7 << 21
    assert dr.computes_results(dc.knob(flags=1 << 20)) and not dr.computes_results(dc.knob(flags=(1 << 22) | 1))
    assert not dr.computes_results(dc.knob(probes=2))
    left_out = [g for g in dc.groups() if g not in dr.census_groups()]
    assert len(left_out) == 4 and all(dc.knob_set(g) == "default_only" for g in left_out)


@pytest.mark.parametrize("shape", dc.FIXED_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_fixed_batches(shape):
    """Both batches of a fixed shape meet their conditions; verify_reference's checksums equal the
    oracle's on them; the planted packets are all zero and give 0xFFFF."""
    stride, length, n, _ = shape
    for with_pseudo in (False, True):
        b = dr.fixed_batch(shape, with_pseudo)
        assert b.host.size == n * stride and b.n == n and (b.lens == length).all()
        dr.check_packets(b)
        assert np.array_equal(b.checksums, dr.oracle_checksums(b.host, b.offs, b.lens, dr.pseudo_of(b.flow_idx)))
        if with_pseudo:
            assert b.origin > 1 << 32 and b.flow_idx[0] == b.origin % dr.NF and list(b.flow_idx[3:5]) == [0, 1]
        else:
            zero = [i for i in range(n) if not b.host[b.offs[i]:b.offs[i] + length].any()]
            assert len(zero) == dr.PLANTED and (b.checksums[zero] == 0xFFFF).all()


def test_fixed_groups_map_to_shapes():
    for g in dr.census_groups():
        if g.startswith("fixed_"):
            shape, mode = dr.fixed_shape(g)
            assert dc.fixed_id(shape, mode) == g and mode in dc.FIXED_MODES


@pytest.mark.parametrize("layout", ["ragged", "packed_bytes"])
def test_zipf_batches(layout):
    """The ragged / 16-byte packed layout and the byte-packed one, on the generator twin's lengths."""
    lens = dr.twin_lengths()
    offs, size = (dr.ragged_layout if layout == "ragged" else dr.packed_bytes_layout)(lens)
    assert len(lens) == dc.N and lens.min() >= 64 and lens.max() <= 9000
    b = dr.packets_batch(size, offs, lens, dr.implicit_flows(dr.PACKED_ORIGIN, dc.N),
                         (2, int(layout == "packed_bytes")))
    dr.check_packets(b)
    assert np.array_equal(b.checksums, dr.oracle_checksums(b.host, b.offs, b.lens, dr.pseudo_of(b.flow_idx)))


def test_ragged_layout_is_the_generator_twins():
    _, offs, lens = dr.oracle().gen_ragged_batch(dr.workloads.CFG4.seed, 0, dc.N, dr.workloads.CFG4.hdr)
    assert np.array_equal(lens.astype(np.int64), dr.twin_lengths())
    assert np.array_equal(offs.astype(np.int64), dr.ragged_layout(dr.twin_lengths())[0])


def test_chains_batch():
    lens = dr.twin_lengths()
    offs, size = dr.ragged_layout(lens)
    b = dr.chains_batch(size, offs, lens, (3,))
    assert b.n == (dc.N + 2) // 3 and b.begin[-1] == dc.N and b.begin[-1] - b.begin[-2] == 1
    dr.check_chains(b)
    assert np.array_equal(b.checksums, dr.oracle_chain_checksums(b))


@pytest.mark.parametrize("stride", (0,) + dc.RING_STRIDES)
def test_rx_frames(stride):
    """Frames of the device generator's shape, packed (stride 0) and in ring slots: all verify
    as built (but a UDP checksum of 0x0000, sent as "none"), and the damaged batch meets the
    RX condition."""
    host, starts, lens = dr.twin_frames(dc.N, 31 if stride else 77, l4_len=stride - 300 if stride else 0,
                                        stride=stride)
    clean = np.array([R.verdict(host[s:s + n].tobytes()) for s, n in zip(starts, lens)])
    assert ((clean == R.VERIFIED) | (clean == R.UNCHECKED)).all() and (clean == R.UNCHECKED).sum() <= 4
    b = dr.frames_batch(host, starts, lens, (stride,))
    dr.check_rx(b)
    assert np.array_equal(b.lens, lens) and (b.host != host).sum() > dc.N // 8
    if stride:  # nothing outside the frames was touched
        rest = np.ones(host.size, dtype=bool)
        for s, n in zip(starts, lens):
            rest[s:s + n] = False
        assert not b.host[rest].any()


def test_tx_frames():
    host, starts, lens = dr.twin_frames(dc.N, 78, checksummed=False)
    b = dr.frames_batch(host, starts, lens, (78,), tx=True)
    dr.check_tx(b)
    assert set(b.done.tolist()) == {2, 3}
    # the filled frames verify, but for a UDP checksum that came out 0x0000
    v = np.array([R.verdict(b.filled[s:s + n].tobytes()) for s, n in zip(starts, lens)])
    assert ((v == R.VERIFIED) | (v == R.UNCHECKED)).all() and (v == R.VERIFIED).sum() > dc.N - 8
    total = int(lens.sum())
    assert np.array_equal(b.filled[total:], b.host[total:])


def test_mismatch_report():
    want = np.arange(20, dtype=np.uint16)
    got = want.copy()
    assert dr.mismatch("g", "k", "kern", got, want, np.full(20, 7)) is None
    got[3:13] += 1
    msg = dr.mismatch("grp", "loads=3", "k_x<1>", got, want, np.full(20, 7))
    assert msg.startswith("grp [loads=3] k_x<1>: 10 of 20 wrong; #3: got 0x4 want 0x3 len 7") and msg.count("#") == 8
    assert "reference" in dr.mismatch("g", "k", "kern", got.view(np.int16), want, np.full(20, 7))
