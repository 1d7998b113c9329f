"""CPU: what tests/test_gpu_streams.py rests on (tests/stream_cases.py).

Second contents: for every group replayed with contents B, B lies on A's layout,
meets the condition A meets (tests/dispatch_results.py's check_*), and its
reference differs from A's in at least 5 % of the elements (tx_fill: the filled
image in at least 5 % of the frames) -- from the references alone, on the
oracle's twin layouts, built by the function the GPU test builds them with.  The
default variant draws the bytes the builders have always drawn
(tests/test_dispatch_results_cases.py and tests/golden/dispatch.json stay as
they are).  The ring frame sets: two different sets of 500 frames, each with at
least 100 frames that verify and 100 that do not, and the forwarding graph's
composed reference does work at every step."""
import json

import numpy as np
import pytest

from tests import dispatch_cases as dc
from tests import dispatch_results as dr
from tests import fwd_reference as F
from tests import rx_reference as R
from tests import stream_cases as sc
from tests.conftest import GOLDEN


@pytest.fixture(scope="module")
def golden():
    return json.loads((GOLDEN / "dispatch.json").read_text())


def test_second_groups_reach_every_default_kernel(golden):
    groups = sc.second_groups(golden)
    assert set(groups) <= set(dr.census_groups()) and len(set(groups)) == len(groups)
    assert {g for g in dr.census_groups() if not g.startswith("fixed_")} <= set(groups)
    assert {sc.default_kernel(golden, g) for g in groups} == {sc.default_kernel(golden, g) for g in dr.census_groups()}
    fixed = [sc.default_kernel(golden, g) for g in groups if g.startswith("fixed_")]
    assert len(fixed) == len(set(fixed)) >= 3  # k_hdr, k_flat_coop and k_flat at the least
    print(f"{len(groups)} of {len(dr.census_groups())} groups replay contents B, {len(fixed)} of them fixed")


def _first(group):
    """Contents A of a group on the CPU: the fixed batch, or the oracle's twin layout."""
    if group.startswith("fixed_"):
        shape, mode = dr.fixed_shape(group)
        return dr.fixed_batch(shape, mode.endswith("_pseudo"))
    lens = dr.twin_lengths()
    if group.startswith("ragged_"):
        offs, size = dr.ragged_layout(lens)
        flows = np.arange(dc.N, dtype=np.int64) % dr.NF
        return dr.packets_batch(size, offs, lens, flows, (2, 2))
    if group.startswith("packed_"):
        by = group.startswith("packed_bytes_")
        offs, size = (dr.packed_bytes_layout if by else dr.ragged_layout)(lens)
        return dr.packets_batch(size, offs, lens, dr.implicit_flows(dr.PACKED_ORIGIN, dc.N), (2, int(by)))
    if group == "chains":
        offs, size = dr.ragged_layout(lens)
        return dr.chains_batch(size, offs, lens, (3,))
    if group == "tx_fill":
        return dr.frames_batch(*dr.twin_frames(dc.N, 78, checksummed=False), (0, 1), tx=True)
    stride = int(group[group.index("[") + 1:-1]) if group.startswith("rx_verify_ring") else 0
    host, starts, lens = dr.twin_frames(dc.N, 31 if stride else 77, l4_len=stride - 300 if stride else 0, stride=stride)
    return dr.frames_batch(host, starts, lens, (stride, 0))


def _batch_keys(golden):
    """One group per batch: the verify and the checksum group of a shape share theirs, and both
    references are compared."""
    seen, out = set(), []
    for g in sc.second_groups(golden):
        key = g
        if g.startswith("fixed_"):
            shape, mode = dr.fixed_shape(g)
            key = ("fixed", shape, mode.endswith("_pseudo"), sc.is_verify(g))
        if key not in seen:
            seen.add(key)
            out.append(g)
    return out


def test_second_contents(golden):
    """B of every replayed group: A's layout, A's condition, and a reference that differs from A's
    in at least 5 % of its elements."""
    shares = {}
    for g in _batch_keys(golden):
        a = _first(g)
        b = sc.second(g, a)
        assert sc.same_layout(g, a, b), g
        sc.check(g, a)
        sc.check(g, b)
        assert (a.host != b.host).any(), g
        shares[g] = sc.different(g, a, b)
        assert sc.want(g, a).dtype == sc.want(g, b).dtype and sc.want(g, a).shape == sc.want(g, b).shape
    print({g: round(s, 3) for g, s in shares.items()})
    low = {g: s for g, s in shares.items() if s < sc.MIN_DIFFERENT}
    assert not low, low


def test_default_variant_is_unchanged():
    """variant 0 is the builders' old key and verify_sealing.damage itself."""
    assert dr.variant_key(11, (1, 2), 0) == [11, 1, 2] and dr.variant_key(14, (3,), 1) == [14, 3, 1]
    shape = dc.FIXED_SHAPES[0]
    assert dr.fixed_batch(shape, True, 0).host.tobytes() == dr.fixed_batch(shape, True).host.tobytes()
    from tests import verify_sealing as vs

    offs, lens = np.arange(96) * 40, np.full(96, 40)  # (a multiple of 8: the shift wraps onto the same classes)
    x, y, z = (np.arange(3840, dtype=np.uint32).astype(np.uint8) for _ in range(3))
    vs.damage(x, offs, lens, np.random.default_rng(5))
    dr.damage(y, offs, lens, np.random.default_rng(5))
    dr.damage(z, offs, lens, np.random.default_rng(5), 1)
    assert np.array_equal(x, y)
    touched = {int(i) % 8 for i in np.unique(np.nonzero(x != z)[0] // 40)}
    assert {0, 2, 5, 7} <= touched <= {0, 1, 2, 5, 6, 7}  # classes 0-2 of variant 0, 5-7 of variant 1


def test_ring_frame_sets():
    a, b = sc.ring_frames("A"), sc.ring_frames("B")
    for frames in (a, b):
        sc.check_ring_frames(frames)
    assert len(a) == len(b) and sum(x != y for x, y in zip(a, b)) >= len(a) * 9 // 10
    va, vb = (np.array([R.verdict(f) for f in s]) for s in (a, b))
    assert np.mean(va != vb) >= sc.MIN_DIFFERENT


@pytest.mark.parametrize("which", ["A", "B"])
def test_forward_reference_does_work_at_every_step(which):
    r = sc.forward_reference(which)
    n = len(r.frames)
    assert (r.done[r.ok != R.VERIFIED] == 0).all()
    assert all(x == y for x, y, k in zip(r.frames, r.rewritten, r.ok) if k != R.VERIFIED)
    assert int((r.done == F.DONE).sum()) >= 100
    assert sum(x != y for x, y in zip(r.frames, r.rewritten)) >= 100
    # a rewritten frame that verified still verifies: ok2 is the first verdict wherever the slot was DONE
    assert np.array_equal(r.ok2[r.done == F.DONE], r.ok[r.done == F.DONE])
    assert sum(x != y for x, y in zip(r.rewritten, r.filled)) >= 50 and len(r.tx_done) == n


@pytest.mark.parametrize("stride", [1024, 9216])
def test_aligned_frames(stride):
    frames = sc.aligned_frames(stride)
    assert len(frames) == sc.ALIGN_N and max(map(len, frames)) <= stride
    # the longest frames that fit: over 256 bytes (more than 16 chunks) at 1,024, over 1,024 at 9,216
    assert max(map(len, frames)) > (256 if stride == 1024 else 1024)
    v = np.array([R.verdict(f) for f in frames])
    assert int((v == R.VERIFIED).sum()) >= 20 and int((v != R.VERIFIED).sum()) >= 20


def test_calls_outside_the_census_have_two_contents():
    """The prepared-table and the update cases: A and B differ in (nearly) every expected element,
    and the update changes every packet."""
    for family in (4, 6):
        a, b = sc.prepare_case(family, 0), sc.prepare_case(family, 1)
        assert a.records.size == b.records.size and (a.records != b.records).any()
        assert np.mean(a.checksums != b.checksums) >= 0.9
    for with_pseudo in (False, True):
        a, b = sc.update_case(with_pseudo, 0), sc.update_case(with_pseudo, 1)
        assert a.before.size == a.n * a.stride and np.mean(a.after != b.after) >= 0.9
        rows = (a.before != a.after).reshape(a.n, a.stride)
        assert rows[:, :a.length].any(axis=1).sum() >= a.n - 2 and not rows[:, a.length:].any()
    from tests.test_tx_ring_cases import reference_fill

    for which in "AB":  # the ring frame sets give pipck_tx_fill_ring work to do
        frames = sc.ring_frames(which)
        assert sum(x != y for x, y in zip(frames, reference_fill(frames, 0)[0])) >= 50
