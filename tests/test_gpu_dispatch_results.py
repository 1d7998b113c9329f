"""GPU: what every launch of the dispatch table computes.  tests/test_gpu_dispatch.py
pins WHICH kernel instantiation each entry point launches under each tuning knob;
here the same launches -- every group of tests/dispatch_cases.py with the general
or the ring knob set, under every knob that computes results -- run on batches
with real contents (tests/dispatch_results.py) and each one is checked for:

    the return code and kernel name of tests/golden/dispatch.json, so that a result
    is credited to the instantiation that produced it;
    results equal to the reference, element for element, written into a view of a
    buffer poisoned with 0xA5 before every launch, the 256 guard bytes on each side
    intact and the device error word 0;
    tx_fill: the arena restored from a pristine copy before every knob, then the
    whole arena image and the done bytes equal to tests/tx_reference.py's.

Every argument that can steer the selection is the table's (Batches.launcher):
stride, length, n, the arena's misalignment, whether a pseudo-header is passed,
n_flows, the descriptors, lengths and tile indices of the device generators.  Only
the bytes, the flow table and the flow origin (non-zero here) differ.

Left out: the four default-only groups of 8M headers (the default launch at full
size is held to pip by the full-size parity tests), and the knobs that compute no
or wrong results by design (flags bits 21-23, a non-zero probes word), by their
fields.  tests/test_dispatch_results_cases.py counts what is left, 5,847 launches
reaching every kernel of the golden table but the probe kernels, and holds the
inputs and references to the CPU oracle.

What it found when it was written: k_packed under flags bit 4 (no packed-tile
addressing) summed the chunks of the previous tile that its line-aligned row grid
loads ahead of a tile's first packet, so that packet's result was wrong in every
tile not starting on a 128-byte line -- invisible on an all-zero arena."""
import json
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pip_amd import _lib, engine  # noqa: E402
from pip_amd.workloads import CFG4  # noqa: E402
from tests import dispatch_cases as dc  # noqa: E402
from tests import dispatch_results as dr  # noqa: E402
from tests.conftest import GOLDEN  # noqa: E402
from tests.test_gpu_verify import GUARD, POISON  # noqa: E402

DEV = "cuda"
_CACHE: dict = {}  # device inputs and their references, shared by the groups on one batch (never modified)


@pytest.fixture(scope="module")
def golden():
    return json.loads((GOLDEN / "dispatch.json").read_text())


@pytest.fixture(scope="module", autouse=True)
def gpu():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    engine.require_gpu()
    yield
    dc.reset_knobs()
    torch.cuda.synchronize()
    _CACHE.clear()


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _pseudo():
    """The device pseudo-header bases of dispatch_results.flows()."""
    return _cached("pseudo", lambda: engine.prepare_flows(4, engine.flows_to_device(4, dr.flows()[0]), dr.NF))


def _u16(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint16).astype(np.int64)


def _put(arena, host) -> None:
    assert arena.numel() == host.size
    arena.copy_(torch.from_numpy(host))


# ----------------------------------------------------------------------------
# the groups: device inputs as Batches.launcher passes them, contents and references of dispatch_results
# ----------------------------------------------------------------------------
def _fixed_inputs(shape, with_pseudo):
    stride, length, n, off = shape
    b = dr.fixed_batch(shape, with_pseudo)
    dr.check_packets(b)
    base = torch.full((off + n * stride + 4096,), POISON, dtype=torch.uint8, device=DEV)  # poison after the batch
    assert base.data_ptr() % 256 == 0
    arena = base[off:off + n * stride]
    _put(arena, b.host)
    return b, arena


def _desc_inputs():
    """gen_ragged's arena and descriptors, the bytes replaced; (batch, arena, desc)."""
    arena, desc, _ = engine.gen_ragged(dc.N, 0, CFG4.seed, CFG4.hdr, dr.NF)
    d = desc.cpu().numpy()
    b = dr.packets_batch(arena.numel(), d[:, 0], d[:, 1] & 0xFFFFFFFF, (d[:, 1] >> 32) & 0xFFFFFFFF, (2, 2))
    dr.check_packets(b)
    assert 0 <= int(b.flow_idx.min()) and int(b.flow_idx.max()) < dr.NF
    _put(arena, b.host)
    return b, arena, desc


def _packed_inputs(bytes_layout):
    """gen_packed's / gen_packed_bytes' arena, lengths and tile index, the bytes replaced."""
    gen, layout = (engine.gen_packed_bytes, dr.packed_bytes_layout) if bytes_layout else \
        (engine.gen_packed, dr.ragged_layout)
    arena, lens16, index, lengths = gen(dc.N, 0, CFG4.seed, CFG4.hdr)
    lens = lengths.cpu().numpy().astype(np.int64)
    assert np.array_equal(lens, _u16(lens16))
    offs, size = layout(lens)
    assert size <= arena.numel()
    b = dr.packets_batch(arena.numel(), offs, lens, dr.implicit_flows(dr.PACKED_ORIGIN, dc.N), (2, int(bytes_layout)))
    dr.check_packets(b)
    _put(arena, b.host)
    return b, arena, lens16, index


def _chains_inputs():
    arena, desc, _ = engine.gen_ragged(dc.N, 0, CFG4.seed, CFG4.hdr, dr.NF)
    d = desc.cpu().numpy()
    b = dr.chains_batch(arena.numel(), d[:, 0], d[:, 1] & 0xFFFFFFFF, (3,))
    dr.check_chains(b)
    _put(arena, b.host)
    begin = torch.from_numpy(b.begin).to(DEV)
    assert begin.tolist() == list(range(0, dc.N, 3)) + [dc.N]
    return b, arena, desc, begin, torch.zeros(b.n, dtype=torch.int32, device=DEV)


def _frames_inputs(group):
    """The generators' frames (the table's seeds), damaged on the host and uploaded."""
    if group.startswith("rx_verify_ring"):
        stride = int(group[group.index("[") + 1:-1])
        arena, lens16, _ = engine.gen_rx_ring(dc.N, 31, stride, l4_len=stride - 300)
        lens = _u16(lens16)
        starts, index = np.arange(dc.N, dtype=np.int64) * stride, None
    else:
        stride = 0
        arena, lens16, index = engine.gen_rx_frames(dc.N, 78 if group == "tx_fill" else 77,
                                                    checksummed=group != "tx_fill")[:3]
        lens = _u16(lens16)
        starts = np.cumsum(lens) - lens
    b = dr.frames_batch(arena.cpu().numpy(), starts, lens, (stride, int(group == "tx_fill")), tx=group == "tx_fill")
    (dr.check_tx if group == "tx_fill" else dr.check_rx)(b)
    _put(arena, b.host)
    return b, arena, lens16, index, stride


def _case(group) -> SimpleNamespace:
    """launch(res, err): the group's one call, its result in `res` (a uint8 view of 2 * n bytes
    for checksums, of n for verdicts and done bytes); want: the reference; lens: for the report;
    arena / pristine / image: tx_fill's arena, what it is restored from and what it must become."""
    e, c = engine, SimpleNamespace(arena=None)
    if group.startswith("fixed_"):
        shape, mode = dr.fixed_shape(group)
        stride, length, n, _ = shape
        with_pseudo = mode.endswith("_pseudo")
        b, arena = _cached(("fixed", shape, with_pseudo), lambda: _fixed_inputs(shape, with_pseudo))
        pseudo, nf = (_pseudo(), dr.NF) if with_pseudo else (None, None)
        if mode.startswith("verify"):
            c.launch = lambda res, err: e.verify_fixed(arena, stride, length, n, pseudo, nf, None, b.origin, ok=res,
                                                       err=err)
        else:
            c.launch = lambda res, err: e.checksum_fixed(arena, stride, length, n, pseudo, nf, None, b.origin,
                                                         out=res.view(torch.int16), err=err)
        c.want, c.lens = (b.verdicts if mode.startswith("verify") else b.checksums), b.lens
    elif group.startswith("ragged_"):
        b, arena, desc = _cached("ragged", _desc_inputs)
        if group.endswith("verify"):
            c.launch = lambda res, err: e.verify_ragged(arena, desc, _pseudo(), ok=res, err=err)
        else:
            c.launch = lambda res, err: e.checksum_ragged(arena, desc, _pseudo(), out=res.view(torch.int16), err=err)
        c.want, c.lens = (b.verdicts if group.endswith("verify") else b.checksums), b.lens
    elif group.startswith("packed_"):
        by = group.startswith("packed_bytes_")
        b, arena, lens16, index = _cached(("packed", by), lambda: _packed_inputs(by))
        if group.endswith("verify"):
            f = e.verify_packed_bytes if by else e.verify_packed
            c.launch = lambda res, err: f(arena, lens16, index, dc.N, _pseudo(), dr.NF, None, dr.PACKED_ORIGIN, ok=res,
                                          err=err)
        else:
            f = e.checksum_packed_bytes if by else e.checksum_packed
            c.launch = lambda res, err: f(arena, lens16, index, dc.N, _pseudo(), dr.NF, None, dr.PACKED_ORIGIN,
                                          out=res.view(torch.int16), err=err)
        c.want, c.lens = (b.verdicts if group.endswith("verify") else b.checksums), b.lens
    elif group == "chains":
        b, arena, desc, begin, flow = _cached("chains", _chains_inputs)
        c.launch = lambda res, err: e.checksum_chains(arena, desc, begin, flow, _pseudo(), out=res.view(torch.int16),
                                                      err=err)
        c.want, c.lens = b.checksums, b.total_lens
    else:
        b, arena, lens16, index, stride = _cached(group, lambda: _frames_inputs(group))
        if group == "rx_verify_device":
            c.launch = lambda res, err: e.rx_verify_device(arena, lens16, index, dc.N, ok=res, err=err)
        elif group == "tx_fill":
            c.launch = lambda res, err: e.tx_fill_device(arena, lens16, index, dc.N, done=res, err=err)
            c.arena, c.pristine, c.image = arena, torch.from_numpy(b.host).to(DEV), b.filled
        else:
            assert group.startswith("rx_verify_ring")
            c.launch = lambda res, err: e.rx_verify_ring(arena, stride, lens16, dc.N, ok=res, err=err)
        c.want, c.lens, c.starts = (b.done if group == "tx_fill" else b.verdicts), b.lens, b.starts
    return c


def _image_mismatch(group, knob, kernel, got, c):
    """tx_fill's arena against the reference's: None, or the frames that differ."""
    bad_bytes = np.nonzero(got != c.image)[0]
    if not bad_bytes.size:
        return None
    frames = np.unique(np.searchsorted(c.starts, bad_bytes, side="right") - 1)
    inside = bad_bytes < c.starts[-1] + c.lens[-1]

    def at(i):
        return [int(k - c.starts[i]) for k in bad_bytes if c.starts[i] <= k < c.starts[i] + c.lens[i]][:4]

    first = ", ".join(f"#{i}: len {int(c.lens[i])} bytes at {at(i)}" for i in map(int, frames[:8]))
    return (f"{group} [{knob}] {kernel}: arena differs in {frames.size} of {len(c.lens)} frames"
            f"{'' if inside.all() else ' and after the last frame'}; {first}")


@pytest.mark.parametrize("group", dr.census_groups())
def test_launch_results_equal_reference(golden, group):
    want_launch = dc.decode(golden, group)
    knobs = dr.checked_knobs(group)
    assert knobs and set(knobs) <= set(want_launch)
    c = _case(group)  # (asserts the conditions on the inputs before anything is launched on them)
    size = c.want.size * c.want.dtype.itemsize
    buf = torch.empty(GUARD + size + GUARD, dtype=torch.uint8, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    wrong = []
    xw = False
    try:
        for name, k in knobs.items():
            buf.fill_(POISON)
            err.zero_()
            if c.arena is not None:
                c.arena.copy_(c.pristine)
            xw = dc.apply_knob(k, xw)
            try:
                c.launch(buf[GUARD:GUARD + size], err)
                launched = [0, dc.last_kernel()]
            except _lib.PipckError as ex:
                launched = [ex.rc, None]
            if launched != want_launch[name]:
                if launched[1] is None:  # a call that failed: nothing more is launched, by this test or a later one
                    pytest.exit(f"{group} [{name}]: the call returned {launched[0]}, the table has "
                                f"{want_launch[name]}", 3)
                wrong.append(f"{group} [{name}]: launched {launched}, the table has {want_launch[name]}")
                continue
            kernel = launched[1]
            got = buf.cpu().numpy()
            msg = dr.mismatch(group, name, kernel, got[GUARD:GUARD + size].view(c.want.dtype), c.want, c.lens)
            if msg is None and c.arena is not None:
                msg = _image_mismatch(group, name, kernel, c.arena.cpu().numpy(), c)
            if msg is None and not ((got[:GUARD] == POISON).all() and (got[GUARD + size:] == POISON).all()):
                msg = f"{group} [{name}] {kernel}: guard bytes around the results were written"
            if msg is None and int(err.item()) != 0:
                msg = f"{group} [{name}] {kernel}: error word {int(err.item()):#x}"
            if msg:
                wrong.append(msg)
    finally:
        dc.reset_knobs()
    assert not wrong, f"{len(wrong)} of {len(knobs)} launches: " + "\n".join(wrong[:12])
