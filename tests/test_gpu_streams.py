"""GPU: the context the device calls run in.  The kernels are held to their
references at every shape and knob elsewhere; here the same calls run where a
forwarder runs them -- on a side stream behind queued work, as a captured and
replayed graph, on rings at every 16-byte phase with result pointers at odd
bytes, with an error word that already holds a bit, and from four host threads
at once -- and every result is held to the same references
(tests/dispatch_results.py, tests/stream_cases.py, rx / tx / fwd_reference).

1. Side stream.  The inputs' device buffers and the result buffer hold poison,
   err holds ERR0.  On a fresh torch.cuda.Stream (non-blocking: the null stream
   does not order with it) a delay kernel is queued, then the copies that put
   the real inputs in place, then the call.  When the call (or the last call of
   a chain) returns, an event recorded right behind the delay must not have
   completed -- so nothing in the call or between the calls of a chain waited
   for the stream -- and stream.query() must be False.  After the stream is
   drained the results equal the reference, the guards are intact and err is
   ERR0 exactly.  Work sent to any other stream runs before its inputs exist:
   it reads poison, or its results are never rewritten.  Only contents are
   poisoned; descriptors, lengths and indices that steer addresses stay in
   place (but where a call computes an index, its lengths are poisoned).
   Every call is warmed once on the null stream first: the code objects are
   loaded and engine._check_packed has cached the index's total.  That cache is
   keyed on the index tensor's version counter, so an index that a case
   poisons is poisoned through a tensor with a counter of its own.
   The delay is DELAY_MS = 50 ms of torch.cuda._sleep, calibrated once with two
   events; a delay too short fails the assertions, it cannot pass.

2. Graphs.  One torch.cuda.graph per case, a linear chain on the capturing
   stream (no fork or join), warmed on a side stream first.  Replayed with
   contents A, B, A: before each replay the inputs are copied in place, the
   result buffer re-poisoned and err set to ERR0, on the replaying stream.

3. Rings at allocation + 16, + 48, + 112; u8 results at + 1 and + 3, u16 at + 2.

4. err preset to ERR0: a refusing call leaves ERR0 | 1 << code, a clean one ERR0.

5. Four host threads with a stream each; two streams on one jumbo ring.

6. engine._check_packed reads no index total while a stream is being captured."""
import json
import threading
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pip_amd import _lib, engine  # noqa: E402
from pip_amd.workloads import CFG4  # noqa: E402
from tests import dispatch_cases as dc  # noqa: E402
from tests import dispatch_results as dr  # noqa: E402
from tests import fwd_reference as F  # noqa: E402
from tests import rx_reference as R  # noqa: E402
from tests import stream_cases as sc  # noqa: E402
from tests import test_gpu_dispatch_results as tgd  # noqa: E402
from tests.conftest import GOLDEN  # noqa: E402
from tests.test_fwd_reference import assign, reference_rewrite, rule_table  # noqa: E402
from tests.test_gpu_tx_fill_ring import GUARD as RING_GUARD  # noqa: E402
from tests.test_gpu_tx_fill_ring import POISON as DONE_POISON  # noqa: E402
from tests.test_gpu_tx_fill_ring import _check  # noqa: E402
from tests.test_gpu_verify import GUARD, POISON  # noqa: E402
from tests.test_tx_ring_cases import reference_fill, ring_image, ring_lens  # noqa: E402

DEV = "cuda"
ERR0 = 0x40000000
ERANGE_BIT, EINVAL_BIT = 1 << _lib.PIPCK_ERANGE, 1 << _lib.PIPCK_EINVAL
DELAY_MS = 50
N = dc.N
_STAGE: dict = {}  # device copies of host contents, shared by the tests (never modified)
_CYCLES: list = []


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
    _STAGE.clear()
    tgd._CACHE.clear()


def _delay() -> None:
    """DELAY_MS of busy GPU on the current stream (torch.cuda._sleep, calibrated once with two events)."""
    if not _CYCLES:
        torch.cuda._sleep(1_000_000)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        torch.cuda._sleep(10_000_000)
        end.record()
        end.synchronize()
        _CYCLES.append(10_000_000 / start.elapsed_time(end))
    torch.cuda._sleep(int(DELAY_MS * _CYCLES[0]))


def _dev(key, host) -> "torch.Tensor":
    """The device copy of a host array, made once."""
    if key not in _STAGE:
        _STAGE[key] = torch.from_numpy(np.array(host, copy=True)).to(DEV)
    return _STAGE[key]


def _err() -> "torch.Tensor":
    return torch.zeros(1, dtype=torch.int32, device=DEV)


def _guarded(nbytes: int, lead: int = GUARD):
    """(buffer, the result view of nbytes at `lead`): GUARD bytes behind the view."""
    buf = torch.empty(lead + nbytes + GUARD, dtype=torch.uint8, device=DEV)
    return buf, buf[lead:lead + nbytes]


def _held(name, buf, want, lens=None, kernel="", lead: int = GUARD, poison: int = POISON) -> None:
    """The result view equals `want` element for element and the bytes around it are poison."""
    got = buf.cpu().numpy()
    size = want.size * want.dtype.itemsize
    body = np.frombuffer(got[lead:lead + size].tobytes(), dtype=want.dtype)
    msg = dr.mismatch(name, "default", kernel, body, want, np.zeros(want.size) if lens is None else lens)
    assert msg is None, msg
    assert (got[:lead] == poison).all() and (got[lead + size:] == poison).all(), \
        f"{name} {kernel}: guard bytes around the results were written"


def _image(name, arena, want) -> None:
    got = arena.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert not bad.size, f"{name}: {bad.size} bytes of the arena differ from the reference image, first at {bad[:8]}"


def _word(err) -> int:
    return int(err.item()) & 0xFFFFFFFF


# ----------------------------------------------------------------------------
# cases: inputs (device tensor, {content: staged copy}), poisoned result buffers, call(), check(content)
# ----------------------------------------------------------------------------
def _cache_key(group):
    if group.startswith("fixed_"):
        shape, mode = dr.fixed_shape(group)
        return ("fixed", shape, mode.endswith("_pseudo"))
    if group.startswith("ragged_"):
        return "ragged"
    if group.startswith("packed_"):
        return ("packed", group.startswith("packed_bytes_"))
    return group


def _census_case(group, second: bool = False) -> SimpleNamespace:
    """The group's default launch of tests/test_gpu_dispatch_results.py, its arena as an input."""
    c = tgd._case(group)
    key = _cache_key(group)
    a, arena = tgd._CACHE[key][:2]
    batches = {"A": a}
    if second:
        batches["B"] = sc.second(group, a)
        sc.check(group, batches["B"])
        assert sc.same_layout(group, a, batches["B"]) and sc.different(group, a, batches["B"]) >= sc.MIN_DIFFERENT
    assert sc.want(group, a) is c.want
    stage = {k: _dev((key, k), b.host) for k, b in batches.items()}
    buf, res = _guarded(c.want.size * c.want.dtype.itemsize)
    err = _err()

    def check(content, kernel=""):
        b = batches[content]
        _held(group, buf, sc.want(group, b), c.lens, kernel)
        if group == "tx_fill":
            _image(group, arena, b.filled)

    return SimpleNamespace(name=group, inputs=[(arena, stage)], bufs=[(buf, POISON)], err=err,
                           call=lambda: c.launch(res, err), check=check, contents=tuple(batches))


def _prepare_case(family: int) -> SimpleNamespace:
    """pipck_flows4/6_prepare into a poisoned table, then a fixed checksum that uses the table."""
    cases = {k: sc.prepare_case(family, v) for k, v in (("A", 0), ("B", 1))}
    a = cases["A"]
    flows = torch.empty(a.records.size, dtype=torch.uint8, device=DEV)
    arena = torch.empty(a.host.size, dtype=torch.uint8, device=DEV)
    tbuf, table = _guarded(4 * dr.NF)
    buf, res = _guarded(2 * a.n)
    err = _err()
    pseudo = table.view(torch.int32)
    fn = f"pipck_flows{family}_prepare"

    def call():
        _lib.call(fn, engine._ptr(flows), dr.NF, engine._ptr(pseudo), engine.current_stream())
        engine.checksum_fixed(arena, a.stride, a.length, a.n, pseudo, dr.NF, None, a.origin, out=res.view(torch.int16),
                              err=err)

    def check(content, kernel=""):
        _held(fn, buf, cases[content].checksums, a.lens, kernel)
        got = tbuf.cpu().numpy()
        assert (got[:GUARD] == POISON).all() and (got[GUARD + 4 * dr.NF:] == POISON).all(), f"{fn}: guards written"

    return SimpleNamespace(name=fn, inputs=[(flows, {k: _dev((fn, k, "f"), c.records) for k, c in cases.items()}),
                                            (arena, {k: _dev((fn, k, "a"), c.host) for k, c in cases.items()})],
                           bufs=[(tbuf, POISON), (buf, POISON)], err=err, call=call, check=check, contents=("A", "B"))


def _index_case(bytes_layout: bool) -> SimpleNamespace:
    """pipck_packed_index / pipck_packed_bytes_index from poisoned-then-restored lengths into a
    poisoned index, then the packed checksum call on the fresh index."""
    group = "packed_bytes_checksum" if bytes_layout else "packed_checksum"
    tgd._case(group)
    a, arena, lens16, index = tgd._CACHE[("packed", bytes_layout)]
    batches = {"A": a, "B": sc.second(group, a)}
    want_index = index.cpu().numpy()
    tiles = want_index.size
    ibuf, iview = _guarded(8 * tiles)
    # ONE tensor object with a version counter of its own (a .data alias): engine._check_packed caches on
    # the object and its version, and poisoning ibuf must not make the side-stream call read the total again
    fresh = ibuf.data[GUARD:GUARD + 8 * tiles].view(torch.int64)
    assert fresh.data_ptr() == iview.data_ptr()
    buf, res = _guarded(2 * N)
    err = _err()
    f = engine.checksum_packed_bytes if bytes_layout else engine.checksum_packed
    make = engine.packed_bytes_index if bytes_layout else engine.packed_index
    fn = "pipck_packed_bytes_index" if bytes_layout else "pipck_packed_index"
    assert make(lens16, N).cpu().numpy().tolist() == want_index.tolist()

    def call():
        _lib.call(fn, engine._ptr(lens16), N, engine._ptr(fresh), engine.current_stream(lens16.device))
        f(arena, lens16, fresh, N, tgd._pseudo(), dr.NF, None, dr.PACKED_ORIGIN, out=res.view(torch.int16), err=err)

    def check(content, kernel=""):
        _held(fn + " (the index)", ibuf, want_index, None, kernel)
        _held(fn + " then " + group, buf, batches[content].checksums, a.lens, kernel)

    key = ("packed", bytes_layout)
    lens_stage = _dev((key, "lens"), lens16.cpu().numpy())
    return SimpleNamespace(name=fn, inputs=[(arena, {k: _dev((key, k), b.host) for k, b in batches.items()}),
                                            (lens16, {"A": lens_stage, "B": lens_stage})],
                           bufs=[(ibuf, POISON), (buf, POISON)], err=err, call=call, check=check, contents=("A", "B"))


def _update_case(with_pseudo: bool) -> SimpleNamespace:
    """pipck_update_fixed_n in place, with and without the two pseudo tables."""
    cases = {k: sc.update_case(with_pseudo, v) for k, v in (("A", 0), ("B", 1))}
    a = cases["A"]
    name = "pipck_update_fixed_n" + (" (pseudo tables)" if with_pseudo else "")
    arena = torch.empty(a.before.size, dtype=torch.uint8, device=DEV)
    new = torch.empty(a.new.size, dtype=torch.uint8, device=DEV)
    old_t = new_t = None
    if with_pseudo:
        old_t, new_t = (engine.prepare_flows(4, _dev(("flows4", k), np.frombuffer(sc.flow_tables(4, k)[0], dtype=np.uint8)),
                                             dr.NF) for k in (0, 1))
    err = _err()

    def call():
        engine.update_fixed(arena, a.stride, a.n, 0, a.length, a.ck_off, a.edit_off, a.edit_len, new, a.edit_len, old_t,
                            new_t, dr.NF if with_pseudo else None, None, a.origin, err=err)

    return SimpleNamespace(name=name, inputs=[(arena, {k: _dev((name, k, "a"), c.before) for k, c in cases.items()}),
                                              (new, {k: _dev((name, k, "n"), c.new) for k, c in cases.items()})],
                           bufs=[], err=err, call=call, contents=("A", "B"),
                           check=lambda content, kernel="": _image(name, arena, cases[content].after))


def _ring_case(which: str, stride: int = 4096) -> SimpleNamespace:
    """pipck_tx_fill_ring ("tx") or pipck_fwd_rewrite_ring with DEC_TTL among the rules ("fwd") on
    the ring frame sets A and B (other frames and other lengths) in slots of `stride`."""
    sets = {k: list(sc.ring_frames(k)) for k in "AB"}
    n = len(sets["A"])
    ring = torch.empty(n * stride + RING_GUARD, dtype=torch.uint8, device=DEV)
    lens = torch.empty(n, dtype=torch.int16, device=DEV)
    done = torch.empty(n + 32, dtype=torch.uint8, device=DEV)
    err = _err()
    name = {"tx": "pipck_tx_fill_ring", "fwd": "pipck_fwd_rewrite_ring"}[which]
    inputs = [(ring, {k: _dev(("ring", stride, k), ring_image(f, stride, RING_GUARD)) for k, f in sets.items()}),
              (lens, {k: _dev(("ring lens", k), ring_lens(f)) for k, f in sets.items()})]
    if which == "tx":
        want = {k: reference_fill(f, 0) for k, f in sets.items()}
        call = lambda: engine.tx_fill_ring(ring, stride, lens, n, done=done[16:n + 16], err=err)  # noqa: E731
    else:
        rules = engine.make_fwd_rules(list(rule_table()))
        assert any(r["ops"] & F.DEC_TTL for r in rule_table())
        rule_of = torch.empty(n, dtype=torch.int32, device=DEV)
        inputs.append((rule_of, {k: _dev(("rule_of", k), assign(f).view(np.int32)) for k, f in sets.items()}))
        want = {k: reference_rewrite(f, assign(f), F.UDP_ZERO_AS_ONES) for k, f in sets.items()}
        assert all((d == F.DONE).sum() >= 50 for _, d in want.values())
        call = lambda: engine.fwd_rewrite_ring(ring, stride, lens, rules, rule_of, n, flags=F.UDP_ZERO_AS_ONES,  # noqa: E731
                                               done=done[16:n + 16], err=err)

    def check(content, kernel=""):
        frames, want_done = want[content]
        _check(f"{name} (frame set {content}) {kernel}", sets[content], stride, ring.cpu().numpy(), done.cpu().numpy(),
               ring_image(frames, stride, RING_GUARD), want_done)

    return SimpleNamespace(name=name, inputs=inputs, bufs=[(done, DONE_POISON)], err=err, call=call, check=check,
                           contents=("A", "B"))


def _index_rx_tx_case() -> SimpleNamespace:
    """packed_bytes_index -> rx_verify_device -> tx_fill_device on ONE arena (tx_fill's frames):
    the verdicts are those of the unfilled frames, then the arena holds the filled image."""
    tgd._case("tx_fill")
    a, arena, lens16, index, _ = tgd._CACHE["tx_fill"]
    frames = [a.host[int(s):int(s) + int(k)].tobytes() for s, k in zip(a.starts, a.lens)]
    verdicts = np.array([R.verdict(f) for f in frames], dtype=np.uint8)
    want_index = index.cpu().numpy()
    ibuf, iview = _guarded(8 * want_index.size)
    fresh = ibuf.data[GUARD:GUARD + 8 * want_index.size].view(torch.int64)  # (its own version counter, as _index_case)
    assert fresh.data_ptr() == iview.data_ptr()
    okbuf, ok = _guarded(N)
    dbuf, done = _guarded(N)
    err = _err()

    def call():
        _lib.call("pipck_packed_bytes_index", engine._ptr(lens16), N, engine._ptr(fresh), engine.current_stream())
        engine.rx_verify_device(arena, lens16, fresh, N, ok=ok, err=err)
        engine.tx_fill_device(arena, lens16, fresh, N, done=done, err=err)

    def check(content, kernel=""):
        _held("index -> rx -> tx (the index)", ibuf, want_index)
        _held("index -> rx -> tx (verdicts)", okbuf, verdicts, a.lens)
        _held("index -> rx -> tx (done)", dbuf, a.done, a.lens)
        _image("index -> rx -> tx", arena, a.filled)

    return SimpleNamespace(name="index -> rx_verify_device -> tx_fill_device",
                           inputs=[(arena, {"A": _dev(("tx_fill", "A"), a.host)})],
                           bufs=[(ibuf, POISON), (okbuf, POISON), (dbuf, POISON)], err=err, call=call, check=check,
                           contents=("A",))


def _chains_twice_case() -> SimpleNamespace:
    """checksum_chains (two kernels and a scratch buffer) queued twice back to back into two result buffers."""
    c = tgd._case("chains")
    a, arena = tgd._CACHE["chains"][:2]
    (b1, r1), (b2, r2) = _guarded(2 * a.n), _guarded(2 * a.n)
    err = _err()

    def call():
        c.launch(r1, err)
        c.launch(r2, err)

    def check(content, kernel=""):
        _held("chains (first call)", b1, a.checksums, a.total_lens)
        _held("chains (second call)", b2, a.checksums, a.total_lens)

    return SimpleNamespace(name="chains twice", inputs=[(arena, {"A": _dev(("chains", "A"), a.host)})],
                           bufs=[(b1, POISON), (b2, POISON)], err=err, call=call, check=check, contents=("A",))


EXTRA = {"flows4_prepare": lambda: _prepare_case(4), "flows6_prepare": lambda: _prepare_case(6),
         "packed_index": lambda: _index_case(False), "packed_bytes_index": lambda: _index_case(True),
         "update_fixed_n": lambda: _update_case(False), "update_fixed_n_pseudo": lambda: _update_case(True),
         "tx_fill_ring": lambda: _ring_case("tx"), "fwd_rewrite_ring": lambda: _ring_case("fwd")}
CHAINED = {"index_rx_tx": _index_rx_tx_case, "chains_twice": _chains_twice_case}


def _default_knob(group) -> None:
    dc.apply_knob(dc.knobs_of(group)["default"], False)  # (ring groups: the table's default has the feedback off)


# ----------------------------------------------------------------------------
# 1. a side stream, behind a delay, with no host synchronisation
# ----------------------------------------------------------------------------
def _on_a_side_stream(case, content="A") -> None:
    for dst, stage in case.inputs:  # warm on the null stream
        dst.copy_(stage[content])
    case.call()
    torch.cuda.synchronize()
    for dst, _ in case.inputs:
        dst.fill_(POISON)
    for buf, poison in case.bufs:
        buf.fill_(poison)
    case.err.fill_(ERR0)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        _delay()
        delay_done = torch.cuda.Event()
        delay_done.record()
        for dst, stage in case.inputs:
            dst.copy_(stage[content])
        case.call()
        delayed, busy = not delay_done.query(), not s.query()
    s.synchronize()
    assert delayed, (f"{case.name}: the delay had ended when the call returned -- the call, or a call of the chain, "
                     f"synchronised the host, or {DELAY_MS} ms of delay ran out")
    assert busy, f"{case.name}: the stream was idle when the call returned"
    case.check(content)
    assert _word(case.err) == ERR0, f"{case.name}: error word {_word(case.err):#x}"


@pytest.mark.parametrize("group", dr.census_groups())
def test_side_stream_census(group):
    try:
        _default_knob(group)
        _on_a_side_stream(_census_case(group))
    finally:
        dc.reset_knobs()


@pytest.mark.parametrize("name", list(EXTRA) + list(CHAINED))
def test_side_stream_other_calls(name):
    _on_a_side_stream({**EXTRA, **CHAINED}[name]())


# ----------------------------------------------------------------------------
# 2. graph capture and replay
# ----------------------------------------------------------------------------
def _captured(case, order=("A", "B", "A"), kernel=None) -> None:
    first = order[0]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # the warm-up torch asks for, on a side stream
        for dst, stage in case.inputs:
            dst.copy_(stage[first])
        case.call()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        case.call()
    launched = dc.last_kernel()
    if kernel is not None:
        assert launched == kernel, f"{case.name}: captured {launched}, the table's default is {kernel}"
    for k, content in enumerate(order):
        for dst, stage in case.inputs:
            dst.copy_(stage[content])
        for buf, poison in case.bufs:
            buf.fill_(poison)
        case.err.fill_(ERR0)
        g.replay()
        torch.cuda.synchronize()
        case.check(content, launched)
        assert _word(case.err) == ERR0, f"{case.name} (replay {k}, contents {content}): error word {_word(case.err):#x}"


@pytest.mark.parametrize("group", dr.census_groups())
def test_graph_census(golden, group):
    second = group in sc.second_groups(golden)
    try:
        _default_knob(group)
        _captured(_census_case(group, second), ("A", "B", "A") if second else ("A", "A"),
                  kernel=sc.default_kernel(golden, group))
    finally:
        dc.reset_knobs()


@pytest.mark.parametrize("name", list(EXTRA))
def test_graph_other_calls(name):
    _captured(EXTRA[name]())


def _ring_contents(stride, n, seed):
    """A dense jumbo ring of the device generator and four damaged contents of it with their verdicts."""
    ring, lens16, _ = engine.gen_rx_ring(n, seed, stride, l4_len=stride - 300)
    host, lens = ring.cpu().numpy(), tgd._u16(lens16)
    starts = np.arange(n, dtype=np.int64) * stride
    contents = [dr.frames_batch(host, starts, lens, (stride, 0), variant=v) for v in range(4)]
    for b in contents:
        dr.check_rx(b)
    assert all(np.mean(contents[0].verdicts != b.verdicts) >= sc.MIN_DIFFERENT for b in contents[1:])
    return lens16, contents


@pytest.mark.parametrize("seen", [True, False], ids=["a ring the feedback knows", "a ring never seen"])
def test_graph_ring_takes_slot_groups(seen):
    """pipck_rx_verify_ring_n under capture: k_ring whatever the ring's feedback says, no feedback
    entry made, R.verdict per frame on every replay; afterwards the uncaptured call is as before."""
    stride, n = 4096, 197
    engine.tune()
    lens16, contents = _ring_contents(stride, n, 23)
    base = torch.full((80 + n * stride + 4096,), POISON, dtype=torch.uint8, device=DEV)
    ring = base[80:80 + n * stride] if not seen else base[256:256 + n * stride]  # (+80: no other test's ring address)
    stage = [_dev(("dense ring", v), b.host) for v, b in enumerate(contents)]
    buf, ok = _guarded(n)
    err = _err()

    def uncaptured(k):
        err.fill_(ERR0)
        buf.fill_(POISON)
        engine.rx_verify_ring(ring, stride, lens16, n, ok=ok, err=err)
        name = dc.last_kernel()
        torch.cuda.synchronize()
        _held(f"rx_verify_ring (uncaptured, contents {k})", buf, contents[k].verdicts, contents[k].lens, name)
        assert _word(err) == ERR0
        return name

    ring.copy_(stage[0])
    if seen:
        kernels = [uncaptured(0) for _ in range(6)]
        assert "k_ring_rx" in kernels[-1], kernels
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        engine.rx_verify_ring(ring, stride, lens16, n, ok=ok, err=err)
    assert "k_ring<" in dc.last_kernel(), dc.last_kernel()
    for k in (1, 2, 3):
        ring.copy_(stage[k])
        buf.fill_(POISON)
        err.fill_(ERR0)
        g.replay()
        torch.cuda.synchronize()
        _held(f"rx_verify_ring (replay, contents {k})", buf, contents[k].verdicts, contents[k].lens, "k_ring")
        assert _word(err) == ERR0
    # afterwards: a ring never seen starts on k_ring; either ring reaches the row stream again within six
    # reported launches.  The first launch on k_ring shows only that no entry was made WITH feedback active
    # in the replays (they would have reported a dense ring): an entry made during capture whose kernel
    # got no feedback argument starts on k_ring as well, and nothing the library exports tells them apart.
    # (The unseen ring has no warm-up before the capture, by its nature; the known ring's is the six calls.)
    kernels = [uncaptured(3) for _ in range(6)]
    if not seen:
        assert "k_ring<" in kernels[0], kernels
    assert "k_ring_rx" in kernels[-1], kernels


@pytest.mark.parametrize("kind", ["tx_fill_device", "rx_verify_device"])
def test_graph_cold_index_through_the_engine(kind):
    """engine.tx_fill_device / rx_verify_device captured cold: the index is computed inside the
    capture, a tensor engine._check_packed has never seen, so the capture holds no host read."""
    group = "tx_fill" if kind == "tx_fill_device" else kind
    tgd._case(group)
    a, arena, lens16, index, _ = tgd._CACHE[group]
    stage = _dev((group, "A"), a.host)
    buf, res = _guarded(N)
    err = _err()
    f = getattr(engine, kind)
    arena.copy_(stage)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        f(arena, lens16, index, N, **{"done" if group == "tx_fill" else "ok": res}, err=err)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    seen = set(engine._packed_total)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fresh = engine.packed_bytes_index(lens16, N)
        f(arena, lens16, fresh, N, **{"done" if group == "tx_fill" else "ok": res}, err=err)
    assert set(engine._packed_total) == seen  # nothing read, nothing cached
    for _ in range(2):
        arena.copy_(stage)
        buf.fill_(POISON)
        err.fill_(ERR0)
        g.replay()
        torch.cuda.synchronize()
        _held(kind, buf, sc.want(group, a), a.lens)
        if group == "tx_fill":
            _image(kind, arena, a.filled)
        assert _word(err) == ERR0
    assert fresh.cpu().numpy().tolist() == index.cpu().numpy().tolist()
    # outside a capture the host-side guard is what it was: one read for the new index, then the bound
    with pytest.raises(ValueError):
        f(arena[:4096], lens16, fresh, N)
    assert id(fresh) in engine._packed_total


def test_graph_forwarding_path():
    """rx_verify_ring -> torch.where -> fwd_rewrite_ring -> rx_verify_ring -> copy_ -> tx_fill_ring as
    one graph at a 4,096-byte stride, replayed on frame sets A, B, A; everything against the
    references composed on the CPU (stream_cases.forward_reference)."""
    stride = 4096
    refs = {k: sc.forward_reference(k) for k in "AB"}
    n = len(refs["A"].frames)
    ring = torch.empty(n * stride + RING_GUARD, dtype=torch.uint8, device=DEV)
    ring2 = torch.empty_like(ring)
    lens = torch.empty(n, dtype=torch.int16, device=DEV)
    assigned = torch.empty(n, dtype=torch.int32, device=DEV)
    rule_of = torch.empty(n, dtype=torch.int32, device=DEV)
    no_rule = torch.full((n,), -1, dtype=torch.int32, device=DEV)  # PIPCK_FWD_NO_RULE, 0xFFFFFFFF
    assert engine.FWD_NO_RULE == 0xFFFFFFFF
    rules = engine.make_fwd_rules(list(rule_table()))
    bufs = [torch.empty(n + 32, dtype=torch.uint8, device=DEV) for _ in range(4)]
    ok, done, ok2, tx_done = (b[16:n + 16] for b in bufs)
    err = _err()
    stage = {k: (_dev(("ring", stride, k), ring_image(r.frames, stride, RING_GUARD)), _dev(("ring lens", k), ring_lens(r.frames)),
                 _dev(("rule_of", k), r.rule_of.view(np.int32))) for k, r in refs.items()}

    def restore(k):
        ring.copy_(stage[k][0])
        lens.copy_(stage[k][1])
        assigned.copy_(stage[k][2])
        ring2.fill_(POISON)
        rule_of.fill_(0)
        for b in bufs:
            b.fill_(DONE_POISON)
        err.fill_(ERR0)

    def path():
        engine.rx_verify_ring(ring, stride, lens, n, ok=ok, err=err)
        torch.where(ok == R.VERIFIED, assigned, no_rule, out=rule_of)
        engine.fwd_rewrite_ring(ring, stride, lens, rules, rule_of, n, flags=F.UDP_ZERO_AS_ONES, done=done, err=err)
        engine.rx_verify_ring(ring, stride, lens, n, ok=ok2, err=err)
        ring2.copy_(ring)
        engine.tx_fill_ring(ring2, stride, lens, n, done=tx_done, err=err)

    engine.tune()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        restore("A")
        path()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        path()
    for k in ("A", "B", "A"):
        restore(k)
        g.replay()
        torch.cuda.synchronize()
        r = refs[k]
        for what, b, want in (("ok", bufs[0], r.ok), ("ok2", bufs[2], r.ok2)):
            _held(f"forwarding graph ({what}, frame set {k})", b, want, None, lead=16, poison=DONE_POISON)
            assert b.numel() == 16 + want.size + 16
        _check(f"forwarding graph (rewrite, frame set {k})", r.frames, stride, ring.cpu().numpy(), bufs[1].cpu().numpy(),
               ring_image(r.rewritten, stride, RING_GUARD), r.done)
        _check(f"forwarding graph (TX fill, frame set {k})", r.frames, stride, ring2.cpu().numpy(),
               bufs[3].cpu().numpy(), ring_image(r.filled, stride, RING_GUARD), r.tx_done)
        assert _word(err) == ERR0


# ----------------------------------------------------------------------------
# 3. ring bases at every 16-byte phase; result pointers at odd bytes
# ----------------------------------------------------------------------------
RX_SCHEDULES = {"default": {}, "own": dict(ring_own_slots=True, ring_adapt=False),
                "coop": dict(ring_all_coop=True, ring_adapt=False), "rows": dict(alt_flat_schedule=True)}
LEAD = 256  # the ring's allocation starts LEAD - phase ... the ring itself at LEAD + phase


def _phased_ring(frames, stride, phase):
    """(allocation, ring view at allocation + phase, host image of the whole allocation)."""
    n = len(frames)
    img = np.full(phase + n * stride + RING_GUARD, POISON, dtype=np.uint8)
    img[phase:] = ring_image(frames, stride, RING_GUARD)
    base = torch.from_numpy(img).to(DEV)
    assert base.data_ptr() % 128 == 0
    ring = base[phase:]
    assert ring.data_ptr() % 128 == phase and ring.data_ptr() % 16 == 0
    return base, ring, img


@pytest.mark.parametrize("phase", [16, 48, 112])
@pytest.mark.parametrize("stride", [1024, 9216])
def test_ring_base_at_every_16_byte_phase(stride, phase):
    frames = list(sc.aligned_frames(stride))
    n = len(frames)
    lens = torch.from_numpy(ring_lens(frames)).to(DEV)
    verdicts = np.array([R.verdict(f) for f in frames], dtype=np.uint8)
    err = _err()

    def whole(path, base, done, img, want_frames, want_done):
        got = base.cpu().numpy()
        assert (got[:phase] == POISON).all(), f"{path}: bytes in front of the ring were written"
        _check(path, frames, stride, got[phase:], done.cpu().numpy(), ring_image(want_frames, stride, RING_GUARD), want_done)
        assert _word(err) == ERR0, path

    try:
        for schedule, knobs in RX_SCHEDULES.items():
            engine.tune(**knobs)
            base, ring, img = _phased_ring(frames, stride, phase)
            done = torch.full((n + 32,), DONE_POISON, dtype=torch.uint8, device=DEV)
            err.fill_(ERR0)
            engine.rx_verify_ring(ring, stride, lens, n, ok=done[16:n + 16], err=err)
            name = dc.last_kernel()
            assert ("k_ring_rx" if schedule == "rows" else "k_ring<") in name, (schedule, name)
            whole(f"rx_verify_ring ({schedule}, stride {stride}, +{phase}) {name}", base, done, img, frames, verdicts)
        engine.tune()
        for which in ("tx", "fwd"):
            base, ring, img = _phased_ring(frames, stride, phase)
            done = torch.full((n + 32,), DONE_POISON, dtype=torch.uint8, device=DEV)
            err.fill_(ERR0)
            if which == "tx":
                engine.tx_fill_ring(ring, stride, lens, n, done=done[16:n + 16], err=err)
                want = reference_fill(frames, 0)
            else:
                ro = torch.from_numpy(assign(frames).view(np.int32)).to(DEV)
                engine.fwd_rewrite_ring(ring, stride, lens, engine.make_fwd_rules(list(rule_table())), ro, n,
                                        flags=F.UDP_ZERO_AS_ONES, done=done[16:n + 16], err=err)
                want = reference_rewrite(frames, assign(frames), F.UDP_ZERO_AS_ONES)
            whole(f"{which} ring (stride {stride}, +{phase}) {dc.last_kernel()}", base, done, img, *want)
    finally:
        engine.tune()


def _first_fixed(golden, kernel, knob, verify):
    for g in dr.census_groups():
        if g.startswith("fixed_verify" if verify else "fixed_checksum") and \
                f"::{kernel}" in (dc.decode(golden, g)[knob][1] or ""):
            return g
    raise AssertionError(f"no fixed {'verify' if verify else 'checksum'} group launches {kernel} under {knob}")


# (kernel, knob): k_hdr takes batches of 4,099 headers under a loads knob only (by default from 8M headers on)
ODD_POINTER_CASES = [("k_hdr<", "loads=8"), ("k_flat_coop<", "default"), ("k_flat<", "default"),
                     ("k_packedb<", "default")]


@pytest.mark.parametrize("kernel,knob", ODD_POINTER_CASES)
def test_result_pointers_at_odd_bytes(golden, kernel, knob):
    """u16 results at allocation + 2, u8 results at + 1 and + 3 (pipck_hdr.hip has a fast path
    keyed on the result pointer's alignment), inside poisoned buffers."""
    try:
        for verify, offsets in ((False, (2,)), (True, (1, 3))):
            group = f"packed_bytes_{'verify' if verify else 'checksum'}" if kernel == "k_packedb<" else \
                _first_fixed(golden, kernel, knob, verify)
            assert dr.computes_results(dc.knobs_of(group)[knob])
            c = tgd._case(group)
            size = c.want.size * c.want.dtype.itemsize
            err = _err()
            dc.apply_knob(dc.knobs_of(group)[knob], False)
            for off in offsets:
                buf, res = _guarded(size, lead=off)
                assert buf.data_ptr() % 256 == 0 and res.data_ptr() % 4 == off
                buf.fill_(POISON)
                err.fill_(ERR0)
                c.launch(res, err)
                name = dc.last_kernel()
                torch.cuda.synchronize()
                assert name == dc.decode(golden, group)[knob][1] and f"::{kernel}" in name, name
                _held(f"{group} (results at +{off})", buf, c.want, c.lens, name, lead=off)
                assert _word(err) == ERR0
    finally:
        dc.reset_knobs()


@pytest.mark.parametrize("off", [1, 3])
def test_ring_result_pointers_at_odd_bytes(off):
    stride = 1024
    frames = list(sc.aligned_frames(stride))
    n = len(frames)
    lens = torch.from_numpy(ring_lens(frames)).to(DEV)
    err = _err()
    rules = engine.make_fwd_rules(list(rule_table()))
    ro = torch.from_numpy(assign(frames).view(np.int32)).to(DEV)
    calls = {"rx": (lambda ring, res: engine.rx_verify_ring(ring, stride, lens, n, ok=res, err=err),
                    (frames, np.array([R.verdict(f) for f in frames], dtype=np.uint8))),
             "tx": (lambda ring, res: engine.tx_fill_ring(ring, stride, lens, n, done=res, err=err),
                    reference_fill(frames, 0)),
             "fwd": (lambda ring, res: engine.fwd_rewrite_ring(ring, stride, lens, rules, ro, n, flags=F.UDP_ZERO_AS_ONES,
                                                               done=res, err=err),
                     reference_rewrite(frames, assign(frames), F.UDP_ZERO_AS_ONES))}
    for which, (call, (want_frames, want_done)) in calls.items():
        ring = torch.from_numpy(ring_image(frames, stride, RING_GUARD)).to(DEV)
        buf, res = _guarded(n, lead=off)
        assert res.data_ptr() % 4 == off
        buf.fill_(POISON)
        err.fill_(ERR0)
        call(ring, res)
        torch.cuda.synchronize()
        _held(f"{which} ring (results at +{off})", buf, want_done, None, dc.last_kernel(), lead=off)
        _image(f"{which} ring (results at +{off})", ring, ring_image(want_frames, stride, RING_GUARD))
        assert _word(err) == ERR0


# ----------------------------------------------------------------------------
# 4. the error word is OR-ed
# ----------------------------------------------------------------------------
def _refusals():
    """{entry point: call(refuse: bool, err)}: with `refuse`, one planted element the device refuses
    (the plants of tests/test_gpu_bounds.py and of the ring refusal tests); without, a clean call."""
    n, nf, stride, length = 64 * 5 + 9, 8, 96, 80
    rng = np.random.default_rng(404)
    arena = torch.from_numpy(rng.integers(0, 256, n * stride, dtype=np.uint8)).to(DEV)
    _, pseudo = engine.gen_flows(4, nf, 77, 6)
    _, pseudo2 = engine.gen_flows(4, nf, 78, 6)
    flows = rng.integers(0, nf, n).astype(np.int32)
    bad = flows.copy()
    bad[[0, 63, 64, n - 1]] = [nf, -1, nf + 1, 1 << 30]  # a flow past the table (-1: 0xFFFFFFFF)
    fl = {False: torch.from_numpy(flows).to(DEV), True: torch.from_numpy(bad).to(DEV)}
    offs = np.arange(n, dtype=np.uint64) * stride
    desc = {r: engine.make_desc(offs, np.full(n, length, dtype=np.uint32), bad if r else flows) for r in (False, True)}
    begin = torch.arange(n + 1, dtype=torch.int64, device=DEV)
    calls = {
        "pipck_checksum_fixed_n": lambda r, e: engine.checksum_fixed(arena, stride, length, n, pseudo, nf, fl[r], err=e),
        "pipck_verify_fixed_n": lambda r, e: engine.verify_fixed(arena, stride, length, n, pseudo, nf, fl[r], err=e),
        "pipck_checksum_ragged_n": lambda r, e: engine.checksum_ragged(arena, desc[r], pseudo, err=e),
        "pipck_verify_ragged_n": lambda r, e: engine.verify_ragged(arena, desc[r], pseudo, err=e),
        "pipck_checksum_chains_n": lambda r, e: engine.checksum_chains(arena, desc[False], begin, fl[r], pseudo, err=e),
        "pipck_update_fixed_n": lambda r, e: engine.update_fixed(arena.clone(), stride, n, 0, length, 16, 24, 0, None, 0,
                                                                 pseudo, pseudo2, nf, fl[r], err=e),
    }
    # the plain ragged and chain forms trust offsets and flows and refuse only a length over 65,535 (not read)
    long_lens = np.full(n, length, dtype=np.uint32)
    long_lens[[0, 64, n - 1]] = 70000
    plain = {False: desc[False], True: engine.make_desc(offs, long_lens, flows)}
    p = engine._ptr

    def plain_ragged(fn, dtype):
        def call(r, e):
            out = torch.empty(n, dtype=dtype, device=DEV)
            _lib.call(fn, p(arena), p(plain[r]), n, p(pseudo), p(out), p(e), engine.current_stream())
        return call

    def plain_chains(r, e):
        out, scratch = torch.empty(n, dtype=torch.int16, device=DEV), torch.empty(n, dtype=torch.int32, device=DEV)
        _lib.call("pipck_checksum_chains", p(arena), p(plain[r]), n, p(begin), p(fl[False]), n, p(pseudo), p(scratch),
                  p(out), p(e), engine.current_stream())

    calls["pipck_checksum_ragged"] = plain_ragged("pipck_checksum_ragged", torch.int16)
    calls["pipck_verify_ragged"] = plain_ragged("pipck_verify_ragged", torch.uint8)
    calls["pipck_checksum_chains"] = plain_chains
    for by in (False, True):
        pa, lens16, index, _ = (engine.gen_packed_bytes if by else engine.gen_packed)(n, 0, CFG4.seed, CFG4.hdr)
        for verify in (False, True):
            f = getattr(engine, ("verify" if verify else "checksum") + "_packed" + ("_bytes" if by else ""))
            calls[f"pipck_{'verify' if verify else 'checksum'}_packed{'_bytes' if by else ''}_n"] = \
                lambda r, e, f=f, pa=pa, lens16=lens16, index=index: f(pa, lens16, index, n, pseudo, nf, fl[r], err=e)
    # byte-packed frames: an index entry that sends a middle tile past the arena (tests/test_gpu_tx_fill.py's
    # plant; the index's total, which the engine's host-side guard reads, is as it was)
    fa, flens, findex = engine.gen_rx_frames(n, 91)[:3]
    moved = findex.clone()
    moved[2] = fa.numel() - 5  # starts inside the arena, ends past it
    pick = {False: findex, True: moved}
    calls["pipck_rx_verify_device"] = lambda r, e: engine.rx_verify_device(fa, flens, pick[r], n, err=e)
    calls["pipck_tx_fill_device"] = lambda r, e: engine.tx_fill_device(fa.clone(), flens, pick[r], n, err=e)
    # rings: a slot length past the stride; the forwarding call also a rule of family 5 (invalid)
    from tests.test_gpu_fwd_ring import _done_pool

    frames = _done_pool()[:sc.ALIGN_N]  # frames every rule of their family rewrites: a refusal has work to refuse
    rn = len(frames)
    assert rn == sc.ALIGN_N
    ring = torch.from_numpy(ring_image(frames, 1024, 65 * 1024)).to(DEV)
    good = ring_lens(frames)
    over = good.copy().view(np.uint16)
    over[[64, rn - 1]] = [1025, 65535]
    rl = {False: torch.from_numpy(good).to(DEV), True: torch.from_numpy(over.view(np.int16)).to(DEV)}
    rules = engine.make_fwd_rules([(F.DEC_TTL, 0), (F.ALL_OPS, 5, bytes(4), bytes(4), 1, 2)])
    ro = {False: torch.zeros(rn, dtype=torch.int32, device=DEV), True: torch.zeros(rn, dtype=torch.int32, device=DEV)}
    ro[True][[3, rn - 2]] = 1
    calls["pipck_rx_verify_ring_n"] = lambda r, e: engine.rx_verify_ring(ring, 1024, rl[r], rn, err=e)
    calls["pipck_tx_fill_ring"] = lambda r, e: engine.tx_fill_ring(ring.clone(), 1024, rl[r], rn, err=e)
    calls["pipck_fwd_rewrite_ring"] = lambda r, e: engine.fwd_rewrite_ring(ring.clone(), 1024, rl[r], rules, ro[False], rn,
                                                                          err=e)
    calls["pipck_fwd_rewrite_ring (invalid rule)"] = \
        lambda r, e: engine.fwd_rewrite_ring(ring.clone(), 1024, rl[False], rules, ro[r], rn, err=e)
    return calls


def test_error_word_is_ored():
    """Every entry point that takes d_err, err preset to ERR0: a refusing call leaves
    ERR0 | 1 << PIPCK_ERANGE (an invalid forwarding rule: | 1 << PIPCK_EINVAL), a clean call ERR0."""
    wrong = []
    err = _err()
    for name, call in _refusals().items():
        bit = EINVAL_BIT if "invalid rule" in name else ERANGE_BIT
        for refuse, want in ((True, ERR0 | bit), (False, ERR0)):
            err.fill_(ERR0)
            call(refuse, err)
            torch.cuda.synchronize()
            if _word(err) != want:
                wrong.append(f"{name} ({'refusing' if refuse else 'clean'}): {_word(err):#x}, want {want:#x}")
    assert not wrong, "\n".join(wrong)


# ----------------------------------------------------------------------------
# 5. four host threads, four streams
# ----------------------------------------------------------------------------
ROUNDS = 20


def test_four_threads_four_streams(golden):
    """A quarter of the census groups' default launches per thread, 20 rounds each on the thread's
    own stream: the launch record is the thread's own, and every result equals its reference."""
    groups = dr.census_groups()
    dc.apply_knob(dc.knobs_of("rx_verify_ring[4096]")["default"], False)  # (the general groups ignore the ring word)
    try:
        cases = {g: _census_case(g) for g in groups}
        for c in cases.values():
            for dst, stage in c.inputs:
                dst.copy_(stage["A"])
            for buf, poison in c.bufs:
                buf.fill_(poison)
            c.err.fill_(ERR0)
        torch.cuda.synchronize()
        failures = []

        def work(mine):
            try:
                s = torch.cuda.Stream()
                with torch.cuda.stream(s):
                    for _ in range(ROUNDS):
                        for g in mine:
                            c = cases[g]
                            if g == "tx_fill":
                                c.inputs[0][0].copy_(c.inputs[0][1]["A"])
                            c.call()
                            name = dc.last_kernel()
                            if name != sc.default_kernel(golden, g):
                                failures.append(f"{g}: this thread's launch record names {name}")
                s.synchronize()
            except Exception as ex:  # noqa: BLE001  (reported by the test's thread)
                failures.append(f"{mine[0]}...: {ex!r}")

        threads = [threading.Thread(target=work, args=(groups[k::4],)) for k in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        torch.cuda.synchronize()
        assert not failures, failures[:8]
        for g, c in cases.items():
            c.check("A")
            assert _word(c.err) == ERR0, g
    finally:
        dc.reset_knobs()


def test_two_streams_one_jumbo_ring():
    """Two threads, a stream each, verify ONE dense ring of 4,096-byte slots concurrently, 20
    rounds: every verdict buffer equals the reference (overlapping calls only mix the heuristic)."""
    stride, n = 4096, 197
    engine.tune()
    lens16, contents = _ring_contents(stride, n, 29)
    b = contents[1]
    ring = _dev(("shared ring", 1), b.host)
    bufs = [[_guarded(n) for _ in range(ROUNDS)] for _ in range(2)]
    errs = [_err().fill_(ERR0) for _ in range(2)]
    for per in bufs:
        for buf, _ in per:
            buf.fill_(POISON)
    torch.cuda.synchronize()
    failures, kernels = [], [[], []]

    def work(k):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                for _, ok in bufs[k]:
                    engine.rx_verify_ring(ring, stride, lens16, n, ok=ok, err=errs[k])
                    kernels[k].append(dc.last_kernel())
            s.synchronize()
        except Exception as ex:  # noqa: BLE001
            failures.append(repr(ex))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    assert not failures, failures
    for k in range(2):
        for r, (buf, _) in enumerate(bufs[k]):
            _held(f"shared ring (stream {k}, round {r})", buf, b.verdicts, b.lens, kernels[k][r])
        assert _word(errs[k]) == ERR0
