"""The host-memory paths across their seams (tests/host_path_cases.py): the
chunked pipelines pipck_host_checksum_fixed, pipck_host_checksum_packed_bytes
and pipck_host_rx_verify_packed at, one short of and one past every cut; the RX
queue with its launches cut where its staging grows; the TX queue through
scripts of refused adds, empty chains, batches of changing size on both of its
paths and a destroy with a batch in flight; and four writer threads with a queue
each over pinned pools of their own and a shared one.

Everything is bit-exact against the table, whose expected values are the plain
references' (tests/test_host_path_cases.py holds the table to them and to its
seams on the CPU).  Result arrays and checksum fields lie inside poisoned
guards, which are checked.  ctypes through pip_amd._lib, as the other host-path
tests."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from pip_amd import _lib  # noqa: E402
from tests import host_path_cases as hp  # noqa: E402
from tests import rx_reference as R  # noqa: E402
from tests import saturation_cases as sc  # noqa: E402

GUARD = 256
POISON = hp.POISON
NF = hp.NF

_CACHE: dict = {}


@pytest.fixture(scope="module", autouse=True)
def lib():
    lib = _lib.load()
    yield lib
    pin = _CACHE.pop("pinned", None)
    _CACHE.clear()
    if pin:
        assert lib.pipck_host_free(C.c_void_p(pin[0])) == _lib.PIPCK_OK


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _fixed_arena(name):
    """The arena of a fixed case, built once for the module and never written."""
    def make():
        a = hp.fixed_arena(name)
        a.setflags(write=False)
        return a
    return _cached(("fixed", name), make)


def _packed_arena(name):
    def make():
        c = hp.packed(name)
        a, lens = c.arena(), c.lens.astype(np.uint16)
        a.setflags(write=False)
        return a, lens
    return _cached(("packed", name), make)


def _pinned_copy(lib, host: np.ndarray) -> int:
    """host's bytes in the module's one pipck_host_alloc buffer (large enough for every arena)."""
    size = 136 << 20
    assert host.size <= size
    pin = _cached("pinned", lambda: (lib.pipck_host_alloc(size), size))
    assert pin[0], "pipck_host_alloc failed"
    C.memmove(pin[0], host.ctypes.data, host.size)
    return pin[0]


def _ctx(lib):
    ctx = C.c_void_p()
    _lib.check("pipck_ctx_create", lib.pipck_ctx_create(-1, C.byref(ctx)))
    return ctx


def _flows(fam, nf=NF):
    """(a host flow table of family fam with nf flows -- kept alive by the caller --, its address, nf); family 0: none."""
    if not fam:
        return None, None, 0
    rec = sc.flows(fam)[0]
    size = len(rec) // NF
    buf = np.frombuffer(rec[:nf * size], dtype=np.uint8).copy()
    return buf, buf.ctypes.data, nf


class Guarded:
    """n results of `dtype` inside poisoned guards, at an even or an odd element offset."""

    def __init__(self, n, dtype, odd=False):
        self.n, self.dtype = n, np.dtype(dtype)
        self.at = GUARD + (self.dtype.itemsize if odd else 0)
        self.buf = np.full(self.at + n * self.dtype.itemsize + GUARD, POISON, dtype=np.uint8)
        assert self.buf.ctypes.data % 16 == 0
        self.ptr = self.buf.ctypes.data + self.at

    def check(self, want, what):
        end = self.at + self.n * self.dtype.itemsize
        got = self.buf[self.at:end].view(self.dtype)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (what, self.n, bad.size, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
        assert (self.buf[:self.at] == POISON).all() and (self.buf[end:] == POISON).all(), what


# ----------------------------------------------------------------------------
# the chunked pipelines
# ----------------------------------------------------------------------------
def _run_fixed(lib, ctx, name, base, n, fam, origin, odd, nf=NF):
    f = hp.FIXED[name]
    keep, flows, nf = _flows(fam, nf)
    out = Guarded(n, np.uint16, odd)
    rc = lib.pipck_host_checksum_fixed(ctx, base, f.stride, f.length, n, fam, flows, nf, origin, out.ptr)
    assert rc == 0, (name, n, fam, origin, lib.pipck_last_error())
    out.check(hp.fixed_expected(name, n, fam, origin, nf or NF), ("fixed", name, n, fam, origin))


@pytest.mark.parametrize("memory", ["pageable", "pinned"])
@pytest.mark.parametrize("name", list(hp.FIXED))
def test_fixed_across_the_chunk_cut(lib, name, memory):
    """pipck_host_checksum_fixed on prefixes of one arena: one packet short of a chunk, a whole
    chunk, one packet more, and two chunks and a packet (the first reuse of a device buffer), under
    each family and flow origin of the table."""
    f = hp.FIXED[name]
    arena = _fixed_arena(name)
    base = arena.ctypes.data if memory == "pageable" else _pinned_copy(lib, arena)
    ctx = _ctx(lib)
    try:
        for n, fam, origin in hp.fixed_variants(f):
            _run_fixed(lib, ctx, name, base, n, fam, origin, odd=memory == "pageable")
    finally:
        lib.pipck_ctx_destroy(ctx)


def _run_packed(lib, ctx, name, base, lens, fam, origin, odd):
    c = hp.packed(name)
    keep, flows, nf = _flows(fam)
    out = Guarded(c.count, np.uint16, odd)
    rc = lib.pipck_host_checksum_packed_bytes(ctx, base, lens.ctypes.data, c.count, fam, flows, nf, origin, out.ptr)
    assert rc == 0, (name, fam, origin, lib.pipck_last_error())
    out.check(c.checksums(fam, origin), ("packed", name, fam, origin))


def _run_rx_packed(lib, ctx, name, base, lens, odd):
    c = hp.packed(name)
    ok = Guarded(c.count, np.uint8, odd)
    good = C.c_uint64(99)
    rc = lib.pipck_host_rx_verify_packed(ctx, base, lens.ctypes.data, c.count, ok.ptr, C.byref(good))
    assert rc == 0, (name, lib.pipck_last_error())
    want = c.verdicts()
    ok.check(want, ("rx packed", name))
    assert good.value == int((want == R.VERIFIED).sum())


@pytest.mark.parametrize("memory", ["pageable", "pinned"])
@pytest.mark.parametrize("name", hp.PACKED_NAMES)
def test_packed_across_the_chunk_cut(lib, name, memory):
    """pipck_host_checksum_packed_bytes and pipck_host_rx_verify_packed over the same lengths: a
    chunk that ends exactly on 64 MiB, the largest overshoot, exactly 2^20 packets, empty packets
    on both sides of a cut, a last chunk of empty packets only."""
    arena, lens = _packed_arena(name)
    base = arena.ctypes.data if memory == "pageable" else _pinned_copy(lib, arena)
    odd = memory == "pageable"
    ctx = _ctx(lib)
    try:
        for fam, origin in hp.PACKED_FLOWS:
            _run_packed(lib, ctx, name, base, lens, fam, origin, odd)
        _run_rx_packed(lib, ctx, name, base, lens, odd)
    finally:
        lib.pipck_ctx_destroy(ctx)


def test_one_context_through_every_pipeline(lib):
    """ONE context: fixed 65,536 (IPv4, a table of 3 flows) -> fixed 20 (no flows; the result
    buffers grow) -> packed (IPv6, 97 flows: the chunk buffers, the packed index and the flow
    table grow) -> RX verdicts (the result buffers hold bytes) -> fixed 9,216.  Every call is checked."""
    ctx = _ctx(lib)
    try:
        big = hp.FIXED["s65536"]
        _run_fixed(lib, ctx, "s65536", _fixed_arena("s65536").ctypes.data, big.arena_packets, 4, 5, False, nf=3)
        _run_fixed(lib, ctx, "s20", _fixed_arena("s20").ctypes.data, hp.FIXED["s20"].arena_packets, 0, 0, True)
        arena, lens = _packed_arena("zeros_at_cut")
        _run_packed(lib, ctx, "zeros_at_cut", arena.ctypes.data, lens, 6, 5, True)
        _run_rx_packed(lib, ctx, "zeros_at_cut", arena.ctypes.data, lens, True)
        _run_fixed(lib, ctx, "s9216", _fixed_arena("s9216").ctypes.data, hp.FIXED["s9216"].arena_packets, 4,
                   hp.fixed_origins(hp.FIXED["s9216"])[3], False)
        _run_rx_packed(lib, ctx, "zero_tail", _packed_arena("zero_tail")[0].ctypes.data, _packed_arena("zero_tail")[1],
                       False)
    finally:
        lib.pipck_ctx_destroy(ctx)


# ----------------------------------------------------------------------------
# the RX queue
# ----------------------------------------------------------------------------
class FramePlaces:
    """Every frame of a pool once in a pinned block (at every residue mod 16) and once in pageable memory."""

    def __init__(self, lib, pool):
        self.lib = lib
        size = int(pool.lens.sum()) + 24 * len(pool.frames) + 64
        self.base = lib.pipck_host_alloc(size)
        assert self.base
        self.heap = [C.create_string_buffer(f, max(len(f), 1)) for f in pool.frames]
        self.pinned, off = [], 5
        for k, f in enumerate(pool.frames):
            C.memmove(self.base + off, f, len(f))
            self.pinned.append(self.base + off)
            off += len(f) + 8 + k % 16
        assert off <= size and len({p % 16 for p in self.pinned}) == 16
        self.heap_at = [C.cast(b, C.c_void_p).value for b in self.heap]

    def pointers(self, seq):
        return [(self.pinned if hp.rxq_pinned(i) else self.heap_at)[int(k)] for i, k in enumerate(seq)]

    def free(self):
        base, self.base = self.base, None
        return self.lib.pipck_host_free(C.c_void_p(base)) if base else _lib.PIPCK_OK


def _rx_verify(lib, q, ptrs, lens, want, what):
    n = len(ptrs)
    arr = (C.c_void_p * n)(*ptrs)
    ln = (C.c_uint32 * n)(*[int(x) for x in lens])
    ok = Guarded(n, np.uint8, odd=True)
    good = C.c_uint64(12345)
    rc = lib.pipck_rx_verify(q, arr, ln, n, ok.ptr, C.byref(good))
    assert rc == 0, (what, lib.pipck_last_error())
    ok.check(want, what)
    assert good.value == int((want == R.VERIFIED).sum()), what


@pytest.mark.parametrize("n", hp.RXQ_COUNTS)
def test_rx_queue_on_its_launch_cuts(lib, n):
    """pipck_rx_verify on a fresh queue with n on, one short of and one past the first and the
    second launch, packets pinned / pageable / pageable / pinned: the staging of the pageable ones
    grows before the first launch and again between launches.  The pool frees right after the call."""
    pool, seq = hp.rxq_sequence(n)
    places = FramePlaces(lib, pool)
    q = C.c_void_p()
    assert lib.pipck_rxq_create(None, C.byref(q)) == 0
    try:
        _rx_verify(lib, q, places.pointers(seq), pool.lens[seq], pool.verdicts[seq], ("rxq", n))
        assert places.free() == _lib.PIPCK_OK  # the call dropped its holds
    finally:
        lib.pipck_rxq_destroy(q)
        places.free()


# ----------------------------------------------------------------------------
# the TX queue
# ----------------------------------------------------------------------------
def _hsegs(segs, address):
    """(array kept alive, POINTER(HSeg) or None, count) of segs = [(region or None, offset, length)]."""
    if segs is None:
        return None, None, 0
    arr = (_lib.HSeg * max(len(segs), 1))()
    for k, (region, off, n) in enumerate(segs):
        arr[k].ptr = address(region, off) if region else None
        arr[k].len = n
    return arr, arr, len(segs)


def _add(lib, q, fam, flow, segs, field, zc, address):
    keep, arr, nseg = _hsegs(segs, address)
    _, src, dst, proto = sc.flows(fam)[1][flow]
    if fam == 4:
        fn = lib.pipck_txq_add4_zc if zc else lib.pipck_txq_add4
        return fn(q, arr, nseg, proto, int.from_bytes(src, "little"), int.from_bytes(dst, "little"), field)
    fn = lib.pipck_txq_add6_zc if zc else lib.pipck_txq_add6
    return fn(q, arr, nseg, proto, src, dst, field)


class Fields:
    """Two-byte checksum fields at odd addresses, 4 bytes apart, inside poisoned guards."""

    def __init__(self, slots):
        self.buf = np.full(GUARD + 4 * slots + GUARD, POISON, dtype=np.uint8)
        assert self.buf.ctypes.data % 4 == 0
        self.slots = slots

    def ptr(self, slot):
        return C.c_void_p(self.buf.ctypes.data + GUARD + 4 * slot + 1)

    def check(self, expect: dict, what, fields_unspecified=False):
        """Stored fields hold htons(expected); every other byte its poison."""
        want = np.full(self.buf.size, POISON, dtype=np.uint8)
        at = GUARD + 4 * np.fromiter(expect.keys(), dtype=np.int64, count=len(expect)) + 1
        v = np.fromiter(expect.values(), dtype=np.int64, count=len(expect))
        want[at], want[at + 1] = v >> 8, v & 0xFF
        same = self.buf == want
        if fields_unspecified:
            every = GUARD + 4 * np.arange(self.slots) + 1
            same[every] = same[every + 1] = True
        bad = np.nonzero(~same)[0]
        assert bad.size == 0, (what, bad.size, ((bad[:8] - GUARD) // 4).tolist(), self.buf[bad[:8]].tolist(),
                               want[bad[:8]].tolist())


def _run_script(lib, name, in_place):
    s = hp.script(name)
    ctx, q = _ctx(lib), C.c_void_p()
    _lib.check("pipck_txq_create", lib.pipck_txq_create(ctx, C.byref(q)))
    heap = s.mem[hp.REGION_AT["H"]:hp.REGION_AT["H"] + hp.REGION_BYTES["H"]].copy()
    base = {"H": heap.ctypes.data}
    for r in ("A", "B"):
        base[r] = lib.pipck_host_alloc(hp.REGION_BYTES[r])
        assert base[r]
        C.memmove(base[r], s.mem[hp.REGION_AT[r]:].ctypes.data, hp.REGION_BYTES[r])
    fields = Fields(s.slots)
    stored = {}

    def done(slots, what):
        stored.update({k: s.expect[k] for k in slots if k in s.expect})
        fields.check(stored, (name, in_place, what), fields_unspecified=not s.expect)

    try:
        if not in_place:
            _lib.check("pipck_txq_inplace_max", lib.pipck_txq_inplace_max(q, 0))
        for k, op in enumerate(s.ops):
            what = (k, op[0])
            if op[0] == "add":
                _, fam, flow, segs, slot, zc, rc = op
                assert _add(lib, q, fam, flow, segs, fields.ptr(slot), zc, lambda r, o: base[r] + o) == rc, (name, op)
            elif op[0] == "add_ip":
                _, (region, off, n), slot, rc = op
                assert lib.pipck_txq_add_ip(q, C.c_void_p(base[region] + off), n, fields.ptr(slot)) == rc, (name, op)
            elif op[0] == "pending":
                assert lib.pipck_txq_pending(q) == op[1], (name, what)
            elif op[0] == "inflight":
                assert lib.pipck_txq_inflight(q) == op[1], (name, what)
            elif op[0] == "free":
                assert lib.pipck_host_free(C.c_void_p(base.pop(op[1]))) == op[2], (name, what, lib.pipck_last_error())
            elif op[0] == "inplace":
                # as written on the in-place run; the copy run takes the other path at every batch
                on = (op[1] is None) == in_place
                _lib.check("pipck_txq_inplace_max", lib.pipck_txq_inplace_max(q, hp.TX_INPLACE_MAX if on else 0))
            elif op[0] in ("submit", "complete", "flush"):
                _lib.check(op[0], getattr(lib, "pipck_txq_" + op[0])(q))
                done(op[1], what)
            elif op[0] == "destroy":
                _lib.check("pipck_txq_destroy", lib.pipck_txq_destroy(q))
                q = None
            else:
                raise AssertionError(op)
        if q is not None:
            assert lib.pipck_txq_pending(q) == 0 and lib.pipck_txq_inflight(q) == 0
        done([], "end")
        assert set(stored) == set(s.expect)
    finally:
        if q is not None:
            lib.pipck_txq_destroy(q)
        rcs = [lib.pipck_host_free(C.c_void_p(base[r])) for r in ("A", "B") if r in base]
        lib.pipck_ctx_destroy(ctx)
    assert rcs == [_lib.PIPCK_OK] * len(rcs)


@pytest.mark.parametrize("in_place", [True, False])
@pytest.mark.parametrize("name", hp.SCRIPT_NAMES)
def test_tx_queue_script(lib, name, in_place):
    """Each script of the table as written, on the in-place path and with inplace_max = 0."""
    _run_script(lib, name, in_place)


# ----------------------------------------------------------------------------
# one queue per writer thread
# ----------------------------------------------------------------------------
def test_four_writer_threads(lib):
    """Four threads, each with a TX queue and a pinned pool of its own (thread 0 with an RX queue as
    well), 20 rounds of staged, _zc and auto-zero-copy batches with segments from their own pool, a
    pool shared by all and pageable memory, while the main thread allocates and frees a fifth
    pinned range: every field and verdict is the reference's, and every pool frees afterwards."""
    shared_at = hp.THREAD_AT["shared"]
    shared = lib.pipck_host_alloc(hp.THREAD_REGIONS["shared"])
    assert shared
    C.memmove(shared, hp.thread_memory(0)[shared_at:].ctypes.data, hp.THREAD_REGIONS["shared"])
    plans = [(hp.thread_memory(t), hp.thread_rounds(t)) for t in range(hp.THREADS)]  # built before the threads start
    rx_pool = hp.pool("medium")
    failures, pools, running = [], [], [hp.THREADS]
    lock = threading.Lock()

    def work(t):
        own, ctx, q, rxq, places = None, None, C.c_void_p(), C.c_void_p(), None
        try:
            mem, rounds = plans[t]
            own = lib.pipck_host_alloc(hp.THREAD_REGIONS["own"])
            assert own
            C.memmove(own, mem.ctypes.data, hp.THREAD_REGIONS["own"])
            heap = mem[hp.THREAD_AT["heap"]:].copy()
            base = {"own": own, "shared": shared, "heap": heap.ctypes.data}
            ctx = _ctx(lib)
            _lib.check("pipck_txq_create", lib.pipck_txq_create(ctx, C.byref(q)))
            if t == 0:
                assert lib.pipck_rxq_create(None, C.byref(rxq)) == 0
                places = FramePlaces(lib, rx_pool)
            for r, (mode, pkts, want) in enumerate(rounds):
                _lib.check("auto_zero_copy", lib.pipck_txq_auto_zero_copy(q, mode == "auto"))
                _lib.check("inplace_max", lib.pipck_txq_inplace_max(q, 0 if (r + t) % 4 == 3 else hp.TX_INPLACE_MAX))
                fields = Fields(len(pkts))
                for k, (fam, flow, segs, ip) in enumerate(pkts):
                    if ip:
                        rc = lib.pipck_txq_add_ip(q, C.c_void_p(base[segs[0][0]] + segs[0][1]), segs[0][2], fields.ptr(k))
                    else:
                        rc = _add(lib, q, fam, flow, segs, fields.ptr(k), mode == "zc", lambda g, o: base[g] + o)
                    _lib.check("add", rc)
                if r % 2:
                    _lib.check("submit", lib.pipck_txq_submit(q))
                    _lib.check("complete", lib.pipck_txq_complete(q))
                else:
                    _lib.check("flush", lib.pipck_txq_flush(q))
                fields.check(dict(enumerate(want)), ("thread", t, "round", r, mode))
                if t == 0:
                    p, seq = hp.thread_rx_round(r)
                    _rx_verify(lib, rxq, places.pointers(seq), p.lens[seq], p.verdicts[seq], ("thread rx", r))
        except Exception as ex:  # noqa: BLE001  (reported by the test's thread)
            failures.append(f"thread {t}: {ex!r}")
        finally:
            if q:
                lib.pipck_txq_destroy(q)
            if rxq:
                lib.pipck_rxq_destroy(rxq)
            if ctx:
                lib.pipck_ctx_destroy(ctx)
            with lock:
                pools.extend(p for p in (own, places.base if places else None) if p)
                running[0] -= 1

    threads = [threading.Thread(target=work, args=(t,)) for t in range(hp.THREADS)]
    for th in threads:
        th.start()
    churned = 0
    while True:  # the registry's writers, for as long as the threads look ranges up
        with lock:
            if not running[0]:
                break
        p = lib.pipck_host_alloc(64 << 10)
        if not p or lib.pipck_host_free(C.c_void_p(p)) != _lib.PIPCK_OK:
            failures.append("the main thread's range: %r" % lib.pipck_last_error())
            break
        churned += 1
    for th in threads:
        th.join()
    freed = [lib.pipck_host_free(C.c_void_p(p)) for p in pools + [shared]]
    assert not failures, failures[:8]
    assert churned >= 1 and len(pools) == hp.THREADS + 1
    assert freed == [_lib.PIPCK_OK] * len(freed)
