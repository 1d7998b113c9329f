"""Every kernel at saturated sums and wide indices (tests/saturation_cases.py):
arenas whose every byte -- gaps, stride padding and the bytes around the packets
included -- is 0xFF, or 0xFF with about one byte in 64 replaced, so that each
accumulator runs at its largest value and a wrong mask adds the largest value
there is; chains of 65,536 to 70,001 segments; flow origins around 2^32 and
2^64; packed indices past 2^32.

Every call goes through a bounded (_n) entry point into a view of a buffer
poisoned with 0xA5 and is checked for: the kernel that ran, results equal to the
reference's, intact guard bytes on both sides, and a zero error word.  All inputs
are inside the documented domain.  Expected values are Python-integer arithmetic
(tests/saturation_cases.py, pinned to pip by tests/test_saturation_reference.py).

Two entry points launch kernels whose names pipck_last_launch does not record
(k_chain_finish after the chain partials of k_ragged, and k_update_fixed): the
chain cases assert the k_ragged instantiation that feeds k_chain_finish, the
update cases have one kernel to run.
"""
import ctypes as C
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pip_amd import _lib, engine  # noqa: E402
from tests import rx_reference as R  # noqa: E402
from tests import saturation_cases as sc  # noqa: E402
from tests import tx_reference as T  # noqa: E402
from tests.test_gpu_parity import PACKEDB_SHAPES, last_kernel  # noqa: E402
from tests.test_gpu_rx import RING_KERNELS, _ring_schedule, _run, _rxq  # noqa: E402
from tests.test_gpu_verify import _tiny_run  # noqa: E402

DEV = "cuda"
NF = sc.NF
GUARD = 256
POISON = 0xA5
LEAD = 16  # bytes of fill before packet 0 and after the last packet

_CACHE: dict = {}


@pytest.fixture(scope="module", autouse=True)
def gpu():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    engine.require_gpu()
    yield
    engine.tune()
    torch.cuda.synchronize()
    _CACHE.clear()


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _drop(*kinds):
    """Forget the cached batches of these kinds (their device and host memory)."""
    for key in [k for k in _CACHE if k[0] in kinds]:
        del _CACHE[key]


def _flows(fam):
    """Device pseudo-header bases of family fam's 97-flow table."""
    return _cached(("flows", fam),
                   lambda: engine.prepare_flows(fam, engine.flows_to_device(fam, sc.flows(fam)[0]), NF))


def _upload(host: np.ndarray, lead: int = 0, misalign: int = 0):
    """A device copy of host with host[lead] `misalign` bytes past a 256-byte boundary; returns the
    view from there to host's end (the bytes before it stay in the allocation)."""
    start = 256 + misalign - lead
    t = torch.zeros(start + host.size + 64, dtype=torch.uint8, device=DEV)
    t[start:start + host.size].copy_(torch.from_numpy(host))
    assert t.data_ptr() % 256 == 0
    return t[256 + misalign:start + host.size]


def _check(call, want: np.ndarray, kernel, suffix=None):
    """call(out, err) with out a view inside a poisoned buffer (int16 for checksums, uint8 for
    verdicts): the kernel's name, the results, the guard bytes and the error word."""
    n, size = len(want), want.dtype.itemsize
    buf = torch.full((GUARD + n * size + GUARD,), POISON, dtype=torch.uint8, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    view = buf[GUARD:GUARD + n * size]
    call(view if size == 1 else view.view(torch.int16), err)
    name = last_kernel()
    if kernel is not None:
        assert kernel in name, (kernel, name)
    if suffix:
        assert name.split("(")[0].endswith(suffix), (suffix, name)
    got = buf.cpu().numpy()
    res = got[GUARD:GUARD + n * size].view(want.dtype)
    bad = np.nonzero(res != want)[0]
    assert bad.size == 0, (name, n, bad.size, bad[:8].tolist(), res[bad[:8]].tolist(), want[bad[:8]].tolist())
    assert (got[:GUARD] == POISON).all() and (got[GUARD + n * size:] == POISON).all(), name
    assert int(err.item()) == 0, name


# ----------------------------------------------------------------------------
# fixed stride
# ----------------------------------------------------------------------------
def _fixed_hosts(fill, stride, length, n, fam, origin=0, nf=NF):
    def make():
        host, at, want = sc.fixed_batch(fill, stride, length, n, fam, origin, nf)
        sealed, at2, ok = sc.sealed_fixed_batch(fill, stride, length, n, fam, origin, nf)
        assert at == at2 == LEAD
        return host, want, sealed, ok
    return _cached(("fixed", fill, stride, length, n, fam, origin, nf), make)


def _run_fixed(fill, stride, length, n, fam, misalign, kernel, origin=0, nf=NF, verify_kernel=None, keep=True):
    """Checksum and verify one saturated batch under the tuning in force."""
    host, want, sealed, ok = _fixed_hosts(fill, stride, length, n, fam, origin, nf)
    key = ("fixed_dev", fill, stride, length, n, fam, origin, nf, misalign)
    dev = _CACHE.get(key) or (_upload(host, LEAD, misalign), _upload(sealed, LEAD, misalign))
    if keep:
        _CACHE[key] = dev
    pseudo = _flows(fam)[:nf] if fam else None
    _check(lambda out, err: engine.checksum_fixed(dev[0], stride, length, n, pseudo, nf, None, origin, out=out,
                                                  err=err), want, kernel)
    _check(lambda o, err: engine.verify_fixed(dev[1], stride, length, n, pseudo, nf, None, origin, ok=o, err=err),
           ok, verify_kernel or kernel)


# (kernel, stride, arena misalignment, tuning): each kernel that takes 64 KiB packets, at its largest shape
JUMBO_SHAPES = [
    ("k_fixed<", 65535, 0, {}),
    ("k_fixed<", 65536, 1, {}),
    ("k_flat_coop<", 65536, 0, {}),
    ("k_flat<", 65536, 0, dict(alt_flat_schedule=True)),
    ("k_flat<", 65552, 0, {}),
    ("k_wave<", 65536, 0, dict(lanes_per_packet=256)),
]


@pytest.mark.parametrize("length", [65535, 65534])
@pytest.mark.parametrize("fill", sc.FILLS)
def test_fixed_jumbo(fill, length):
    """70 packets (one 64-packet boundary, a short last task) of 65,535 / 65,534 saturated bytes."""
    try:
        for kernel, stride, misalign, tune in JUMBO_SHAPES:
            engine.tune(**tune)
            for fam in (0, 4, 6):
                _run_fixed(fill, stride, length, 70, fam, misalign, kernel, origin=5)
    finally:
        engine.tune()
        _drop("fixed", "fixed_dev")


def _short_shapes():
    """(kernel, stride, length, n, families, tuning): every short-packet kernel at its own largest
    shape, n covering two full tasks and a remainder."""
    tiny = _tiny_run(64, 0)
    hdr = 32 * 42  # headers per wave task of k_hdr at 24-byte items
    return [
        # k_small: 4 chunks hold the packet and the largest in-chunk start offset (15): 49 bytes
        ("k_small<", 49, 49, 2 * 256 + 37, (0, 4, 6), {}),
        ("k_small<", 51, 49, 2 * 256 + 37, (0, 4, 6), {}),
        ("k_flat_small<", 1008, 1008, 2 * 260 + 37, (0, 4, 6), {}),
        ("k_flat_small<", 1008, 1007, 2 * 260 + 37, (0, 4, 6), {}),
        # k_flat_tiny's range ends at 64-byte strides; with it forced, 128 bytes reach k_flat_small
        ("k_flat_tiny<", 64, 64, 3 * tiny + 5, (0, 4, 6), dict(force_flat_tiny=True, flat_small=False)),
        ("k_flat_tiny<", 64, 63, 3 * tiny + 5, (0, 4, 6), dict(force_flat_tiny=True, flat_small=False)),
        ("k_flat_small<", 128, 128, 2 * 2048 + 37, (0, 4, 6), dict(force_flat_tiny=True)),
        ("k_hdr<6, 32,", 24, 20, 2 * 4 * hdr + 77, (0,), dict(loads_per_lane=32)),
        ("k_flat<", 1024, 1024, 389, (0, 4, 6), {}),
        ("k_flat<", 1024, 1023, 389, (0, 4, 6), {}),
        ("k_flat_coop<", 1024, 1024, 389, (0, 4, 6), dict(alt_flat_schedule=True)),
        ("k_flat_coop<", 1040, 1040, 389, (0, 4, 6), {}),
        ("k_flat_coop<", 1040, 1025, 389, (0, 4, 6), {}),
        ("k_flat<", 1040, 1040, 389, (0, 4, 6), dict(alt_flat_schedule=True)),
    ]


@pytest.mark.parametrize("fill", sc.FILLS)
def test_fixed_short(fill):
    try:
        for kernel, stride, length, n, fams, tune in _short_shapes():
            engine.tune(**tune)
            for fam in fams:
                _run_fixed(fill, stride, length, n, fam, 0, kernel, origin=7, keep=False)
    finally:
        engine.tune()
        _drop("fixed")


# ----------------------------------------------------------------------------
# ragged
# ----------------------------------------------------------------------------
RAGGED_SHAPES = [("k_ragged<", ", 1u>", {}), ("k_ragged<", ", 4u>", dict(wide_blocks=True)),
                 ("k_ragged<", ", 1u>", dict(packed_tiles=False)), ("k_wave<", None, dict(lanes_per_packet=256))]


@pytest.mark.parametrize("fam", [4, 6, 0])
@pytest.mark.parametrize("fill", sc.FILLS)
def test_ragged_jumbo(fill, fam):
    """64 x 3 + 1 descriptors of 65,535 and 65,534 bytes, each run of 16 starting at every offset
    0..15 mod 16."""
    n = 64 * 3 + 1
    idx = np.arange(n, dtype=np.int64)
    offs = LEAD + idx * 65552 + idx * 7 % 16
    lens = np.where(idx // 16 % 2 == 0, 65535, 65534).astype(np.int64)
    assert {(int(o) % 16, int(ln)) for o, ln in zip(offs, lens)} >= {(r, ln) for r in range(16) for ln in (65535, 65534)}
    flow_idx = sc.flow_indices(11, n, NF)
    ps = sc.pseudo_of(fam, flow_idx)
    size = LEAD + n * 65552 + LEAD
    host = sc.arena(fill, size, fam, 2)
    want = sc.batch(host, offs, lens, ps)
    sealed = sc.arena(fill, size, fam, 3)
    sc.seal_last_word(sealed, offs, lens, ps)
    sc.damage(sealed, offs, lens, [fam, 4])
    ok = sc.verdicts(sealed, offs, lens, ps)
    assert 100 <= int(ok.sum()) < n
    if fill == "dented":
        assert sc.distinct_per_tile(want) >= 32
    arena, arena_v = _upload(host), _upload(sealed)
    desc = engine.make_desc(offs, lens, flow_idx)
    pseudo = _flows(fam) if fam else None
    try:
        for kernel, suffix, tune in RAGGED_SHAPES:
            engine.tune(**tune)
            _check(lambda out, err: engine.checksum_ragged(arena, desc, pseudo, out=out, err=err), want, kernel, suffix)
            _check(lambda o, err: engine.verify_ragged(arena_v, desc, pseudo, ok=o, err=err), ok, kernel, suffix)
    finally:
        engine.tune()


# ----------------------------------------------------------------------------
# packed and byte-packed
# ----------------------------------------------------------------------------
def _packed_lengths(pattern, n):
    if pattern == "mix":
        lens = np.where(np.random.default_rng(n).random(n) < 0.5, 65535, 0)
        lens[0], lens[1], lens[-1] = 0, 65535, 65535
        return lens.astype(np.int64)
    return np.full(n, int(pattern), dtype=np.int64)


FLOW_MODES = ("implicit", "explicit", "none")


def _packed_batches(layout, pattern, n, fill, fam, mode):
    """(arena, sealed arena, lens16, flow_of, origin, expected checksums, expected verdicts)."""
    lens = _packed_lengths(pattern, n)
    unit = lens if layout == "bytes" else (lens + 15) // 16 * 16
    offs = LEAD + np.concatenate([[0], np.cumsum(unit)[:-1]])
    size = LEAD + (int(unit.sum()) + 15) // 16 * 16 + LEAD
    origin = 0 if mode != "implicit" else (1 << 40) + 77
    if mode == "explicit":
        flow_idx = np.random.default_rng([n, fam]).integers(0, NF, n)
    else:
        flow_idx = sc.flow_indices(origin, n, NF)
    ps = sc.pseudo_of(fam if mode != "none" else 0, flow_idx)
    host = sc.arena(fill, size, n, fam, 5)
    want = sc.batch(host, offs, lens, ps)
    sealed = sc.arena(fill, size, n, fam, 6)
    sc.seal_last_word(sealed, offs, lens, ps)
    sc.damage(sealed, offs, lens, [n, fam, 7])
    ok = sc.verdicts(sealed, offs, lens, ps)
    assert 0 < int(ok.sum()) < n
    lens16 = torch.from_numpy(lens.astype(np.uint16).view(np.int16)).to(DEV)
    flow_of = torch.from_numpy(flow_idx.astype(np.int32)).to(DEV) if mode == "explicit" else None
    return _upload(host, LEAD), _upload(sealed, LEAD), lens16, flow_of, origin, want, ok


@pytest.mark.parametrize("pattern", ["65535", "65534", "mix"])
@pytest.mark.parametrize("n", [64, 129])
def test_packed_jumbo(n, pattern):
    """k_packed: whole tiles of 4,096-chunk packets, every ring."""
    lens = _packed_lengths(pattern, n)
    try:
        for fill in sc.FILLS:
            for fam, mode in zip((4, 6, 4), FLOW_MODES):
                arena, arena_v, lens16, flow_of, origin, want, ok = _packed_batches("p16", pattern, n, fill, fam, mode)
                index = engine.packed_index(lens16)
                chunks = np.concatenate([[0], np.cumsum((lens + 15) // 16)])
                assert np.array_equal(index.cpu().numpy(), np.append(chunks[:-1][::64], chunks[-1]))
                pseudo = _flows(fam) if mode != "none" else None
                for ring in (17, 25, 33):
                    engine.tune(0, ring)
                    _check(lambda out, err: engine.checksum_packed(arena, lens16, index, n, pseudo, NF, flow_of, origin,
                                                                   out=out, err=err),
                           want, f"k_packed<false, {ring - 1},")
                    _check(lambda o, err: engine.verify_packed(arena_v, lens16, index, n, pseudo, NF, flow_of, origin,
                                                               ok=o, err=err),
                           ok, f"k_packed<true, {ring - 1},")
    finally:
        engine.tune()


@pytest.mark.parametrize("pattern", ["65535", "65534", "mix"])
@pytest.mark.parametrize("n", [64, 129])
def test_packed_bytes_jumbo(n, pattern):
    """k_packedb at 1, 4 and 8 waves per tile; with 65,535-byte packets every second one starts on
    an odd address."""
    lens = _packed_lengths(pattern, n)
    try:
        for fill in sc.FILLS:
            for fam, mode in zip((6, 4, 6), FLOW_MODES):
                arena, arena_v, lens16, flow_of, origin, want, ok = _packed_batches("bytes", pattern, n, fill, fam,
                                                                                   mode)
                index = engine.packed_bytes_index(lens16)
                total = np.concatenate([[0], np.cumsum(lens)])
                assert np.array_equal(index.cpu().numpy(), np.append(total[:-1][::64], total[-1]))
                pseudo = _flows(fam) if mode != "none" else None
                for waves in (1, 4, 8):
                    engine.tune(loads_per_lane=PACKEDB_SHAPES[waves])
                    _check(lambda out, err: engine.checksum_packed_bytes(arena, lens16, index, n, pseudo, NF, flow_of,
                                                                         origin, out=out, err=err),
                           want, "k_packedb<", f", {waves}>")
                    _check(lambda o, err: engine.verify_packed_bytes(arena_v, lens16, index, n, pseudo, NF, flow_of,
                                                                     origin, ok=o, err=err),
                           ok, "k_packedb<", f", {waves}>")
    finally:
        engine.tune()


# ----------------------------------------------------------------------------
# chains
# ----------------------------------------------------------------------------
CHAIN_KERNEL = "k_ragged<false,"  # the chain-partials instantiation; k_chain_finish follows it unrecorded


def _chain_call(arena, offs, lens, seg_begin, pkt_flow, fam):
    segs = engine.make_desc(np.asarray(offs, dtype=np.uint64), np.asarray(lens, dtype=np.uint32), np.zeros(len(offs)))
    begin = torch.tensor(seg_begin, dtype=torch.int64, device=DEV)
    flow = torch.from_numpy(np.asarray(pkt_flow, dtype=np.int32)).to(DEV) if fam else None
    pseudo = _flows(fam) if fam else None
    return lambda out, err: engine.checksum_chains(arena, segs, begin, flow, pseudo, out=out, err=err)


def _chain_expected(host, offs, lens, seg_begin, pkt_flow, fam):
    table = sc.flows(fam)[1] if fam else None
    return np.array([sc.chain_checksum(host, offs[a:b], lens[a:b], table[pkt_flow[p]] if fam else None)
                     for p, (a, b) in enumerate(zip(seg_begin[:-1], seg_begin[1:]))], dtype=np.uint16)


def _six_segment_case(fill, fam):
    """Case (a): 64 packets of six 65,535-byte saturated segments at odd and even starts."""
    n_pk = 64
    k = np.arange(n_pk * 6, dtype=np.int64)
    offs = (LEAD + k * 65540 + k % 3).tolist()
    lens = [65535] * len(offs)
    host = sc.arena(fill, LEAD + len(offs) * 65540 + LEAD, fam, 8)
    seg_begin = list(range(0, len(offs) + 1, 6))
    pkt_flow = np.random.default_rng([fam, 9]).integers(0, NF, n_pk).tolist()
    pkt_flow[0], pkt_flow[1] = 0, 1
    return host, offs, lens, seg_begin, pkt_flow


@pytest.mark.parametrize("fam", [4, 6, 0])
@pytest.mark.parametrize("fill", sc.FILLS)
def test_chains_six_saturated_segments(fill, fam):
    host, offs, lens, seg_begin, pkt_flow = _six_segment_case(fill, fam)
    want = _chain_expected(host, offs, lens, seg_begin, pkt_flow, fam)
    _check(_chain_call(_upload(host), offs, lens, seg_begin, pkt_flow, fam), want, CHAIN_KERNEL)


def _many_segment_case(fam, flow):
    """Case (b): packets of 65,536, 65,537, 65,538 and 70,001 FF FF segments (alternately at even and
    odd addresses), each between ordinary packets of three random segments."""
    rng = np.random.default_rng([fam, flow, 10])
    blob, offs, lens, seg_begin, pkt_flow = bytearray(rng.integers(0, 256, LEAD, dtype=np.uint8).tobytes()), [], [], [0], []

    def ordinary():
        for ln in (int(rng.integers(1, 3000)), 20, int(rng.integers(0, 9))):
            blob.extend(rng.integers(0, 256, int(rng.integers(0, 4)), dtype=np.uint8).tobytes())
            offs.append(len(blob))
            lens.append(ln)
            blob.extend(rng.integers(0, 256, ln, dtype=np.uint8).tobytes())
        seg_begin.append(len(offs))
        pkt_flow.append(int(rng.integers(0, NF)))

    ordinary()
    for k, count in enumerate(sc.CHAIN_COUNTS):
        blob.extend(bytes(1 + (len(blob) + k) % 2))  # a zero byte or two: the run starts at an even, then an odd address
        base = len(blob)
        blob.extend(b"\xff" * (2 * count))
        offs.extend(range(base, base + 2 * count, 2))
        lens.extend([2] * count)
        seg_begin.append(len(offs))
        pkt_flow.append(flow)
        ordinary()
    blob.extend(bytes(LEAD))
    return np.frombuffer(bytes(blob), dtype=np.uint8), offs, lens, seg_begin, pkt_flow


MANY_FLOWS = [(0, 0), (4, 1), (4, 50), (6, 1), (6, 50), (4, 0)]  # (family, flow of the long chains)


@pytest.mark.parametrize("fam,flow", MANY_FLOWS)
def test_chains_of_65536_to_70001_segments(fam, flow):
    """pip folds after every segment; so must the finish step.  On the parent of this test's commit
    the 65,537-, 65,538- and 70,001-segment packets came back one too high (a u32 sum of the
    segments' folded sums wrapped); the ordinary packets between them must not change either."""
    host, offs, lens, seg_begin, pkt_flow = _many_segment_case(fam, flow)
    want = _chain_expected(host, offs, lens, seg_begin, pkt_flow, fam)
    if not fam:
        assert [int(want[i]) for i in (1, 3, 5, 7)] == [0, 0, 0, 0]
    _check(_chain_call(_upload(host), offs, lens, seg_begin, pkt_flow, fam), want, CHAIN_KERNEL)


@pytest.mark.parametrize("fill", sc.FILLS)
def test_chain_of_65538_descriptors_of_one_region(fill):
    """Case (c): 65,538 descriptors of the same 65,535 saturated bytes; total_len wraps to 65,534."""
    n = 65538
    host = sc.arena(fill, LEAD + 65535 + 1 + LEAD, 11)
    offs, lens = [LEAD + 1] * n + [LEAD, LEAD + 7], [65535] * n + [40, 1]
    seg_begin, pkt_flow = [0, n, n + 2], [60, 61]
    for fam in (4, 6, 0):
        want = _chain_expected(host, offs, lens, seg_begin, pkt_flow, fam)
        _check(_chain_call(_upload(host), offs, lens, seg_begin, pkt_flow, fam), want, CHAIN_KERNEL)


def _txq_checksums(host, offs, lens, seg_begin, pkt_flow, fam, in_place):
    """The packets through pipck_txq_add4 / add6 + flush: the big-endian fields the queue stored."""
    lib = _lib.load()
    ctx, q = C.c_void_p(), C.c_void_p()
    _lib.check("pipck_ctx_create", lib.pipck_ctx_create(-1, C.byref(ctx)))
    _lib.check("pipck_txq_create", lib.pipck_txq_create(ctx, C.byref(q)))
    n_pk = len(seg_begin) - 1
    fields = (C.c_uint8 * (2 * n_pk + 2 * GUARD))(*([POISON] * (2 * n_pk + 2 * GUARD)))
    data = np.ascontiguousarray(host)
    base = data.ctypes.data
    table = sc.flows(fam)[1]
    try:
        if not in_place:
            _lib.check("pipck_txq_inplace_max", lib.pipck_txq_inplace_max(q, 0))
        for p in range(n_pk):
            a, b = seg_begin[p], seg_begin[p + 1]
            raw = np.zeros(max(b - a, 1), dtype=[("ptr", "<u8"), ("len", "<u4"), ("pad", "<u4")])
            raw["ptr"][:b - a] = base + np.asarray(offs[a:b], dtype=np.uint64)
            raw["len"][:b - a] = lens[a:b]
            assert raw.dtype.itemsize == C.sizeof(_lib.HSeg)
            arr = C.cast(raw.ctypes.data, C.POINTER(_lib.HSeg))
            _, src, dst, proto = table[pkt_flow[p]]
            field = C.c_void_p(C.addressof(fields) + GUARD + 2 * p)
            if fam == 4:
                _lib.check("add4", lib.pipck_txq_add4(q, arr, b - a, proto, int.from_bytes(src, "little"),
                                                      int.from_bytes(dst, "little"), field))
            else:
                _lib.check("add6", lib.pipck_txq_add6(q, arr, b - a, proto, src, dst, field))
        _lib.check("pipck_txq_flush", lib.pipck_txq_flush(q))
        name = last_kernel()
    finally:
        lib.pipck_txq_destroy(q)
        lib.pipck_ctx_destroy(ctx)
    assert CHAIN_KERNEL in name, name
    got = np.frombuffer(bytes(fields), dtype=np.uint8)
    assert (got[:GUARD] == POISON).all() and (got[GUARD + 2 * n_pk:] == POISON).all()
    return got[GUARD:GUARD + 2 * n_pk].view(">u2").astype(np.uint16)


@pytest.mark.parametrize("in_place", [True, False])
@pytest.mark.parametrize("fam", [4, 6])
def test_txq_saturated_and_long_chains(fam, in_place):
    """Cases (a) and (b) through the deferred TX queue, which ends in the same finish kernel."""
    for case in (_six_segment_case("dented", fam), _six_segment_case("ff", fam), _many_segment_case(fam, 1),
                 _many_segment_case(fam, 50)):
        host, offs, lens, seg_begin, pkt_flow = case
        want = _chain_expected(host, offs, lens, seg_begin, pkt_flow, fam)
        got = _txq_checksums(host, offs, lens, seg_begin, pkt_flow, fam, in_place)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (bad.tolist(), got[bad].tolist(), want[bad].tolist(),
                               [seg_begin[i + 1] - seg_begin[i] for i in bad])


# ----------------------------------------------------------------------------
# RX verdicts and TX fill
# ----------------------------------------------------------------------------
def _frames(fill, sealed):
    """65,535-byte frames whose L4 message is all fill: TCP, UDP and ICMP over IPv4 with IHL 5 and
    15; TCP, UDP and ICMPv6 over IPv6, bare and behind two extension headers."""
    rng = random.Random(65535)
    out = []
    for fam, proto, options, chain in [(4, p, o, None) for p in (R.TCP, R.UDP, R.ICMP) for o in (0, 40)] + \
            [(6, p, 0, c) for p in (R.TCP, R.UDP, R.ICMP6) for c in (None, [(R.HOPOPTS, 0), (R.DSTOPTS, 1)])]:
        ext = R.ext_chain(chain, proto) if chain else None
        head = (20 + options) if fam == 4 else 40 + (len(ext[0]) if ext else 0)
        l4 = sc.arena(fill, 65535 - head, fam, proto, options).tobytes()
        f = R.build(rng, fam, proto, 0, options=rng.randbytes(options), ext=ext, l4=l4, fill=sealed)
        assert len(f) == 65535
        out.append(f)
    return out


def _rx_set(fill):
    """(frames, reference verdicts): every frame sealed, then with one bit of its L4 message flipped."""
    def make():
        rng = random.Random(7)
        frames = []
        for f in _frames(fill, True):
            a, b = R.l4_range(f)
            q = bytearray(f)
            q[rng.randrange(a, b)] ^= 1 << rng.randrange(8)
            frames += [f, bytes(q)]
        want = np.array([R.verdict(f) for f in frames], dtype=np.uint8)
        assert (want[0::2] == R.VERIFIED).all() and (want[1::2] == (R.IP_OK | R.L4_CHECKED)).all()
        return frames, want
    return _cached(("rx", fill), make)


def _packed_frames(frames):
    blob = np.frombuffer(b"".join(frames) + bytes(32), dtype=np.uint8)
    arena = _upload(blob)
    lens = torch.from_numpy(np.array([len(f) for f in frames], dtype=np.uint16).view(np.int16)).to(DEV)
    return arena, lens, engine.packed_bytes_index(lens)


@pytest.mark.parametrize("waves", [4, 2, 1])
@pytest.mark.parametrize("fill", sc.FILLS)
def test_rx_verify_device_saturated(fill, waves):
    """pipck_rx_verify_device at each block width k_packedb_rx has (4, 2 and 1 waves per tile)."""
    frames, want = _rx_set(fill)
    arena, lens, index = _packed_frames(frames)
    engine.tune(loads_per_lane={4: 0, 2: 28, 1: 32}[waves])
    try:
        _check(lambda ok, err: engine.rx_verify_device(arena, lens, index, ok=ok, err=err), want, "k_packedb_rx<",
               f", {waves}>")
    finally:
        engine.tune()


@pytest.mark.parametrize("schedule", ["groups", "own", "coop", "rows", "slots"])
@pytest.mark.parametrize("fill", sc.FILLS)
def test_rx_verify_ring_saturated(fill, schedule):
    """pipck_rx_verify_ring_n with 64 KiB slots, the ring's feedback off as in the dispatch table."""
    frames, want = _rx_set(fill)
    stride = 65536
    buf = sc.arena(fill, len(frames) * stride + LEAD, 12)  # the byte after each frame, too, is fill
    for i, f in enumerate(frames):
        buf[i * stride:i * stride + len(f)] = np.frombuffer(f, dtype=np.uint8)
    ring = _upload(buf)
    lens = torch.from_numpy(np.array([len(f) for f in frames], dtype=np.uint16).view(np.int16)).to(DEV)
    _ring_schedule(schedule)
    try:
        _check(lambda ok, err: engine.rx_verify_ring(ring, stride, lens, len(frames), ok=ok, err=err), want,
               RING_KERNELS[schedule])
    finally:
        engine.tune()


@pytest.mark.parametrize("fill", sc.FILLS)
def test_rx_verify_host_paths_saturated(fill):
    """pipck_rx_verify (frames in host memory) and pipck_host_rx_verify_packed."""
    frames, want = _rx_set(fill)
    lib, q = _rxq()
    try:
        bufs = [C.create_string_buffer(f, len(f)) for f in frames]
        got = _run(lib, q, [C.cast(b, C.c_void_p).value for b in bufs], [len(f) for f in frames]).copy()
    finally:
        lib.pipck_rxq_destroy(q)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    blob = np.frombuffer(b"".join(frames) + bytes(32), dtype=np.uint8).copy()
    lens = np.array([len(f) for f in frames], dtype=np.uint16)
    ok = np.full(len(frames) + 2 * GUARD, POISON, dtype=np.uint8)
    good = C.c_uint64(99)
    ctx = C.c_void_p()
    assert lib.pipck_ctx_create(-1, C.byref(ctx)) == 0
    try:
        rc = lib.pipck_host_rx_verify_packed(ctx, blob.ctypes.data, lens.ctypes.data, len(frames),
                                             ok.ctypes.data + GUARD, C.byref(good))
        assert rc == 0, lib.pipck_last_error()
    finally:
        lib.pipck_ctx_destroy(ctx)
    assert "k_packedb_rx<" in last_kernel()
    assert np.array_equal(ok[GUARD:-GUARD], want), (ok[GUARD:-GUARD].tolist(), want.tolist())
    assert (ok[:GUARD] == POISON).all() and (ok[-GUARD:] == POISON).all()
    assert good.value == int((want == R.VERIFIED).sum())


@pytest.mark.parametrize("flags", [0, engine.TX_UDP_ZERO_AS_ONES])
@pytest.mark.parametrize("fill", sc.FILLS)
def test_tx_fill_saturated(fill, flags):
    """The same frames with their checksum fields unfilled through pipck_tx_fill_device: the whole
    arena and the done bytes equal tx_reference.fill's."""
    frames = _frames(fill, False)
    filled = [T.fill(f, flags) for f in frames]
    tail = sc.arena(fill, 256, 13).tobytes()  # after the last frame: must come back unchanged
    want_arena = np.frombuffer(b"".join(f for f, _ in filled) + tail, dtype=np.uint8)
    want_done = np.array([d for _, d in filled], dtype=np.uint8)
    assert (want_done & engine.TX_L4_FILLED).all()
    arena = _upload(np.frombuffer(b"".join(frames) + tail, dtype=np.uint8))
    lens = torch.from_numpy(np.array([len(f) for f in frames], dtype=np.uint16).view(np.int16)).to(DEV)
    index = engine.packed_bytes_index(lens)
    _check(lambda done, err: engine.tx_fill_device(arena, lens, index, flags=flags, done=done, err=err), want_done,
           "k_packedb_tx<")
    got = arena.cpu().numpy()
    bad = np.nonzero(got != want_arena)[0]
    assert bad.size == 0, (bad[:8].tolist(), got[bad[:8]].tolist(), want_arena[bad[:8]].tolist())
    # and what was filled in verifies (UDP over IPv4 whose checksum computed to 0 and was sent as "none": unchecked)
    assert all(R.verdict(f) in (R.VERIFIED, R.UNCHECKED) for f, _ in filled)


# ----------------------------------------------------------------------------
# incremental update
# ----------------------------------------------------------------------------
def _update_case(fill, cover_len, edit_len, fam, nat):
    """70 packets at stride 65,536, checksum field in the first word, the edit right after it.
    Rows 0..3 are zero outside the field (the scan of the 0x0000 / 0xFFFF corner), rows 4..7 are
    built so that the NEW sum is a multiple of 0xFFFF."""
    n, stride, ck_off, edit_off = 70, 65536, 0, 2
    rng = np.random.default_rng([cover_len, edit_len, fam, int(nat), 14])
    host = sc.arena(fill, LEAD + n * stride + LEAD, cover_len, edit_len, fam, 15)
    offs = LEAD + np.arange(n, dtype=np.int64) * stride
    new = np.full((n, edit_len), 0xFF, dtype=np.uint8)
    new[1::2] = sc.arena("dented", n * edit_len, 16).reshape(n, edit_len)[1::2]
    for i in range(4):
        host[offs[i]:offs[i] + cover_len] = 0
        new[i] = 0
    new[1, 0], new[3, :2] = 0x80, 0xFF
    old_tab, new_tab = (sc.flows(fam)[1], sc.flows(fam)[1][::-1] if nat else sc.flows(fam)[1]) if fam else (None, None)
    flow_idx = sc.flow_indices(3, n, NF)
    ps_old = (lambda i: old_tab[flow_idx[i]]) if fam else (lambda i: None)
    ps_new = (lambda i: new_tab[flow_idx[i]]) if fam else (lambda i: None)
    for i in range(4, 8):  # one word of the kept bytes brings the new sum to a multiple of 0xFFFF
        pkt = host[offs[i]:offs[i] + cover_len].copy()
        pkt[edit_off:edit_off + edit_len] = new[i]
        pkt[ck_off:ck_off + 2] = 0
        at = (cover_len - 2) & ~1
        if at >= edit_off + edit_len:
            pkt[at:at + 2] = 0
            c = sc.checksum(pkt, ps_new(i))
            host[offs[i] + at], host[offs[i] + at + 1] = c >> 8, c & 0xFF
    for i in range(n):  # the old packets carry pip's checksum
        o = int(offs[i])
        host[o + ck_off:o + ck_off + 2] = 0
        c = sc.checksum(host[o:o + cover_len], ps_old(i))
        host[o + ck_off], host[o + ck_off + 1] = c >> 8, c & 0xFF
    want = host.copy()
    for i in range(n):  # full recomputation by the reference
        o = int(offs[i])
        want[o + edit_off:o + edit_off + edit_len] = new[i]
        want[o + ck_off:o + ck_off + 2] = 0
        c = sc.checksum(want[o:o + cover_len], ps_new(i))
        want[o + ck_off], want[o + ck_off + 1] = c >> 8, c & 0xFF
    del rng
    return host, want, new, (n, stride, ck_off, edit_off), (old_tab, new_tab)


def _rev_flows(fam):
    """Device bases of family fam's table in reverse order (the "new" table of a rewrite)."""
    def make():
        rec = sc.flows(fam)[0]
        size = len(rec) // NF
        rev = b"".join(rec[k * size:(k + 1) * size] for k in reversed(range(NF)))
        return engine.prepare_flows(fam, engine.flows_to_device(fam, rev), NF)
    return _cached(("rev", fam), make)


@pytest.mark.parametrize("fam,nat", [(0, False), (4, True), (6, True), (4, False)])
@pytest.mark.parametrize("cover_len", [65535, 65534])
@pytest.mark.parametrize("fill", sc.FILLS)
def test_update_saturated(fill, cover_len, fam, nat):
    """pipck_update_fixed_n: an edit of 2 bytes and the largest even edit the cover allows, without
    and with old / new pseudo-header tables; the whole arena equals a full recomputation."""
    for edit_len in (2, (cover_len - 2) & ~1):
        host, want, new, (n, stride, ck_off, edit_off), _ = _update_case(fill, cover_len, edit_len, fam, nat)
        ck = want[LEAD:LEAD + n * stride].reshape(n, stride)[:, :2]
        if not fam:
            assert (ck[[0, 2]] == 0xFF).all()  # all-zero packets: pip stores 0xFFFF
        assert any((ck[i] == 0).all() for i in range(4, 8)) or edit_len > 2  # a new sum of k x 0xFFFF: 0x0000
        arena = _upload(host, LEAD)
        new_d = torch.from_numpy(new.reshape(-1).copy()).to(DEV)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        p_old = _flows(fam) if fam else None
        p_new = (_rev_flows(fam) if nat else p_old) if fam else None
        engine.update_fixed(arena, stride, n, 0, cover_len, ck_off, edit_off, edit_len, new_d, edit_len, p_old, p_new,
                            NF if fam else None, None, 3, err=err)
        got = arena.cpu().numpy()
        bad = np.nonzero(got != want[LEAD:])[0]
        assert bad.size == 0, (edit_len, (bad[:8] // stride).tolist(), (bad[:8] % stride).tolist(),
                               got[bad[:8]].tolist(), want[LEAD:][bad[:8]].tolist())
        assert int(err.item()) == 0


# ----------------------------------------------------------------------------
# wide indices
# ----------------------------------------------------------------------------
WIDE_SHAPES = [  # (kernel, stride, length, tuning): every fixed-stride kernel family that takes a pseudo-header
    ("k_fixed<", 101, 100, {}),
    ("k_small<", 35, 34, {}),
    ("k_flat<", 1024, 1000, {}),
    ("k_flat_coop<", 1040, 1040, {}),
    ("k_flat_small<", 144, 130, {}),
    ("k_flat_tiny<", 24, 20, {}),
    ("k_wave<", 101, 100, dict(lanes_per_packet=256)),
]


@pytest.mark.parametrize("origin", sc.FLOW_ORIGINS, ids=[hex(o) for o in sc.FLOW_ORIGINS])
def test_wide_flow_origin_fixed(origin):
    """Implicit flows ((flow_origin + i) mod 2^64) mod n_flows through every fixed-stride kernel.
    On the parent of this test's commit k_flat took the low 32 bits' remainder for the packets of
    a task whose flow_origin + p0 + 64 wrapped past 2^64 (n_flows 3, 65 and 97 differ)."""
    try:
        for kernel, stride, length, tune in WIDE_SHAPES:
            engine.tune(**tune)
            # a batch that crosses 2^64 is launched as the packets before the wrap and those from it on;
            # the name is the second launch's, whose arena starts to_wrap strides in: off the 16-byte
            # grid that k_flat_tiny needs, 24-byte items go to k_small
            to_wrap = (1 << 64) - origin
            if kernel == "k_flat_tiny<" and to_wrap < 300 and to_wrap * stride % 16:
                kernel = "k_small<"
            for nf in sc.FLOW_COUNTS:
                fam = 4 if nf % 2 else 6
                _run_fixed("dented", stride, length, 300, fam, 0, kernel, origin=origin, nf=nf, keep=False)
    finally:
        engine.tune()
        _drop("fixed")


@pytest.mark.parametrize("origin", sc.FLOW_ORIGINS, ids=[hex(o) for o in sc.FLOW_ORIGINS])
def test_wide_flow_origin_packed_and_update(origin):
    n = 300
    lens = np.random.default_rng(17).integers(0, 200, n).astype(np.int64)
    lens[:4] = (0, 1, 2, 199)
    for nf in sc.FLOW_COUNTS:
        fam = 6 if nf % 2 else 4
        flow_idx = sc.flow_indices(origin, n, nf)
        ps = sc.pseudo_of(fam, flow_idx)
        pseudo = _flows(fam)[:nf]
        for layout in ("p16", "bytes"):
            unit = lens if layout == "bytes" else (lens + 15) // 16 * 16
            offs = LEAD + np.concatenate([[0], np.cumsum(unit)[:-1]])
            size = LEAD + (int(unit.sum()) + 15) // 16 * 16 + LEAD
            host = sc.arena("dented", size, 18)
            want = sc.batch(host, offs, lens, ps)
            sealed = host.copy()
            sc.seal_last_word(sealed, offs, lens, ps)
            sc.damage(sealed, offs, lens, [19])
            ok = sc.verdicts(sealed, offs, lens, ps)
            assert 100 < int(ok.sum()) < n
            arena, arena_v = _upload(host, LEAD), _upload(sealed, LEAD)
            lens16 = torch.from_numpy(lens.astype(np.uint16).view(np.int16)).to(DEV)
            if layout == "p16":
                index = engine.packed_index(lens16)
                ck, vf, kernel = engine.checksum_packed, engine.verify_packed, "k_packed<"
            else:
                index = engine.packed_bytes_index(lens16)
                ck, vf, kernel = engine.checksum_packed_bytes, engine.verify_packed_bytes, "k_packedb<"
            _check(lambda out, err: ck(arena, lens16, index, n, pseudo, nf, None, origin, out=out, err=err), want,
                   kernel)
            _check(lambda o, err: vf(arena_v, lens16, index, n, pseudo, nf, None, origin, ok=o, err=err), ok, kernel)
        # pipck_update_fixed_n: 40 covered bytes at stride 64, the field at 16, an edit of the first 8 bytes
        stride, cover, ck_off = 64, 40, 16
        host = sc.arena("dented", LEAD + n * stride + LEAD, 20)
        offs = LEAD + np.arange(n, dtype=np.int64) * stride
        table = sc.flows(fam)[1]
        new_of = lambda i: table[(int(flow_idx[i]) + 1) % nf]  # noqa: E731  (the new table: the old one rotated)
        for i, o in enumerate(offs):
            host[o + ck_off:o + ck_off + 2] = 0
            c = sc.checksum(host[o:o + cover], ps(i))
            host[o + ck_off], host[o + ck_off + 1] = c >> 8, c & 0xFF
        new = sc.arena("dented", n * 8, 21).reshape(n, 8)
        want = host.copy()
        for i, o in enumerate(offs):
            want[o:o + 8] = new[i]
            want[o + ck_off:o + ck_off + 2] = 0
            c = sc.checksum(want[o:o + cover], new_of(i))
            want[o + ck_off], want[o + ck_off + 1] = c >> 8, c & 0xFF
        rec = sc.flows(fam)[0]
        size = len(rec) // NF
        rot = rec[size:nf * size] + rec[:size]
        p_new = engine.prepare_flows(fam, engine.flows_to_device(fam, rot), nf)
        arena = _upload(host, LEAD)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        engine.update_fixed(arena, stride, n, 0, cover, ck_off, 0, 8, torch.from_numpy(new.reshape(-1).copy()).to(DEV), 8,
                            pseudo, p_new, nf, None, origin, err=err)
        got = arena.cpu().numpy()
        bad = np.nonzero(got != want[LEAD:])[0]
        assert bad.size == 0, (nf, (bad[:8] // stride).tolist(), (bad[:8] % stride).tolist())
        assert int(err.item()) == 0


def _index_call(fn, lens16, entries):
    """One index builder into a poisoned int64 buffer; returns its entries."""
    buf = torch.full((GUARD + 8 * entries + GUARD,), POISON, dtype=torch.uint8, device=DEV)
    view = buf[GUARD:GUARD + 8 * entries].view(torch.int64)
    engine.call(fn, C.c_void_p(lens16.data_ptr()), lens16.numel(), C.c_void_p(view.data_ptr()),
                engine.current_stream(lens16.device))
    got = buf.cpu().numpy()
    assert (got[:GUARD] == POISON).all() and (got[GUARD + 8 * entries:] == POISON).all(), fn
    return got[GUARD:GUARD + 8 * entries].view(np.uint64)


def test_packed_bytes_index_past_2_to_the_32():
    """70,001 lengths of 65,535: 4.59e9 bytes, 1,094 tiles (two per scan thread, none for the last)."""
    n = 70001
    lens16 = torch.full((n,), -1, dtype=torch.int16, device=DEV)  # 0xFFFF
    got = _index_call("pipck_packed_bytes_index", lens16, (n + 63) // 64 + 1)
    total = np.concatenate([[0], np.cumsum(np.full(n, 65535, dtype=np.uint64))])
    want = np.append(total[:-1][::64], total[-1])
    assert int(want[-1]) == n * 65535 > 1 << 32
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]


def test_packed_index_chunk_count_past_2_to_the_32():
    """1,048,577 lengths of 65,535: 4,096 chunks each, 2^32 + 4,096 chunks in all."""
    n = (1 << 20) + 1
    lens16 = torch.full((n,), -1, dtype=torch.int16, device=DEV)
    got = _index_call("pipck_packed_index", lens16, (n + 63) // 64 + 1)
    total = np.concatenate([[0], np.cumsum(np.full(n, 4096, dtype=np.uint64))])
    want = np.append(total[:-1][::64], total[-1])
    assert int(want[-1]) == (1 << 32) + 4096
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
