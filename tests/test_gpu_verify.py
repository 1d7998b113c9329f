"""Every batch RX-verify kernel (the VERIFY instantiation of k_fixed, k_small,
k_flat, k_flat_coop, k_flat_small, k_flat_tiny, k_hdr, k_ragged, k_wave,
k_packed and k_packedb) held to tests/verify_reference.py.

The packets carry a correct checksum field (tests/verify_sealing.py: the
field's value comes from the CPU oracle, the flow tables from the host), some
are then damaged, and the expected verdict of every packet is the reference's
verdict of its final bytes -- so most verdicts are 1, which the comparisons of
tests/test_gpu_parity.py over random packets never see.  Every call writes
into a view of a buffer poisoned with 0xA5 and is checked for: the kernel that
ran, verdicts equal to the reference as uint8 (exactly 0 or 1), intact guard
bytes on both sides, and a zero error word.
"""
import ctypes as C
import itertools
import math
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pip_amd import _lib, engine  # noqa: E402
from tests import verify_sealing as vs  # noqa: E402
from tests.test_gpu_parity import (PACKEDB_SHAPES, _packed_case, _packed_lens, _packed_upload,  # noqa: E402
                                   _packedb_upload, _ragged_case, last_kernel, upload)

DEV = "cuda"
NF = 97        # flows per table: flow 0 all zero, flow 1 all 0xFF, the rest random
GUARD = 256    # poisoned bytes on each side of the verdicts
POISON = 0xA5

_CACHE: dict = {}  # sealed batches, shared by the launch shapes that verify them (never modified)


@pytest.fixture(scope="module", autouse=True)
def gpu():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    engine.require_gpu()
    yield
    engine.tune()
    torch.cuda.synchronize()
    _CACHE.clear()


def _flows(fam):
    """(device pseudo-header bases, the reference's per-flow tuples) of family fam."""
    key = ("flows", fam)
    if key not in _CACHE:
        rec, table = vs.flow_table(np.random.default_rng(4000 + fam), fam, NF, 6 if fam == 4 else 17)
        _CACHE[key] = (engine.prepare_flows(fam, engine.flows_to_device(fam, rec), NF), table)
    return _CACHE[key]


def _pseudo_of(fam, flow_idx):
    if not fam:
        return lambda i: None
    table = _flows(fam)[1]
    return lambda i: table[int(flow_idx[i])]


def _seal(oracle, rng, host, offs, lens, pseudo_of):
    """Seal and damage `host` in place; returns (the sealed, undamaged copy, the
    reference's verdict per packet).  Asserts the condition on the inputs."""
    fields = vs.seal(host, offs, lens, pseudo_of, oracle, rng)
    sealed = host.copy()
    vs.damage(host, offs, lens, rng)
    want = vs.expected(host, offs, lens, pseudo_of)
    vs.check_mix(want, lens, fields)
    return sealed, want


def _check(call, want, kernel, shift=0, suffix=None):
    """One verify call into a poisoned buffer: call(ok, err) with ok a view
    `shift` bytes past a 256-byte boundary."""
    n = len(want)
    lo = GUARD + shift
    buf = torch.full((lo + n + GUARD,), POISON, dtype=torch.uint8, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    call(buf[lo:lo + n], err)
    name = last_kernel()
    assert kernel in name, (kernel, name)
    if suffix:
        assert name.split("(")[0].endswith(suffix), (suffix, name)
    got = buf.cpu().numpy()
    res = got[lo:lo + n]
    assert res.dtype == np.uint8 and want.dtype == np.uint8
    bad = np.nonzero(res != want)[0]
    assert bad.size == 0, (name, n, bad.size, bad[:8], res[bad[:8]], want[bad[:8]])
    assert (got[:lo] == POISON).all() and (got[lo + n:] == POISON).all(), name
    assert int(err.item()) == 0, name


# ----------------------------------------------------------------------------
# fixed stride
# ----------------------------------------------------------------------------
def _fixed(oracle, stride, length, n, fam, misalign=0, explicit=False):
    """A sealed-and-damaged fixed-stride batch (cached).  Implicit flows start at a
    non-zero origin.  With stride padding of at least 2 bytes and implicit flows,
    `extras` holds the sealed, undamaged batch with the two bytes past each packet
    zeroed, and the reference's verdicts for flow_origin + 1 and for length + 2."""
    key = ("fixed", stride, length, n, fam, misalign, explicit)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng([1, stride, length, n, fam, misalign, int(explicit)])
    host = rng.integers(0, 256, n * stride + 16, dtype=np.uint8)
    idx = np.arange(n, dtype=np.int64)
    offs, lens = idx * stride, np.full(n, length, dtype=np.int64)
    origin = int(rng.integers(1, 1 << 40))
    flow_idx = rng.integers(0, NF, n) if explicit else (origin + idx) % NF
    pseudo_of = _pseudo_of(fam, flow_idx)
    sealed, want = _seal(oracle, rng, host, offs, lens, pseudo_of)
    b = SimpleNamespace(stride=stride, length=length, n=n, fam=fam, origin=0 if explicit else origin,
                        pseudo=_flows(fam)[0] if fam else None,
                        flow_of=torch.from_numpy(flow_idx.astype(np.int32)).to(DEV) if explicit else None,
                        arena=upload(host, misalign)[1], want=want, extras=None)
    if stride - length >= 2 and not explicit:
        sealed[(offs[:, None] + length + np.arange(2)).ravel()] = 0
        want_next = vs.expected(sealed, offs, lens, _pseudo_of(fam, (origin + 1 + idx) % NF))
        want_long = vs.expected(sealed, offs, lens + 2, pseudo_of)
        # the two zero bytes leave the sum alone; a pseudo-header's length term does not
        assert (want_long == (0 if fam else 1)).all() and (fam or want_next.all())
        b.extras = SimpleNamespace(arena=upload(sealed, misalign)[1], want_next=want_next, want_long=want_long)
    _CACHE[key] = b
    return b


def _verify_fixed(b, kernel, shift=0, long_kernel=None):
    def call(arena, length, origin):
        return lambda ok, err: engine.verify_fixed(arena, b.stride, length, b.n, b.pseudo, NF, b.flow_of, origin,
                                                   ok=ok, err=err)

    _check(call(b.arena, b.length, b.origin), b.want, kernel, shift)
    if b.extras:
        _check(call(b.extras.arena, b.length, b.origin + 1), b.extras.want_next, kernel, shift)
        _check(call(b.extras.arena, b.length + 2, b.origin), b.extras.want_long, long_kernel or kernel, shift)


FIXED_LENGTHS = [2, 3, 17, 33, 1025, 1480, 9217]


def _fixed_cases():
    """(stride, length, misalign, family): every length at the tight, the + 1 and a
    16-byte-multiple stride, each at every misalignment; the family rotates so that
    every (length, stride) and every (length, misalignment) sees all three."""
    for li, length in enumerate(FIXED_LENGTHS):
        for si, stride in enumerate((length, length + 1, (length + 15) // 16 * 16 + 16)):
            for mi, misalign in enumerate((0, 1, 13)):
                yield stride, length, misalign, (0, 4, 6)[(li + si + mi) % 3]


@pytest.mark.parametrize("lanes", [1, 4, 16, 64, 256])  # 256: k_wave, one packet per wave
def test_fixed_kernel(oracle, lanes):
    kernel = "k_wave<" if lanes == 256 else f"k_fixed<{lanes},"
    engine.tune(lanes)
    try:
        for stride, length, misalign, fam in _fixed_cases():
            n = 67 if length > 9000 else (131 if length > 1000 else 300)
            _verify_fixed(_fixed(oracle, stride, length, n, fam, misalign), kernel)
        _verify_fixed(_fixed(oracle, 1488, 1480, 131, 6, 13, explicit=True), kernel)
    finally:
        engine.tune()


def _small_fits(misalign, stride, length):
    """launch_fixed's test for k_small: the packet and the largest in-chunk offset
    of a packet start fit 4 chunks."""
    g = math.gcd(stride, 16)
    return (misalign % g + 16 - g + length + 15) // 16 <= 4


@pytest.mark.parametrize("misalign", [0, 1, 13])
def test_small_kernel(oracle, misalign):
    """k_small: every length 2..49 at tight, odd, 8- and 16-aligned strides, batches of
    one packet and around one block.  flat_tiny / flat_small off: with an aligned arena
    the 8- and 16-byte-multiple strides would take the row streams."""
    engine.tune(flat_tiny=False, flat_small=False)
    try:
        k = 0
        for length in range(2, 50):
            for stride in sorted({length, length + 1, length + 3, (length + 7) // 8 * 8, (length + 15) // 16 * 16,
                                  24 if length <= 24 else length}):
                n, fam = (1, 255, 256, 257)[k % 4], (0, 4, 6)[k // 4 % 3]
                k += 1
                assert _small_fits(misalign, stride, length)
                longer = "k_small<" if _small_fits(misalign, stride, length + 2) else "k_fixed<"
                _verify_fixed(_fixed(oracle, stride, length, n, fam, misalign), "k_small<", long_kernel=longer)
        _verify_fixed(_fixed(oracle, 24, 20, 1001, 4, misalign, explicit=True), "k_small<")
    finally:
        engine.tune()


def _tiny_run(stride, rows):
    """Packets per wave task of k_flat_tiny (mirrors launch_fixed)."""
    hpp = stride // 8
    odd, pow2 = hpp, 1
    while odd % 2 == 0:
        odd, pow2 = odd // 2, pow2 * 2
    G = odd * max(1, pow2 // 2)
    P = G * 128 // hpp
    return max(1, min(2048 // P, (rows or 12) // G)) * P


@pytest.mark.parametrize("ring,rows,nt", [(0, 0, True), (4, 4, True), (16, 64, True), (8, 2, False), (16, 8, True)])
def test_flat_tiny_kernel(oracle, ring, rows, nt):
    """k_flat_tiny (8-byte-multiple strides up to 64 B; at 64 B with flat_small off):
    batches around one wave task and a capped grid that loops, verdict arrays 4-byte
    aligned (vector stores) and one byte off.  The 128-B stride is past the kernel's
    range and reaches k_flat_small, pinned as such."""
    try:
        for stride in (8, 24, 40, 64, 128):
            run = _tiny_run(stride, rows)
            lengths = sorted({2, min(20, stride), stride - 1, stride})
            cases = list(zip(itertools.cycle(lengths), (run - 1, run, run + 1, 3 * run + 5))) + [(stride, 1)]
            for k, (length, n) in enumerate(cases):
                fam = (0, 4, 6)[(k + stride // 8) % 3]
                if not fam and stride == 24 and ring in (8, 16):
                    fam = 4  # bare 24-byte items with a forced ring of 8 / 16 are k_hdr's
                engine.tune(0, ring, 1 if n > 2 * run else 0, plain_loads=not nt, nt_loads=nt, rows_per_task=rows,
                            force_flat_tiny=True, flat_small=stride > 64)
                tiny_ring = ring if ring in (8, 16) else 4
                kernel = "k_flat_small<16, true," if stride > 64 else f"k_flat_tiny<{tiny_ring}, true,"
                for shift in (0, 1):
                    _verify_fixed(_fixed(oracle, stride, length, n, fam), kernel, shift=shift)
        engine.tune(0, ring, 0, plain_loads=not nt, nt_loads=nt, rows_per_task=rows, force_flat_tiny=True)
        _verify_fixed(_fixed(oracle, 24, 20, 2003, 6, explicit=True), "k_flat_tiny<")
    finally:
        engine.tune()


@pytest.mark.parametrize("blocks", [0, 1, 9])
def test_flat_small_kernel(oracle, blocks):
    """k_flat_small (aligned arena, 16-byte-multiple strides from 64 B to under 1 KiB):
    full, odd and chunk-short packets, one and several blocks, a capped grid.  The
    16- and 48-B strides are below its range: a verify call takes k_flat_tiny there,
    pinned as such.  A 1-byte packet (stride 16, length stride - 15) has no checksum
    field to carry, so that length is left to the parity tests."""
    engine.tune(blocks=blocks)
    try:
        k = 0
        for stride in (16, 48, 80, 144, 496, 1008):
            for length in (stride, stride - 1, stride - 15):
                if length < 2:
                    continue
                n, fam = (65, 1000, 3301)[k % 3], (0, 4, 6)[(k + k // 3) % 3]
                k += 1
                kernel = "k_flat_small<16, true," if stride >= 64 else "k_flat_tiny<4, true,"
                _verify_fixed(_fixed(oracle, stride, length, n, fam), kernel)
        _verify_fixed(_fixed(oracle, 96, 90, 2001, 6, explicit=True), "k_flat_small<")
    finally:
        engine.tune()


FLAT_CASES = [(1024, 1024), (1024, 1023), (1040, 1025), (1504, 1480), (2048, 17), (9216, 8980), (65536, 65535)]


def _flat_batch(oracle, ci):
    """Batches of a few block tasks that end short (389 = 2 x 192 + 5 at 1 KiB); the
    1,504-B one carries explicit flow indices."""
    stride, length = FLAT_CASES[ci]
    n = 11 if stride > 20000 else (97 if stride > 4096 else 389)
    return _fixed(oracle, stride, length, n, (4, 0, 6, 4, 6, 0, 6)[ci], explicit=ci == 3)


FLAT_ARMS = [(r, nt, xcd, "") for r in (2, 3, 9, 33) for nt in (False, True) for xcd in (False, True)] + \
    [(9, True, False, "plain"), (2, False, True, "plain"), (33, True, True, "wave"), (3, False, False, "wave")]


@pytest.mark.parametrize("rows,nt,xcd,stores", FLAT_ARMS)
def test_flat_kernel(oracle, rows, nt, xcd, stores):
    """k_flat at every row depth (plain and ring-pipelined), load policy and XCD deal,
    uncapped and capped grids; the plain-store and wave-store arms of the verdicts."""
    try:
        for ci, (stride, _) in enumerate(FLAT_CASES):
            b = _flat_batch(oracle, ci)
            for blocks in (0, 1, 9):
                engine.tune(0, rows, blocks, plain_loads=not nt, nt_loads=nt, xcd_groups=xcd,
                            alt_flat_schedule=stride not in (1024, 2048), plain_result_stores=stores == "plain",
                            wave_stores=stores == "wave")
                _verify_fixed(b, f"k_flat<{rows // 2 * 2}, {'true' if rows % 2 else 'false'}, true,")
    finally:
        engine.tune()


@pytest.mark.parametrize("ring,rows,plain", [(g, r, False) for g in (17, 25, 33) for r in (0, 2, 96)] +
                         [(33, 0, True), (17, 2, True)])
def test_flat_coop_kernel(oracle, ring, rows, plain):
    """k_flat_coop: every ring, tiny, default and large block tasks (8 to 256 packets),
    the last task of every batch cut short; the plain-store arm."""
    try:
        for ci, (stride, _) in enumerate(FLAT_CASES):
            engine.tune(0, ring, 0, rows_per_task=rows, alt_flat_schedule=stride in (1024, 2048),
                        plain_result_stores=plain)
            _verify_fixed(_flat_batch(oracle, ci), f"k_flat_coop<{ring - 1}, true,")
    finally:
        engine.tune()


@pytest.mark.parametrize("stride", [20, 24])
@pytest.mark.parametrize("ring,rows", [(32, 0), (8, 1), (33, 0), (17, 3)])
def test_hdr_kernel(oracle, stride, ring, rows):
    """k_hdr: 20-byte headers at both strides, one task per wave and the block-cooperative
    row order; batches ending inside a row and around a wave and a block task; verdict
    arrays at 16-byte alignment (vector stores) and off it."""
    engine.tune(0, ring, 0, rows_per_task=rows)
    try:
        pr = 48 if stride == 20 else 42  # headers per row
        ns = {1, 47, 48, 49}
        for per in ((rows or 32) * pr, (rows or 64) * pr):  # the kernel's wave task; the parity test's
            ns |= {per - 1, per, per + 1, 4 * per + 7}
        ns = sorted(ns)
        for k, n in enumerate(ns):
            b = _fixed(oracle, stride, 20, n, 0)
            for shift in (0, 1, 5, 15) if n == ns[-1] else ((0, 1, 5, 15)[k % 4],):
                _verify_fixed(b, f"k_hdr<{stride // 4}, {ring // 8 * 8}, true,", shift=shift)
    finally:
        engine.tune()


# ----------------------------------------------------------------------------
# ragged (descriptors)
# ----------------------------------------------------------------------------
def _tiny_segment_layout(rng):
    """The layout of test_ragged_tiny_segment_tiles: tiles of 0..16-byte segments at
    16-byte slots, tiles of 0..49 bytes at random offsets, a tile of long segments."""
    n = 64 * 30 + 17
    lens = rng.integers(0, 50, n).astype(np.int64)
    tiny = np.arange(n) < 64 * 12
    lens[tiny] = rng.integers(0, 17, int(tiny.sum()))
    lens[64 * 5:64 * 5 + 3] = 16
    lens[64 * 20:64 * 21] = rng.integers(0, 3000, 64)
    lens[64 * 22 + 3] = 65535
    offs = np.zeros(n, dtype=np.int64)
    pos = 0
    for i in range(n):
        pos = (pos + 15) // 16 * 16 if tiny[i] else pos + int(rng.integers(0, 20))
        offs[i] = pos
        pos += int(lens[i])
    return offs, lens, pos


def _ragged(oracle, kind, misalign, fam):
    """A sealed-and-damaged descriptor batch (cached).  "ragged": _ragged_case (permuted,
    gaps, lengths to 3000) plus one 65,535-byte segment; "packed": _packed_case;
    "tiny": the tiny-segment layout."""
    key = ("ragged", kind, misalign, fam)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng([2, ["ragged", "packed", "tiny"].index(kind), misalign, fam])
    if kind == "ragged":
        offs, lens, size = _ragged_case(rng, 64 * 23 + 5, 3000)
        at = int(rng.integers(0, len(lens)))
        offs, lens = np.insert(offs.astype(np.int64), at, size + 3), np.insert(lens.astype(np.int64), at, 65535)
        size += 3 + 65535
    elif kind == "packed":
        offs, lens, size = _packed_case(rng, 64 * 12 + 9)
        offs, lens = offs.astype(np.int64), lens.astype(np.int64)
    else:
        offs, lens, size = _tiny_segment_layout(rng)
    n = len(lens)
    host = rng.integers(0, 256, size + 64, dtype=np.uint8)
    origin = int(rng.integers(1, 1 << 20))
    flow_idx = (origin + np.arange(n)) % NF
    _, want = _seal(oracle, rng, host, offs, lens, _pseudo_of(fam, flow_idx))
    b = SimpleNamespace(n=n, arena=upload(host, misalign)[1], desc=engine.make_desc(offs, lens, flow_idx),
                        pseudo=_flows(fam)[0] if fam else None, want=want)
    _CACHE[key] = b
    return b


def _verify_ragged(b, kernel, suffix=None):
    _check(lambda ok, err: engine.verify_ragged(b.arena, b.desc, b.pseudo, ok=ok, err=err), b.want, kernel,
           suffix=suffix)


@pytest.mark.parametrize("rows", [2, 3, 9, 17, 33])
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("xcd", [False, True])
def test_ragged_launch_shapes(oracle, rows, wide, xcd):
    """k_ragged at plain and pipelined row depths, 1- and 4-wave blocks, with and without
    XCD groups, grids of 1 and 9 blocks and the uncapped one; arena misaligned by 0 and 7."""
    try:
        for misalign, fam in ((0, 4), (7, 6)):
            b = _ragged(oracle, "ragged", misalign, fam)
            for blocks in (1, 9, 0):
                engine.tune(0, rows, blocks, xcd_groups=xcd, wide_blocks=wide)
                _verify_ragged(b, "k_ragged<", suffix=f", {4 if wide else 1}u>")
    finally:
        engine.tune()


@pytest.mark.parametrize("rows", [0, 4, 9, 33])
@pytest.mark.parametrize("packed", [True, False])
def test_ragged_packed_tiles(oracle, rows, packed):
    """Tiles packed at 16-byte granularity (and tiles broken on purpose), through the
    packed-tile path and with it off; with and without a pseudo-header."""
    engine.tune(0, rows, packed_tiles=packed)
    try:
        for fam in (4, 0):
            _verify_ragged(_ragged(oracle, "packed", 0, fam), "k_ragged<")
    finally:
        engine.tune()


@pytest.mark.parametrize("misalign", [0, 3, 8])
@pytest.mark.parametrize("tiny", [True, False])
def test_ragged_tiny_segment_tiles(oracle, misalign, tiny):
    engine.tune(tiny_tiles=tiny)
    try:
        _verify_ragged(_ragged(oracle, "tiny", misalign, 4), "k_ragged<")
    finally:
        engine.tune()


@pytest.mark.parametrize("nl", [0, 2, 16])
def test_ragged_wave_arm(oracle, nl):
    """k_wave on descriptors: one packet per wave, several passes per packet."""
    engine.tune(256, nl)
    try:
        for kind, misalign, fam in (("ragged", 0, 4), ("ragged", 7, 6), ("tiny", 3, 0)):
            _verify_ragged(_ragged(oracle, kind, misalign, fam), "k_wave<")
    finally:
        engine.tune()


# ----------------------------------------------------------------------------
# packed layouts (lengths + a per-64 index)
# ----------------------------------------------------------------------------
FLOW_MODES = [(4, False), (6, True), (0, False)]  # implicit flows from an origin, explicit indices, no pseudo-header


def _packed(oracle, layout, shape, n, fam, explicit):
    """A sealed-and-damaged batch in the 16-byte packed ("p16") or the byte-packed
    ("bytes") layout (cached).  Below 64 packets, packet 0 has at least 2 bytes."""
    key = ("packed", layout, shape, n, fam, explicit)
    if key in _CACHE:
        return _CACHE[key]
    shapes = ["tiny", "short", "mixed", "edge", "jumbo", "sixteen"]
    rng = np.random.default_rng([3, layout == "bytes", shapes.index(shape), n, fam])
    if shape == "sixteen":  # the smallest lengths the byte-packed chunk stream takes
        lens = rng.choice([16, 17, 18, 31, 32, 33, 47], n).astype(np.uint32)
    else:
        lens = _packed_lens(rng, shape, n)
    if n < 64 and lens[0] < 2:
        lens[0] = 2
    host, offs, arena, lens16, index = (_packed_upload if layout == "p16" else _packedb_upload)(rng, lens)
    origin = int(rng.integers(1, 1 << 40))
    flow_idx = rng.integers(0, NF, n) if explicit else (origin + np.arange(n)) % NF
    _, want = _seal(oracle, rng, host, offs.astype(np.int64), lens.astype(np.int64), _pseudo_of(fam, flow_idx))
    arena.copy_(torch.from_numpy(host))  # the upload helper copied the bytes before they were sealed
    b = SimpleNamespace(n=n, arena=arena, lens16=lens16, index=index, origin=0 if explicit else origin,
                        pseudo=_flows(fam)[0] if fam else None, want=want,
                        flow_of=torch.from_numpy(flow_idx.astype(np.int32)).to(DEV) if explicit else None)
    _CACHE[key] = b
    return b


PACKED_CASES = [(s, n) for s in ("tiny", "short", "mixed", "edge") for n in (1, 63, 64, 65, 1000)] + [("jumbo", 5)]


@pytest.mark.parametrize("shape,n", PACKED_CASES)
def test_packed_kernel(oracle, shape, n):
    """k_packed: both mixed-row paths and rings of 16 and 32 rows; implicit flows,
    explicit flow indices, no pseudo-header."""
    try:
        for fam, explicit in FLOW_MODES:
            b = _packed(oracle, "p16", shape, n, fam, explicit)
            for marks, ring in itertools.product((False, True), (17, 33)):
                engine.tune(0, ring, packed_marks_only=marks)
                _check(lambda ok, err: engine.verify_packed(b.arena, b.lens16, b.index, n, b.pseudo, NF, b.flow_of,
                                                            b.origin, ok=ok, err=err),
                       b.want, f"k_packed<true, {ring - 1},")
    finally:
        engine.tune()


@pytest.mark.parametrize("tile_waves", [1, 4, 8])
@pytest.mark.parametrize("shape,n", PACKED_CASES + [("sixteen", n) for n in (1, 63, 64, 65, 1000)])
def test_packed_bytes_kernel(oracle, shape, n, tile_waves):
    """k_packedb at 1, 4 and 8 waves per tile: packets at every byte alignment, so the
    checksum field's two bytes sit at odd addresses and split across chunks."""
    engine.tune(loads_per_lane=PACKEDB_SHAPES[tile_waves])
    try:
        for fam, explicit in FLOW_MODES:
            b = _packed(oracle, "bytes", shape, n, fam, explicit)
            _check(lambda ok, err: engine.verify_packed_bytes(b.arena, b.lens16, b.index, n, b.pseudo, NF, b.flow_of,
                                                              b.origin, ok=ok, err=err),
                   b.want, "k_packedb<", suffix=f", {tile_waves}>")
    finally:
        engine.tune()


# ----------------------------------------------------------------------------
# the plain (unbounded) entry points, which the engine never calls
# ----------------------------------------------------------------------------
def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def test_plain_entry_points(oracle):
    lib = _lib.load()
    stream = engine.current_stream()
    engine.tune()

    def run(fn, *args):
        _lib.check(fn, getattr(lib, fn)(*args))

    for ci in (2, 3):  # implicit flows; explicit flow indices (n_flows is then unused: 0)
        b = _flat_batch(oracle, ci)
        _check(lambda ok, err: run("pipck_verify_fixed", _p(b.arena), b.stride, b.length, b.n, _p(b.pseudo),
                                   0 if b.flow_of is not None else NF, _p(b.flow_of), b.origin, _p(ok), stream),
               b.want, "k_flat_coop<")
    r = _ragged(oracle, "ragged", 7, 6)
    _check(lambda ok, err: run("pipck_verify_ragged", _p(r.arena), _p(r.desc), r.n, _p(r.pseudo), _p(ok), _p(err),
                               stream), r.want, "k_ragged<")
    for layout, fn, kernel in (("p16", "pipck_verify_packed", "k_packed<"),
                               ("bytes", "pipck_verify_packed_bytes", "k_packedb<")):
        for fam, explicit in FLOW_MODES:
            p = _packed(oracle, layout, "mixed", 1000, fam, explicit)
            _check(lambda ok, err: run(fn, _p(p.arena), _p(p.lens16), _p(p.index), p.n, _p(p.pseudo),
                                       0 if explicit else NF, _p(p.flow_of), p.origin, _p(ok), stream),
                   p.want, kernel)
