"""pipck_fwd_classify_ring / pipck_fwd_classify_device (include/pipck.h, k_fwd_classify_ring and
k_fwd_classify_device in pip_amd/csrc/pipck_fwdcls.hip) against tests/fwd_classify_reference.py.
Every comparison is whole-buffer: d_rule_of and d_class inside poisoned buffers with 16 poisoned
elements on either side, and the arena -- the call is read-only -- byte for byte with what was
uploaded.  The frame sets, key sets and hand-made tables: tests/test_fwd_classify_reference.py.
No test provokes a fault: every planted bad index or length is one the call is specified to refuse."""
import functools
import random

import numpy as np
import pytest

from tests import fwd_classify_reference as K
from tests import fwd_reference as F
from tests import rx_reference as R
from tests.test_fwd_classify_reference import (TABLE_SLOTS, chain_table, classes, frame_of_key, frame_set,
                                               near_miss_tables, ordinary_table, wrap_table)
from tests.test_fwd_reference import rule_table
from tests.test_gpu_fwd_device import PAD, _padded_arena
from tests.test_gpu_fwd_ring import _structured
from tests.test_gpu_rx import _last_kernel
from tests.test_gpu_tx_fill import _blob, _device, _starts
from tests.test_tx_ring_cases import ring_image, ring_lens

pytestmark = pytest.mark.gpu

KERNELS = {"ring": "k_fwd_classify_ring", "packed": "k_fwd_classify_device"}
LAYOUTS = ("ring", "packed")
POISON, POISON32 = 0xEE, 0xEEEEEEEE
GUARD = 4096  # bytes of pattern behind a ring's last slot, inside the allocation
ERANGE_BIT = 1 << 2
MISS_RULE, OTHER_RULE = 3, 14  # the tests' defaults: all five ops on IPv4; DEC_TTL alone on either family
RULES = rule_table() + (F.rule(F.DEC_TTL, 0),)  # rule 14: what a router gives frames without a key
ENDS = (0, 63, 64, 255, 256)  # a wave's and a block's first and last frame; the batch's last is added per test


def _dev_table(table):
    """The table's bytes at the END of a device allocation, behind 1,024 bytes of pattern."""
    import torch

    raw = K.table_bytes(table)
    buf = torch.full((1024 + len(raw),), 0xA7, dtype=torch.uint8, device="cuda")
    buf[1024:] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to("cuda")
    t = buf[1024:].view(-1, 48)
    assert t.data_ptr() % 16 == 0 and t.data_ptr() + t.numel() == buf.data_ptr() + buf.numel()
    return t


@functools.lru_cache(maxsize=None)
def _class_of(frame):
    return K.frame_class(frame)


def _want(frames, table, miss_rule, other_rule, ok=None, ok_mask=3, refused=()):
    """(rule_of u32, class u8) by the reference; `refused`: indices the layout refuses."""
    rules, cls = np.empty(len(frames), dtype=np.uint32), np.empty(len(frames), dtype=np.uint8)
    refused = set(refused)
    for i, f in enumerate(frames):
        if i in refused:
            rules[i], cls[i] = K.NO_RULE, 0
        elif ok is not None and int(ok[i]) & ok_mask != ok_mask:
            rules[i], cls[i] = K.NO_RULE, K.PASSED
        else:
            c = _class_of(f)
            if c == K.MALFORMED:
                rules[i], cls[i] = K.NO_RULE, 0
            elif c == K.NO_KEY:
                rules[i], cls[i] = other_rule, K.UNKEYED
            else:
                r = K.lookup(table, c)
                rules[i], cls[i] = (miss_rule, K.MISS) if r is None else (r, K.HIT)
    return rules, cls


def _outputs(n):
    import torch

    rule_buf = torch.full((n + 32,), POISON32 - (1 << 32), dtype=torch.int32, device="cuda")
    cls_buf = torch.full((n + 32,), POISON, dtype=torch.uint8, device="cuda")
    return rule_buf, cls_buf, torch.zeros(1, dtype=torch.int32, device="cuda")


def _check_outputs(path, n, rule_buf, cls_buf, want_rules, want_cls, frames=None):
    """Both result buffers whole: 16 poisoned elements, the n results, 16 poisoned elements."""
    got_r = rule_buf.cpu().numpy().view(np.uint32)
    want_r = np.concatenate([np.full(16, POISON32, np.uint32), want_rules, np.full(16, POISON32, np.uint32)])
    if not np.array_equal(got_r, want_r):
        bad = np.nonzero(got_r != want_r)[0]
        i = int(bad[0]) - 16
        raise AssertionError(f"{path}: d_rule_of differs at {len(bad)} elements, first {i} of {n}: got "
                             f"{int(got_r[i + 16]):#x} want {int(want_r[i + 16]):#x}"
                             + (f" frame {frames[i][:96].hex()} length {len(frames[i])}" if frames and 0 <= i < n else ""))
    if cls_buf is not None:
        got_c = cls_buf.cpu().numpy()
        want_c = np.concatenate([np.full(16, POISON, np.uint8), want_cls, np.full(16, POISON, np.uint8)])
        if not np.array_equal(got_c, want_c):
            bad = np.nonzero(got_c != want_c)[0]
            i = int(bad[0]) - 16
            raise AssertionError(f"{path}: d_class differs at {len(bad)} elements, first {i} of {n}: got "
                                 f"{int(got_c[i + 16])} want {int(want_c[i + 16])}")


def _classify_and_check(path, layout, frames, table, miss_rule=MISS_RULE, other_rule=OTHER_RULE, ok=None, ok_mask=3,
                        stride=1024, with_cls=True, with_err=True, want=None, dev_table=None):
    """One call over a fresh upload of `frames` in `layout`, held to the reference whole-buffer;
    returns (rule_of tensor view, want rules, want classes)."""
    import torch

    from pip_amd import engine

    frames = list(frames)
    n = len(frames)
    rule_buf, cls_buf, err = _outputs(n)
    t = _dev_table(table) if dev_table is None else dev_table
    ok_t = None if ok is None else torch.from_numpy(np.asarray(ok, dtype=np.uint8)).to("cuda")
    kw = dict(n=n, miss_rule=miss_rule, other_rule=other_rule, ok=ok_t, ok_mask=ok_mask, rule_of=rule_buf[16:n + 16],
              cls=cls_buf[16:n + 16] if with_cls else None, err=err if with_err else None)
    if layout == "ring":
        img = ring_image(frames, stride, GUARD)
        arena = torch.from_numpy(img).to("cuda")
        got = engine.fwd_classify_ring(arena, stride, torch.from_numpy(ring_lens(frames)).to("cuda"), t, **kw)
    else:
        img = _blob(frames)
        arena, lens, tile_off = _device(frames)
        assert arena.data_ptr() % 128 == 0
        got = engine.fwd_classify_device(arena, lens, tile_off, t, **kw)
    assert KERNELS[layout] in _last_kernel(), _last_kernel()
    assert got.data_ptr() == rule_buf.data_ptr() + 64 and got.dtype == torch.int32
    want_rules, want_cls = want or _want(frames, table, miss_rule, other_rule, ok, ok_mask)
    _check_outputs(path, n, rule_buf, cls_buf if with_cls else None, want_rules, want_cls, frames)
    if not with_cls:
        assert bool((cls_buf == POISON).all())
    assert int(err.item()) == 0
    assert np.array_equal(arena.cpu().numpy(), img), f"{path}: the arena was written"
    return got, want_rules, want_cls


def _census(cls):
    return {v: int((cls == v).sum()) for v in (K.HIT, K.MISS, K.UNKEYED, 0)}


# ---------------------------------------------------------------------------- 1. the short set
@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_classify_short_set_behind_fillers(lead):
    """Frames of 20 to 51 bytes back to back, two or three frames' headers in one 16-byte chunk, the
    whole batch behind a filler of 0 to 3 bytes (version 2: malformed), so every frame meets every
    start residue; under every ordinary table size."""
    frames = ([bytes([0x25]) + bytes(lead - 1)] if lead else []) + list(frame_set("short"))
    for n_slots in TABLE_SLOTS:
        table = ordinary_table("short", n_slots)[2]
        _, _, cls = _classify_and_check(f"pipck_fwd_classify_device (short set, lead {lead}, {n_slots} slots)", "packed",
                                        frames, table)
        c = _census(cls)
        assert c[K.HIT] >= 1 and c[K.MISS] >= 1 and c[K.UNKEYED] == 20 and c[0] == 28 + bool(lead), c
        assert c[K.HIT] + c[K.MISS] == 144


def test_classify_short_set_in_a_ring():
    frames = frame_set("short")
    for n_slots in TABLE_SLOTS:
        _classify_and_check(f"pipck_fwd_classify_ring (short set, {n_slots} slots)", "ring", frames,
                            ordinary_table("short", n_slots)[2])


# ---------------------------------------------------------------------------- 2. the structured set
@pytest.mark.parametrize("stride", [1024, 9216, 65536])
def test_classify_structured_set_ring(stride):
    """Every class, IPv4 options at every IHL, extension chains around and past the window: every
    frame that fits the stride (at 65,536 the frames over 9,216 bytes and 64 others)."""
    frames = list(_structured(stride))
    _, _, cls = _classify_and_check(f"pipck_fwd_classify_ring (structured set, stride {stride})", "ring", frames,
                                    ordinary_table("structured", 4096)[2], stride=stride)
    if stride == 9216:
        far = [f for f in frames if isinstance(_class_of(f), bytes) and f[0] >> 4 == 6 and f[6] in (0, 60, 44)
               and len(f) > 200]
        assert far, "no key behind a long extension chain"
    c = _census(cls)
    assert stride == 65536 or (c[K.HIT] >= 100 and c[K.MISS] >= 100 and c[K.UNKEYED] >= 50 and c[0] >= 20), c


@pytest.mark.parametrize("n_slots", TABLE_SLOTS)
def test_classify_structured_set_packed(n_slots):
    frames = list(frame_set("structured"))
    assert len(frames) == 2983 and any(len(f) == 65535 for f in frames)
    _, _, cls = _classify_and_check(f"pipck_fwd_classify_device (structured set, {n_slots} slots)", "packed", frames,
                                    ordinary_table("structured", n_slots)[2])
    c = _census(cls)
    assert c[K.HIT] >= 1 and c[K.MISS] >= 1 and c[K.HIT] + c[K.MISS] == 2596 and c[K.UNKEYED] == 311 and c[0] == 76, c


# ---------------------------------------------------------------------------- 3. fuzz
@functools.lru_cache(maxsize=None)
def _fuzz_want(n_slots):
    return _want(frame_set("fuzz"), ordinary_table("fuzz", n_slots)[2], MISS_RULE, OTHER_RULE)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n_slots", [64, 4096])
def test_classify_mutation_fuzz(layout, n_slots):
    """The 20,000 mutated frames of the RX reference test and the planted-TTL frames."""
    frames = frame_set("fuzz")
    want = _fuzz_want(n_slots)
    c = _census(want[1])
    assert c[K.HIT] >= 30 and c[K.MISS] >= 1000 and c[K.HIT] + c[K.MISS] == 7273 and c[K.UNKEYED] == 11102 and \
        c[0] == 2465, c
    _classify_and_check(f"pipck_fwd_classify ({layout}, fuzz, {n_slots} slots)", layout, frames,
                        ordinary_table("fuzz", n_slots)[2], want=want)


# ---------------------------------------------------------------------------- 4. counts
@pytest.mark.parametrize("layout", LAYOUTS)
def test_classify_frame_counts(layout):
    """A lone frame, and partial last waves and blocks for a wave of 64 and a block of 256 frames."""
    rng = random.Random(257)
    pool = [f for f in frame_set("fuzz") if len(f) <= 1024]
    table = ordinary_table("fuzz", 4096)[2]
    for n in (1, 2, 63, 64, 65, 255, 256, 257):
        frames = [rng.choice(pool) for _ in range(n)]
        _classify_and_check(f"pipck_fwd_classify ({layout}, {n} frames)", layout, frames, table)


# ---------------------------------------------------------------------------- 5. the engine's table
def test_make_fwd_table_uploads_the_reference_bytes():
    from pip_amd import engine

    keys, rules, table = ordinary_table("structured", 4096)
    t = engine.make_fwd_table(keys, rules, 4096)
    assert tuple(t.shape) == (4096, 48) and t.data_ptr() % 16 == 0
    assert t.cpu().numpy().tobytes() == K.table_bytes(table)
    frames = list(frame_set("short")) + [frame_of_key(k) for k in keys[:100]]
    for layout in LAYOUTS:
        _, _, cls = _classify_and_check(f"pipck_fwd_classify ({layout}, make_fwd_table)", layout, frames, table,
                                        dev_table=t)
        assert _census(cls)[K.HIT] >= 100


# ---------------------------------------------------------------------------- 6. hand-made tables
@pytest.mark.parametrize("layout", LAYOUTS)
def test_classify_probe_chain_of_64_and_the_bound(layout):
    """64 slots filled by 64 keys of one home slot: hits at probes 1 to 64; a 65th key of that home
    is absent and no entry is empty, so its search ends at the bound of 64 probes."""
    keys, absent, table = chain_table()
    frames = [frame_of_key(k, bytes(i % 4)) for i, k in enumerate(keys)] + [frame_of_key(absent)] * 3 + \
        list(frame_set("short"))[:64]
    _, rules, cls = _classify_and_check(f"pipck_fwd_classify ({layout}, chain of 64)", layout, frames, table,
                                        miss_rule=0xABCD)
    assert rules[:64].tolist() == [100 + i for i in range(64)] and (cls[:64] == K.HIT).all()
    assert rules[64:67].tolist() == [0xABCD] * 3 and (cls[64:67] == K.MISS).all()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_classify_probe_chain_wraps_the_table_end(layout):
    keys, table = wrap_table()
    absent = chain_table()[1]
    frames = [frame_of_key(k) for k in keys] + [frame_of_key(absent)] + list(frame_set("short"))[:70]
    _, rules, cls = _classify_and_check(f"pipck_fwd_classify ({layout}, wrapping chain)", layout, frames, table)
    assert rules[:4].tolist() == [5, 6, 7, MISS_RULE] and cls[:4].tolist() == [K.HIT, K.HIT, K.HIT, K.MISS]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_classify_near_miss_entries(layout):
    """An entry with the key's tag whose key differs in one byte of src, dst, sport, dport, proto,
    family or pad, and one with the right key under a wrong tag: each a miss; the exact entry a hit
    whose rule is PIPCK_FWD_NO_RULE."""
    key, tables = near_miss_tables()
    frames = [frame_of_key(key, bytes(i)) for i in range(4)] + list(frame_set("short"))[:70]
    for name, table in tables.items():
        _, rules, cls = _classify_and_check(f"pipck_fwd_classify ({layout}, near miss in {name})", layout, frames, table)
        assert rules[:4].tolist() == [MISS_RULE] * 4 and (cls[:4] == K.MISS).all(), name
    exact = [None] * 16
    exact[K.key_hash(key) & 15] = (key, K.NO_RULE, K.key_hash(key) | 0x80000000)
    _, rules, cls = _classify_and_check(f"pipck_fwd_classify ({layout}, exact entry)", layout, frames, exact)
    assert rules[:4].tolist() == [K.NO_RULE] * 4 and (cls[:4] == K.HIT).all()


# ---------------------------------------------------------------------------- 7. miss_rule / other_rule
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("miss_rule,other_rule", [(K.NO_RULE, K.NO_RULE), (0, 0xFFFFFFFE), (K.NO_RULE, 14),
                                                  (0x80000000, K.NO_RULE)])
def test_classify_miss_and_other_rule(layout, miss_rule, other_rule):
    frames = frame_set("short")
    _, rules, cls = _classify_and_check(f"pipck_fwd_classify ({layout}, miss {miss_rule:#x}, other {other_rule:#x})",
                                        layout, frames, ordinary_table("short", 64)[2], miss_rule=miss_rule,
                                        other_rule=other_rule)
    assert (rules[cls == K.MISS] == miss_rule).all() and (rules[cls == K.UNKEYED] == other_rule).all()
    assert (cls == K.MISS).sum() >= 50 and (cls == K.UNKEYED).sum() == 20


# ---------------------------------------------------------------------------- 8. the verdict gate
def _hit_batch(n=2 * 256 + 7):
    """n shortest frames of bound keys (every one a hit), and their table."""
    keys, rules, table = ordinary_table("fuzz", 4096)
    rng = random.Random(8)
    frames = [frame_of_key(rng.choice(keys), bytes(rng.randrange(4))) for _ in range(n)]
    return frames, table


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("ok_mask", [0, 3, 7])
def test_classify_verdict_gate(layout, ok_mask):
    """Verdicts 0, 1, 3, 5 and 6 planted at a wave's and a block's first and last frame and at the
    batch's last frame among verified frames (7); every frame is one that would hit, so a gated
    frame that was classified all the same shows as a rule other than PIPCK_FWD_NO_RULE."""
    frames, table = _hit_batch()
    n = len(frames)
    ok = np.full(n, 7, dtype=np.uint8)
    for k, i in enumerate(ENDS + (n - 1,)):
        ok[i] = (0, 1, 3, 5, 6, 3)[k]
    _, rules, cls = _classify_and_check(f"pipck_fwd_classify ({layout}, gate, ok_mask {ok_mask})", layout, frames, table,
                                        ok=ok, ok_mask=ok_mask)
    passed = {0: 0, 3: 4, 7: 6}[ok_mask]
    assert int((cls == K.PASSED).sum()) == passed and int((cls == K.HIT).sum()) == n - passed
    assert (rules[cls == K.PASSED] == K.NO_RULE).all() and (rules[cls == K.HIT] != K.NO_RULE).all()


# ---------------------------------------------------------------------------- 9. refusals, 10. optional outputs
@pytest.mark.parametrize("with_cls,with_err", [(True, True), (False, True), (True, False), (False, False)])
def test_classify_ring_refuses_lengths_past_the_stride(with_cls, with_err):
    """Lengths of stride + 1, stride + 16 and 65,535 planted at wave, block and ring ends over
    slots that hold a frame that would hit: PIPCK_FWD_NO_RULE, class 0, PIPCK_ERANGE; every other
    slot as without the tampering.  d_class and d_err are optional."""
    import torch

    from pip_amd import engine

    frames, table = _hit_batch()
    n, stride = len(frames), 1024
    plants = ENDS + (n - 1,)
    lens = ring_lens(frames).view(np.uint16).copy()
    for k, i in enumerate(plants):
        lens[i] = (stride + 1, stride + 16, 65535)[k % 3]
    want_rules, want_cls = _want(frames, table, MISS_RULE, OTHER_RULE, refused=plants)
    assert (want_cls == K.HIT).sum() == n - len(plants)
    img = ring_image(frames, stride, GUARD)
    ring = torch.from_numpy(img).to("cuda")
    rule_buf, cls_buf, err = _outputs(n)
    engine.fwd_classify_ring(ring, stride, torch.from_numpy(lens.view(np.int16)).to("cuda"), _dev_table(table), n=n,
                             miss_rule=MISS_RULE, other_rule=OTHER_RULE, rule_of=rule_buf[16:n + 16],
                             cls=cls_buf[16:n + 16] if with_cls else None, err=err if with_err else None)
    assert KERNELS["ring"] in _last_kernel()
    _check_outputs("pipck_fwd_classify_ring (lengths past the stride)", n, rule_buf, cls_buf if with_cls else None,
                   want_rules, want_cls, frames)
    assert with_cls or bool((cls_buf == POISON).all())
    assert int(err.item()) == (ERANGE_BIT if with_err else 0)
    assert np.array_equal(ring.cpu().numpy(), img)


@pytest.mark.parametrize("with_cls,with_err", [(True, True), (False, False)])
@pytest.mark.parametrize("plant", ["tiles first, middle and last", "arena one byte short"])
def test_classify_device_bounded_by_the_arena(plant, with_cls, with_err):
    """A stale tile index (d_tile_off[t] = arena_bytes - 100 at the first, a middle and the last
    tile) and an arena_bytes one byte short of the batch: the frames of a refused tile get
    PIPCK_FWD_NO_RULE and class 0, PIPCK_ERANGE is set, every other tile is as in the clean run.
    arena_bytes is the batch's bytes; 128 KiB of pattern follow in the allocation.  The C ABI
    directly, no Python guard."""
    import torch

    from pip_amd import _lib, engine

    lib = _lib.load()
    frames, table = _hit_batch()
    n, tiles = len(frames), (len(frames) + 63) // 64
    starts = _starts(frames)
    refused = (0, 4, tiles - 1) if plant.startswith("tiles") else (tiles - 1,)
    assert all(int(starts[min(64 * (t + 1), n)] - starts[64 * t]) > 100 for t in refused)
    want_rules, want_cls = _want(frames, table, MISS_RULE, OTHER_RULE,
                                 refused=[i for t in refused for i in range(64 * t, min(64 * (t + 1), n))])
    arena, nbytes, img = _padded_arena(frames)
    lens_t = torch.from_numpy(ring_lens(frames)).to("cuda")
    tile_off = engine.packed_bytes_index(lens_t)
    assert int(tile_off[tiles].item()) == nbytes and arena.numel() == nbytes + PAD
    arena_bytes = nbytes
    if plant.startswith("tiles"):
        for t in refused:
            tile_off[t] = nbytes - 100
    else:
        arena_bytes = nbytes - 1
    rule_buf, cls_buf, err = _outputs(n)
    t = _dev_table(table)
    rc = lib.pipck_fwd_classify_device(arena.data_ptr(), arena_bytes, lens_t.data_ptr(), tile_off.data_ptr(), n,
                                       t.data_ptr(), t.shape[0], MISS_RULE, OTHER_RULE, None, 3,
                                       rule_buf.data_ptr() + 64, cls_buf.data_ptr() + 16 if with_cls else None,
                                       err.data_ptr() if with_err else None, None)
    assert rc == 0, lib.pipck_last_error()
    torch.cuda.synchronize()
    assert KERNELS["packed"] in _last_kernel()
    _check_outputs(f"pipck_fwd_classify_device ({plant})", n, rule_buf, cls_buf if with_cls else None, want_rules,
                   want_cls, frames)
    assert with_cls or bool((cls_buf == POISON).all())
    assert int(err.item()) == (ERANGE_BIT if with_err else 0)
    assert np.array_equal(arena.cpu().numpy(), img)


def test_classify_argument_errors_launch_nothing():
    import torch

    from pip_amd import _lib, engine

    lib = _lib.load()
    frames, table = _hit_batch(70)
    n = len(frames)
    arena, lens, tile_off = _device(frames)
    engine.rx_verify_device(arena, lens, tile_off)  # this thread's last recorded launch: no classify kernel
    last = _last_kernel()
    assert "k_fwd_classify" not in last
    t = _dev_table(table)
    rule_buf, cls_buf, err = _outputs(n)
    a, nb, ln, to, tb, ro = arena.data_ptr(), arena.numel(), lens.data_ptr(), tile_off.data_ptr(), t.data_ptr(), \
        rule_buf.data_ptr() + 64
    for args, why in (((None, nb, ln, to, n, tb, 4096, 0, 0, None, 3, ro, None, None, None), "null arena"),
                      ((a, nb, ln, None, n, tb, 4096, 0, 0, None, 3, ro, None, None, None), "null index"),
                      ((a, nb, ln, to, n, None, 4096, 0, 0, None, 3, ro, None, None, None), "null table"),
                      ((a, nb, ln, to, n, tb, 4096, 0, 0, None, 3, None, None, None, None), "null rule_of"),
                      ((a, nb, ln, to, n, tb, 4095, 0, 0, None, 3, ro, None, None, None), "4,095 slots"),
                      ((a, nb, ln, to, n, tb + 8, 2048, 0, 0, None, 3, ro, None, None, None), "misaligned table"),
                      ((a, nb, ln, to, n, tb, 4096, 0, 0, None, 8, ro, None, None, None), "ok_mask 8"),
                      ((a + 64, nb, ln, to, n, tb, 4096, 0, 0, None, 3, ro, None, None, None), "arena 64 mod 128")):
        assert lib.pipck_fwd_classify_device(*args) == _lib.PIPCK_EINVAL, why
        assert b"pipck_fwd_classify_device" in lib.pipck_last_error(), why
        assert _last_kernel() == last, why
    assert lib.pipck_fwd_classify_device(a, nb, ln, to, 0, tb, 4096, 0, 0, None, 3, ro, None, None, None) == _lib.PIPCK_OK
    assert _last_kernel() == last
    with pytest.raises(ValueError):
        engine.fwd_classify_device(arena, lens, tile_off, t.flatten())
    with pytest.raises(ValueError):
        engine.fwd_classify_device(arena, lens, tile_off, t, rule_of=rule_buf[:n - 1])
    with pytest.raises(ValueError):
        engine.fwd_classify_device(arena, lens, tile_off, t, ok=cls_buf[:n - 1])
    with pytest.raises(ValueError):
        engine.fwd_classify_ring(arena, 1024, lens, t, n=n)  # the arena is no ring of n slots
    torch.cuda.synchronize()
    assert _last_kernel() == last
    assert bool((rule_buf == POISON32 - (1 << 32)).all()) and bool((cls_buf == POISON).all())


# ---------------------------------------------------------------------------- 11. stream and graph
@pytest.mark.parametrize("layout", LAYOUTS)
def test_classify_on_a_side_stream_and_in_a_graph(layout):
    """The call on a side stream; then captured into a graph -- one kernel -- and the graph
    replayed twice over fresh contents copied to the same addresses (the second time other frames
    of the same lengths), each replay held to the reference."""
    import torch

    from pip_amd import engine

    rng = random.Random(77)
    pool = [f for f in frame_set("fuzz") if len(f) <= 1024]
    by_len = {}
    for f in pool:
        by_len.setdefault(len(f), []).append(f)
    frames_a = [rng.choice(pool) for _ in range(300)]
    frames_b = [rng.choice(by_len[len(f)]) for f in frames_a]
    assert sum(a != b for a, b in zip(frames_a, frames_b)) >= 100
    n, stride = 300, 1024
    table = ordinary_table("fuzz", 4096)[2]
    want = {"A": _want(frames_a, table, MISS_RULE, OTHER_RULE), "B": _want(frames_b, table, MISS_RULE, OTHER_RULE)}
    assert not np.array_equal(want["A"][0], want["B"][0])
    image = (lambda fr: ring_image(fr, stride, GUARD)) if layout == "ring" else (lambda fr: _blob(fr).copy())
    imgs = {"A": image(frames_a), "B": image(frames_b)}
    stage = {k: torch.from_numpy(v).to("cuda") for k, v in imgs.items()}
    arena = stage["A"].clone()
    lens = torch.from_numpy(ring_lens(frames_a)).to("cuda")
    tile_off = engine.packed_bytes_index(lens)
    t = _dev_table(table)
    rule_buf, cls_buf, err = _outputs(n)

    def call():
        kw = dict(n=n, miss_rule=MISS_RULE, other_rule=OTHER_RULE, rule_of=rule_buf[16:n + 16], cls=cls_buf[16:n + 16],
                  err=err)
        if layout == "ring":
            engine.fwd_classify_ring(arena, stride, lens, t, **kw)
        else:
            engine.fwd_classify_device(arena, lens, tile_off, t, **kw)

    def check(path, which):
        torch.cuda.synchronize()
        _check_outputs(path, n, rule_buf, cls_buf, *want[which])
        assert int(err.item()) == 0 and np.array_equal(arena.cpu().numpy(), imgs[which])

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    s.synchronize()
    assert KERNELS[layout] in _last_kernel()
    check(f"pipck_fwd_classify ({layout}, side stream)", "A")
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for k, which in enumerate(("A", "B")):
        arena.copy_(stage[which])
        rule_buf.fill_(POISON32 - (1 << 32))
        cls_buf.fill_(POISON)
        err.zero_()
        g.replay()
        check(f"pipck_fwd_classify ({layout}, graph replay {k}, contents {which})", which)


# ---------------------------------------------------------------------------- 12. the pipeline
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("ok_mask", [3, 7])
def test_verify_classify_rewrite_on_one_stream(layout, ok_mask):
    """rx_verify -> classify -> fwd_rewrite enqueued on one stream with no host work between them
    equals the composition of rx_reference.verdict, fwd_classify_reference.classify and
    fwd_reference.rewrite: verdicts, rule indices, classes, done bytes and the whole arena."""
    import torch

    from pip_amd import engine

    frames = list(frame_set("fuzz"))
    n, stride = len(frames), 1024
    keys, rules, table = ordinary_table("fuzz", 4096)
    want_ok = np.array([R.verdict(f) for f in frames], dtype=np.uint8)
    want_rules, want_cls = _want(frames, table, K.NO_RULE, OTHER_RULE, want_ok, ok_mask)
    out = [(f, 0) if int(r) == K.NO_RULE else F.rewrite(f, RULES[int(r)], 0) for f, r in zip(frames, want_rules)]
    want_frames, want_done = [f for f, _ in out], np.array([d for _, d in out], dtype=np.uint8)
    assert (want_cls == K.PASSED).sum() >= 1000 and (want_done == F.DONE).sum() >= 500
    assert (want_done[want_cls == K.HIT] == F.DONE).sum() >= 20
    t, rule_t = _dev_table(table), engine.make_fwd_rules(list(RULES))
    rule_buf, cls_buf, err = _outputs(n)
    ok = torch.full((n,), POISON, dtype=torch.uint8, device="cuda")
    done = torch.full((n,), POISON, dtype=torch.uint8, device="cuda")
    kw = dict(n=n, miss_rule=K.NO_RULE, other_rule=OTHER_RULE, ok=ok, ok_mask=ok_mask, rule_of=rule_buf[16:n + 16],
              cls=cls_buf[16:n + 16], err=err)
    if layout == "ring":
        arena = torch.from_numpy(ring_image(frames, stride, GUARD)).to("cuda")
        lens = torch.from_numpy(ring_lens(frames)).to("cuda")
        engine.rx_verify_ring(arena, stride, lens, n, ok=ok, err=err)
        rule_of = engine.fwd_classify_ring(arena, stride, lens, t, **kw)
        engine.fwd_rewrite_ring(arena, stride, lens, rule_t, rule_of, n, done=done, err=err)
        want_img = ring_image(want_frames, stride, GUARD)
    else:
        arena, lens, tile_off = _device(frames)
        engine.rx_verify_device(arena, lens, tile_off, n, ok=ok, err=err)
        rule_of = engine.fwd_classify_device(arena, lens, tile_off, t, **kw)
        engine.fwd_rewrite_device(arena, lens, tile_off, rule_t, rule_of, n, done=done, err=err)
        want_img = _blob(want_frames)
    torch.cuda.synchronize()
    assert np.array_equal(ok.cpu().numpy(), want_ok)
    _check_outputs(f"verify -> classify -> rewrite ({layout}, ok_mask {ok_mask})", n, rule_buf, cls_buf, want_rules,
                   want_cls, frames)
    assert np.array_equal(done.cpu().numpy(), want_done)
    assert np.array_equal(arena.cpu().numpy(), want_img)
    assert int(err.item()) == 0
