"""CPU: the ring builder and the frame sets of the pipck_tx_fill_ring GPU tests
(tests/test_gpu_tx_fill_ring.py), and the conditions those tests rest on.

pipck_tx_fill_ring (include/pipck.h; k_ring_tx in pip_amd/csrc/pipck_txring.hip)
fills frames that sit in the fixed-size slots of a device ring.  Its blocks of 64
slots choose a stream from their lengths -- S8 / S16 / S32 for frames up to 128 /
256 / 512 bytes, else the row stream on each wave's own slots ("own") or dealt
round-robin ("coop") -- so a test only covers what its ring's lengths reach.
branch_census restates that choice in plain integers; the "shapes" rings are
built so that the census shows every branch, in full blocks and in a partial
last block of 1 and of 63 slots.  tests/tx_reference.fill stays the one
reference of what a frame must hold afterwards."""
import ctypes as C
import functools
import random
import re
from pathlib import Path

import numpy as np

from tests import rx_reference as R
from tests import tx_reference as T
from tests.test_gpu_rx_reference import fuzz_frames, structured_set
from tests.test_tx_reference import corner_frames, pip_frames, preset, shaped_frames

ROOT = Path(__file__).resolve().parents[1]
PRESETS = ("zero", "random", "correct")
BRANCHES_1K = ("S8", "S16", "S32", "own")
TAILS = (1, 63)  # slots in the partial last block

_SLOT_FILL = np.arange(251, dtype=np.uint8) + 1  # 1..251, period 251: non-zero, and no multiple of 16 or of a stride
_GUARD_FILL = 255 - np.arange(241, dtype=np.uint8)  # 255..15, period 241


def ring_image(frames, stride, guard):
    """uint8[len(frames) * stride + guard]: slot i holds frame i, then -- to the
    slot's end -- a non-zero pattern that depends on the position (a sum that runs
    past the frame, or a store past it, must show: not zeros); after the last
    slot, `guard` bytes of another pattern, inside the same allocation."""
    n = len(frames)
    img = np.empty(n * stride + guard, dtype=np.uint8)
    img[:n * stride] = np.resize(_SLOT_FILL, n * stride)
    img[n * stride:] = np.resize(_GUARD_FILL, guard)
    for i, f in enumerate(frames):
        assert len(f) <= stride, (i, len(f), stride)
        img[i * stride:i * stride + len(f)] = np.frombuffer(f, dtype=np.uint8)
    return img


def ring_lens(frames):
    """The frames' lengths as the int16 view of u16 that the device tensors carry."""
    return np.array([len(f) for f in frames], dtype=np.uint16).view(np.int16)


def reference_fill(frames, flags):
    """([tx_reference.fill(frame, flags)[0]], done bytes): the expected ring is
    ring_image of the first with the same stride and guard."""
    filled = [T.fill(f, flags) for f in frames]
    return [f for f, _ in filled], np.array([d for _, d in filled], dtype=np.uint8)


def branch_census(lens, stride):
    """The stream each block of 64 slots takes, as k_ring_tx's prologue chooses it:
    refused lengths (> stride) count as 0; cmax = max ceil(L / 16); <= 8 / 16 /
    32 chunks: S8 / S16 / S32; otherwise T = sum of ceil(chunks / 64), "coop"
    when T >= 2 * (slots in the block), else "own"."""
    out = []
    lens = [int(x) for x in lens]
    for b0 in range(0, len(lens), 64):
        chunks = [((0 if L > stride else L) + 15) // 16 for L in lens[b0:b0 + 64]]
        nb, cmax = len(chunks), max(chunks)
        if cmax <= 8:
            out.append("S8")
        elif cmax <= 16:
            out.append("S16")
        elif cmax <= 32:
            out.append("S32")
        else:
            out.append("coop" if sum((c + 63) // 64 for c in chunks) >= 2 * nb else "own")
    return out


# ---- the shapes rings --------------------------------------------------------------

TINY = (b"", b"\x45", b"\x45" + bytes(14), b"\x60" + bytes(9), b"\x45" + bytes(18), b"\x60" + bytes(18))
# 0 bytes, under 16 bytes, under 20 bytes


def _sized(rng, fam, proto, total, **kw):
    """A frame of exactly `total` bytes (checksum fields left random)."""
    f = R.build(rng, fam, proto, 64, fill=False, **kw)
    f = R.build(rng, fam, proto, 64 + total - len(f), fill=False, **kw)
    assert len(f) == total
    return f


@functools.lru_cache(maxsize=None)
def _pool():
    return tuple(shaped_frames()) + tuple(f for _, f, _ in corner_frames())


def _block(rng, count, lo, hi, extra=()):
    """`count` frames of at most `hi` bytes whose longest lies in (lo, hi]: both
    ends of the class (hi and lo + 1 bytes), `extra`, the tiny frames -- as far
    as the block has room, in that order -- and a sample of the shaped and corner
    frames that fit."""
    ends = [_sized(rng, 4, R.TCP, hi), _sized(rng, 6, R.UDP, lo + 1)]
    frames = (ends + list(extra) + list(TINY))[:count]
    fit = [f for f in _pool() if len(f) <= hi]
    frames += [rng.choice(fit) for _ in range(count - len(frames))]
    rng.shuffle(frames)
    assert len(frames) == count and lo < max(map(len, frames)) <= hi
    return frames


def _block_1k(rng, branch, count):
    if branch == "S8":  # the corner frames live here (all <= 85 bytes), in the full blocks
        corners = [f for _, f, _ in corner_frames()]
        return _block(rng, count, 48, 128, extra=corners if count == 64 else corners[:count // 3])
    if branch == "S16":
        return _block(rng, count, 128, 256)
    if branch == "S32":
        return _block(rng, count, 256, 512)
    # "own": short frames and ONE frame of 513..1,024 bytes (one row item: T < 2 * count)
    long_one = _sized(rng, rng.choice([4, 6]), rng.choice([R.TCP, R.UDP]), rng.choice([513, 700, 1024]))
    if count == 1:
        return [long_one]
    frames = _block(rng, count - 1, 48, 512) + [long_one]
    rng.shuffle(frames)
    return frames


@functools.lru_cache(maxsize=None)
def _jumbo_pool():
    rng = random.Random(9216)
    # 9,000-byte frames: TCP over IPv4 with an 8,980-byte and UDP over IPv6 with an 8,960-byte message
    return (R.build(rng, 4, R.TCP, 8980, fill=False), R.build(rng, 6, R.UDP, 8960, fill=False),
            R.build(rng, 4, R.UDP, 4001, options=rng.randbytes(20), fill=False),
            R.build(rng, 6, R.ICMP6, 3000, ext=R.ext_chain([(R.HOPOPTS, 40)], R.ICMP6), fill=False) + bytes(99),
            R.build(rng, 4, R.ICMP, 2047, fill=False)) + tuple(f for f in shaped_frames() if 1024 < len(f) <= 9216)


def _block_9k(rng, count):
    """`count` frames, each over 1,024 bytes (two rows or more each: "coop")."""
    pool = _jumbo_pool()
    frames = list(pool[:min(5, count)]) + [rng.choice(pool) for _ in range(count - min(5, count))]
    rng.shuffle(frames)
    assert all(1024 < len(f) <= 9216 for f in frames)
    return frames


@functools.lru_cache(maxsize=None)
def shapes_rings():
    """((name, stride, frames), ...): at stride 1,024 one ring per (branch of the
    partial last block, its slot count), each with two full blocks of every
    branch S8, S16, S32 and "own" before it; at stride 9,216 two full "coop"
    blocks of frames over 1,024 bytes, a block that mixes 9,000-byte frames with
    tiny and short ones, and a partial "coop" block of 1 and of 63 slots; at
    stride 65,536 one block of 65,535-byte frames among short ones."""
    rings = []
    for branch in BRANCHES_1K:
        for tail in TAILS:
            rng = random.Random(1024 + 97 * BRANCHES_1K.index(branch) + tail)
            frames = []
            for b in BRANCHES_1K * 2:
                frames += _block_1k(rng, b, 64)
            frames += _block_1k(rng, branch, tail)
            rings.append((f"1024-{branch}-{tail}", 1024, tuple(frames)))
    for tail in TAILS:
        rng = random.Random(9216 + tail)
        frames = _block_9k(rng, 64) + _block_9k(rng, 64)
        mixed = list(_jumbo_pool()[:2]) * 10 + [TINY[k % len(TINY)] for k in range(12)] + \
            [rng.choice([f for f in _pool() if len(f) <= 512]) for _ in range(32)]
        rng.shuffle(mixed)
        frames += mixed + _block_9k(rng, tail)
        rings.append((f"9216-coop-{tail}", 9216, tuple(frames)))
    rng = random.Random(65536)
    big = [R.build(rng, 4, R.TCP, 65515, fill=False), R.build(rng, 4, R.UDP, 65515, options=b"", fill=False),
           R.build(rng, 6, R.TCP, 65495, fill=False)]
    assert [len(f) for f in big] == [65535] * 3
    block = big + [TINY[k] for k in range(len(TINY))] + [rng.choice(_pool()) for _ in range(64 - 3 - len(TINY))]
    rng.shuffle(block)
    rings.append(("65536-rows", 65536, tuple(block)))
    return tuple(rings)


@functools.lru_cache(maxsize=None)
def shapes_preset(name, how):
    """The frames of shapes ring `name` with the fields the call writes pre-set (`how`)."""
    frames = dict((n, f) for n, _, f in shapes_rings())[name]
    rng = random.Random(PRESETS.index(how) * 1000 + len(frames))
    return tuple(preset(rng, f, how) for f in frames)


@functools.lru_cache(maxsize=None)
def shapes_reference(name, how, flags):
    return reference_fill(shapes_preset(name, how), flags)


def assert_shapes_census():
    """What the shapes rings are for: every branch at least twice in full blocks,
    and every branch in a partial last block of 1 and of 63 slots."""
    last = {}
    full = {}
    for name, stride, frames in shapes_rings():
        census = branch_census([len(f) for f in frames], stride)
        tail = len(frames) % 64
        for b in census[:len(frames) // 64]:
            full[b] = full.get(b, 0) + 1
        if tail:
            last.setdefault(census[-1], set()).add(tail)
        if stride == 1024:
            want = list(BRANCHES_1K * 2) + [name.split("-")[1]]
            assert census == want, (name, census)
            assert [b for b in BRANCHES_1K if census.count(b) < 2] == [], (name, census)
        elif stride == 9216:
            assert census == ["coop"] * 4, (name, census)
            for jumbo in _jumbo_pool()[:2]:  # the 9,000-byte TCP/IPv4 and UDP/IPv6 frames, in a full block
                assert len(jumbo) == 9000 and jumbo in frames[:64] and jumbo in frames[64:128]
            assert all(len(f) > 1024 for f in frames[:128])
        else:
            assert census == ["coop"] and sum(len(f) == 65535 for f in frames) >= 3, (name, census)
    assert set(full) == set(BRANCHES_1K) | {"coop"} and min(full.values()) >= 2, full
    assert last == {b: set(TAILS) for b in BRANCHES_1K + ("coop",)}, last
    # the corner frames, all of them, in S8 blocks; tiny frames in several blocks
    corners = {f for _, f, _ in corner_frames()}
    assert len(corners) == 27 and max(map(len, corners)) <= 85
    for name, stride, frames in shapes_rings():
        if stride == 1024:
            assert corners <= set(frames[:64]) and corners <= set(frames[256:320]), name
    name, stride, frames = shapes_rings()[0]
    for probe in (lambda f: len(f) == 0, lambda f: 0 < len(f) < 16, lambda f: 16 <= len(f) < 20):
        assert len({i // 64 for i, f in enumerate(frames) if probe(f)}) >= 3
    assert any(len(f) == 0 for f in shapes_rings()[-1][2]) and any(len(f) == 0 for f in shapes_rings()[-2][2])


# ---- the conditions -----------------------------------------------------------------


def test_ring_image_marks_every_byte_outside_the_frames():
    frames = [b"\x45" + bytes(30), b"", bytes(1024), b"\x60" + bytes(99)]
    img = ring_image(frames, 1024, 4096)
    assert img.size == 4 * 1024 + 4096
    for i, f in enumerate(frames):
        assert img[i * 1024:i * 1024 + len(f)].tobytes() == f
        rest = img[i * 1024 + len(f):(i + 1) * 1024]
        assert (rest != 0).all()
    assert (img[4096:] != 0).all()
    assert img[1024:2048].tobytes() != img[3072:4096].tobytes()  # the pattern depends on the position
    assert img[4096:8192].tobytes() != img[:4096].tobytes()
    want = ring_image(reference_fill(frames, 0)[0], 1024, 4096)
    assert want.shape == img.shape


def test_branch_census_restates_the_blocks_choice():
    assert branch_census([0] * 64, 1024) == ["S8"]
    assert branch_census([128] * 64 + [129], 1024) == ["S8", "S16"]
    assert branch_census([256, 0, 19], 1024) == ["S16"]
    assert branch_census([257] + [60] * 63, 1024) == ["S32"]
    assert branch_census([512] * 64, 1024) == ["S32"]
    assert branch_census([513] + [60] * 63, 1024) == ["own"]
    assert branch_census([1024], 1024) == ["own"] and branch_census([1025], 2048) == ["coop"]
    assert branch_census([1025] * 64, 9216) == ["coop"]
    assert branch_census([9000] * 7 + [60] * 57, 9216) == ["own"]  # 7 * 9 + 57 = 120 < 128
    assert branch_census([9000] * 8 + [60] * 56, 9216) == ["coop"]  # 8 * 9 + 56 = 128
    assert branch_census([1025, 65535, 60], 1024) == ["S8"]  # refused lengths count as 0
    assert branch_census([65535] + [0] * 63, 65536) == ["own"]  # 64 rows in one slot: 64 < 128
    assert branch_census([65535] * 2 + [0] * 62, 65536) == ["coop"]


def test_shapes_rings_reach_every_branch():
    assert_shapes_census()
    for name, stride, frames in shapes_rings():
        assert max(map(len, frames)) <= stride
    # the reference has both fields to fill, one, and none, in these rings
    done = np.concatenate([shapes_reference(name, "random", 0)[1] for name, _, _ in shapes_rings()])
    assert np.bincount(done, minlength=4).min() >= 20, np.bincount(done, minlength=4)


def test_fuzz_frames_fit_1k_slots_and_reach_every_done_value():
    frames = fuzz_frames()
    assert max(map(len, frames)) == 812  # <= 1,024: a 1,024-byte ring leaves none out
    for flags in (0, T.UDP_ZERO_AS_ONES):
        counts = np.bincount(reference_fill(frames, flags)[1], minlength=4)
        assert counts.size == 4 and counts.min() >= 100, counts
        assert counts.tolist() == [7227, 5828, 4046, 2899], counts
    # the fuzz alone reaches two of the five branches: hence the shapes rings
    assert set(branch_census([len(f) for f in frames], 1024)) == {"S32", "own"}


def test_pip_frames_fit_9k_slots():
    assert max(map(len, pip_frames())) <= 9000


def test_structured_set_long_frames():
    frames, names, _ = structured_set()
    over_1k = [(n, len(f)) for f, n in zip(frames, names) if len(f) > 1024]
    assert {n for n, _ in over_1k} == {"long", "v6_ext_len_255"} and len(over_1k) == 8, over_1k
    assert [ln for _, ln in over_1k if ln > 9216] == [65535]


def test_abi_declares_and_exports_tx_fill_ring():
    from pip_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pipck.h").read_text(), flags=re.S)
    m = re.search(r"\bint\s+pipck_tx_fill_ring\s*\(([^)]*)\)\s*;", text)
    assert m, "include/pipck.h does not declare pipck_tx_fill_ring"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 8, params
    assert [p.split()[-1].lstrip("*") for p in params] == ["d_arena", "slot_stride", "d_lens", "n_slots", "flags",
                                                           "d_done", "d_err", "stream"]
    assert int(re.search(r"#define PIPCK_VERSION_MINOR (\d+)", text).group(1)) >= 5
    assert "1.5: pipck_tx_fill_ring" in re.sub(r"\s+", " ", (ROOT / "include" / "pipck.h").read_text())
    restype, argtypes = _lib.SIGNATURES["pipck_tx_fill_ring"]
    assert restype is C.c_int32 or restype is C.c_int
    assert len(argtypes) == 8 and argtypes[1] is C.c_uint64 and argtypes[3] is C.c_uint64 and argtypes[4] is C.c_uint32
    lib = _lib.load()
    assert hasattr(lib, "pipck_tx_fill_ring")
    assert lib.pipck_version() & 0xFFFF >= 5
    # n_slots == 0 returns before any pointer check; unknown flag bits are refused with the function's name
    assert lib.pipck_tx_fill_ring(None, 0, None, 0, 0, None, None, None) == _lib.PIPCK_OK
    assert lib.pipck_tx_fill_ring(C.c_void_p(16), 1024, C.c_void_p(16), 1, 2, C.c_void_p(16), None, None) == \
        _lib.PIPCK_EINVAL
    assert b"pipck_tx_fill_ring" in lib.pipck_last_error()
