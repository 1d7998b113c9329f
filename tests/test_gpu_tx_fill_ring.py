"""pipck_tx_fill_ring (include/pipck.h, k_ring_tx in pip_amd/csrc/pipck_txring.hip)
against tests/tx_reference.py: every assertion compares the WHOLE ring after the
call, byte for byte -- the frames, the non-zero pattern that fills each slot
behind its frame, and the guard after the last slot -- with the ring built from
tx_reference.fill, and the done bytes, inside a poisoned buffer, with the
reference's.  So a sum that runs past a frame, a store outside the two checksum
fields and a done byte outside [0, n) fail like a wrong checksum does.  The
builder, the frame sets and the conditions they meet: tests/test_tx_ring_cases.py."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

from tests import rx_reference as R
from tests import tx_reference as T
from tests.test_gpu_rx import _last_kernel
from tests.test_gpu_rx_reference import fuzz_frames, structured_set
from tests.test_tx_reference import corner_frames, pip_frames, preset, shaped_frames
from tests.test_tx_ring_cases import (PRESETS, assert_shapes_census, branch_census, reference_fill, ring_image,
                                      ring_lens, shapes_preset, shapes_reference, shapes_rings)

pytestmark = pytest.mark.gpu

KERNEL = "k_ring_tx<8, 12>"
GUARD = 4096  # bytes after the last slot, inside the allocation: must come back unchanged
POISON = 0xEE  # done[-16:0) and done[n:n+16)
SCHEDULES = {"default": {}, "ring_own_slots": {"ring_own_slots": True}, "ring_all_coop": {"ring_all_coop": True}}


def _check(path, frames, stride, got_img, got_done, want_img, want_done):
    """Whole rings and done bytes equal, or the first differing slots in full."""
    n = len(frames)
    got_img, got_done = np.asarray(got_img), np.asarray(got_done)
    assert got_img.shape == want_img.shape and got_done.shape == (n + 32,)
    assert (got_done[:16] == POISON).all() and (got_done[n + 16:] == POISON).all(), f"{path}: done written outside [0, n)"
    got_done = got_done[16:n + 16]
    if np.array_equal(got_img, want_img) and np.array_equal(got_done, want_done):
        return
    bad_bytes = np.nonzero(got_img != want_img)[0]
    bad = sorted(set((bad_bytes // stride).tolist()) | set(np.nonzero(got_done != want_done)[0].tolist()))
    msgs = []
    for i in bad[:4]:
        if i >= n:
            msgs.append("the guard after the last slot was written")
            continue
        where = [int(k) - i * stride for k in bad_bytes if i * stride <= k < (i + 1) * stride][:8]
        a = i * stride
        msgs.append(f"slot {i}: {frames[i][:96].hex()} length {len(frames[i])} bytes differing at {where} got "
                    f"{bytes(got_img[a:a + stride][where]).hex()} want {bytes(want_img[a:a + stride][where]).hex()} "
                    f"done got {int(got_done[i])} want {int(want_done[i])}")
    raise AssertionError(f"{len(bad)} of {n} slots differ on {path}: " + "; ".join(msgs))


def _fill_and_check(path, frames, stride, flags, reference=None, guard=GUARD):
    """One call on a fresh ring of `frames`, held to the reference (computed here
    unless given: (filled frames, done)); returns the device ring, lengths and
    the poisoned done buffer."""
    import torch

    from pip_amd import engine

    n = len(frames)
    ring = torch.from_numpy(ring_image(frames, stride, guard)).to("cuda")
    lens = torch.from_numpy(ring_lens(frames)).to("cuda")
    done = torch.full((n + 32,), POISON, dtype=torch.uint8, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    engine.tx_fill_ring(ring, stride, lens, n, flags=flags, done=done[16:n + 16], err=err)
    assert KERNEL in _last_kernel(), _last_kernel()
    want_frames, want_done = reference or reference_fill(frames, flags)
    _check(path, frames, stride, ring.cpu().numpy(), done.cpu().numpy(), ring_image(want_frames, stride, guard),
           want_done)
    assert int(err.item()) == 0
    return ring, lens, done


@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_tx_fill_ring_shapes(schedule):
    """The shapes rings -- every stream of the block's choice, in full blocks and in
    a partial last block of 1 and 63 slots, at strides 1,024, 9,216 and 65,536 --
    with the fields pre-set to zero, random bytes and their correct value, under
    both flag values, by the default choice and with either row stream forced."""
    from pip_amd import engine

    assert_shapes_census()  # before the first GPU call
    engine.tune(**SCHEDULES[schedule])
    try:
        for name, stride, _ in shapes_rings():
            for how in PRESETS:
                for flags in (0, T.UDP_ZERO_AS_ONES):
                    _fill_and_check(f"pipck_tx_fill_ring (ring {name}, {schedule}, fields {how}, flags {flags})",
                                    list(shapes_preset(name, how)), stride, flags,
                                    reference=shapes_reference(name, how, flags))
    finally:
        engine.tune()


@functools.lru_cache(maxsize=None)
def _structured(stride):
    """The RX reference test's structured set, every frame that fits the slot."""
    frames, names, _ = structured_set()
    keep = [i for i, f in enumerate(frames) if len(f) <= stride]
    long_classes = sum(1 for n in names if n in ("long", "v6_ext_len_255"))
    assert len(frames) - len(keep) <= long_classes and (stride < 65536 or len(keep) == len(frames))
    return tuple(frames[i] for i in keep), tuple(names[i] for i in keep)


@pytest.mark.parametrize("stride", [1024, 9216, 65536])
def test_tx_fill_ring_structured_set(stride):
    """IPv4 options, extension chains, link padding, the 0x0000 / 0xFFFF corners;
    at 9,216 the v6_ext_len_255 frames, whose L4 field lies beyond the 96-byte
    window and is read and stored from the frame's own bytes; at 65,536 the
    65,535-byte frame.  Every preset of the fields under both flag values (at
    65,536, a ring of 186 MiB, the random preset alone)."""
    frames, names = _structured(stride)
    if stride >= 9216:
        far = [f for f, n in zip(frames, names) if n == "v6_ext_len_255" and len(f) > 1024]
        assert far and all(at >= 96 for f in far for at, _ in T.fields(f)) and any(T.fields(f) for f in far)
    assert (stride == 65536) == any(len(f) == 65535 for f in frames)
    for how in (PRESETS if stride < 65536 else ("random",)):
        rng = random.Random(stride + PRESETS.index(how))
        mine = [preset(rng, f, how) for f in frames]
        for flags in (0, T.UDP_ZERO_AS_ONES):
            _fill_and_check(f"pipck_tx_fill_ring (structured set, stride {stride}, fields {how}, flags {flags})", mine,
                            stride, flags)


@functools.lru_cache(maxsize=None)
def _fuzz_reference(flags):
    return reference_fill(fuzz_frames(), flags)


@pytest.mark.parametrize("schedule", ["default", "ring_all_coop"])
@pytest.mark.parametrize("flags", [0, T.UDP_ZERO_AS_ONES])
def test_tx_fill_ring_mutation_fuzz(flags, schedule):
    """The 20,000 mutated frames of the RX reference test in 1,024-byte slots."""
    from pip_amd import engine

    frames = list(fuzz_frames())
    counts = np.bincount(_fuzz_reference(flags)[1], minlength=4)
    assert counts.size == 4 and counts.min() >= 100, counts
    assert set(branch_census([len(f) for f in frames], 1024)) == {"S32", "own"}
    engine.tune(**SCHEDULES[schedule])
    try:
        _fill_and_check(f"pipck_tx_fill_ring (fuzz, {schedule}, flags {flags})", frames, 1024, flags,
                        reference=_fuzz_reference(flags))
    finally:
        engine.tune()


def test_tx_fill_ring_slot_counts():
    """1, 63, 64, 65 and 129 slots: a lone slot, a block's last lane, a partial
    last block after one and after two full ones."""
    rng = random.Random(65)
    pool = [f for f in shaped_frames() if len(f) <= 2048]
    for n in (1, 63, 64, 65, 129):
        _fill_and_check(f"pipck_tx_fill_ring ({n} slots)", rng.sample(pool, n), 2048, 0)


def test_tx_fill_ring_length_past_the_slot_is_refused():
    """Lengths 1,025 and 65,535 planted at a block's first slot, a block's last
    slot and the ring's last slot, over frames that have both fields to fill:
    those slots are neither read nor written and get done 0, PIPCK_ERANGE is set,
    and every other slot is filled as without the tampering.  d_err = NULL is
    accepted.  The C ABI directly, no Python guard; the allocation carries 65 KiB
    of guard after the last slot, so a kernel that honoured a planted length
    would stay inside it and show in the comparison."""
    import torch

    from pip_amd import _lib

    lib = _lib.load()
    stride, guard = 1024, 65 * 1024
    rng = random.Random(1025)
    n = 3 * 64 + 7
    frames = rng.sample([f for f in shaped_frames() if len(f) <= stride], n)
    both = [f for f in shaped_frames() if len(f) <= stride and T.fill(f)[1] == 3]
    for plants in ({64: 1025, 127: 65535, n - 1: 1025}, {64: 65535, 127: 1025, 128: 1025, n - 1: 65535}):
        for i in plants:
            frames[i] = rng.choice(both)
        filled, want_done = reference_fill(frames, 0)
        assert all(want_done[i] == 3 for i in plants)  # the refused slots had work to refuse
        want_frames = [frames[i] if i in plants else f for i, f in enumerate(filled)]
        want_done = want_done.copy()
        want_done[list(plants)] = 0
        lens_host = ring_lens(frames).copy().view(np.uint16)
        for i, length in plants.items():
            lens_host[i] = length
        for with_err in (True, False):
            ring = torch.from_numpy(ring_image(frames, stride, guard)).to("cuda")
            lens = torch.from_numpy(lens_host.view(np.int16)).to("cuda")
            done = torch.full((n + 32,), POISON, dtype=torch.uint8, device="cuda")
            err = torch.zeros(1, dtype=torch.int32, device="cuda")
            assert ring.numel() == n * stride + guard and guard >= 65536
            rc = lib.pipck_tx_fill_ring(ring.data_ptr(), stride, lens.data_ptr(), n, 0, done.data_ptr() + 16,
                                        err.data_ptr() if with_err else None, None)
            assert rc == 0, lib.pipck_last_error()
            torch.cuda.synchronize()
            assert KERNEL in _last_kernel()
            _check(f"pipck_tx_fill_ring (lengths past the slot at {sorted(plants)})", frames, stride,
                   ring.cpu().numpy(), done.cpu().numpy(), ring_image(want_frames, stride, guard), want_done)
            assert int(err.item()) == ((1 << _lib.PIPCK_ERANGE) if with_err else 0)


@functools.lru_cache(maxsize=None)
def _mixed_frames():
    """6,000 fuzz frames, the shaped frames and the corner frames (all within 4,096 bytes)."""
    return tuple(list(fuzz_frames()[:6000]) + shaped_frames() + [f for _, f, _ in corner_frames()])


@pytest.mark.parametrize("flags", [0, T.UDP_ZERO_AS_ONES])
def test_tx_fill_ring_twice_changes_no_byte(flags):
    """A second call on the filled ring: the field is taken as zero, so nothing changes."""
    import torch

    from pip_amd import engine

    frames = list(_mixed_frames())
    ring, lens, done = _fill_and_check("pipck_tx_fill_ring (first call)", frames, 4096, flags)
    once = ring.clone()
    again = engine.tx_fill_ring(ring, 4096, lens, len(frames), flags=flags)
    assert KERNEL in _last_kernel()
    assert torch.equal(ring, once) and torch.equal(again, done[16:len(frames) + 16])


@pytest.mark.parametrize("flags", [0, T.UDP_ZERO_AS_ONES])
def test_tx_fill_ring_then_rx_verify_ring_round_trip(flags):
    """Derived check: pipck_rx_verify_ring_n on the filled ring gives
    rx_reference.verdict of the reference-filled frames."""
    from pip_amd import engine

    frames = list(_mixed_frames())
    want = np.array([R.verdict(f) for f in reference_fill(frames, flags)[0]], dtype=np.uint8)
    assert (want == R.VERIFIED).sum() > 1000
    ring, lens, _ = _fill_and_check("pipck_tx_fill_ring (before RX)", frames, 4096, flags)
    got = engine.rx_verify_ring(ring, 4096, lens, len(frames)).cpu().numpy()
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]


def test_tx_fill_ring_equals_the_packed_path():
    """The frames of the shapes rings through pipck_tx_fill_device, byte-packed:
    the same bytes in every frame and the same done."""
    import torch

    from pip_amd import engine

    for name, stride, _ in shapes_rings():
        frames = list(shapes_preset(name, "random"))
        n = len(frames)
        for flags in (0, T.UDP_ZERO_AS_ONES):
            ring, lens, done = _fill_and_check(f"pipck_tx_fill_ring (ring {name}, flags {flags})", frames, stride, flags,
                                               reference=shapes_reference(name, "random", flags))
            arena = torch.from_numpy(np.frombuffer(b"".join(frames) + bytes(256), dtype=np.uint8).copy()).to("cuda")
            packed_done = engine.tx_fill_device(arena, lens, engine.packed_bytes_index(lens), flags=flags)
            assert "k_packedb_tx<" in _last_kernel()
            img = ring.cpu().numpy()
            from_ring = b"".join(img[i * stride:i * stride + len(f)].tobytes() for i, f in enumerate(frames))
            assert arena.cpu().numpy().tobytes() == from_ring + bytes(256), (name, flags)
            assert torch.equal(packed_done, done[16:n + 16]), (name, flags)


def test_tx_fill_ring_writes_pips_wire_bytes():
    """The packets pip's compiled stack emitted (tests/golden/stack_replay.txt),
    their checksum fields scrambled, in 9,216-byte slots: filled, they are pip's bytes."""
    rng = random.Random(11)
    pkts = pip_frames()
    scrambled = [preset(rng, p, "random") for p in pkts]
    assert all(q != p for p, q in zip(pkts, scrambled))
    ring, _, done = _fill_and_check("pipck_tx_fill_ring (pip's packets)", scrambled, 9216, 0)
    assert np.array_equal(ring.cpu().numpy(), ring_image(pkts, 9216, GUARD))
    assert done.cpu().numpy()[16:len(pkts) + 16].tolist() == [3 if p[0] >> 4 == 4 else 2 for p in pkts]


def test_tx_fill_ring_argument_errors_launch_nothing():
    """Null pointers, a misaligned arena, strides outside the rule and unknown
    flag bits: PIPCK_EINVAL with the function's name, and no launch; n = 0
    returns PIPCK_OK."""
    import torch

    from pip_amd import _lib, engine

    lib = _lib.load()
    stride = 1024
    frames = [f for f in shaped_frames() if len(f) <= stride][:70]
    n = len(frames)
    ring = torch.from_numpy(ring_image(frames, stride, GUARD)).to("cuda")
    lens = torch.from_numpy(ring_lens(frames)).to("cuda")
    engine.rx_verify_ring(ring, stride, lens, n)  # this thread's last recorded launch: not the TX kernel
    before, last = ring.clone(), _last_kernel()
    assert "k_ring<" in last and "k_ring_tx" not in last
    done = torch.full((n,), POISON, dtype=torch.uint8, device="cuda")
    a, ln, dn = ring.data_ptr(), lens.data_ptr(), done.data_ptr()
    assert a % 16 == 0
    u64 = C.c_uint64
    for args, why in (((None, u64(stride), ln, n, 0, dn, None, None), "null arena"),
                      ((a, u64(stride), None, n, 0, dn, None, None), "null lengths"),
                      ((a, u64(stride), ln, n, 0, None, None, None), "null done"),
                      ((a + 8, u64(stride), ln, n, 0, dn, None, None), "misaligned arena"),
                      ((a, u64(1008), ln, n, 0, dn, None, None), "stride under 1,024"),
                      ((a, u64(1032), ln, n, 0, dn, None, None), "stride no multiple of 16"),
                      ((a, u64(65552), ln, 1, 0, dn, None, None), "stride over 65,536"),
                      ((a, u64(0), ln, n, 0, dn, None, None), "stride 0"),
                      ((a, u64((1 << 32) + 1024), ln, 1, 0, dn, None, None), "stride 1,024 mod 2^32"),
                      ((a, u64(stride), ln, n, 2, dn, None, None), "unknown flag bit"),
                      ((a, u64(stride), ln, n, 0x80000001, dn, None, None), "unknown flag bit beside a known one")):
        assert lib.pipck_tx_fill_ring(*args) == _lib.PIPCK_EINVAL, why
        assert b"pipck_tx_fill_ring" in lib.pipck_last_error(), why
        assert _last_kernel() == last, why
    assert lib.pipck_tx_fill_ring(None, 0, None, 0, 0, None, None, None) == _lib.PIPCK_OK
    assert lib.pipck_tx_fill_ring(a, u64(stride), ln, 0, 1, dn, None, None) == _lib.PIPCK_OK
    assert _last_kernel() == last
    torch.cuda.synchronize()
    assert torch.equal(ring, before) and bool((done == POISON).all())
