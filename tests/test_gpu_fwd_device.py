"""pipck_fwd_rewrite_device (include/pipck.h, k_fwd_device in pip_amd/csrc/pipck_fwddev.hip)
against tests/fwd_reference.py: every assertion compares the WHOLE arena after the
call, byte for byte -- the frames back to back and the 256-byte guard pattern behind
the last one, inside the arena -- with the arena built from fwd_reference.rewrite, and
the done bytes, inside a poisoned buffer with 16 bytes on either side, with the
reference's.  So a store outside the named fields and their two checksum fields, a
store into a neighbouring frame that shares a dword, a 16-byte chunk or a 128-byte
line, a store into a frame that is not DONE and a done byte outside [0, n) fail like a
wrong checksum does.  The rule table, the assignment and the frame sets:
tests/test_fwd_reference.py; the short set: tests/test_fwd_device_cases.py."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

from tests import fwd_reference as F
from tests import rx_reference as R
from tests import tx_reference as T
from tests.test_fwd_device_cases import short_set
from tests.test_fwd_reference import (DPORT, DST4, SPORT, SRC4, assign, far_tcp_frames, filled, fuzz_ring_frames,
                                      reference_rewrite, rule_index, rule_table)
from tests.test_gpu_rx import _last_kernel
from tests.test_gpu_rx_reference import fuzz_frames, structured_set
from tests.test_gpu_tx_fill import _blob, _check, _device, _filler, _starts
from tests.test_tx_ring_cases import ring_image, ring_lens

pytestmark = pytest.mark.gpu

KERNEL = "k_fwd_device"
FLAGS = (0, F.UDP_ZERO_AS_ONES)
POISON = 0xEE  # done[-16:0) and done[n:n+16)
NO_RULE = 0xFFFFFFFF
ERANGE_BIT, EINVAL_BIT = 1 << 2, 1 << 1


def _table(rules, device="cuda"):
    from pip_amd import engine

    return engine.make_fwd_rules(list(rules), device=device)


def _i32(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to("cuda")


def _reference(frames, rule_of, flags, rules=None):
    """reference_rewrite, with NO_RULE passing over a frame: untouched, done 0."""
    rules = rule_table() if rules is None else rules
    out = [(f, 0) if int(r) == NO_RULE else F.rewrite(f, rules[int(r)], flags) for f, r in zip(frames, rule_of)]
    return [f for f, _ in out], np.array([d for _, d in out], dtype=np.uint8)


def _check_done(path, n, done_buf):
    """The 16 poisoned bytes on either side of the done bytes are untouched; returns done[0:n)."""
    got = done_buf.cpu().numpy()
    assert got.size == n + 32
    assert (got[:16] == POISON).all() and (got[n + 16:] == POISON).all(), f"{path}: a done byte outside [0, n)"
    return got[16:n + 16]


def _rewrite_and_check(path, frames, rule_of, flags, rules=None, reference=None):
    """One call on a fresh arena of `frames` under rules[rule_of[i]] (rule 0 where rule_of is None),
    held to the reference (computed here unless given: (frames, done)); returns the device arena,
    lengths, index and the done bytes."""
    import torch

    from pip_amd import engine

    rules = rule_table() if rules is None else rules
    n = len(frames)
    arena, lens, tile_off = _device(frames)
    assert arena.data_ptr() % 128 == 0
    done = torch.full((n + 32,), POISON, dtype=torch.uint8, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    ro = None if rule_of is None else _i32(rule_of)
    got = engine.fwd_rewrite_device(arena, lens, tile_off, _table(rules), ro, n, flags=flags, done=done[16:n + 16],
                                    err=err)
    assert KERNEL in _last_kernel(), _last_kernel()
    assert got.data_ptr() == done.data_ptr() + 16
    want_frames, want_done = reference or _reference(frames, [0] * n if rule_of is None else rule_of, flags, rules)
    _check(path, frames, arena.cpu().numpy(), _check_done(path, n, done), _blob(want_frames), want_done)
    assert int(err.item()) == 0
    return arena, lens, tile_off, done[16:n + 16]


# ---------------------------------------------------------------------------- 1. the short set
@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_fwd_device_short_set(lead):
    """Frames of 20 to 51 bytes back to back: two or three frames' fields in one 16-byte chunk, a
    neighbour's bytes in the dword of a stored field.  The assignment shifted through all seven ops
    sets under both flag values; with lead 1, 2, 3 the whole batch behind a filler frame of so many
    bytes (version 2, PIPCK_FWD_NO_RULE), so every frame meets every start parity."""
    frames = ([bytes([0x25]) + bytes(lead - 1)] if lead else []) + list(short_set())
    for shift in range(7):
        rule_of = np.array([rule_index(f, (i + shift) % 7) for i, f in enumerate(frames)], dtype=np.uint32)
        if lead:
            rule_of[0] = NO_RULE
        for flags in FLAGS:
            _rewrite_and_check(f"pipck_fwd_rewrite_device (short set, lead {lead}, shift {shift}, flags {flags})",
                               frames, rule_of, flags)


# ---------------------------------------------------------------------------- 2. the structured set
def test_fwd_device_structured_set():
    """Every class at every start residue mod 16, the 65,535-byte frame, IPv4 options at every IHL,
    extension chains around and past the window (the far TCP frames among them): every frame under
    every ops set of its family (the assignment shifted seven times), both flag values in turn."""
    frames = list(structured_set()[0])
    assert len(frames) == 2983 and any(len(f) == 65535 for f in frames)
    far = far_tcp_frames()
    assert far and all(f in frames for f in far)
    census = np.bincount(reference_rewrite(frames, assign(frames), 0)[1], minlength=5)
    assert (census[F.DONE], census[F.UNHANDLED], census[0], census[F.EXPIRED]) == (2279, 621, 76, 7), census
    for shift in range(7):
        rule_of = np.array([rule_index(f, (i + shift) % 7) for i, f in enumerate(frames)], dtype=np.uint32)
        flags = FLAGS[shift & 1]
        _rewrite_and_check(f"pipck_fwd_rewrite_device (structured set, shift {shift}, flags {flags})", frames, rule_of,
                           flags)


# ---------------------------------------------------------------------------- 3. straddles
def _stored_fields(f):
    """First bytes of the fields the all-ops rule stores in filled frame f: the TTL halfword, IPv4
    bytes 10-11, each address, the port pair and the L4 field."""
    l4 = R.l4_range(f)[0]
    proto = T._upper(f)[0]
    head = [8, 10, 12, 16] if f[0] >> 4 == 4 else [6, 8, 24]
    return head + [l4, l4 + R.CSUM_AT[proto]]


@functools.lru_cache(maxsize=None)
def _straddles():
    """(frames, rule_of): filled frames placed behind filler frames, as tx_structured places them,
    so that each stored field's first byte falls at 15 mod 16 and at 127 mod 128 -- the field then
    straddles a chunk or a line, and the frame starts at an odd address or at 2 mod 4; frames 63
    and 64, either side of a tile boundary, share a chunk and a dword."""
    rng = random.Random(1627)
    frames, off = [], 0

    def put(f):
        nonlocal off
        frames.append(f)
        off += len(f)

    kinds = [T.fill(R.build(rng, fam, proto, 75, options=options, ext=ext, fill=False), 0)[0]
             for fam, proto, options, ext in ((4, R.TCP, b"", None), (4, R.UDP, b"", None),
                                              (4, R.TCP, rng.randbytes(40), None), (6, R.TCP, b"", None),
                                              (6, R.UDP, b"", None),
                                              (6, R.UDP, b"", R.ext_chain([(R.DSTOPTS, 1)], R.UDP)))]
    hits = set()
    for f in kinds[:2]:  # the tile boundary first: frames 63 and 64 back to back at an odd address
        while len(frames) < 63:
            put(_filler(16 + rng.randrange(32)))
        if len(frames) == 63:  # frame 63 starts at 3 mod 16, frame 64 95 bytes on at 2 mod 16
            pad = (3 - off) % 16
            frames[-1] = frames[-1] + bytes(pad)
            off += pad
        put(f)
    assert len(frames) == 65 and _starts(frames)[63] % 16 == 3 and _starts(frames)[64] % 16 == 2
    for f in kinds:
        assert F.rewrite(f, rule_table()[rule_index(f, 3)])[1] == F.DONE
        for field in _stored_fields(f):
            for mod in (16, 128):
                put(_filler(16 + (mod - 1 - field - off - 16) % mod))
                assert (off + field) % mod == mod - 1
                hits.add((f[0] >> 4, field, mod))
                put(f)
    assert len(hits) >= 2 * (6 + 5)
    return tuple(frames), np.array([rule_index(f, 3) for f in frames], dtype=np.uint32)


def test_fwd_device_straddling_fields():
    frames, rule_of = _straddles()
    for flags in FLAGS:
        _rewrite_and_check(f"pipck_fwd_rewrite_device (straddles, flags {flags})", list(frames), rule_of, flags)


# ---------------------------------------------------------------------------- 4. fuzz
@functools.lru_cache(maxsize=None)
def _fuzz_reference(flags):
    frames = fuzz_ring_frames()
    return reference_rewrite(frames, assign(frames), flags)


@pytest.mark.parametrize("flags", FLAGS)
def test_fwd_device_mutation_fuzz(flags):
    """The 20,000 mutated frames of the RX reference test and the planted-TTL frames, byte-packed."""
    frames = list(fuzz_ring_frames())
    counts = np.bincount(_fuzz_reference(flags)[1], minlength=5)
    assert counts[F.DONE] >= 5000 and counts[F.UNHANDLED] >= 5000 and counts[0] >= 1000 and counts[F.EXPIRED] >= 200
    _rewrite_and_check(f"pipck_fwd_rewrite_device (fuzz, flags {flags})", frames, assign(frames), flags,
                       reference=_fuzz_reference(flags))


# ---------------------------------------------------------------------------- 5. counts
def test_fwd_device_frame_counts():
    """A lone frame, and partial last tiles and blocks for a wave of 64 and a block of 256 frames."""
    rng = random.Random(257)
    pool = [f for f in filled("shaped") if len(f) <= 2048]
    for n in (1, 63, 64, 65, 255, 256, 257):
        frames = [rng.choice(pool) for _ in range(n)]
        _rewrite_and_check(f"pipck_fwd_rewrite_device ({n} frames)", frames, assign(frames), 0)


def test_fwd_device_without_rule_of_every_frame_takes_rule_0():
    rng = random.Random(3)
    frames = rng.sample([f for f in filled("shaped") if len(f) <= 1024], 300)
    for rules in ((rule_table()[3], rule_table()[10]),  # all five ops on IPv4: the IPv6 frames are UNHANDLED
                  (F.rule(F.DEC_TTL | F.SET_SPORT, 0, sport=SPORT),)):
        want = reference_rewrite(frames, [0] * len(frames), 0, rules)
        assert (want[1] == F.DONE).sum() >= 50 and (want[1] == F.UNHANDLED).sum() >= 50
        _rewrite_and_check("pipck_fwd_rewrite_device (d_rule_of NULL)", frames, None, 0, rules=rules, reference=want)


# ---------------------------------------------------------------------------- 6. filled frames
@pytest.mark.parametrize("which", ["shaped", "corner", "pip"])
def test_fwd_device_filled_frames(which):
    """Frames whose checksums verify -- every family, protocol, option length and extension
    shape; the corners of the sum; the packets pip's stack emitted -- under both flag values."""
    frames = list(filled(which))
    assert len(frames) >= 20
    for shift in (0, 3):
        rule_of = np.array([rule_index(f, (i + shift) % 7) for i, f in enumerate(frames)], dtype=np.uint32)
        for flags in FLAGS:
            _rewrite_and_check(f"pipck_fwd_rewrite_device ({which} frames, shift {shift}, flags {flags})", frames,
                               rule_of, flags)


# ---------------------------------------------------------------------------- 7. refusals
def _done_pool(limit=1024):
    """Filled shaped frames that the all-ops rule of their family rewrites."""
    return [f for f in filled("shaped") if len(f) <= limit and F.rewrite(f, rule_table()[rule_index(f, 3)])[1] == F.DONE]


REFUSAL_RULES = (rule_table()[3], rule_table()[10],  # all five ops, family 4 and family 6
                 F.rule(F.ALL_OPS | 32, 4, SRC4, DST4, SPORT, DPORT),  # an unknown ops bit
                 F.rule(F.ALL_OPS, 5, SRC4, DST4, SPORT, DPORT),  # family 5
                 F.rule(F.SET_SRC | F.DEC_TTL, 0, SRC4))  # family 0 with an address
# behind the passed table, in the same allocation: valid rules with other addresses -- an honoured index rewrites
BEHIND = tuple(F.rule(F.ALL_OPS, fam, bytes([9, 9, 9, k]) * (1 if fam == 4 else 4),
                      bytes([7, 7, 7, k]) * (1 if fam == 4 else 4), SPORT, DPORT) for k in range(4) for fam in (4, 6))
PAD = 128 * 1024  # patterned allocation behind the batch's bytes


def _refusal_batch():
    rng = random.Random(1025)
    n = 2 * 256 + 7
    pool = [f for f in _done_pool() if len(f) >= 40]
    frames = [rng.choice(pool) for _ in range(n)]
    rule_of = np.array([int(f[0] >> 4 == 6) for f in frames], dtype=np.uint32)
    clean_frames, clean_done = reference_rewrite(frames, rule_of, 0, REFUSAL_RULES)
    assert (clean_done == F.DONE).all() and max(map(len, frames)) <= 1024
    return frames, rule_of, clean_frames, clean_done


def _padded_arena(frames):
    """(device arena, batch bytes, host image): the frames, then PAD bytes of pattern in the same allocation."""
    import torch

    body = b"".join(frames)
    pattern = bytes((29 * i + 5) & 0xFF for i in range(256)) * (PAD // 256)
    img = np.frombuffer(body + pattern, dtype=np.uint8)
    return torch.from_numpy(img.copy()).to("cuda"), len(body), img


def _run_abi(path, frames, lens_t, tile_off, rule_of, arena, arena_bytes, rules_ptr, n_rules, with_err, want_img,
             want_done, bit):
    import torch

    from pip_amd import _lib

    lib = _lib.load()
    n = len(frames)
    done = torch.full((n + 32,), POISON, dtype=torch.uint8, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    ro = _i32(rule_of)
    rc = lib.pipck_fwd_rewrite_device(arena.data_ptr(), arena_bytes, lens_t.data_ptr(), tile_off.data_ptr(), n,
                                      rules_ptr, n_rules, ro.data_ptr(), 0, done.data_ptr() + 16,
                                      err.data_ptr() if with_err else None, None)
    assert rc == 0, lib.pipck_last_error()
    torch.cuda.synchronize()
    assert KERNEL in _last_kernel()
    _check(path, frames, arena.cpu().numpy(), _check_done(path, n, done), want_img, want_done)
    assert int(err.item()) == (bit if with_err else 0)


@pytest.mark.parametrize("plant", ["tiles first, middle and last", "arena one byte short"])
def test_fwd_device_bounded_by_the_arena(plant):
    """A stale tile index (d_tile_off[t] = arena_bytes - 100 at the first, a middle and the last
    tile) and an arena_bytes one byte short of the batch: the refused tiles are neither read nor
    written, their frames get done 0 and PIPCK_ERANGE is set; every other tile is as in the clean
    run.  arena_bytes is the batch's bytes and 128 KiB of pattern follow in the allocation, so a
    kernel that honoured the stale index would write into the pattern and fail the comparison.
    d_err = NULL is accepted.  The C ABI directly, no Python guard."""
    import torch

    from pip_amd import _lib, engine

    assert (ERANGE_BIT, EINVAL_BIT) == (1 << _lib.PIPCK_ERANGE, 1 << _lib.PIPCK_EINVAL)
    frames, rule_of, clean_frames, clean_done = _refusal_batch()
    n, tiles = len(frames), (len(frames) + 63) // 64
    starts = _starts(frames)
    refused = (0, 4, tiles - 1) if plant.startswith("tiles") else (tiles - 1,)
    assert all(int(starts[min(64 * (t + 1), n)] - starts[64 * t]) > 100 for t in refused)
    want_frames, want_done = list(clean_frames), clean_done.copy()
    for t in refused:
        for i in range(64 * t, min(64 * (t + 1), n)):
            want_frames[i], want_done[i] = frames[i], 0
    rules = _table(REFUSAL_RULES)
    for with_err in (True, False):
        arena, nbytes, img = _padded_arena(frames)
        want_img = img.copy()
        want_img[:nbytes] = np.frombuffer(b"".join(want_frames), dtype=np.uint8)
        lens_t = torch.from_numpy(ring_lens(frames)).to("cuda")
        tile_off = engine.packed_bytes_index(lens_t)
        assert int(tile_off[tiles].item()) == nbytes and arena.numel() == nbytes + PAD
        arena_bytes = nbytes
        if plant.startswith("tiles"):
            for t in refused:
                tile_off[t] = nbytes - 100
        else:
            arena_bytes = nbytes - 1
        _run_abi(f"pipck_fwd_rewrite_device ({plant})", frames, lens_t, tile_off, rule_of, arena, arena_bytes,
                 rules.data_ptr(), len(REFUSAL_RULES), with_err, want_img, want_done, ERANGE_BIT)


# kind -> (planted rule index, the bit d_err must hold)
REFUSALS = {"rule index n_rules": (len(REFUSAL_RULES), ERANGE_BIT),
            "rule index n_rules + 7": (len(REFUSAL_RULES) + 7, ERANGE_BIT),
            "unknown ops bit": (2, EINVAL_BIT), "family 5": (3, EINVAL_BIT), "family 0 with SET_SRC": (4, EINVAL_BIT),
            "PIPCK_FWD_NO_RULE": (NO_RULE, 0)}


@pytest.mark.parametrize("kind", list(REFUSALS))
def test_fwd_device_rule_refusals(kind):
    """Each kind planted at a tile's and a block's first and last frame and at the batch's last
    frame, over frames that would be DONE: those frames are unchanged with done 0, d_err holds
    exactly the expected bit (none for PIPCK_FWD_NO_RULE), every other frame is as without the
    tampering.  The passed table is followed in its allocation by eight valid rules with other
    addresses, so an honoured index past n_rules shows as a rewritten frame."""
    import torch

    from pip_amd import engine

    frames, rule_of, clean_frames, clean_done = _refusal_batch()
    n = len(frames)
    index, bit = REFUSALS[kind]
    plants = (63, 64, 255, 256, n - 1)
    rule_of = rule_of.copy()
    want_frames, want_done = list(clean_frames), clean_done.copy()
    for i in plants:
        rule_of[i] = index
        want_frames[i], want_done[i] = frames[i], 0
    table = _table(REFUSAL_RULES + BEHIND)
    assert table.shape[0] == len(REFUSAL_RULES) + 8 > len(REFUSAL_RULES) + 7 and table.data_ptr() % 16 == 0
    assert all(F.rule_valid(r) for r in BEHIND)
    for with_err in (True, False):
        arena, nbytes, img = _padded_arena(frames)
        want_img = img.copy()
        want_img[:nbytes] = np.frombuffer(b"".join(want_frames), dtype=np.uint8)
        lens_t = torch.from_numpy(ring_lens(frames)).to("cuda")
        tile_off = engine.packed_bytes_index(lens_t)
        _run_abi(f"pipck_fwd_rewrite_device ({kind} at {plants})", frames, lens_t, tile_off, rule_of, arena, nbytes,
                 table.data_ptr(), len(REFUSAL_RULES), with_err, want_img, want_done, bit)


def test_fwd_device_refused_tile_does_not_consult_its_rules():
    """An invalid rule on a frame of a tile past the arena gives no PIPCK_EINVAL bit: ERANGE alone."""
    import torch

    from pip_amd import engine

    frames, rule_of, clean_frames, clean_done = _refusal_batch()
    n, tiles = len(frames), (len(frames) + 63) // 64
    rule_of = rule_of.copy()
    rule_of[n - 1] = 3  # family 5, in the last tile
    want_frames, want_done = list(clean_frames), clean_done.copy()
    for i in range(64 * (tiles - 1), n):
        want_frames[i], want_done[i] = frames[i], 0
    arena, nbytes, img = _padded_arena(frames)
    want_img = img.copy()
    want_img[:nbytes] = np.frombuffer(b"".join(want_frames), dtype=np.uint8)
    lens_t = torch.from_numpy(ring_lens(frames)).to("cuda")
    tile_off = engine.packed_bytes_index(lens_t)
    tile_off[tiles - 1] = nbytes - 100
    rules = _table(REFUSAL_RULES)  # (held in a name: the call below takes its address)
    _run_abi("pipck_fwd_rewrite_device (invalid rule in a refused tile)", frames, lens_t, tile_off, rule_of, arena,
             nbytes, rules.data_ptr(), len(REFUSAL_RULES), True, want_img, want_done, ERANGE_BIT)


# ---------------------------------------------------------------------------- 8. argument errors
def test_fwd_device_argument_errors_launch_nothing():
    """Null pointers, a misaligned arena or rule table, no rules and unknown flag bits:
    PIPCK_EINVAL with the function's name, and no launch; n = 0 returns PIPCK_OK."""
    import torch

    from pip_amd import _lib, engine

    lib = _lib.load()
    frames = _done_pool()[:70]
    n = len(frames)
    arena, lens, tile_off = _device(frames)
    engine.rx_verify_device(arena, lens, tile_off)  # this thread's last recorded launch: not the rewrite kernel
    before, last = arena.clone(), _last_kernel()
    assert "k_packedb_rx<" in last and KERNEL not in last
    done = torch.full((n,), POISON, dtype=torch.uint8, device="cuda")
    rules = _table(rule_table())
    a, nb, ln, to, dn = arena.data_ptr(), C.c_uint64(arena.numel()), lens.data_ptr(), tile_off.data_ptr(), done.data_ptr()
    rl, nr = rules.data_ptr(), rules.shape[0]
    assert a % 128 == 0 and rl % 16 == 0
    for args, why in (((None, nb, ln, to, n, rl, nr, None, 0, dn, None, None), "null arena"),
                      ((a, nb, None, to, n, rl, nr, None, 0, dn, None, None), "null lengths"),
                      ((a, nb, ln, None, n, rl, nr, None, 0, dn, None, None), "null index"),
                      ((a, nb, ln, to, n, rl, nr, None, 0, None, None, None), "null done"),
                      ((a, nb, ln, to, n, None, nr, None, 0, dn, None, None), "null rule table"),
                      ((a, nb, ln, to, n, rl, 0, None, 0, dn, None, None), "n_rules 0"),
                      ((a, nb, ln, to, n, rl + 8, nr - 1, None, 0, dn, None, None), "misaligned rule table"),
                      ((a + 64, nb, ln, to, n, rl, nr, None, 0, dn, None, None), "arena 64 mod 128"),
                      ((a + 16, nb, ln, to, n, rl, nr, None, 0, dn, None, None), "arena 16 mod 128"),
                      ((a, nb, ln, to, n, rl, nr, None, 2, dn, None, None), "unknown flag bit"),
                      ((a, nb, ln, to, n, rl, nr, None, 0x80000001, dn, None, None),
                       "unknown flag bit beside a known one"),
                      ((None, nb, None, None, n, None, 0, None, 4, None, None, None), "flags before pointers")):
        assert lib.pipck_fwd_rewrite_device(*args) == _lib.PIPCK_EINVAL, why
        assert b"pipck_fwd_rewrite_device" in lib.pipck_last_error(), why
        assert _last_kernel() == last, why
    assert b"flag" in lib.pipck_last_error()  # the flag check comes first
    assert lib.pipck_fwd_rewrite_device(None, 0, None, None, 0, None, 0, None, 0, None, None, None) == _lib.PIPCK_OK
    assert lib.pipck_fwd_rewrite_device(a, nb, ln, to, 0, rl, nr, None, 1, dn, None, None) == _lib.PIPCK_OK
    assert _last_kernel() == last
    torch.cuda.synchronize()
    assert torch.equal(arena, before) and bool((done == POISON).all())
    # the engine wrapper's own checks
    with pytest.raises(ValueError):
        engine.fwd_rewrite_device(arena, lens, tile_off, rules, n=n + 10 ** 6)
    with pytest.raises(ValueError):
        engine.fwd_rewrite_device(arena, lens, tile_off, rules.flatten())
    with pytest.raises(ValueError):
        engine.fwd_rewrite_device(arena, lens, tile_off, rules, rule_of=_i32(np.zeros(n - 1, dtype=np.uint32)))
    with pytest.raises(ValueError):
        engine.fwd_rewrite_device(arena[:arena.numel() // 2], lens, tile_off, rules)
    assert _last_kernel() == last
    torch.cuda.synchronize()
    assert torch.equal(arena, before) and bool((done == POISON).all())


# ---------------------------------------------------------------------------- 9. derived checks
@functools.lru_cache(maxsize=None)
def _verified_frames():
    """6,000 fuzz frames, the filled shaped frames (the IPv6 chains of 2 KiB among them) and
    the filled corner frames: all within 4,096 bytes."""
    frames = tuple(list(fuzz_frames()[:6000]) + list(filled("shaped")) + list(filled("corner")))
    assert max(map(len, frames)) <= 4096
    return frames


def test_fwd_device_keeps_every_rx_verdict():
    """pipck_rx_verify_device before and after a rewrite with the flag set gives the same verdict
    for every DONE frame (and for every other frame: it is untouched)."""
    from pip_amd import engine

    frames = list(_verified_frames())
    arena, lens, tile_off = _device(frames)
    before = engine.rx_verify_device(arena, lens, tile_off).cpu().numpy()
    assert np.array_equal(before, np.array([R.verdict(f) for f in frames], dtype=np.uint8))
    arena, lens, tile_off, done = _rewrite_and_check("pipck_fwd_rewrite_device (before RX)", frames, assign(frames),
                                                     F.UDP_ZERO_AS_ONES)
    after = engine.rx_verify_device(arena, lens, tile_off).cpu().numpy()
    rewritten = done.cpu().numpy() == F.DONE
    assert np.array_equal(after[rewritten], before[rewritten]), np.nonzero(rewritten & (after != before))[0][:8]
    assert (before[rewritten] == R.VERIFIED).sum() >= 1000
    assert np.array_equal(after[~rewritten], before[~rewritten])


@pytest.mark.parametrize("flags", FLAGS)
def test_fwd_device_equals_tx_fill_device_on_verified_frames(flags):
    """pipck_tx_fill_device on a copy of the rewritten arena changes no byte of a DONE frame that
    verified before, apart from 0x0000 against 0xFFFF in a checksum field."""
    from pip_amd import engine

    frames = list(_verified_frames())
    arena, lens, tile_off, done = _rewrite_and_check("pipck_fwd_rewrite_device (before TX fill)", frames,
                                                     assign(frames), flags)
    full = arena.clone()
    engine.tx_fill_device(full, lens, tile_off, flags=flags)
    assert "k_packedb_tx<" in _last_kernel()
    a, b = arena.cpu().numpy(), full.cpu().numpy()
    rewritten = done.cpu().numpy() == F.DONE
    starts = _starts(frames)
    checked = 0
    for i, f in enumerate(frames):
        if not rewritten[i] or R.verdict(f) != R.VERIFIED:
            continue
        checked += 1
        x, y = a[starts[i]:starts[i + 1]], b[starts[i]:starts[i + 1]]
        diff = np.nonzero(x != y)[0]
        if diff.size == 0:
            continue
        at = [k for k, _ in T.fields(bytes(x))]
        assert diff.size == 2 and diff[0] in at and diff[1] == diff[0] + 1 and \
            {bytes(x[diff]), bytes(y[diff])} == {b"\0\0", b"\xff\xff"}, (i, diff, f[:96].hex())
    assert checked >= 1000, checked
    assert np.array_equal(a[starts[-1]:], b[starts[-1]:])


def test_fwd_device_equals_fwd_rewrite_ring():
    """The same frames in the slots of a ring at stride 4,096 through pipck_fwd_rewrite_ring: the
    same frame bytes and the same done values."""
    import torch

    from pip_amd import engine

    frames = list(_verified_frames())
    n, stride = len(frames), 4096
    rule_of = assign(frames)
    arena, _, _, done = _rewrite_and_check("pipck_fwd_rewrite_device (before the ring)", frames, rule_of,
                                           F.UDP_ZERO_AS_ONES)
    ring = torch.from_numpy(ring_image(frames, stride, 4096)).to("cuda")
    ring_done = engine.fwd_rewrite_ring(ring, stride, torch.from_numpy(ring_lens(frames)).to("cuda"),
                                        _table(rule_table()), _i32(rule_of), n, flags=F.UDP_ZERO_AS_ONES)
    assert "k_fwd_ring" in _last_kernel()
    assert torch.equal(ring_done, done)
    a, r = arena.cpu().numpy(), ring.cpu().numpy()
    starts = _starts(frames)
    for i, f in enumerate(frames):
        assert np.array_equal(a[starts[i]:starts[i + 1]], r[i * stride:i * stride + len(f)]), i


# ---------------------------------------------------------------------------- 10. stream and graph
def test_fwd_device_on_a_side_stream_and_in_a_graph():
    """The call on a side stream; then captured into a graph -- one kernel, no branches -- and the
    graph replayed twice over fresh contents copied to the same addresses, each replay held to the
    reference (the second over other frames of the same lengths)."""
    import torch

    from pip_amd import engine

    rng = random.Random(77)
    pool = _done_pool()
    frames_a = [rng.choice(pool) for _ in range(300)]
    by_len = {}
    for f in pool:
        by_len.setdefault((len(f), f[0] >> 4), []).append(f)
    frames_b = [rng.choice(by_len[(len(f), f[0] >> 4)]) for f in frames_a]
    n = len(frames_a)
    rule_of = assign(frames_a)
    assert np.array_equal(rule_of, assign(frames_b))
    flags = F.UDP_ZERO_AS_ONES
    want = {k: _reference(fr, rule_of, flags) for k, fr in (("A", frames_a), ("B", frames_b))}
    assert (want["A"][1] == F.DONE).sum() >= 100
    stage = {k: torch.from_numpy(_blob(fr).copy()).to("cuda") for k, fr in (("A", frames_a), ("B", frames_b))}
    arena, lens, tile_off = _device(frames_a)
    rules, ro = _table(rule_table()), _i32(rule_of)
    done = torch.full((n + 32,), POISON, dtype=torch.uint8, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")

    def call():
        engine.fwd_rewrite_device(arena, lens, tile_off, rules, ro, n, flags=flags, done=done[16:n + 16], err=err)

    def check(path, which):
        torch.cuda.synchronize()
        fr = frames_a if which == "A" else frames_b
        _check(path, fr, arena.cpu().numpy(), _check_done(path, n, done), _blob(want[which][0]), want[which][1])
        assert int(err.item()) == 0

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    s.synchronize()
    assert KERNEL in _last_kernel()
    check("pipck_fwd_rewrite_device (side stream)", "A")
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    assert KERNEL in _last_kernel()
    for k, which in enumerate(("A", "B")):
        arena.copy_(stage[which])
        done.fill_(POISON)
        err.zero_()
        g.replay()
        check(f"pipck_fwd_rewrite_device (graph replay {k}, contents {which})", which)
