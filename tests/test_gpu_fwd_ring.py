"""pipck_fwd_rewrite_ring (include/pipck.h, k_fwd_ring in pip_amd/csrc/pipck_fwd.hip)
against tests/fwd_reference.py: every assertion compares the WHOLE ring after the
call, byte for byte -- the frames, the non-zero pattern that fills each slot
behind its frame, and the guard after the last slot -- with the ring built from
fwd_reference.rewrite, and the done bytes, inside a poisoned buffer, with the
reference's.  So a store outside the named fields and their two checksum fields,
a store into a frame that is not DONE and a done byte outside [0, n) fail like a
wrong checksum does.  The rule table, the assignment and the frame sets:
tests/test_fwd_reference.py."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

from tests import fwd_reference as F
from tests import rx_reference as R
from tests import tx_reference as T
from tests.test_fwd_reference import (DPORT, DST4, SPORT, SRC4, assign, far_tcp_frames, filled, fuzz_ring_frames,
                                      reference_rewrite, rule_index, rule_table)
from tests.test_gpu_rx import _last_kernel
from tests.test_gpu_rx_reference import fuzz_frames, structured_set
from tests.test_gpu_tx_fill_ring import GUARD, POISON, _check
from tests.test_tx_ring_cases import ring_image, ring_lens

pytestmark = pytest.mark.gpu

KERNEL = "k_fwd_ring"
FLAGS = (0, F.UDP_ZERO_AS_ONES)


def _table(rules, device="cuda"):
    from pip_amd import engine

    return engine.make_fwd_rules(list(rules), device=device)


def _rewrite_and_check(path, frames, stride, rule_of, flags, rules=None, reference=None, guard=GUARD):
    """One call on a fresh ring of `frames` under rules[rule_of[i]] (rule 0 where rule_of is
    None), held to the reference (computed here unless given: (frames, done)); returns the
    device ring, lengths and the poisoned done buffer."""
    import torch

    from pip_amd import engine

    rules = rule_table() if rules is None else rules
    n = len(frames)
    ring = torch.from_numpy(ring_image(frames, stride, guard)).to("cuda")
    lens = torch.from_numpy(ring_lens(frames)).to("cuda")
    done = torch.full((n + 32,), POISON, dtype=torch.uint8, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    ro = None if rule_of is None else torch.from_numpy(np.asarray(rule_of, dtype=np.uint32).view(np.int32)).to("cuda")
    got = engine.fwd_rewrite_ring(ring, stride, lens, _table(rules), ro, n, flags=flags, done=done[16:n + 16], err=err)
    assert KERNEL in _last_kernel(), _last_kernel()
    assert got.data_ptr() == done.data_ptr() + 16
    want_frames, want_done = reference or reference_rewrite(frames, [0] * n if rule_of is None else rule_of, flags,
                                                            rules)
    _check(path, frames, stride, ring.cpu().numpy(), done.cpu().numpy(), ring_image(want_frames, stride, guard),
           want_done)
    assert int(err.item()) == 0
    return ring, lens, done


@functools.lru_cache(maxsize=None)
def _fuzz_reference(flags):
    frames = fuzz_ring_frames()
    return reference_rewrite(frames, assign(frames), flags)


@pytest.mark.parametrize("flags", FLAGS)
def test_fwd_ring_mutation_fuzz(flags):
    """The 20,000 mutated frames of the RX reference test and the planted-TTL frames in
    1,024-byte slots, family by the version nibble and the seven ops sets cycling."""
    frames = list(fuzz_ring_frames())
    counts = np.bincount(_fuzz_reference(flags)[1], minlength=5)
    assert counts[F.DONE] >= 5000 and counts[F.UNHANDLED] >= 5000 and counts[0] >= 1000 and counts[F.EXPIRED] >= 200
    _rewrite_and_check(f"pipck_fwd_rewrite_ring (fuzz, flags {flags})", frames, 1024, assign(frames), flags,
                       reference=_fuzz_reference(flags))


@functools.lru_cache(maxsize=None)
def _structured(stride):
    """The structured set: every frame that fits; at 65,536 the frames over 9,216 bytes and 64 others."""
    frames, _, _ = structured_set()
    if stride < 65536:
        return tuple(f for f in frames if len(f) <= stride)
    rng = random.Random(65536)
    long_ones = [f for f in frames if len(f) > 9216]
    assert long_ones and max(map(len, long_ones)) == 65535
    return tuple(long_ones + rng.sample([f for f in frames if len(f) <= 9216], 64))


@pytest.mark.parametrize("stride", [1024, 9216, 65536])
def test_fwd_ring_structured_set(stride):
    """IPv4 options at every IHL, extension chains around and past the 96-byte window, link
    padding, the 0x0000 / 0xFFFF corners, malformed and long frames: every frame under every
    ops set of its family (the assignment shifted seven times), both flag values in turn."""
    frames = list(_structured(stride))
    if stride >= 9216:
        far = far_tcp_frames()
        assert far and (stride == 65536 or all(f in frames for f in far))
    for shift in range(7):
        rule_of = np.array([rule_index(f, (i + shift) % 7) for i, f in enumerate(frames)], dtype=np.uint32)
        flags = FLAGS[shift & 1]
        _rewrite_and_check(f"pipck_fwd_rewrite_ring (structured set, stride {stride}, shift {shift}, flags {flags})",
                           frames, stride, rule_of, flags)


@pytest.mark.parametrize("which,stride", [("shaped", 2048), ("corner", 2048), ("pip", 9216)])
def test_fwd_ring_filled_frames(which, stride):
    """Frames whose checksums verify -- every family, protocol, option length and extension
    shape; the corners of the sum; the packets pip's stack emitted -- under both flag values."""
    frames = [f for f in filled(which) if len(f) <= stride]
    assert len(frames) >= 20 and (which == "shaped" or len(frames) == len(filled(which)))
    for shift in (0, 3):
        rule_of = np.array([rule_index(f, (i + shift) % 7) for i, f in enumerate(frames)], dtype=np.uint32)
        for flags in FLAGS:
            _rewrite_and_check(f"pipck_fwd_rewrite_ring ({which} frames, shift {shift}, flags {flags})", frames, stride,
                               rule_of, flags)


def _done_pool(stride=1024):
    """Filled shaped frames that the all-ops rule of their family rewrites."""
    return [f for f in filled("shaped")
            if len(f) <= stride and F.rewrite(f, rule_table()[rule_index(f, 3)])[1] == F.DONE]


def test_fwd_ring_slot_counts():
    """A lone slot, and partial last blocks for a wave of 64 and a block of 256 slots."""
    rng = random.Random(257)
    pool = [f for f in filled("shaped") if len(f) <= 2048]
    for n in (1, 63, 64, 65, 129, 255, 256, 257):
        frames = [rng.choice(pool) for _ in range(n)]
        _rewrite_and_check(f"pipck_fwd_rewrite_ring ({n} slots)", frames, 2048, assign(frames), 0)


def test_fwd_ring_without_rule_of_every_slot_takes_rule_0():
    rng = random.Random(3)
    frames = rng.sample([f for f in filled("shaped") if len(f) <= 1024], 300)
    for rules in ((rule_table()[3], rule_table()[10]),  # all five ops on IPv4: the IPv6 frames are UNHANDLED
                  (F.rule(F.DEC_TTL | F.SET_SPORT, 0, sport=SPORT),)):
        want = reference_rewrite(frames, [0] * len(frames), 0, rules)
        assert (want[1] == F.DONE).sum() >= 50 and (want[1] == F.UNHANDLED).sum() >= 50
        _rewrite_and_check("pipck_fwd_rewrite_ring (d_rule_of NULL)", frames, 1024, None, 0, rules=rules,
                           reference=want)


REFUSAL_RULES = (rule_table()[3], rule_table()[10],  # all five ops, family 4 and family 6
                 F.rule(F.ALL_OPS | 32, 4, SRC4, DST4, SPORT, DPORT),  # an unknown ops bit
                 F.rule(F.ALL_OPS, 5, SRC4, DST4, SPORT, DPORT),  # family 5
                 F.rule(F.SET_SRC | F.DEC_TTL, 0, SRC4))  # family 0 with an address
ERANGE_BIT, EINVAL_BIT = 1 << 2, 1 << 1
# kind -> (planted length, planted rule index, the bit d_err must hold)
REFUSALS = {"length 1,025": (1025, None, ERANGE_BIT), "length 65,535": (65535, None, ERANGE_BIT),
            "rule index n_rules": (None, len(REFUSAL_RULES), ERANGE_BIT),
            "rule index 0xFFFFFFFE": (None, 0xFFFFFFFE, ERANGE_BIT),
            "unknown ops bit": (None, 2, EINVAL_BIT), "family 5": (None, 3, EINVAL_BIT),
            "family 0 with SET_SRC": (None, 4, EINVAL_BIT), "PIPCK_FWD_NO_RULE": (None, 0xFFFFFFFF, 0)}


@pytest.mark.parametrize("kind", list(REFUSALS))
def test_fwd_ring_refusals(kind):
    """Each kind planted at a wave's and a block's first and last slot and at the ring's last
    slot, over frames that would be DONE: those slots are unchanged with done 0, d_err holds
    exactly the expected bit (none for PIPCK_FWD_NO_RULE), and every other slot is as without
    the tampering.  d_err = NULL is accepted.  The C ABI directly, no Python guard; 65 KiB of
    guard after the last slot, so a kernel that honoured a planted length would stay inside
    the allocation and show in the comparison; the rule table ends where its allocation ends,
    so an index past it has nothing mapped to read."""
    import torch

    from pip_amd import _lib

    assert (ERANGE_BIT, EINVAL_BIT) == (1 << _lib.PIPCK_ERANGE, 1 << _lib.PIPCK_EINVAL)
    lib = _lib.load()
    stride, guard = 1024, 65 * 1024
    rng = random.Random(1025)
    n = 2 * 256 + 7
    frames = [rng.choice(_done_pool()) for _ in range(n)]
    rule_of = np.array([int(f[0] >> 4 == 6) for f in frames], dtype=np.uint32)
    clean_frames, clean_done = reference_rewrite(frames, rule_of, 0, REFUSAL_RULES)
    assert (clean_done == F.DONE).all()
    plants = (64, 127, 256, 511, n - 1)
    length, index, bit = REFUSALS[kind]
    lens_host = ring_lens(frames).copy().view(np.uint16)
    want_frames, want_done = list(clean_frames), clean_done.copy()
    for i in plants:
        if length is not None:
            lens_host[i] = length
        else:
            rule_of[i] = index
        want_frames[i], want_done[i] = frames[i], 0
    table = torch.empty(2 << 20, dtype=torch.uint8, device="cuda")  # a segment of its own: the table at its end
    raw = _table(REFUSAL_RULES)
    table[-raw.numel():] = raw.flatten()
    rules_ptr = table.data_ptr() + table.numel() - raw.numel()
    assert rules_ptr % 16 == 0
    for with_err in (True, False):
        ring = torch.from_numpy(ring_image(frames, stride, guard)).to("cuda")
        lens = torch.from_numpy(lens_host.view(np.int16)).to("cuda")
        ro = torch.from_numpy(rule_of.view(np.int32)).to("cuda")
        done = torch.full((n + 32,), POISON, dtype=torch.uint8, device="cuda")
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        assert ring.numel() == n * stride + guard and guard >= 65536
        rc = lib.pipck_fwd_rewrite_ring(ring.data_ptr(), stride, lens.data_ptr(), n, rules_ptr, len(REFUSAL_RULES),
                                        ro.data_ptr(), 0, done.data_ptr() + 16, err.data_ptr() if with_err else None,
                                        None)
        assert rc == 0, lib.pipck_last_error()
        torch.cuda.synchronize()
        assert KERNEL in _last_kernel()
        _check(f"pipck_fwd_rewrite_ring ({kind} at {plants})", frames, stride, ring.cpu().numpy(), done.cpu().numpy(),
               ring_image(want_frames, stride, guard), want_done)
        assert int(err.item()) == (bit if with_err else 0)


def test_fwd_ring_argument_errors_launch_nothing():
    """Null pointers, a misaligned arena or rule table, no rules, strides outside the rule and
    unknown flag bits: PIPCK_EINVAL with the function's name, and no launch; n = 0 returns
    PIPCK_OK."""
    import torch

    from pip_amd import _lib, engine

    lib = _lib.load()
    stride = 1024
    frames = _done_pool()[:70]
    n = len(frames)
    ring = torch.from_numpy(ring_image(frames, stride, GUARD)).to("cuda")
    lens = torch.from_numpy(ring_lens(frames)).to("cuda")
    engine.rx_verify_ring(ring, stride, lens, n)  # this thread's last recorded launch: not the rewrite kernel
    before, last = ring.clone(), _last_kernel()
    assert "k_ring<" in last and KERNEL not in last
    done = torch.full((n,), POISON, dtype=torch.uint8, device="cuda")
    rules = _table(rule_table())
    a, ln, dn, rl, nr = ring.data_ptr(), lens.data_ptr(), done.data_ptr(), rules.data_ptr(), rules.shape[0]
    assert a % 16 == 0 and rl % 16 == 0
    u64 = C.c_uint64
    for args, why in (((None, u64(stride), ln, n, rl, nr, None, 0, dn, None, None), "null arena"),
                      ((a, u64(stride), None, n, rl, nr, None, 0, dn, None, None), "null lengths"),
                      ((a, u64(stride), ln, n, rl, nr, None, 0, None, None, None), "null done"),
                      ((a, u64(stride), ln, n, None, nr, None, 0, dn, None, None), "null rule table"),
                      ((a, u64(stride), ln, n, rl, 0, None, 0, dn, None, None), "n_rules 0"),
                      ((a, u64(stride), ln, n, rl + 8, nr - 1, None, 0, dn, None, None), "misaligned rule table"),
                      ((a + 8, u64(stride), ln, n, rl, nr, None, 0, dn, None, None), "misaligned arena"),
                      ((a, u64(1008), ln, n, rl, nr, None, 0, dn, None, None), "stride under 1,024"),
                      ((a, u64(1032), ln, n, rl, nr, None, 0, dn, None, None), "stride no multiple of 16"),
                      ((a, u64(65552), ln, 1, rl, nr, None, 0, dn, None, None), "stride over 65,536"),
                      ((a, u64(0), ln, n, rl, nr, None, 0, dn, None, None), "stride 0"),
                      ((a, u64((1 << 32) + 1024), ln, 1, rl, nr, None, 0, dn, None, None), "stride 1,024 mod 2^32"),
                      ((a, u64(stride), ln, n, rl, nr, None, 2, dn, None, None), "unknown flag bit"),
                      ((a, u64(stride), ln, n, rl, nr, None, 0x80000001, dn, None, None),
                       "unknown flag bit beside a known one")):
        assert lib.pipck_fwd_rewrite_ring(*args) == _lib.PIPCK_EINVAL, why
        assert b"pipck_fwd_rewrite_ring" in lib.pipck_last_error(), why
        assert _last_kernel() == last, why
    assert lib.pipck_fwd_rewrite_ring(None, 0, None, 0, None, 0, None, 0, None, None, None) == _lib.PIPCK_OK
    assert lib.pipck_fwd_rewrite_ring(a, u64(stride), ln, 0, rl, nr, None, 1, dn, None, None) == _lib.PIPCK_OK
    assert _last_kernel() == last
    torch.cuda.synchronize()
    assert torch.equal(ring, before) and bool((done == POISON).all())
    # the engine wrapper's own checks
    with pytest.raises(ValueError):
        engine.fwd_rewrite_ring(ring, stride, lens, rules, n=n + 10 ** 6)
    with pytest.raises(ValueError):
        engine.fwd_rewrite_ring(ring, stride, lens, rules.flatten())
    assert _last_kernel() == last


@functools.lru_cache(maxsize=None)
def _verified_frames():
    """6,000 fuzz frames, the filled shaped frames (the IPv6 chains of 2 KiB among them) and
    the filled corner frames: all within 4,096 bytes."""
    frames = tuple(list(fuzz_frames()[:6000]) + list(filled("shaped")) + list(filled("corner")))
    assert max(map(len, frames)) <= 4096
    return frames


def test_fwd_ring_keeps_every_rx_verdict():
    """Derived check: pipck_rx_verify_ring_n before and after a rewrite with the flag set gives
    the same verdict for every DONE slot."""
    from pip_amd import engine

    frames = list(_verified_frames())
    n = len(frames)
    import torch

    ring = torch.from_numpy(ring_image(frames, 4096, GUARD)).to("cuda")
    lens = torch.from_numpy(ring_lens(frames)).to("cuda")
    before = engine.rx_verify_ring(ring, 4096, lens, n).cpu().numpy()
    assert np.array_equal(before, np.array([R.verdict(f) for f in frames], dtype=np.uint8))
    ring, lens, done = _rewrite_and_check("pipck_fwd_rewrite_ring (before RX)", frames, 4096, assign(frames),
                                          F.UDP_ZERO_AS_ONES)
    after = engine.rx_verify_ring(ring, 4096, lens, n).cpu().numpy()
    rewritten = done.cpu().numpy()[16:n + 16] == F.DONE
    assert np.array_equal(after[rewritten], before[rewritten]), np.nonzero(rewritten & (after != before))[0][:8]
    assert (before[rewritten] == R.VERIFIED).sum() >= 1000
    assert np.array_equal(after[~rewritten], before[~rewritten])


@pytest.mark.parametrize("flags", FLAGS)
def test_fwd_ring_equals_tx_fill_ring_on_verified_frames(flags):
    """Second derived check: pipck_tx_fill_ring on a copy of the rewritten ring changes no byte
    of a DONE frame that verified before, apart from 0x0000 against 0xFFFF in a checksum field."""
    from pip_amd import engine

    frames = list(_verified_frames())
    n, stride = len(frames), 4096
    ring, lens, done = _rewrite_and_check("pipck_fwd_rewrite_ring (before TX fill)", frames, stride, assign(frames),
                                          flags)
    full = ring.clone()
    engine.tx_fill_ring(full, stride, lens, n, flags=flags)
    assert "k_ring_tx<" in _last_kernel()
    a, b = ring.cpu().numpy(), full.cpu().numpy()
    rewritten = done.cpu().numpy()[16:n + 16] == F.DONE
    checked = 0
    for i, f in enumerate(frames):
        if not rewritten[i] or R.verdict(f) != R.VERIFIED:
            continue
        checked += 1
        x, y = a[i * stride:i * stride + len(f)], b[i * stride:i * stride + len(f)]
        diff = np.nonzero(x != y)[0]
        if diff.size == 0:
            continue
        at = [k for k, _ in T.fields(bytes(x))]
        assert diff.size == 2 and diff[0] in at and diff[1] == diff[0] + 1 and \
            {bytes(x[diff]), bytes(y[diff])} == {b"\0\0", b"\xff\xff"}, (i, diff, f[:96].hex())
    assert checked >= 1000, checked
    assert np.array_equal(a[n * stride:], b[n * stride:])
