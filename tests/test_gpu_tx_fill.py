"""pipck_tx_fill_device (include/pipck.h, k_packedb_tx in pip_amd/csrc/pipck_packedb.hip)
against tests/tx_reference.py, the plain reference written from the header's prose:
every assertion compares the WHOLE arena after the call, byte for byte, with the
arena built from tx_reference.fill -- so a byte stored outside a frame's two
checksum fields fails like a wrong checksum does -- and the done bytes with the
reference's.  tests/test_tx_reference.py pins the reference itself on the CPU."""
import functools
import random

import numpy as np
import pytest

from tests import rx_reference as R
from tests import tx_reference as T
from tests.test_gpu_rx import _last_kernel, tile_waves  # noqa: F401  (tile_waves: a fixture)
from tests.test_gpu_rx_reference import assert_alignment, fuzz_frames, structured_set
from tests.test_tx_reference import CORNER_KINDS, corner_frames, pip_frames, preset, shaped_frames

GUARD = bytes((37 * i + 11) & 0xFF for i in range(256))  # after the last frame: must come back unchanged
PRESETS = ("zero", "random", "correct")


def _starts(frames):
    return np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64)


def _blob(frames):
    """The frames back to back and the guard pattern after the last one."""
    return np.frombuffer(b"".join(frames) + GUARD, dtype=np.uint8)


def _device(frames):
    """(arena, lens, tile_off) on the device: the byte-packed layout, the guard inside the arena."""
    import torch

    from pip_amd import engine

    arena = torch.from_numpy(_blob(frames).copy()).to("cuda")
    lens = torch.from_numpy(np.array([len(f) for f in frames], dtype=np.uint16).view(np.int16)).to("cuda")
    return arena, lens, engine.packed_bytes_index(lens)


def _reference(frames, flags):
    """(the arena the call must leave, its done bytes) by tx_reference.fill."""
    filled = [T.fill(f, flags) for f in frames]
    return _blob([f for f, _ in filled]), np.array([d for _, d in filled], dtype=np.uint8)


def _tx_kernel_waves():
    name = _last_kernel().split("(")[0]
    assert "k_packedb_tx<" in name, name
    return int(name.rsplit(",", 1)[1].rstrip("> "))


def _check(path, frames, got_arena, got_done, want_arena, want_done):
    """Whole arenas and done bytes equal, or the first differing frames in full."""
    got_arena, got_done = np.asarray(got_arena), np.asarray(got_done)
    assert got_arena.shape == want_arena.shape and got_done.shape == want_done.shape
    if np.array_equal(got_arena, want_arena) and np.array_equal(got_done, want_done):
        return
    starts = _starts(frames)
    bad_bytes = np.nonzero(got_arena != want_arena)[0]
    bad = sorted(set(np.searchsorted(starts, bad_bytes, side="right") - 1) | set(np.nonzero(got_done != want_done)[0]))
    msgs = []
    for i in map(int, bad[:4]):
        if i >= len(frames):
            msgs.append("the guard after the last frame was written")
            continue
        a, b = int(starts[i]), int(starts[i + 1])
        where = [int(k) - a for k in bad_bytes if a <= k < b][:8]
        msgs.append(f"frame {i}: {frames[i][:96].hex()} length {b - a} start {a} (mod 16: {a % 16}) bytes differing at "
                    f"{where} got {bytes(got_arena[a:b][where]).hex()} want {bytes(want_arena[a:b][where]).hex()} "
                    f"done got {int(got_done[i])} want {int(want_done[i])}")
    raise AssertionError(f"{len(bad)} of {len(frames)} frames differ on {path}: " + "; ".join(msgs))


def _fill_and_check(path, frames, flags, waves=None, reference=None):
    """One call on a fresh arena of `frames`, held to the reference (computed here
    unless given); returns the device arena, lengths, index and done bytes."""
    import torch

    from pip_amd import engine

    arena, lens, tile_off = _device(frames)
    done = torch.full((len(frames),), 0xEE, dtype=torch.uint8, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    engine.tx_fill_device(arena, lens, tile_off, flags=flags, done=done, err=err)
    if waves is not None:
        assert _tx_kernel_waves() == waves
    want_arena, want_done = reference or _reference(frames, flags)
    _check(path, frames, arena.cpu().numpy(), done.cpu().numpy(), want_arena, want_done)
    assert int(err.item()) == 0
    return arena, lens, tile_off, done


def _filler(n):
    """A frame of n >= 16 bytes that is not written (version 2)."""
    return bytes([0x25]) + bytes(n - 1)


@functools.lru_cache(maxsize=None)
def tx_structured():
    """(frames, names, starts): the RX reference test's structured set (every class
    at every start residue mod 16, the 65,535-byte frame) without its frames under
    16 bytes; then the corner frames and frames whose IPv4 header, TCP and UDP
    checksum fields each straddle a 128-byte line (the field's first byte is a
    line's last) -- all of these in streamed tiles; then, from a tile boundary,
    the corner and straddling frames once more followed by the frames under 16
    bytes, whose tile is summed lane per frame."""
    frames, names, off = [], [], 0
    rng = random.Random(128)

    def put(f, name):
        nonlocal off
        frames.append(f)
        names.append(name)
        off += len(f)

    def corners_and_straddles(tag):
        for kind, f, _ in corner_frames():
            put(f, tag + "corner_" + kind)
        r = random.Random(129)
        for fam, proto, options, ext in ((4, R.TCP, b"", None), (4, R.UDP, b"", None),
                                         (4, R.TCP, r.randbytes(40), None), (6, R.TCP, b"", None),
                                         (6, R.UDP, b"", None), (6, R.UDP, b"", R.ext_chain([(R.DSTOPTS, 9)], R.UDP))):
            f = R.build(r, fam, proto, 75, options=options, ext=ext, fill=False)
            at = R.l4_range(f)[0] + R.CSUM_AT[proto]
            for field in ([10] if fam == 4 else []) + [at]:  # once per field: its first byte at 127 mod 128
                put(_filler(16 + (127 - field - off - 16) % 128), "filler")
                assert (off + field) % 128 == 127
                put(f, tag + "straddle")

    rx_frames, rx_names, _ = structured_set()
    tiny = [f for f, n in zip(rx_frames, rx_names) if n == "tiny"]
    assert tiny and all(len(f) < 16 for f in tiny) and rx_names[-len(tiny):] == ("tiny",) * len(tiny)
    for f, n in zip(rx_frames[:-len(tiny)], rx_names):
        put(f, n)
    corners_and_straddles("")
    while len(frames) % 64:
        put(_filler(16 + rng.randrange(32)), "filler")
    corners_and_straddles("lane_")
    for f in tiny:
        put(f, "tiny")
    return tuple(frames), tuple(names), _starts(frames)[:-1]


@functools.lru_cache(maxsize=None)
def _structured_preset(how):
    rng = random.Random(PRESETS.index(how))
    return tuple(preset(rng, f, how) for f in tx_structured()[0])


@functools.lru_cache(maxsize=None)
def _structured_reference(how, flags):
    return _reference(_structured_preset(how), flags)


@functools.lru_cache(maxsize=None)
def _fuzz_reference(flags):
    return _reference(fuzz_frames(), flags)


@pytest.mark.gpu
def test_tx_fill_structured_set(tile_waves):
    """The structured set, the corner frames and the line-straddling fields, each
    frame's fields pre-set to zero, to random bytes and to their correct value,
    under each block width and both flag values."""
    frames, names, starts = tx_structured()
    n_rx = len(structured_set()[0]) - names.count("tiny")
    assert_alignment(names[:n_rx], starts[:n_rx])
    assert any(len(f) == 65535 for f in frames)
    lane_tiles = {i // 64 for i, f in enumerate(frames) if len(f) < 16}  # tiles summed lane per frame
    for tag in ("", "lane_"):  # every corner kind and every straddling field, streamed and in the lane path
        mine = [i for i, n in enumerate(names) if n.startswith(tag + "corner_") or n == tag + "straddle"]
        assert all((i // 64 in lane_tiles) == bool(tag) for i in mine), tag
        assert {names[i] for i in mine} == {tag + "corner_" + k for k in CORNER_KINDS} | {tag + "straddle"}
        line = {"ip": 0, "tcp": 0, "udp": 0}
        for i in mine:
            if names[i].endswith("straddle"):
                for at, bit in T.fields(frames[i]):
                    if (int(starts[i]) + at) % 128 == 127:
                        kind = "ip" if bit == T.IP_FILLED else "tcp" if at - R.l4_range(frames[i])[0] == 16 else "udp"
                        line[kind] += 1
        assert min(line.values()) >= 2, (tag, line)
    for how in PRESETS:
        for flags in (0, T.UDP_ZERO_AS_ONES):
            _fill_and_check(f"pipck_tx_fill_device ({tile_waves} waves, fields {how}, flags {flags})",
                            list(_structured_preset(how)), flags, waves=tile_waves,
                            reference=_structured_reference(how, flags))


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, T.UDP_ZERO_AS_ONES])
def test_tx_fill_mutation_fuzz(flags):
    """The 20,000 mutated frames of the RX reference test.  The reference's done
    reaches each of 0, 1, 2 and 3 at least 100 times -- asserted before the GPU runs."""
    frames = list(fuzz_frames())
    counts = np.bincount(_fuzz_reference(flags)[1], minlength=4)
    assert counts.size == 4 and counts.min() >= 100, counts
    _fill_and_check(f"pipck_tx_fill_device (fuzz, flags {flags})", frames, flags, waves=4,
                    reference=_fuzz_reference(flags))


@pytest.mark.gpu
def test_tx_fill_batch_sizes_and_the_lane_path():
    """1, 63, 64, 65 and 129 frames (a tile's last lane, a partial last tile, two
    tile boundaries), and a tile that mixes one frame under 16 bytes with jumbo
    frames (summed lane per frame, headers read from memory)."""
    rng = random.Random(65)
    pool = [f for f in shaped_frames() if len(f) < 2200]
    for n in (1, 63, 64, 65, 129):
        _fill_and_check(f"pipck_tx_fill_device ({n} frames)", rng.sample(pool, n), 0)
    jumbo = [R.build(rng, fam, proto, n, fill=False) for fam, proto, n in
             ((4, R.TCP, 8980), (6, R.UDP, 8960), (4, R.UDP, 65515), (6, R.TCP, 9001), (4, R.ICMP, 4001))]
    jumbo.append(R.build(rng, 6, R.ICMP6, 3000, ext=R.ext_chain([(R.HOPOPTS, 40)], R.ICMP6), fill=False) + bytes(99))
    mixed = jumbo[:3] + [b"\x45" + bytes(9)] + jumbo[3:] + rng.sample(pool, 70)  # 64 in the lane path, 13 streamed
    assert len(mixed[3]) < 16 and len(mixed) > 64
    for flags in (0, 1):
        _fill_and_check(f"pipck_tx_fill_device (a frame under 16 B among jumbo frames, flags {flags})", mixed, flags)


@functools.lru_cache(maxsize=None)
def _mixed_frames():
    """3,000 fuzz frames, the shaped frames and the corner frames."""
    return tuple(list(fuzz_frames()[:3000]) + shaped_frames() + [f for _, f, _ in corner_frames()])


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, T.UDP_ZERO_AS_ONES])
def test_tx_fill_twice_changes_no_byte(flags):
    """A second call on the filled arena: the field is taken as zero, so nothing changes."""
    import torch

    from pip_amd import engine

    frames = list(_mixed_frames())
    arena, lens, tile_off, done = _fill_and_check("pipck_tx_fill_device (first call)", frames, flags)
    once = arena.clone()
    again = engine.tx_fill_device(arena, lens, tile_off, flags=flags)
    assert torch.equal(arena, once) and torch.equal(again, done)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, T.UDP_ZERO_AS_ONES])
def test_tx_fill_then_rx_verify_round_trip(flags):
    """Derived check: pipck_rx_verify_device on the filled arena gives
    rx_reference.verdict of the reference-filled frames."""
    from pip_amd import engine

    frames = list(_mixed_frames())
    arena, lens, tile_off, _ = _fill_and_check("pipck_tx_fill_device (before RX)", frames, flags)
    want = np.array([R.verdict(T.fill(f, flags)[0]) for f in frames], dtype=np.uint8)
    got = engine.rx_verify_device(arena, lens, tile_off).cpu().numpy()
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    assert (want == R.VERIFIED).sum() > 1000


@pytest.mark.gpu
def test_tx_fill_bounded_by_the_arena(tile_waves):
    """A tile index that sends one middle tile and the last tile past arena_bytes:
    those tiles are neither read nor written, their frames get done 0 and
    PIPCK_ERANGE is set; every other tile is filled as without the tampering.
    d_err = NULL is accepted.  (No Python guard: the C ABI directly.)"""
    import torch

    from pip_amd import _lib

    lib = _lib.load()
    rng = random.Random(9)
    frames = rng.sample([f for f in shaped_frames() if len(f) < 2200], 5 * 64 + 7)
    frames[2 * 64 + 1] = frames[-1] = shaped_frames()[0]  # TCP over IPv4: both fields to fill, in each refused tile
    n, tiles = len(frames), 6
    starts = _starts(frames)
    want_arena, want_done = _reference(frames, 0)
    want_arena, want_done = want_arena.copy(), want_done.copy()
    for t in (2, tiles - 1):  # the tampered tiles: as they were, done 0
        a, b = int(starts[64 * t]), int(starts[min(64 * (t + 1), n)])
        want_arena[a:b] = _blob(frames)[a:b]
        want_done[64 * t:64 * (t + 1)] = 0
    for with_err in (True, False):
        arena, lens, tile_off = _device(frames)
        nbytes = arena.numel()
        assert int(tile_off[tiles].item()) == nbytes - len(GUARD)
        tile_off[2] = nbytes - 5  # starts inside the arena, ends past it
        tile_off[tiles - 1] = nbytes + 4096  # starts past it
        done = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        rc = lib.pipck_tx_fill_device(arena.data_ptr(), nbytes, lens.data_ptr(), tile_off.data_ptr(), n, 0,
                                      done.data_ptr(), err.data_ptr() if with_err else None, None)
        assert rc == 0, lib.pipck_last_error()
        torch.cuda.synchronize()
        assert _tx_kernel_waves() == tile_waves
        _check("pipck_tx_fill_device (tiles 2 and 5 past the arena)", frames, arena.cpu().numpy(), done.cpu().numpy(),
               want_arena, want_done)
        assert int(err.item()) == ((1 << _lib.PIPCK_ERANGE) if with_err else 0)
    filled = _reference(frames, 0)[1]
    assert filled[64 * 2:64 * 3].max() == 3 and filled[64 * 5:].max() == 3  # the refused tiles had work to refuse


@pytest.mark.gpu
def test_tx_fill_argument_errors_launch_nothing():
    """Unknown flag bits, a misaligned arena and null pointers: PIPCK_EINVAL and
    no launch; n = 0 returns PIPCK_OK."""
    import torch

    from pip_amd import _lib

    lib = _lib.load()
    frames = shaped_frames()[:70]
    from pip_amd import engine

    arena, lens, tile_off = _device(frames)
    engine.rx_verify_device(arena, lens, tile_off)  # this thread's last recorded launch: not the TX kernel
    before, last = arena.clone(), _last_kernel()
    assert "k_packedb_rx<" in last
    n = len(frames)
    done = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    a, nb, ln, to, dn = arena.data_ptr(), arena.numel(), lens.data_ptr(), tile_off.data_ptr(), done.data_ptr()
    assert a % 128 == 0
    for args, why in (((a, nb, ln, to, n, 2, dn, None, None), "unknown flag bit"),
                      ((a, nb, ln, to, n, 0x80000001, dn, None, None), "unknown flag bit beside a known one"),
                      ((a + 64, nb - 64, ln, to, n, 0, dn, None, None), "misaligned arena"),
                      ((None, nb, ln, to, n, 0, dn, None, None), "null arena"),
                      ((a, nb, None, to, n, 0, dn, None, None), "null lengths"),
                      ((a, nb, ln, None, n, 0, dn, None, None), "null index"),
                      ((a, nb, ln, to, n, 0, None, None, None), "null done")):
        assert lib.pipck_tx_fill_device(*args) == _lib.PIPCK_EINVAL, why
        assert b"pipck_tx_fill_device" in lib.pipck_last_error(), why
        assert _last_kernel() == last, why
    assert lib.pipck_tx_fill_device(None, 0, None, None, 0, 0, None, None, None) == _lib.PIPCK_OK
    assert lib.pipck_tx_fill_device(a, nb, ln, to, 0, 1, dn, None, None) == _lib.PIPCK_OK
    assert _last_kernel() == last
    torch.cuda.synchronize()
    assert torch.equal(arena, before) and bool((done == 0xEE).all())


@pytest.mark.gpu
def test_tx_fill_writes_pips_wire_bytes():
    """The packets pip's compiled stack emitted (tests/golden/stack_replay.txt),
    their checksum fields scrambled, in one arena: filled, they are pip's bytes."""
    rng = random.Random(11)
    pkts = pip_frames()
    scrambled = [preset(rng, p, "random") for p in pkts]
    assert all(q != p for p, q in zip(pkts, scrambled))
    arena, _, _, done = _fill_and_check("pipck_tx_fill_device (pip's packets)", scrambled, 0)
    assert arena.cpu().numpy().tobytes() == b"".join(pkts) + GUARD
    assert done.cpu().numpy().tolist() == [3 if p[0] >> 4 == 4 else 2 for p in pkts]
