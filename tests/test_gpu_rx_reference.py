"""Every path that produces RX verdicts (include/pipck.h, PIPCK_RX_*) against
tests/rx_reference.py, a plain reference written from the header's prose and
the RFCs it cites -- bit for bit, and never one path against another:

    pipck_rx_verify               host rx_parse + k_rx_verify
    pipck_rx_verify_device        k_packedb_rx (rx_from_window)
    pipck_host_rx_verify_packed   the same kernel behind chunked DMA
    pipck_rx_verify_ring_n        k_ring, k_ring_rx, k_ring_slots

over a structured set (IPv4 options at every IHL, IPv6 upper-layer offsets
around the 80-byte register window, link padding across it, the 0x0000 / 0xFFFF
corners, malformed and long frames, each class at every start residue mod 16 of
the byte-packed layout) and a mutation fuzz built with rx_reference.build, so
that IPv4 frames carry options.  tests/test_rx_reference.py pins the reference
itself on the CPU."""
import ctypes as C
import functools
import random
import struct
from pathlib import Path

import numpy as np
import pytest

from tests import rx_reference as R
from tests.test_gpu_rx import (RING_KERNELS, _device_batch, _last_kernel, _ring, _ring_schedule, _run,
                               _rx_kernel_waves, _rxq, tile_waves)  # noqa: F401  (tile_waves: a fixture)

TABLE = Path(__file__).resolve().parent / "golden" / "rx_verdicts.txt"
HDR_ONLY = (1, 4, 5, 8, 10, 11)  # IPv4 header bytes that only the header checksum covers
PADDINGS = (1, 2, 3, 15, 16, 17, 63, 64, 130)
IP_ENDS = (59, 60, 79, 80, 81, 96)
SHORT = 420  # every class but the long ones stays within this many bytes


def table():
    """tests/golden/rx_verdicts.txt: [(frame, verdict, why)], labelled by hand."""
    out = []
    for ln in TABLE.read_text().splitlines():
        if ln and not ln.startswith("#"):
            head, why = ln.split(" # ", 1)
            v, hx = head.split()
            out.append((bytes.fromhex(hx), int(v), why))
    return out


def _variants(rng, frame):
    """The frame; one bit of its L4 message damaged; and, IPv4 only, one bit of a
    header byte that only the header checksum covers."""
    out = [frame]
    a, b = R.l4_range(frame)
    if b > a:
        q = bytearray(frame)
        q[rng.randrange(a, b)] ^= 1 << rng.randrange(8)
        out.append(bytes(q))
    if frame[0] >> 4 == 4:
        q = bytearray(frame)
        q[rng.choice(HDR_ONLY)] ^= 1 << rng.randrange(8)
        out.append(bytes(q))
    return out


def _udp4_zero_sum(rng, field):
    """UDP over IPv4 whose correct checksum computes to 0 (the exact sum with a
    zero field is a non-zero multiple of 0xFFFF), stored as `field`."""
    f = bytearray(R.build(rng, 4, R.UDP, 0, l4=rng.randbytes(6) + bytes(6), fill=False))
    f[26:28] = b"\0\0"
    s = R.wsum(f[20:]) + R.wsum(f[12:20]) + R.UDP + 12
    f[28:30] = struct.pack(">H", R.csum_field(s))  # a data word that brings the sum to k * 0xFFFF
    assert R.verifies(R.wsum(f[20:]) + R.wsum(f[12:20]) + R.UDP + 12)
    f[26:28] = struct.pack(">H", field)
    return bytes(f)


def _classes():
    """{class name: [frames]} of the structured set, in layout order."""
    rng = random.Random(2718)
    cls = {}

    # IPv4 with options: every IHL 6..15 x {TCP, UDP, UDP without checksum, ICMP, GRE}
    out = cls.setdefault("v4_options", [])
    for ihl in range(6, 16):
        for proto, nosum, least in ((R.TCP, False, 20), (R.UDP, False, 8), (R.UDP, True, 8), (R.ICMP, False, 8),
                                    (47, False, 0)):
            for l4len in (least, least + 1, 61, 300):
                out += _variants(rng, R.build(rng, 4, proto, l4len, options=rng.randbytes(4 * (ihl - 5)),
                                              no_udp_sum=nosum))

    # IPv6: the upper layer at every multiple of 8 from 48 to 104, behind 1-3 option headers
    out = cls.setdefault("v6_offsets", [])
    for off in range(48, 105, 8):
        units = (off - 40) // 8
        for nhdr in range(1, min(3, units) + 1):
            sizes = [1] * nhdr
            sizes[rng.randrange(nhdr)] += units - nhdr
            chain = [((R.HOPOPTS, R.DSTOPTS, R.DSTOPTS)[i], n - 1) for i, n in enumerate(sizes)]
            for proto in (R.TCP, R.UDP, R.ICMP6):
                for l4len in (R.MIN_L4[proto], 61, 300):
                    f = R.build(rng, 6, proto, l4len, ext=R.ext_chain(chain, proto))
                    assert R.l4_range(f)[0] == off
                    out += _variants(rng, f)

    # an atomic fragment header before, at and after byte 80 (and first), then the same with M set
    out = cls.setdefault("v6_fragment_header", [])
    for at in (40, 72, 80, 88):
        lead = [(R.DSTOPTS, (at - 40) // 8 - 1)] if at > 40 else []
        for proto in (R.TCP, R.UDP, R.ICMP6):
            for l4len in (R.MIN_L4[proto], 61):
                out += _variants(rng, R.build(rng, 6, proto, l4len, ext=R.ext_chain(lead + [(R.FRAGMENT, 0)], proto)))
            out.append(R.build(rng, 6, proto, 61, ext=R.ext_chain(lead + [(R.FRAGMENT, 1)], proto)))
            out.append(R.build(rng, 6, proto, 61, ext=R.ext_chain(lead + [(R.FRAGMENT, 0x0100)], proto)))

    # one header with Hdr Ext Len 255 (2,048 bytes): the upper layer far past the window
    out = cls.setdefault("v6_ext_len_255", [])
    for proto in (R.TCP, R.UDP, R.ICMP6):
        out += _variants(rng, R.build(rng, 6, proto, 61, ext=R.ext_chain([(R.DSTOPTS, 255)], proto)))

    # exactly 8 walkable headers (checked) and 9 (unchecked), and 8 before a routing header
    out = cls.setdefault("v6_chain_cap", [])
    eight = [(R.HOPOPTS, 0), (R.DSTOPTS, 0), (R.FRAGMENT, 0), (R.DSTOPTS, 0)] * 2
    for proto in (R.TCP, R.UDP, R.ICMP6):
        for chain in (eight, eight + [(R.DSTOPTS, 0)], eight + [(R.FRAGMENT, 0)], eight + [(R.ROUTING, 0)],
                      eight[:7], [(R.DSTOPTS, 1)] * 8, [(R.DSTOPTS, 1)] * 9):
            out += _variants(rng, R.build(rng, 6, proto, 61, ext=R.ext_chain(chain, proto)))

    # link padding after an IP length that ends below, on and above byte 80, odd and even
    out = cls.setdefault("link_padding", [])
    for end in IP_ENDS:
        for fam, proto in ((4, R.TCP), (4, R.UDP), (4, R.ICMP), (6, R.TCP), (6, R.UDP), (6, R.ICMP6)):
            l4len = end - (20 if fam == 4 else 40)
            if l4len < R.MIN_L4[proto]:
                continue  # a truncated payload: in malformed_and_truncated
            for pad in PADDINGS:
                for ff in (False, True):
                    f = R.build(rng, fam, proto, l4len)
                    assert len(f) == end
                    out += [v + (b"\xff" * pad if ff else rng.randbytes(pad)) for v in _variants(rng, f)]

    # the 0x0000 / 0xFFFF corners of the sum
    out = cls.setdefault("sum_corners", [])
    z = bytes
    out.append(R.build(rng, 4, R.ICMP, 0, l4=z(8), fill=False))                      # all zero: 5
    out.append(R.build(rng, 4, R.ICMP, 0, l4=z(64), fill=False))
    out.append(R.build(rng, 4, R.ICMP, 0, l4=z(8) + b"\xff\xff", fill=False))         # one ffff word: 7
    out.append(R.build(rng, 4, R.ICMP, 0, l4=z(70) + b"\xff\xff" + z(4), fill=False))  # past byte 80
    out.append(R.build(rng, 4, R.ICMP, 0, l4=z(62) + b"\xff\xff" + z(3), fill=False, options=z(8)))
    out.append(R.build(rng, 4, R.ICMP, 0, l4=z(2) + b"\xff\xff\xff\xff" + z(2), fill=False))  # exactly 2 x 0xFFFF
    out.append(R.build(rng, 4, R.ICMP, 0, l4=z(2) + b"\xff\xff" + z(90) + b"\xff\xff", fill=False))
    out.append(R.build(rng, 4, R.ICMP, 0, l4=b"\xff" * 64, fill=False))               # 32 x 0xFFFF
    out.append(R.build(rng, 4, R.ICMP, 0, l4=b"\xff" * 63, fill=False))
    out.append(R.build(rng, 4, R.ICMP, 0, l4=z(8)))                                   # zero message, field ffff
    for fam in (4, 6):
        for proto, sizes in ((R.TCP, (20, 21, 61, 300)), (R.UDP, (8, 9, 61, 300))):
            for n in sizes:
                out.append(R.build(rng, fam, proto, 0, l4=z(n)))                      # zero body, correct checksum
                out.append(R.build(rng, fam, proto, 0, l4=b"\xff" * n))
        out.append(R.build(rng, fam, R.UDP, 0, l4=rng.randbytes(6) + z(2) + rng.randbytes(12), fill=False))
    out.append(R.build(rng, 6, R.UDP, 0, l4=z(8), fill=False))                        # UDP/IPv6 field 0: 5
    for _ in range(3):
        out.append(_udp4_zero_sum(rng, 0xFFFF))                                       # computes to 0, sent as ffff: 7
        out.append(_udp4_zero_sum(rng, 0))                                            # sent as "none": 3
    assert all(len(f) <= SHORT for f in out)

    # malformed lengths and truncated L4 headers
    out = cls.setdefault("malformed_and_truncated", [])
    tcp4, tcp6 = R.build(rng, 4, R.TCP, 40), R.build(rng, 6, R.TCP, 40)
    out += [z(16), z(19), tcp4[:16], tcp4[:19], tcp6[:17], z(20), z(64)]
    out += [bytes([v << 4 | 5]) + tcp4[1:] for v in (0, 1, 3, 5, 7, 15)]               # not IPv4 / IPv6
    out += [tcp6[:n] for n in range(20, 40)]                                           # version 6 under 40 bytes
    out += [tcp6[:n] for n in (40, 59, 79)]                                            # 40 + payload > frame
    out += [tcp4[:n] for n in (20, 39, 59)]                                            # total length > frame
    for ihl in (0, 1, 4):
        out.append(bytes([0x40 | ihl]) + tcp4[1:])                                     # IHL < 5
    for options in (b"", rng.randbytes(4), rng.randbytes(40)):
        hl = 20 + len(options)
        whole = R.build(rng, 4, R.TCP, 40, options=options)
        for total in (0, 19, hl - 1, hl, len(whole) + 1, 0xFFFF):                      # total < header, = header, > frame
            q = bytearray(whole)
            q[2:4] = struct.pack(">H", total)
            q[10:12] = b"\0\0"
            q[10:12] = struct.pack(">H", R.csum_field(R.wsum(q[:hl])))
            out.append(bytes(q))
        for proto in (R.TCP, R.UDP, R.ICMP):
            for n in sorted({0, 1, 7, R.MIN_L4[proto] - 1}):
                out.append(R.build(rng, 4, proto, n, options=options))                 # L4 under its minimum
                out.append(R.build(rng, 4, proto, n, options=options) + rng.randbytes(30))
    for chain in ([], [(R.DSTOPTS, 0)], [(R.HOPOPTS, 2), (R.FRAGMENT, 0)]):
        for proto in (R.TCP, R.UDP, R.ICMP6):
            for n in sorted({0, 1, 7, R.MIN_L4[proto] - 1}):
                e = R.ext_chain(chain, proto) if chain else None
                out.append(R.build(rng, 6, proto, n, ext=e))
                out.append(R.build(rng, 6, proto, n, ext=e) + b"\xff" * 41)
    for units, cut in ((1, 4), (1, 7), (2, 8), (2, 15), (32, 100)):                    # a header that does not fit
        f = bytearray(R.build(rng, 6, R.UDP, 0, ext=R.ext_chain([(R.DSTOPTS, units - 1)], R.UDP)))
        f = f[:40 + cut]
        f[4:6] = struct.pack(">H", cut)
        out += [bytes(f), bytes(f) + rng.randbytes(70)]
    f = bytearray(R.build(rng, 6, R.UDP, 20, ext=R.ext_chain([(R.HOPOPTS, 0), (R.FRAGMENT, 0)], R.UDP)))
    f[4:6] = struct.pack(">H", 12)                                                     # half a fragment header
    out.append(bytes(f))
    assert all(len(f) <= SHORT for f in out)

    cls["table"] = [f for f, _, _ in table() if len(f) >= 16]

    # long frames (the 65,545-byte one is the host path's alone: HOST_ONLY)
    cls["long"] = [R.build(rng, 4, R.TCP, 65515), R.build(rng, 4, R.TCP, 8980)]
    assert [len(f) for f in cls["long"]] == [65535, 9000]

    # frames under 16 bytes, last: leaving them out moves no other frame
    cls["tiny"] = [b"\x45" + z(14), b"\x60" + z(9), b"\x45", b""]
    return cls


def _filler(delta):
    """A frame of 16 + delta bytes (verdict 0) that moves the next start by delta mod 16."""
    return bytes([0x25]) + bytes(15 + delta)


@functools.lru_cache(maxsize=None)
def structured_set():
    """(frames, class of each frame, start offset of each frame back to back).
    Laid out so that every class starts at every residue 0..15 mod 16 at least
    once (a class of fewer than 16 frames: each frame at a residue of its own),
    with filler frames and repeated frames where the lengths alone do not."""
    frames, names, off = [], [], 0

    def put(f, name):
        nonlocal off
        frames.append(f)
        names.append(name)
        off += len(f)

    def move_to(residue):
        delta = (residue - off) % 16
        if delta:
            put(_filler(delta), "filler")

    for name, members in _classes().items():
        seen = set()
        if len(members) < 16:
            for f in members:
                if off % 16 in seen:
                    move_to(min(set(range(16)) - seen))
                seen.add(off % 16)
                put(f, name)
            continue
        for f in members:
            seen.add(off % 16)
            put(f, name)
        short = [f for f in members if len(f) <= SHORT] or members
        for k, residue in enumerate(sorted(set(range(16)) - seen)):
            move_to(residue)
            put(short[k * 7 % len(short)], name)
    starts = np.concatenate([[0], np.cumsum([len(f) for f in frames])[:-1]]).astype(np.int64)
    return tuple(frames), tuple(names), starts


@functools.lru_cache(maxsize=None)
def host_only():
    """The 65,535-byte frame with 10 bytes of link padding: past every u16 length."""
    frames, names, _ = structured_set()
    f = frames[names.index("long")] + bytes(range(10))
    assert len(f) == 65545
    return f


@functools.lru_cache(maxsize=None)
def reference_verdicts():
    return np.array([R.verdict(f) for f in structured_set()[0]], dtype=np.uint8)


def assert_alignment(names, starts):
    """Every class at every start residue mod 16; a class under 16 frames, each
    frame at a residue of its own."""
    by_class = {}
    for name, s in zip(names, starts):
        by_class.setdefault(name, []).append(int(s) % 16)
    for name, res in by_class.items():
        if name == "filler":
            continue
        if len(res) < 16:
            assert len(set(res)) == len(res), (name, res)
        else:
            assert set(res) == set(range(16)), (name, sorted(set(range(16)) - set(res)))


def check(path, frames, starts, got, want):
    """got == want, or the first differing frames in full."""
    bad = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    assert bad.size == 0, f"{bad.size} of {len(frames)} frames differ on {path}: " + "; ".join(
        f"frame {i}: {frames[i][:96].hex()} length {len(frames[i])} start residue {int(starts[i]) % 16} "
        f"path {path} reference {int(want[i])} got {int(got[i])}" for i in map(int, bad[:4]))


@functools.lru_cache(maxsize=None)
def fuzz_frames():
    """20,000 frames by the recipe of test_rx_device_parser_fuzz_equals_host_parser
    (tests/test_gpu_rx.py) -- random protocol and next-header chains, fragment
    fields, header fields or any byte overwritten, truncation, link padding --
    built with rx_reference.build, so 40 % of the IPv4 frames carry 4-40 bytes
    of options."""
    rng = random.Random(77)
    frames = []
    for k in range(20000):
        fam = rng.choice([4, 6])
        proto = rng.choice([6, 17, 1, 58, 47]) if fam == 4 else rng.choice([6, 17, 58, 1, 50])
        ext = None
        if fam == 6 and rng.random() < 0.3:
            chain = [(rng.choice([0, 60, 44, 43]), rng.choice([0, 1, 3, 20])) for _ in range(rng.randint(1, 3))]
            chain = [(t, a if t != 44 else rng.choice([0, 1, 8])) for t, a in chain]
            ext = R.ext_chain(chain, proto)
        options = rng.randbytes(4 * rng.randint(1, 10)) if fam == 4 and rng.random() < 0.4 else b""
        p = bytearray(R.build(rng, fam, proto, rng.randint(0, 300), options=options, ext=ext,
                              frag=rng.choice([0, 0, 0, 0x2000, 0x0010]) if fam == 4 else 0,
                              no_udp_sum=(k + 1) % 7 == 0))
        for _ in range(rng.choice([0, 0, 1, 2])):  # mutate header fields or any byte
            i = rng.randrange(0, min(len(p), 64)) if rng.random() < 0.7 else rng.randrange(len(p))
            p[i] = rng.randrange(256)
        r = rng.random()
        if r < 0.1:
            p = p[:rng.randrange(0, len(p) + 1)]  # truncated
        elif r < 0.2:
            p += rng.randbytes(rng.randint(1, 120))  # link padding
        frames.append(bytes(p))
    return tuple(frames)


def assert_fuzz_condition(frames, want):
    """The fuzz reaches every verdict, and option-carrying frames that verify."""
    counts = np.bincount(want, minlength=8)
    assert counts.size == 8 and counts.min() >= 100, counts
    opts = sum(1 for f, w in zip(frames, want) if w == 7 and f[0] >> 4 == 4 and f[0] & 15 > 5)
    assert opts >= 300, opts


# ---- the paths -------------------------------------------------------------------


def _host_path(frames, pinned):
    """pipck_rx_verify over heap buffers, or over the same frames at odd
    addresses of one pinned block: (verdicts, address of each frame)."""
    lib, q = _rxq()
    try:
        if not pinned:
            bufs = [C.create_string_buffer(f, max(len(f), 1)) for f in frames]
            ptrs = [C.cast(b, C.c_void_p).value for b in bufs]
            return _run(lib, q, ptrs, [len(f) for f in frames]).copy(), ptrs
        base = lib.pipck_host_alloc(sum(len(f) + 8 for f in frames) + 64)
        assert base
        try:
            ptrs, off = [], 5
            for i, f in enumerate(frames):
                C.memmove(base + off, f, len(f))
                ptrs.append(base + off)
                off += len(f) + (i % 8)
            return _run(lib, q, ptrs, [len(f) for f in frames]).copy(), ptrs
        finally:
            assert lib.pipck_host_free(C.c_void_p(base)) == 0
    finally:
        lib.pipck_rxq_destroy(q)


@pytest.mark.gpu
@pytest.mark.parametrize("pinned", [False, True])
def test_rx_verify_against_the_reference(pinned):
    """pipck_rx_verify: the whole structured set and the frame of 65,545 bytes
    (u32 lengths), from the heap and in place from a pinned block at odd addresses."""
    frames, names, _ = structured_set()
    frames = list(frames) + [host_only()]
    want = np.append(reference_verdicts(), R.verdict(host_only()))
    got, ptrs = _host_path(frames, pinned)
    if pinned:
        assert len({p % 16 for p in ptrs}) == 16
    check("pipck_rx_verify (%s)" % ("pinned" if pinned else "heap"), frames, ptrs, got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("tiny", [True, False])
def test_rx_verify_device_against_the_reference(tile_waves, tiny):
    """pipck_rx_verify_device under each block width: with the frames under 16
    bytes (their tiles read headers from memory) and without (every tile streamed)."""
    from pip_amd import engine

    frames, names, starts = structured_set()
    want = reference_verdicts()
    keep = [i for i, f in enumerate(frames) if tiny or len(f) >= 16]
    assert tiny or (len(frames) - len(keep) == names.count("tiny") and keep == list(range(len(keep))))
    frames, names, starts, want = [frames[i] for i in keep], [names[i] for i in keep], starts[keep], want[keep]
    assert_alignment(names, starts)
    arena, lens, tile_off = _device_batch(frames)
    got = engine.rx_verify_device(arena, lens, tile_off).cpu().numpy()
    assert _rx_kernel_waves() == tile_waves
    check("pipck_rx_verify_device (%d waves)" % tile_waves, frames, starts, got, want)


@pytest.mark.gpu
def test_host_rx_verify_packed_against_the_reference():
    """pipck_host_rx_verify_packed: the structured set back to back in host memory."""
    from pip_amd import _lib

    frames, names, starts = structured_set()
    assert_alignment(names, starts)
    lib = _lib.load()
    blob = np.frombuffer(b"".join(frames) + bytes(32), dtype=np.uint8).copy()
    lens = np.array([len(f) for f in frames], dtype=np.uint16)
    ctx = C.c_void_p()
    assert lib.pipck_ctx_create(-1, C.byref(ctx)) == 0
    try:
        ok = np.full(len(frames), 0xEE, dtype=np.uint8)
        good = C.c_uint64(99)
        rc = lib.pipck_host_rx_verify_packed(ctx, blob.ctypes.data, lens.ctypes.data, len(frames), ok.ctypes.data,
                                             C.byref(good))
        assert rc == 0, lib.pipck_last_error()
    finally:
        lib.pipck_ctx_destroy(ctx)
    check("pipck_host_rx_verify_packed", frames, starts, ok, reference_verdicts())
    assert good.value == int((ok == R.VERIFIED).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", ["groups", "own", "coop", "rows", "slots"])
@pytest.mark.parametrize("stride", [1024, 9216])
def test_rx_verify_ring_against_the_reference(stride, schedule):
    """pipck_rx_verify_ring_n under each schedule: every frame that fits the slot."""
    import torch

    from pip_amd import engine

    frames, names, _ = structured_set()
    want = reference_verdicts()
    keep = [i for i, f in enumerate(frames) if len(f) <= stride]
    # no more than the long frames are left out: every frame of at most SHORT bytes, so every
    # class but the two long ones, is present at either stride
    long_ones = [i for i, f in enumerate(frames) if len(f) > SHORT]
    assert set(range(len(frames))) - set(keep) <= set(long_ones)
    assert {names[i] for i in long_ones} == {"long", "v6_ext_len_255"} and len(long_ones) <= 10
    assert {names[i] for i in keep} >= set(names) - {"long", "v6_ext_len_255"}
    sub = [frames[i] for i in keep]
    ring, lens = _ring(sub, stride)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    _ring_schedule(schedule)
    try:
        got = engine.rx_verify_ring(ring, stride, lens, err=err).cpu().numpy()
        assert RING_KERNELS[schedule] in _last_kernel()
    finally:
        engine.tune()
    assert int(err.item()) == 0
    check(f"pipck_rx_verify_ring_n (stride {stride}, {schedule})", sub, np.zeros(len(sub), dtype=np.int64), got,
          want[keep])


@pytest.mark.gpu
def test_rx_mutation_fuzz_against_the_reference():
    """20,000 mutated frames, 40 % of the IPv4 ones with options, through
    pipck_rx_verify and pipck_rx_verify_device (default block width): each
    equals the reference.  Every verdict 0..7 occurs at least 100 times and at
    least 300 option-carrying frames verify -- asserted before anything runs."""
    from pip_amd import engine

    frames = list(fuzz_frames())
    want = np.array([R.verdict(f) for f in frames], dtype=np.uint8)
    assert_fuzz_condition(frames, want)
    starts = np.concatenate([[0], np.cumsum([len(f) for f in frames])[:-1]])
    got, ptrs = _host_path(frames, False)
    check("pipck_rx_verify (heap)", frames, ptrs, got, want)
    arena, lens, tile_off = _device_batch(frames)
    dev = engine.rx_verify_device(arena, lens, tile_off).cpu().numpy()
    assert _rx_kernel_waves() == 4
    check("pipck_rx_verify_device", frames, starts, dev, want)
