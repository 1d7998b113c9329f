"""A plain reference of the per-call exact path (include/pipck.h, pipck_host_sum)
and the table of inputs it is held to.

The rule is pip's loop (pip_checksum.cpp:13-33, chained as at :110-112), in
Python integers:

    s = init mod 2^32
    for each segment:  s = (s + W) mod 2^32;  s = fold(fold(s))
    W = the sum of the segment's big-endian 16-bit words, an odd last byte
        being the high byte of a zero-padded word -- separately per segment

fold(x) = (x & 0xFFFF) + (x >> 16); an empty list is one empty segment.  numpy
only adds up a segment's even-offset and odd-offset bytes (W = 256 * A + B);
both totals become Python integers before anything else happens to them, so no
fixed-width arithmetic is part of the reference.  No ctypes, no oracle, nothing
of pip_amd.  tests/test_host_sum_reference.py holds this module to pip first;
tests/test_gpu_host_sum.py then holds every mode of pipck_host_sum to it.

chain_sum_nowrap() is the same loop without the "mod 2^32", and wraps() says
whether a segment's addition passed 2^32: together they show that a table case
can tell an accumulator that wraps from one that does not.

The table (table(), stale_sequence()) is seeded: a case is rebuilt from its
name alone.  Classes:

    counts     chains of 0..200 segments, lengths cycling through LENGTH_CYCLE
    tiny       thousands of one-byte and empty segments
    inline     1..5 segments around the resident block's 2,048-chunk pass
    wrap       initial sums near 2^32 on short data, and a wrap in a later segment
    threshold  staged bytes at and one chunk past ZERO_COPY_MAX
"""
import functools
from collections import namedtuple

import numpy as np

MASK32 = 0xFFFFFFFF
# pipck_host_sum serves a request zero-copy (mode 2) or through the resident
# block (modes 3, 4) while its staged bytes -- need() -- stay within this
ZERO_COPY_MAX = 68 << 10
# the resident block sums chains of up to this many segments in its one-pass loop
INLINE_SEGS = 5

Case = namedtuple("Case", "name cls segs init")

COUNTS = (0, 1, 2, 4, 5, 6, 7, 8, 63, 64, 65, 66, 127, 128, 129, 130, 200)
LENGTH_CYCLE = (0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 255, 256, 257)
COUNT_INITS = (0, 0xFFFF, 0x10000, 0xFFFF0000, 0xFFFFFFFF, None)  # None: one random u32
WRAP_INITS = (0xFFFFFFFF, 0xFFFFFF00, 0xFFFF0000)
WRAP_LENGTHS = (1, 2, 3, 20, 1480)
WRAP_CHAINS = (1, 5, 6, 65)
CLASSES = ("counts", "tiny", "inline", "wrap", "threshold")


# ----------------------------------------------------------------------------
# the rule
# ----------------------------------------------------------------------------
def word_sum(seg) -> int:
    """Exact sum of the big-endian 16-bit words of seg (odd last byte: high byte)."""
    a = np.frombuffer(bytes(seg), dtype=np.uint8)
    even = int(a[0::2].sum(dtype=np.uint64))
    odd = int(a[1::2].sum(dtype=np.uint64))
    return 256 * even + odd


def fold(x: int) -> int:
    return (x & 0xFFFF) + (x >> 16)


def chain_sum(segs, init: int) -> int:
    s = init & MASK32
    for seg in (segs if len(segs) else [b""]):
        s = (s + word_sum(seg)) & MASK32
        s = fold(fold(s))
    return s


def chain_sum_nowrap(segs, init: int) -> int:
    """chain_sum with an accumulator that never wraps (what a wider register would give)."""
    s = init & MASK32
    for seg in (segs if len(segs) else [b""]):
        s = s + word_sum(seg)
        s = fold(fold(s))
    return s


def wraps(segs, init: int) -> bool:
    """True iff some segment's addition passes 2^32 in chain_sum."""
    s = init & MASK32
    for seg in (segs if len(segs) else [b""]):
        s += word_sum(seg)
        if s > MASK32:
            return True
        s = fold(fold(s & MASK32))
    return False


# ----------------------------------------------------------------------------
# the staging arithmetic of pipck_host_sum
# ----------------------------------------------------------------------------
def _up16(n: int) -> int:
    return (n + 15) & ~15


def need(lens) -> int:
    """Staged bytes of a request: the 16-byte-per-segment table, then every
    segment padded to 16 bytes (pipck_host_sum: need = table + padded bytes)."""
    return _up16(16 * len(lens)) + sum(_up16(n) for n in lens)


def case_need(case) -> int:
    return need([len(s) for s in case.segs])


def threshold_lengths(nseg: int, over: bool):
    """nseg equal-as-possible segment lengths whose need() is exactly
    ZERO_COPY_MAX (over=False), or whose last segment is one byte longer, which
    costs one more 16-byte chunk (over=True)."""
    room = ZERO_COPY_MAX - _up16(16 * nseg)
    assert room % 16 == 0 and room // 16 >= nseg
    chunks = [room // 16 // nseg] * nseg
    chunks[0] += room // 16 - sum(chunks)
    lens = [16 * c for c in chunks]
    if over:
        lens[-1] += 1
    return lens


# ----------------------------------------------------------------------------
# the table
# ----------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng([20261020, *key])


def _rand(rng, n: int) -> bytes:
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _u32(rng) -> int:
    return int(rng.integers(0, 1 << 32, dtype=np.uint64))


def _counts():
    out = []
    for nseg in COUNTS:
        for k, init in enumerate(COUNT_INITS):
            rng = _rng(1, nseg, k)
            off = int(rng.integers(0, len(LENGTH_CYCLE)))
            segs = [_rand(rng, LENGTH_CYCLE[(off + i) % len(LENGTH_CYCLE)]) for i in range(nseg)]
            tag = "rand" if init is None else "%08x" % init
            out.append(Case("counts_n%d_%s" % (nseg, tag), "counts", segs, _u32(rng) if init is None else init))
    return out


def _tiny():
    rng = _rng(2)
    return [
        Case("tiny_2000x1", "tiny", [_rand(rng, 1) for _ in range(2000)], _u32(rng)),
        Case("tiny_2200x1", "tiny", [_rand(rng, 1) for _ in range(2200)], _u32(rng)),
        Case("tiny_4000x0", "tiny", [b""] * 4000, 0x12345678),
    ]


def _inline():
    out = []
    shapes = [[n] for n in (32767, 32768, 32769, 32784, 65535)]
    shapes += [[0, 13000, 1, 0, 20001], [16, 0, 16], [0, 0, 0, 0, 7], [7, 0, 0, 0, 0], [6553] * 5]
    # a zero-length segment at the first, the middle and the last place
    fill = (33, 1, 4097, 17, 255)
    for n in (2, 3, 5):
        for pos in sorted({0, n // 2, n - 1}):
            shapes.append([0 if i == pos else fill[i] for i in range(n)])
    for k, lens in enumerate(shapes):
        rng = _rng(3, k)
        out.append(Case("inline_" + "_".join(map(str, lens)), "inline", [_rand(rng, n) for n in lens], _u32(rng)))
    return out


def _wrap():
    out = []
    for a, init in enumerate(WRAP_INITS):
        for n in WRAP_LENGTHS:
            for nseg in WRAP_CHAINS:
                rng = _rng(4, a, n, nseg)
                out.append(Case("wrap_%08x_%dB_rand_x%d" % (init, n, nseg), "wrap",
                                [_rand(rng, n) for _ in range(nseg)], init))
                out.append(Case("wrap_%08x_%dB_ff_x%d" % (init, n, nseg), "wrap", [b"\xff" * n] * nseg, init))
    rng = _rng(5)
    # the wrap happens in a later segment: 65,538 words of 0xFFFF pass 2^32 on their own
    for init in (0, 0xFFFF, _u32(rng)):
        out.append(Case("wrap_later_3_131076ff_5_%08x" % init, "wrap",
                        [_rand(rng, 3), b"\xff" * 131076, _rand(rng, 5)], init))
    # more wraps on requests over ZERO_COPY_MAX (staged in modes 2-4, zero-copy in mode 1)
    out.append(Case("wrap_big_70000ff_fffffff0", "wrap", [b"\xff" * 70000], 0xFFFFFFF0))
    out.append(Case("wrap_big_2200x1_ffffffff", "wrap", [b"\x80"] + [_rand(rng, 1) for _ in range(2199)], 0xFFFFFFFF))
    out.append(Case("wrap_big_7x9999_ffff8000", "wrap", [_rand(rng, 9999) for _ in range(7)], 0xFFFF8000))
    return out


def _threshold():
    out = []
    for nseg in (1, 2):
        for over in (False, True):
            rng = _rng(6, nseg, int(over))
            lens = threshold_lengths(nseg, over)
            out.append(Case("threshold_%s_%s" % ("over" if over else "at", "_".join(map(str, lens))), "threshold",
                            [_rand(rng, n) for n in lens], 0xFFFF0000))
    return out


@functools.lru_cache(maxsize=None)
def table():
    """Every independent case, built once per process; never modified."""
    cases = tuple(_counts() + _tiny() + _inline() + _wrap() + _threshold())
    assert len({c.name for c in cases}) == len(cases)
    return cases


@functools.lru_cache(maxsize=None)
def expected():
    """name -> chain_sum of every table() case, computed once per process."""
    return {c.name: chain_sum(c.segs, c.init) for c in table()}


def by_class(cls: str):
    return [c for c in table() if c.cls == cls]


def _zero_calls(tag: str):
    out = [Case("stale_%s_zero_%d" % (tag, n), "stale", [bytes(n)], 0) for n in range(49)]
    out.append(Case("stale_%s_zero_1_17_33" % tag, "stale", [bytes(1), bytes(17), bytes(33)], 0))
    out.append(Case("stale_%s_zero_1_17_33_x2" % tag, "stale", [bytes(1), bytes(17), bytes(33)] * 2, 0))
    return out


@functools.lru_cache(maxsize=None)
def stale_sequence():
    """An ORDERED sequence for one context: 0xFF-filled calls leave 0xFF in the
    staging buffer, and the all-zero calls after them sum to 0 only if nothing
    past a segment's length is added.  The 1.5 MiB call outgrows the staging
    buffer's first allocation (1 MiB), so the calls after it run on a new one."""
    seq = [Case("stale_fill_4096ff", "stale", [b"\xff" * 4096], 0)]
    seq += _zero_calls("a")
    seq.append(Case("stale_grow_1572864ff", "stale", [b"\xff" * (3 << 19)], 0))
    seq += _zero_calls("b")
    return tuple(seq)
