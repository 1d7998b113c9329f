"""Saturated inputs and wide indices, with their expected values in Python
integers: the cases of tests/test_gpu_saturation.py, pinned on the CPU by
tests/test_saturation_reference.py.  numpy only (as a byte container and a
seeded generator); no torch, no ctypes, nothing of pip_amd.

Random bytes average 0x7FFF per 16-bit word and use half of an accumulator's
range; the inputs here use all of it.  Every expected value comes from the plain
references the suite already has:

    tests/verify_reference.py     the words of a range and the pseudo-header terms
    tests/host_sum_reference.py   word_sum (the same words, added up by numpy into
                                  Python integers) and fold
    tests/verify_sealing.py       the flow table: flow 0 all zero, flow 1 all 0xFF
                                  with protocol 255, the rest random

Fills.  Both apply to EVERY byte of an arena -- gaps, stride padding and the bytes
before and after the packets -- so a wrong tail mask adds the largest value there is:

    ff       every byte 0xFF
    dented   0xFF with one byte of every 64 (at a random place of each 64-byte
             block) replaced by a random byte: "about one in 64", and no packet of
             64 bytes or more is left without one

Chains.  pip folds after every segment (pip_checksum.cpp:110-112); the expected
value of a chain is that loop replayed on the segments' exact word sums:

    sum = pseudo-header terms            (0 without one)
    per segment:  sum = fold(fold((sum + W) mod 2^32))
    result = ~sum & 0xFFFF

so a chain of 70,001 segments, or one whose descriptors all alias the same bytes,
costs one word sum per DISTINCT segment.  total_len in the pseudo-header is the
u32 sum of the segment lengths (include/pipck.h).

Implicit flows.  Packet i of a batch without flow_of uses flow
((flow_origin + i) mod 2^64) mod n_flows (include/pipck.h).
"""
import functools

import numpy as np

from tests import host_sum_reference as hs
from tests import verify_reference as vr
from tests import verify_sealing as vs

NF = 97
FILLS = ("ff", "dented")
MASK32, MASK64 = (1 << 32) - 1, (1 << 64) - 1
PROTO = {4: 6, 6: 17}  # of the random flows (as tests/test_gpu_verify.py)

# the segment counts of the chain cases: a wrapping-u32 sum of folded 0xFFFF segment sums first
# differs from pip's loop at 65,538 segments (65,537 with a pseudo-header); see u32_model()
CHAIN_COUNTS = (65536, 65537, 65538, 70001)
# flow origins around 2^32 and 2^64, and table sizes: a power of two hides a 32-bit remainder
FLOW_ORIGINS = ((1 << 32) - 40, (1 << 32) - 1, 1 << 32, (1 << 64) - 200, (1 << 64) - 32, (1 << 64) - 1)
FLOW_COUNTS = (1, 3, 64, 65, 97)


@functools.lru_cache(maxsize=None)
def flows(fam: int):
    """(pipck_flow4 / pipck_flow6 records as bytes, the reference's tuple per flow)."""
    return vs.flow_table(np.random.default_rng(4000 + fam), fam, NF, PROTO[fam])


def arena(fill: str, size: int, *key) -> np.ndarray:
    """`size` bytes of fill "ff" or "dented" (seeded by key)."""
    a = np.full(size, 0xFF, dtype=np.uint8)
    if fill == "dented":
        rng = np.random.default_rng([64, size, *key])
        blocks = (size + 63) // 64
        at = np.arange(blocks) * 64 + rng.integers(0, 64, blocks)
        keep = at < size
        a[at[keep]] = rng.integers(0, 256, blocks, dtype=np.uint8)[keep]
    else:
        assert fill == "ff", fill
    return a


# ----------------------------------------------------------------------------
# single packets
# ----------------------------------------------------------------------------
def words(b) -> int:
    """Exact sum of the big-endian 16-bit words of b (odd last byte: high byte)."""
    return hs.word_sum(b)


def pseudo_terms(pseudo, total_len: int) -> int:
    """Address words + protocol + hi16(total_len) + lo16(total_len); 0 without a pseudo-header."""
    if pseudo is None:
        return 0
    _, src, dst, proto = pseudo
    return vr._words(bytes(src)) + vr._words(bytes(dst)) + proto + (total_len >> 16) + (total_len & 0xFFFF)


def fold16(s: int) -> int:
    while s >> 16:
        s = hs.fold(s)
    return s


def ones_sum(data, pseudo=None) -> int:
    """verify_reference.ones_sum, with numpy adding up the words (64 KiB packets by the hundred)."""
    b = bytes(data)
    return fold16(words(b) + pseudo_terms(pseudo, len(b)))


def checksum(data, pseudo=None) -> int:
    return 0xFFFF ^ ones_sum(data, pseudo)


def verdict(data, pseudo=None) -> int:
    return 1 if ones_sum(data, pseudo) == 0xFFFF else 0


def implicit_flow(flow_origin: int, i: int, n_flows: int) -> int:
    return ((flow_origin + i) & MASK64) % n_flows


def flow_indices(flow_origin: int, n: int, n_flows: int) -> np.ndarray:
    return np.array([implicit_flow(flow_origin, i, n_flows) for i in range(n)], dtype=np.int64)


def batch(host: np.ndarray, offs, lens, pseudo_of) -> np.ndarray:
    """checksum() of every packet (uint16)."""
    return np.array([checksum(host[int(o):int(o) + int(n)], pseudo_of(i)) for i, (o, n) in enumerate(zip(offs, lens))],
                    dtype=np.uint16)


def seal_last_word(host: np.ndarray, offs, lens, pseudo_of, skip=lambda i: False) -> None:
    """Store each packet's checksum, computed with its last whole word zeroed, big-endian into that
    word, in place (packets under 2 bytes and those `skip` names are left alone).  The field is the
    last word so that the rest of a saturated packet stays saturated."""
    for i, (o, n) in enumerate(zip(offs, lens)):
        o, n = int(o), int(n)
        if n < 2 or skip(i):
            continue
        at = o + ((n - 2) & ~1)
        host[at:at + 2] = 0
        c = checksum(host[o:o + n], pseudo_of(i))
        host[at], host[at + 1] = c >> 8, c & 0xFF


def verdicts(host: np.ndarray, offs, lens, pseudo_of) -> np.ndarray:
    return np.array([verdict(host[int(o):int(o) + int(n)], pseudo_of(i)) for i, (o, n) in enumerate(zip(offs, lens))],
                    dtype=np.uint8)


def distinct_per_tile(results: np.ndarray) -> int:
    """The smallest number of distinct values among the full 64-packet tiles of `results`."""
    full = len(results) // 64
    assert full >= 1
    return min(len(set(results[64 * t:64 * t + 64].tolist())) for t in range(full))


# ----------------------------------------------------------------------------
# fixed-stride batches
# ----------------------------------------------------------------------------
def fixed_batch(fill: str, stride: int, length: int, n: int, fam: int, flow_origin: int = 0, n_flows: int = NF):
    """(host bytes with 16 bytes of fill before and after, the offset of packet 0 in them,
    expected checksums).  Implicit flows of family fam (0: no pseudo-header)."""
    host = arena(fill, 16 + n * stride + 16, stride, length, n, fam)
    offs, lens = 16 + np.arange(n, dtype=np.int64) * stride, np.full(n, length, dtype=np.int64)
    return host, 16, batch(host, offs, lens, pseudo_of(fam, flow_indices(flow_origin, n, n_flows)))


def pseudo_of(fam: int, flow_idx):
    if not fam:
        return lambda i: None
    table = flows(fam)[1]
    return lambda i: table[int(flow_idx[i])]


def sealed_fixed_batch(fill: str, stride: int, length: int, n: int, fam: int, flow_origin: int = 0,
                       n_flows: int = NF):
    """fixed_batch with every packet's last word sealed, then every third packet damaged (one bit
    of a byte before the field); returns (host, offset of packet 0, expected verdicts)."""
    host = arena(fill, 16 + n * stride + 16, stride, length, n, fam, 1)
    offs, lens = 16 + np.arange(n, dtype=np.int64) * stride, np.full(n, length, dtype=np.int64)
    ps = pseudo_of(fam, flow_indices(flow_origin, n, n_flows))
    seal_last_word(host, offs, lens, ps)
    damage(host, offs, lens, [stride, length, n, fam])
    return host, 16, verdicts(host, offs, lens, ps)


def damage(host, offs, lens, key) -> None:
    """Flip one bit in every third packet of at least 3 bytes, before its last whole word."""
    rng = np.random.default_rng([3, *key])
    for i, (o, n) in enumerate(zip(offs, lens)):
        if i % 3 == 1 and n >= 3:
            host[int(o) + int(rng.integers(0, (int(n) - 2) & ~1 or 1))] ^= 1 << int(rng.integers(0, 8))


# ----------------------------------------------------------------------------
# chains
# ----------------------------------------------------------------------------
def chain_replay(word_sums, lens, pseudo=None) -> int:
    """pip_inet{,6}_checksum_buf on segments given by their exact word sums and lengths."""
    total_len = sum(int(n) for n in lens) & MASK32
    s = pseudo_terms(pseudo, total_len) & MASK32
    for w in word_sums:
        s = hs.fold(hs.fold((s + int(w)) & MASK32))
    return 0xFFFF ^ (s & 0xFFFF)


def chain_checksum(host: np.ndarray, offs, lens, pseudo=None) -> int:
    """chain_replay over the segments host[off:off + len], each DISTINCT segment summed once.
    A chain of no segments is pip's one empty segment."""
    cache = {}
    ws = []
    for o, n in zip(offs, lens):
        o, n = int(o), int(n)
        key = host[o:o + n].tobytes() if n <= 16 else (o, n)  # short segments: by their bytes
        if key not in cache:
            cache[key] = words(host[o:o + n])
        ws.append(cache[key])
    return chain_replay(ws or [0], lens, pseudo)


def u32_model(n_segs: int, seg_fold: int, pseudo_total: int) -> int:
    """What a kernel gives that adds the segments' folded sums into a u32 with no fold between
    them and then folds (pseudo_total + F) mod 2^32: the model of the finding this module's
    chain counts were chosen for."""
    F = (n_segs * seg_fold) & MASK32
    return 0xFFFF ^ fold16((pseudo_total + F) & MASK32)
