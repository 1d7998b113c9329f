"""The seams of the host-memory paths, with their expected values: the cases of
tests/test_gpu_host_paths.py, pinned on the CPU by tests/test_host_path_cases.py.
numpy only; no torch, no ctypes, nothing of pip_amd, no oracle.

The host ABI (include/pipck.h: pipck_host_checksum_fixed,
pipck_host_checksum_packed_bytes, pipck_host_rx_verify_packed, pipck_txq_*,
pipck_rx_verify) wraps kernels that other tests already hold to references.
What it adds is ordering, offsets and buffer reuse: chunks cut at a byte or a
packet count, two device buffers taken in turn, staging that grows while
records hold offsets into it, holds on pinned ranges.  A case here puts a batch
ON such a seam, and is built so that the likely mistakes give another answer:

    * packets come from a pool of a few hundred distinct ones, cycled; the pool
      size divides no chunk size, so packet i and packet i + m (m: the packets
      of i's chunk) are different packets and a stale or swapped buffer shows;
    * no chunk size is a multiple of the 97 flows, so an implicit flow that
      restarts at every chunk (wrong model a) picks other flows;
    * results written at chunk-relative offsets (wrong model b) leave the tail
      of the result array at its poison.

Expected values come only from the plain references already in the tree:
saturation_cases.checksum / chain_checksum / pseudo_terms / implicit_flow /
flows, and rx_reference.verdict / build.  A packet's word sum is computed once
per DISTINCT packet (saturation_cases.words); combining it with the per-index
pseudo-header terms is vectorised, with the sums asserted below 2^63.
"""
import functools
import random
import struct
from collections import namedtuple

import numpy as np

from tests import rx_reference as R
from tests import saturation_cases as sc

NF = sc.NF
POISON = 0xA5
POISON16 = 0xA5A5

# The seam constants, restated.  tests/test_host_path_cases.py reads the lines
# that define them in pip_amd/csrc and fails when one no longer matches.
HOST_CHUNK_BYTES = 64 << 20      # pipck_host.hip: a fixed chunk is 64 MiB / stride packets; a packed chunk closes at >= this
HOST_CHUNK_PACKETS = 1 << 20     # pipck_host.hip: ... or at this many packets
RX_FIRST_LAUNCH = 1024           # pipck_rx.hip: packets of the first launch of a call
RX_LAUNCH = 4096                 # pipck_rx.hip: packets of every later launch
RX_STAGE_BYTES = 64 << 10        # pipck_rx.hip: first size of the staging of unpinned packets
TX_STAGE_BYTES = 1 << 20         # pipck_txq.hip: first size of a batch's staging
TX_INPLACE_MAX = 32 << 20        # pipck_txq.hip: largest flush that runs without copy commands
MAX_LEN = 65535

PIPCK_OK, PIPCK_EINVAL, PIPCK_ERANGE = 0, 1, 2


# ----------------------------------------------------------------------------
# combining word sums with per-index pseudo-header terms
# ----------------------------------------------------------------------------
def flow_indices(origin: int, n: int, nf: int) -> np.ndarray:
    """saturation_cases.implicit_flow of packets 0..n-1, in uint64 arithmetic (which wraps at 2^64
    as the rule does); the ends and the wrap are checked against the rule itself."""
    idx = (np.full(n, origin, dtype=np.uint64) + np.arange(n, dtype=np.uint64)) % np.uint64(nf)
    probe = {0, n - 1, n // 2}
    wrap = (1 << 64) - origin
    probe |= {i for i in (wrap - 1, wrap, wrap + 1) if 0 <= i < n}
    for i in probe:
        assert int(idx[i]) == sc.implicit_flow(origin, i, nf), (origin, i)
    return idx.astype(np.int64)


@functools.lru_cache(maxsize=None)
def _flow_terms(fam: int, nf: int) -> np.ndarray:
    """pseudo_terms of each flow at length 0 (the length adds itself: lengths here are below 2^16)."""
    table = sc.flows(fam)[1]
    assert sc.pseudo_terms(table[2], 0x1234) == sc.pseudo_terms(table[2], 0) + 0x1234
    return np.array([sc.pseudo_terms(table[f], 0) for f in range(nf)], dtype=np.uint64)


def combine(wsums: np.ndarray, lens: np.ndarray, fam: int, flow_idx) -> np.ndarray:
    """checksum() of packets given by word sum and length: ~fold(W + pseudo_terms(flow, len))."""
    s = wsums.astype(np.uint64)
    if fam:
        assert int(lens.max(initial=0)) <= MAX_LEN
        s = s + _flow_terms(fam, int(np.max(flow_idx)) + 1)[flow_idx] + lens.astype(np.uint64)
    assert int(s.max(initial=0)) < 1 << 63
    while (s >> np.uint64(16)).any():
        s = (s & np.uint64(0xFFFF)) + (s >> np.uint64(16))
    return (np.uint64(0xFFFF) ^ s).astype(np.uint16)


def chunk_relative(want: np.ndarray, chunks, poison) -> np.ndarray:
    """Wrong model (b): every chunk's results stored from element 0 of the result array."""
    out = np.full(len(want), poison, dtype=want.dtype)
    first = 0
    for m in chunks:
        out[:m] = want[first:first + m]
        first += m
    return out


def shifted_differs(want: np.ndarray, chunks) -> float:
    """The share of packets i whose result differs from packet i + m's and from packet i + 2m's
    (m: the packets of i's chunk), over those i with a packet i + m."""
    n = len(want)
    m = np.repeat(np.asarray(chunks, dtype=np.int64), chunks)
    i = np.arange(n, dtype=np.int64)
    one = i + m < n
    assert one.any()
    differs = want[i[one]] != want[i[one] + m[one]]
    two = i[one] + 2 * m[one] < n
    differs[two] &= want[i[one][two]] != want[i[one][two] + 2 * m[one][two]]
    return float(differs.mean())


# ----------------------------------------------------------------------------
# fixed stride: pipck_host_checksum_fixed
# ----------------------------------------------------------------------------
Fixed = namedtuple("Fixed", "name stride length pool_size per_chunk arena_packets families prefixes")


def _fixed(name, stride, length, pool_size, families, whole):
    pc = max(1, HOST_CHUNK_BYTES // stride)
    n = 2 * pc + 1 if whole else pc + 1
    return Fixed(name, stride, length, pool_size, pc, n, families, (pc - 1, pc, pc + 1, n) if whole else (n,))


FIXED = {f.name: f for f in (
    _fixed("s65536", 65536, 65535, 251, (0, 4, 6), True),   # len < stride: the copy ends one byte short
    _fixed("s65521", 65521, 65521, 251, (0, 4, 6), True),   # odd: every chunk starts at another residue
    _fixed("s9216", 9216, 8980, 509, (0, 4, 6), True),
    _fixed("s20", 20, 20, 509, (0,), False),                # IPv4 headers, no pseudo-header
)}


def fixed_origins(f: Fixed):
    """0, 5, just below 2^32, and one that puts the 2^64 wrap inside chunk 1."""
    return (0, 5, (1 << 32) - 3, (1 << 64) - f.per_chunk - 2)


def fixed_variants(f: Fixed):
    """(n, family, flow origin) of every call on f's arena: each prefix with each family, the
    origins taken in turn; the whole arena with every origin."""
    out = []
    for n in f.prefixes:
        for k, fam in enumerate(f.families):
            origins = fixed_origins(f) if (fam and n == f.arena_packets) else (fixed_origins(f)[(k + n) % 4],)
            out += [(n, fam, o if fam else 0) for o in origins]
    return out


@functools.lru_cache(maxsize=None)
def fixed_pool(name: str):
    """(pool_size x stride bytes, word sum of each packet's first `length` bytes).  Packet 0 is
    all 0xFF and packet 1 all zero; the rest random."""
    f = FIXED[name]
    rng = np.random.default_rng([20, f.stride, f.length])
    pool = rng.integers(0, 256, (f.pool_size, f.stride), dtype=np.uint8)
    pool[0], pool[1] = 0xFF, 0
    wsum = np.array([sc.words(pool[k, :f.length]) for k in range(f.pool_size)], dtype=np.uint64)
    return pool, wsum


def fixed_arena(name: str) -> np.ndarray:
    """arena_packets packets: packet i is pool packet i mod pool_size."""
    f = FIXED[name]
    pool = fixed_pool(name)[0].reshape(-1)
    return np.tile(pool, -(-f.arena_packets // f.pool_size))[:f.arena_packets * f.stride]


def fixed_chunks(f: Fixed, n: int):
    return [min(f.per_chunk, n - first) for first in range(0, n, f.per_chunk)]


def fixed_expected(name: str, n: int, fam: int, origin: int = 0, nf: int = NF, restart=None) -> np.ndarray:
    """Checksums of the first n packets.  restart: wrong model (a), the chunks that restart the
    implicit flow at flow_origin."""
    f = FIXED[name]
    wsum = fixed_pool(name)[1][np.arange(n) % f.pool_size]
    idx = None
    if fam:
        if restart:
            idx = np.concatenate([flow_indices(origin, m, nf) for m in restart])
        else:
            idx = flow_indices(origin, n, nf)
    return combine(wsum, np.full(n, f.length, dtype=np.int64), fam, idx)


# ----------------------------------------------------------------------------
# frames: one pool per size class, the verdicts cycling
# ----------------------------------------------------------------------------
# the verdict of pool frame k is VERDICT_CYCLE[k % 7]: with a chunk size that is no multiple of 7,
# packet i and packet i + m then ALWAYS differ in verdict
VERDICT_CYCLE = (7, 5, 3, 0, 1, 6, 4)


def frame(rng: random.Random, verdict: int, length: int) -> bytes:
    """A frame of `length` bytes that rx_reference.verdict gives `verdict`: valid UDP over IPv4 (7);
    that with a bit of its L4 message flipped (5), of its TTL (6), of both (4); GRE (3); truncated
    TCP, or from 48 bytes an IPv6 extension header that runs past the payload (1); a version
    nibble of 5, or under 20 bytes (0)."""
    if verdict == 0 and length < 20:
        return rng.randbytes(length)
    if verdict == 3:
        f = bytearray(R.build(rng, 4, 47, length - 20))
    elif verdict == 1 and length < 40:
        f = bytearray(R.build(rng, 4, R.TCP, length - 20))
    elif verdict == 1:
        assert length >= 56
        f = bytearray(struct.pack(">IHBB16s16s", 0x60000000, 8, R.HOPOPTS, 64, rng.randbytes(16), rng.randbytes(16)) +
                      bytes([R.UDP, 1]) + rng.randbytes(length - 42))
    else:
        assert length >= 28
        f = bytearray(R.build(rng, 4, R.UDP, length - 20))
        if verdict in (5, 4):
            f[20] ^= 1 << rng.randrange(8)  # the source port: part of the L4 message only
        if verdict in (6, 4):
            f[8] ^= 1 << rng.randrange(8)   # the TTL: part of the header only
        if verdict == 0:
            f[0] = 0x55
    assert len(f) == length and R.verdict(bytes(f)) == verdict, (verdict, length)
    return bytes(f)


SMALL_LENGTHS = {7: (28, 40), 5: (28, 40), 6: (28, 40), 4: (28, 40), 3: (20, 40), 0: (0, 19), 1: (20, 39)}
POOL_SHAPES = {"big": (7 * 31, 20000, MAX_LEN), "medium": (7 * 37, 170, 300), "small": (7 * 43, 0, 40)}

Pool = namedtuple("Pool", "frames lens wsums verdicts")


def _pool_of(frames) -> Pool:
    return Pool(list(frames), np.array([len(f) for f in frames], dtype=np.int64),
                np.array([sc.words(f) for f in frames], dtype=np.uint64),
                np.array([R.verdict(f) for f in frames], dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def pool(kind: str) -> Pool:
    size, lo, hi = POOL_SHAPES[kind]
    rng = random.Random("host-path-" + kind)
    frames = []
    for k in range(size):
        v = VERDICT_CYCLE[k % 7]
        a, b = SMALL_LENGTHS[v] if kind == "small" else (lo, hi)
        frames.append(frame(rng, v, rng.randint(a, b)))
    return _pool_of(frames)


# ----------------------------------------------------------------------------
# byte-packed: host_packed_chunks, behind pipck_host_checksum_packed_bytes and pipck_host_rx_verify_packed
# ----------------------------------------------------------------------------
def cut(lens: np.ndarray):
    """The cutter of pipck_host.hip, from its comment: whole packets, a chunk closes once it holds
    at least HOST_CHUNK_BYTES bytes or HOST_CHUNK_PACKETS packets.  Packets per chunk."""
    cum = np.cumsum(lens, dtype=np.int64)
    n, first, out = len(lens), 0, []
    while first < n:
        base = int(cum[first - 1]) if first else 0
        j = int(np.searchsorted(cum, base + HOST_CHUNK_BYTES, side="left"))  # first packet that reaches the target
        m = min(j - first + 1, HOST_CHUNK_PACKETS, n - first)
        out.append(m)
        first += m
    return out


class Packed:
    """A sequence of frames as runs of (frame ids, repeats); ids index self.frames."""

    def __init__(self, name):
        self.name = name
        self.p = _pool_of(pool("big").frames + pool("small").frames + [b""])
        self.ids = {"big": np.arange(0, len(pool("big").frames)),
                    "small": len(pool("big").frames) + np.arange(len(pool("small").frames))}
        self.zero = len(self.p.frames) - 1
        self.runs = []
        self.bytes = 0
        self.count = 0
        self.phase = {"big": 0, "small": 0}
        self.rng = random.Random("packed-" + name)

    def _run(self, ids, repeats=1):
        ids = np.asarray(ids, dtype=np.int64)
        if len(ids) and repeats:
            self.runs.append((ids, repeats))
            self.bytes += int(self.p.lens[ids].sum()) * repeats
            self.count += len(ids) * repeats

    def cycle(self, kind, count):
        """`count` frames of the pool, going on where the last cycle() of that pool stopped."""
        ids, size = self.ids[kind], len(self.ids[kind])
        ph = self.phase[kind]
        head = min(count, (size - ph) % size)
        self._run(ids[ph:ph + head])
        full, tail = divmod(count - head, size)
        self._run(ids, full)
        self._run(ids[:tail])
        self.phase[kind] = (ph + count) % size

    def one(self, verdict, length):
        f = frame(self.rng, verdict, length)
        self.p = Pool(self.p.frames + [f], np.append(self.p.lens, len(f)),
                      np.append(self.p.wsums, np.uint64(sc.words(f))), np.append(self.p.verdicts, np.uint8(verdict)))
        self._run([len(self.p.frames) - 1])

    def zeros(self, count):
        self._run([self.zero], count)

    def fill_to(self, total, trim=0):
        """Big frames, then one or more valid frames of the length that is left: self.bytes == total.
        trim: that many big frames fewer (the frames that make up the rest are longer, or more)."""
        lens = self.p.lens[np.roll(self.ids["big"], -self.phase["big"])]
        cum = self.bytes + np.cumsum(np.tile(lens, (total - self.bytes) // int(lens.sum()) + 2))
        self.cycle("big", int(np.searchsorted(cum, total - 28, side="right")) - trim)
        while total - self.bytes > MAX_LEN:
            self.one(7, 40000)
        self.one(7, total - self.bytes)
        assert self.bytes == total

    # ---- what the tests read ----
    @functools.cached_property
    def seq(self) -> np.ndarray:
        return np.concatenate([np.tile(ids, r) for ids, r in self.runs])

    @functools.cached_property
    def lens(self) -> np.ndarray:
        out = self.p.lens[self.seq]
        assert len(out) == self.count and int(out.sum()) == self.bytes and int(out.max()) <= MAX_LEN
        return out

    @functools.cached_property
    def chunks(self):
        return cut(self.lens)

    def arena(self) -> np.ndarray:
        blobs = [np.frombuffer(b"".join(self.p.frames[i] for i in ids), dtype=np.uint8) for ids, _ in self.runs]
        return np.concatenate([np.tile(b, r) for b, (_, r) in zip(blobs, self.runs)] + [np.zeros(64, dtype=np.uint8)])

    def packet(self, i: int) -> bytes:
        return self.p.frames[int(self.seq[i])]

    def verdicts(self) -> np.ndarray:
        return self.p.verdicts[self.seq]

    def checksums(self, fam, origin=0, nf=NF, restart=False) -> np.ndarray:
        idx = None
        if fam:
            idx = (np.concatenate([flow_indices(origin, m, nf) for m in self.chunks]) if restart
                   else flow_indices(origin, self.count, nf))
        return combine(self.p.wsums[self.seq], self.lens, fam, idx)


PACKED_NAMES = ("bytes_exact", "overshoot_max", "count_exact", "zeros_at_cut", "zero_tail")
ZERO_RUN = 50


def _build_packed(name: str, trim: int) -> Packed:
    c = Packed(name)
    if name == "bytes_exact":       # the byte total reaches 64 MiB exactly at a packet end
        c.fill_to(HOST_CHUNK_BYTES, trim)
        c.cycle("big", 300)
    elif name == "overshoot_max":   # 64 MiB - 1, then the longest packet there is
        c.fill_to(HOST_CHUNK_BYTES - 1, trim)
        c.one(7, MAX_LEN)
        c.cycle("big", 300)
    elif name == "count_exact":     # 2^20 packets of 0..40 bytes, then 3 more
        c.cycle("small", HOST_CHUNK_PACKETS + 3)
    elif name == "zeros_at_cut":
        # a byte cut with empty packets before the packet that crosses and right after it; then a
        # count cut whose last packets and whose next chunk's first packets are empty
        c.fill_to(HOST_CHUNK_BYTES - 1000, trim)
        c.zeros(ZERO_RUN)
        c.one(5, 3000)
        c.zeros(ZERO_RUN)
        c.cycle("small", HOST_CHUNK_PACKETS - 2 * ZERO_RUN)
        c.zeros(ZERO_RUN)
        c.zeros(ZERO_RUN)
        c.cycle("small", 6000)
    elif name == "zero_tail":       # a last chunk of empty packets only: nothing is copied for it
        # its 200 empty packets (verdict 0) stand 1,5xx packets after the first 200: none of those has verdict 0
        c._run(c.ids["big"][c.p.verdicts[c.ids["big"]] != 0][:100], 2)
        c.fill_to(HOST_CHUNK_BYTES - 1000, trim)
        c.one(5, 3000)
        c.zeros(200)
    else:
        raise KeyError(name)
    return c


def discriminates(c: Packed) -> bool:
    """The conditions on a packed case's inputs (tests/test_host_path_cases.py asserts them): no
    chunk but the last is a multiple of the verdict cycle (so of a pool size) or of the flow
    count, and 99 % of the packets differ in verdict from those one and two chunks on."""
    return all(m % 7 and m % NF for m in c.chunks[:-1]) and shifted_differs(c.verdicts(), c.chunks) >= 0.99


@functools.lru_cache(maxsize=None)
def packed(name: str) -> Packed:
    """The case, with the fewest big frames left out of its first chunk that make it discriminate
    (the chunk's packet count follows from the frames' lengths; this moves it by one or two)."""
    for trim in range(8):
        c = _build_packed(name, trim)
        if discriminates(c):
            return c
    raise AssertionError(name)


# (family, flow origin) of the checksum runs over each packed case
PACKED_FLOWS = ((6, 5), (4, (1 << 64) - 700), (0, 0))


# ----------------------------------------------------------------------------
# RX queue: pipck_rx_verify
# ----------------------------------------------------------------------------
RXQ_COUNTS = (1023, 1024, 1025, 5119, 5120, 5121)


def rxq_pinned(i: int) -> bool:
    """Packet i lies in pinned memory: pinned, pageable, pageable, pinned, ..."""
    return i % 4 in (0, 3)


def rxq_sequence(n: int):
    """(pool, frame id of each packet): the medium pool, cycled."""
    p = pool("medium")
    return p, np.arange(n) % len(p.frames)


def rxq_copied_bounds(n: int):
    """(lower, upper) bound of the staging bytes the first n packets need.  A frame whose verdict
    has the L4-checked bit is copied up to the end of its L4 message at least (lower); no frame
    takes more than its length rounded up to 16 (upper)."""
    p, seq = rxq_sequence(n)
    ends = np.array([R.l4_range(f)[1] if v & R.L4_CHECKED else 0 for f, v in zip(p.frames, p.verdicts)])
    unpinned = np.array([not rxq_pinned(i) for i in range(n)])
    return int(ends[seq][unpinned].sum()), int(((p.lens[seq][unpinned] + 15) & ~15).sum())


# ----------------------------------------------------------------------------
# TX queue scripts
# ----------------------------------------------------------------------------
# Memory regions of a script: A and B are pinned pools (pipck_host_alloc), H is pageable.
REGION_BYTES = {"A": 256 << 10, "B": 64 << 10, "H": 512 << 10}
REGION_AT = {"A": 0, "B": REGION_BYTES["A"], "H": REGION_BYTES["A"] + REGION_BYTES["B"]}


@functools.lru_cache(maxsize=None)
def region_bytes(seed: str = "txq") -> np.ndarray:
    """The contents of A, B and H, in that order, in one array."""
    rng = np.random.default_rng([7, *seed.encode()])
    return rng.integers(0, 256, sum(REGION_BYTES.values()), dtype=np.uint8)


class Script:
    """An ordered list of operations on one TX queue.  Operations (tuples):

        ("add", family, flow, segs, slot, zc, rc)   segs: None (nseg 0, null segs) or a list of
                                                     (region or None, offset, length)
        ("add_ip", (region, offset, length), slot, rc)
        ("pending", n)   ("inflight", n)             what the queue must report
        ("free", region, rc)                         pipck_host_free of a pinned pool
        ("inplace", bytes or None)                   pipck_txq_inplace_max (None: the default)
        ("submit", slots)  ("complete", slots)  ("flush", slots)
                                                     slots: the fields that are stored by now
        ("destroy",)

    expect[slot] is the checksum of every accepted add; a refused add's field keeps its poison."""

    def __init__(self, name, seed="txq"):
        self.name, self.seed = name, seed
        self.mem = region_bytes(seed)
        self.rng = random.Random("script-" + name)
        self.ops, self.expect, self.queued, self.flight = [], {}, [], []
        self.slots = 0

    def seg(self, region, length, odd=None):
        """A segment of `length` bytes at a random offset of the region."""
        off = self.rng.randrange(0, REGION_BYTES[region] - length + 1)
        if odd is not None:
            off = min(off | 1, REGION_BYTES[region] - length) if odd else off & ~1
        return (region, off, length)

    def _slot(self):
        self.slots += 1
        return self.slots - 1

    def add(self, fam, segs, zc=False, rc=PIPCK_OK, flow=None):
        flow = self.rng.randrange(NF) if flow is None else flow
        slot = self._slot()
        self.ops.append(("add", fam, flow, segs, slot, zc, rc))
        if rc == PIPCK_OK:
            real = [(REGION_AT[r] + o, n) if r else (0, 0) for r, o, n in segs or []]
            self.expect[slot] = sc.chain_checksum(self.mem, [o for o, _ in real], [n for _, n in real],
                                                  sc.flows(fam)[1][flow])
            self.queued.append(slot)
        return slot

    def add_ip(self, seg, rc=PIPCK_OK):
        slot = self._slot()
        self.ops.append(("add_ip", seg, slot, rc))
        if rc == PIPCK_OK:
            at = REGION_AT[seg[0]] + seg[1]
            self.expect[slot] = sc.checksum(self.mem[at:at + seg[2]])
            self.queued.append(slot)
        return slot

    def op(self, *t):
        self.ops.append(t)

    def pending(self):
        self.ops.append(("pending", len(self.queued)))

    def submit(self):
        done, self.flight = self.flight, (self.queued or [])
        self.queued = []
        self.ops.append(("submit", done))
        self.ops.append(("inflight", len(self.flight)))

    def complete(self):
        done, self.flight = self.flight, []
        self.ops.append(("complete", done))

    def flush(self):
        self.ops.append(("flush", self.flight + self.queued))
        self.flight, self.queued = [], []


def _good(s: Script, k: int, zc_from=None):
    """Packet k of a run of ordinary ones: v4 and v6 in turn, 1-3 segments of 1-1,400 bytes; from
    region zc_from read in place, else copied from H."""
    fam = (4, 6)[k % 2]
    region = zc_from or "H"
    segs = [s.seg(region, s.rng.randint(1, 1400)) for _ in range(1 + k % 3)]
    return s.add(fam, segs, zc=bool(zc_from))


SCRIPT_NAMES = ("rollback", "erange_mid_batch", "ip_lengths", "empty_chains", "sizes", "destroy_inflight")
SIZES_BATCHES = (3000, 1, 0, 7, 3000)


@functools.lru_cache(maxsize=None)
def script(name: str) -> Script:
    s = Script(name)
    if name == "rollback":
        for k in range(5):
            _good(s, k, zc_from="A" if k in (1, 3) else None)  # staged bytes, segments and a hold on A are queued
        s.add(4, [(None, 0, 0), s.seg("B", 700), s.seg("H", 300)], zc=True, rc=PIPCK_EINVAL)
        s.pending()
        s.op("free", "B", PIPCK_OK)  # the only hold on B was the refused packet's
        for k in range(5, 10):
            _good(s, k, zc_from="A" if k in (6, 7, 9) else None)
        s.pending()
        s.flush()
    elif name == "erange_mid_batch":
        _good(s, 0)
        s.add(4, [s.seg("H", 100), s.seg("H", MAX_LEN + 1)], rc=PIPCK_ERANGE)
        _good(s, 1, zc_from="A")
        s.add_ip(s.seg("H", MAX_LEN + 1), rc=PIPCK_ERANGE)
        s.add(6, [s.seg("H", 100), s.seg("H", MAX_LEN)])
        s.add_ip(s.seg("H", MAX_LEN))
        s.add(6, [s.seg("A", MAX_LEN + 1)], zc=True, rc=PIPCK_ERANGE)
        _good(s, 2)
        s.pending()
        s.flush()
    elif name == "ip_lengths":
        for k, n in enumerate((0, 20, 21, 24, 60, MAX_LEN, 20)):
            s.add_ip(s.seg("H", n, odd=k % 2))
        s.pending()
        s.flush()
    elif name == "empty_chains":
        _good(s, 0)
        s.add(4, None)
        _good(s, 1)
        s.add(6, None)
        s.add(4, [(None, 0, 0)])
        s.add(6, None, flow=1)
        _good(s, 2)
        s.pending()
        s.flush()
    elif name == "sizes":
        # batch 0 in flight while batch 1 is queued, and so on; the copy path and the in-place path in turn
        for b, count in enumerate(SIZES_BATCHES):
            s.op("inplace", 0 if b % 2 == 0 else None)
            for k in range(count):
                if k % 5 == 4:
                    s.add_ip(s.seg("H", 20 + 4 * (k % 11)))
                else:
                    s.add((4, 6)[k % 2], [s.seg("H", s.rng.randint(300, 800)) for _ in range(1 + k % 3)])
            s.pending()
            s.submit()
        s.complete()
    elif name == "destroy_inflight":
        for k in range(40):
            _good(s, k, zc_from="A")
        s.submit()
        s.op("destroy")
        s.op("free", "A", PIPCK_OK)
        s.expect = {}  # the fields of a batch that never completed are unspecified
    else:
        raise KeyError(name)
    return s


def script_staged_bytes(s: Script):
    """Per batch (ended by a submit or flush), the bytes its copied segments take in the staging,
    each 16-byte aligned as pipck_txq.hip's comment says."""
    out, cur = [], 0
    for op in s.ops:
        if op[0] == "add" and op[6] == PIPCK_OK and not op[5]:
            cur += sum((n + 15) & ~15 for _, _, n in op[3] or [])
        elif op[0] == "add_ip" and op[3] == PIPCK_OK:
            cur += (op[1][2] + 15) & ~15
        elif op[0] in ("submit", "flush"):
            out.append(cur)
            cur = 0
    return out


# ----------------------------------------------------------------------------
# threads: one TX queue per writer thread
# ----------------------------------------------------------------------------
THREADS, ROUNDS = 4, 20
THREAD_REGIONS = {"own": 128 << 10, "shared": 128 << 10, "heap": 128 << 10}  # own and shared are pinned
THREAD_AT = {"own": 0, "shared": 128 << 10, "heap": 256 << 10}
ROUND_MODES = ("staged", "zc", "auto")  # plain adds; _zc adds of pinned segments; plain adds on an auto-zero-copy queue


@functools.lru_cache(maxsize=None)
def thread_memory(t: int) -> np.ndarray:
    """own | shared | heap of thread t; `shared` is the same bytes for every thread."""
    mem = np.random.default_rng([11, t]).integers(0, 256, sum(THREAD_REGIONS.values()), dtype=np.uint8)
    a = THREAD_AT["shared"]
    mem[a:a + THREAD_REGIONS["shared"]] = np.random.default_rng([11, 99]).integers(0, 256, THREAD_REGIONS["shared"],
                                                                                  dtype=np.uint8)
    return mem


@functools.lru_cache(maxsize=None)
def thread_rounds(t: int):
    """[(mode, [(family, flow, segs, ip)], [expected checksum])] per round: ip is true for an
    add_ip of segs[0]; segs are (region, offset, length)."""
    rng = random.Random("thread-%d" % t)
    mem = thread_memory(t)
    out = []
    for r in range(ROUNDS):
        mode = ROUND_MODES[(r + t) % 3]
        regions = {"staged": ("heap", "own", "shared"), "zc": ("own", "shared"), "auto": ("heap", "own", "shared")}[mode]
        pkts, want = [], []
        for k in range(rng.randint(1, 40)):
            segs = []
            for _ in range(rng.randint(0, 4) if mode != "zc" else rng.randint(1, 4)):
                reg = rng.choice(regions)
                n = rng.choice((0, 1, 20, rng.randint(1, 1500), rng.randint(1, 9000)))
                segs.append((reg, rng.randrange(0, THREAD_REGIONS[reg] - n + 1), n))
            ip = mode != "zc" and k % 7 == 3 and len(segs) >= 1
            fam, flow = (4, 6)[rng.randrange(2)], rng.randrange(NF)
            if ip:
                segs = segs[:1]
                at = THREAD_AT[segs[0][0]] + segs[0][1]
                want.append(sc.checksum(mem[at:at + segs[0][2]]))
            else:
                want.append(sc.chain_checksum(mem, [THREAD_AT[g] + o for g, o, _ in segs], [n for _, _, n in segs],
                                              sc.flows(fam)[1][flow]))
            pkts.append((fam, flow, segs, ip))
        out.append((mode, pkts, want))
    return out


RX_THREAD_FRAMES = 96


def thread_rx_round(r: int):
    """(pool, frame ids) the thread with an RX queue verifies in round r: pinned and pageable as rxq_pinned says."""
    p = pool("medium")
    return p, (np.arange(RX_THREAD_FRAMES) * 3 + 17 * r) % len(p.frames)
