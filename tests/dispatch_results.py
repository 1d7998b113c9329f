"""What tests/test_gpu_dispatch_results.py launches on and compares with: batch
contents, expected results and the conditions the inputs meet, for every group
of tests/dispatch_cases.py that takes tuning knobs.  numpy and the CPU oracle
only (no torch, no GPU); tests/test_dispatch_results_cases.py pins all of it on
the CPU.

The census.  Every group whose knob set is "general" or "ring", under every
knob of that set that computes results: a knob whose flags carry bit 21, 22 or
23 (pipck_tune.hpp kProbeBits) or whose probes word is non-zero
(kProbeHdrInPlace) computes none or wrong ones by design and is left out, by
its fields.  census() counts, from tests/golden/dispatch.json, the launches
checked and the kernel instantiations they reach.

No reference is written here.  The expected values come from the references the
suite already holds to pip:

    tests/verify_reference.py   ones_sum (checksum = 0xFFFF ^ ones_sum) and, through
                                verify_sealing.expected, the verdict of a packet
    tests/saturation_cases.py   chain_checksum: pip's loop over a chain's segments
    tests/rx_reference.py       the PIPCK_RX_* bits of a frame
    tests/tx_reference.py       the frame with its fields filled and the PIPCK_TX_* bits

Contents.  Random bytes, sealed by tests/verify_sealing.py (the checksum field
of every packet made correct by the CPU oracle) and then damaged by it, so a
checksum call returns 0x0000 for most packets and a verify call 1; IPv4 flows
from verify_sealing.flow_table (flow 0 all zero, flow 1 all 0xFF), implicit
flows from a non-zero origin.  A batch without a pseudo-header also holds eight
all-zero packets, whose checksum is 0xFFFF -- a value no packet with a
pseudo-header has, the length term being non-zero.  One batch serves the
checksum and the verify group of its shape.

Layouts.  The fixed-stride layouts are the case table's.  The descriptor and
packed layouts, and the RX / TX frames, are the device generators' (the GPU test
downloads them); on the CPU the oracle's generator twin gives the same ragged
layouts, and twin_frames() builds frames of gen_rx_frames' shape -- the same
lengths and header fields, other random bytes, as that generator draws them on
the device.
"""
import functools
from types import SimpleNamespace

import numpy as np

from pip_amd import engine, workloads
from tests import dispatch_cases as dc
from tests import rx_reference as R
from tests import saturation_cases as sc
from tests import tx_reference as T
from tests import verify_reference as vr
from tests import verify_sealing as vs

NF = workloads.N_FLOWS
PROTO = 6
# flags bits and probes under which a launch computes no or wrong results (pipck_tune.hpp kProbeBits)
PROBE_FLAGS = sum(1 << engine.TUNE_BITS[name] for name in ("loads_only", "no_task_end", "end_no_store"))
PROBE_KERNELS = ("k_flat_probe<", "k_flat_coop_probe<")
PLANTED = 8  # all-zero packets in a batch without a pseudo-header


# ----------------------------------------------------------------------------
# the census
# ----------------------------------------------------------------------------
def computes_results(knob: dict) -> bool:
    return not (knob["flags"] & PROBE_FLAGS) and not knob["probes"]


def census_groups() -> list[str]:
    return [g for g in dc.groups() if dc.knob_set(g) in ("general", "ring")]


def checked_knobs(group: str) -> dict[str, dict]:
    return {name: k for name, k in dc.knobs_of(group).items() if computes_results(k)}


def is_probe_kernel(name: str) -> bool:
    return any(p in name for p in PROBE_KERNELS)


def census(golden: dict) -> SimpleNamespace:
    """From the golden table: `checked` / `excluded`, {kernel name: launches} of the launches the
    GPU test checks and of those the rule leaves out (probe knobs, the default-only groups), and
    `table`, the number of launches in the whole table."""
    checked, excluded, table = {}, {}, 0
    for g in dc.groups():
        keep = checked_knobs(g) if g in census_groups() else {}
        for knob, (rc, name) in dc.decode(golden, g).items():
            table += 1
            side = checked if knob in keep else excluded
            side[name] = side.get(name, 0) + 1
    return SimpleNamespace(checked=checked, excluded=excluded, table=table)


# ----------------------------------------------------------------------------
# flows and the oracle
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle():
    from oracle.oracle import Oracle

    return Oracle()


@functools.lru_cache(maxsize=None)
def flows():
    """(NF pipck_flow4 records as bytes, the reference's (family, src, dst, proto) per flow)."""
    return vs.flow_table(np.random.default_rng(4004), 4, NF, PROTO)


def pseudo_of(flow_idx):
    if flow_idx is None:
        return lambda i: None
    table = flows()[1]
    return lambda i: table[int(flow_idx[i])]


def implicit_flows(origin: int, n: int) -> np.ndarray:
    return (origin + np.arange(n, dtype=np.int64)) % NF


def checksums(host, offs, lens, ps) -> np.ndarray:
    """0xFFFF ^ verify_reference.ones_sum of every packet's bytes as they are now (uint16)."""
    return np.array([0xFFFF ^ vr.ones_sum(host[int(o):int(o) + int(n)], ps(i))
                     for i, (o, n) in enumerate(zip(offs, lens))], dtype=np.uint16)


def oracle_checksums(host, offs, lens, ps) -> np.ndarray:
    """The same values by the CPU oracle's ip_checksum / inet_checksum."""
    orc = oracle()
    out = np.zeros(len(lens), dtype=np.uint16)
    for i, (o, n) in enumerate(zip(offs, lens)):
        data, p = host[int(o):int(o) + int(n)].tobytes(), ps(i)
        out[i] = orc.ip_checksum(data) if p is None else orc.inet_checksum(data, p[3], p[1], p[2])
    return out


# ----------------------------------------------------------------------------
# packets at given places: the fixed, ragged and packed groups
# ----------------------------------------------------------------------------
def variant_key(tag: int, key, variant: int) -> list:
    """The rng key of a builder: [tag, *key], with a non-zero `variant` appended -- other contents
    on the same layout; variant 0 draws the bytes these builders have always drawn."""
    return [tag, *key] + ([variant] if variant else [])


def damage(host, offs, lens, rng, variant: int = 0) -> None:
    """verify_sealing.damage with its index classes shifted by 3 * variant: packet i is damaged as
    class (i + 3 * variant) % 8, so the packets that fail in variant 1 (i % 8 in {5, 7}) are not
    those of variant 0 (i % 8 in {0, 2}).  Variant 0 is verify_sealing.damage itself."""
    if variant:
        offs, lens = np.roll(np.asarray(offs), 3 * variant), np.roll(np.asarray(lens), 3 * variant)
    vs.damage(host, offs, lens, rng)


def packets_batch(size: int, offs, lens, flow_idx, key, planted: int = 0, variant: int = 0) -> SimpleNamespace:
    """`size` random bytes whose packets (offs, lens; flows flow_idx, None: no pseudo-header) are
    sealed and then damaged; `planted` packets, spread over the batch, are zeroed after that.
    Gives host, offs, lens, the field offsets, and the reference's verdicts and checksums of the
    final bytes.  `variant`: second contents on the same layout (variant_key, damage)."""
    rng = np.random.default_rng(variant_key(11, key, variant))
    host = rng.integers(0, 256, size, dtype=np.uint8)
    offs, lens = np.asarray(offs, dtype=np.int64), np.asarray(lens, dtype=np.int64)
    n = len(lens)
    ps = pseudo_of(flow_idx)
    fields = vs.seal(host, offs, lens, ps, oracle(), rng)
    damage(host, offs, lens, rng, variant)
    for k in range(planted):
        i = n * (2 * k + 1) // (2 * planted)
        host[offs[i]:offs[i] + lens[i]] = 0
    return SimpleNamespace(host=host, offs=offs, lens=lens, n=n, fields=fields, flow_idx=flow_idx, planted=planted,
                           verdicts=vs.expected(host, offs, lens, ps), checksums=checksums(host, offs, lens, ps))


def fixed_shape(group: str):
    """((stride, length, n, arena offset), mode) of a fixed group of the case table."""
    mode = group[len("fixed_"):group.index("[")]
    return next(s for s in dc.FIXED_SHAPES if dc.fixed_id(s, mode) == group), mode


@functools.lru_cache(maxsize=None)
def fixed_batch(shape, with_pseudo: bool, variant: int = 0) -> SimpleNamespace:
    """The batch of one fixed shape, shared by its checksum and its verify group: exactly
    n * stride bytes, the stride padding random.  `origin`: the flow origin of the call."""
    stride, length, n, off = shape
    origin = NF * ((1 << 30) + 5 * stride + length) - 3 if with_pseudo else 0  # packets 3 and 4 on flows 0 and 1
    b = packets_batch(n * stride, np.arange(n, dtype=np.int64) * stride, np.full(n, length),
                      implicit_flows(origin, n) if with_pseudo else None,
                      (1, stride, length, n, off, int(with_pseudo)), planted=0 if with_pseudo else PLANTED,
                      variant=variant)
    b.origin = origin
    return b


def check_packets(b: SimpleNamespace) -> None:
    """The conditions on a batch of packets: the verify mix of verify_sealing.check_mix, at least 8
    checksums of 0x0000 and, without a pseudo-header, at least 8 of 0xFFFF (never one with)."""
    vs.check_mix(b.verdicts, b.lens, b.fields)
    assert np.array_equal(b.verdicts, (b.checksums == 0).astype(np.uint8))
    assert int((b.checksums == 0).sum()) >= 8
    ones = int((b.checksums == 0xFFFF).sum())
    assert ones >= PLANTED if b.flow_idx is None else ones == 0, ones


# the twin layouts of the device generators' Zipf batch (the oracle's generator twin)
@functools.lru_cache(maxsize=None)
def twin_lengths() -> np.ndarray:
    return oracle().zipf_lengths(workloads.CFG4.seed, 0, dc.N).astype(np.int64)


def ragged_layout(lens):
    """(offsets, arena bytes) of gen_ragged / gen_packed: every packet at the next 16-byte boundary."""
    chunks = (np.asarray(lens, dtype=np.int64) + 15) // 16
    return (np.cumsum(chunks) - chunks) * 16, max(int(chunks.sum()) * 16, 16)


def packed_bytes_layout(lens):
    """(offsets, arena bytes) of gen_packed_bytes: back to back, the arena rounded up to 16 bytes."""
    lens = np.asarray(lens, dtype=np.int64)
    return np.cumsum(lens) - lens, max((int(lens.sum()) + 15) // 16 * 16, 16)


PACKED_ORIGIN = (1 << 33) + 77  # the flow origin of the packed and byte-packed calls


# ----------------------------------------------------------------------------
# chains
# ----------------------------------------------------------------------------
def chain_begin(n_segs: int) -> np.ndarray:
    """The case table's chains: three descriptors per packet, the last packet what is left."""
    return np.array(list(range(0, n_segs, 3)) + [n_segs], dtype=np.int64)


def chains_batch(size: int, offs, lens, key, variant: int = 0) -> SimpleNamespace:
    """`size` random bytes under the descriptors (offs, lens), grouped by chain_begin, every chain
    on flow 0.  A 16-bit field at offset 16 of every chain's first segment is given the value that
    brings the chain's checksum to 0x0000 (the oracle's chain checksum with the field zeroed), then
    the first segments are damaged.  `checksums`: saturation_cases.chain_checksum of the final bytes."""
    rng = np.random.default_rng(variant_key(12, key, variant))
    host = rng.integers(0, 256, size, dtype=np.uint8)
    offs, lens = np.asarray(offs, dtype=np.int64), np.asarray(lens, dtype=np.int64)
    begin = chain_begin(len(lens))
    flow0 = flows()[1][0]
    assert int(lens.min()) >= 18
    for a, b in zip(begin[:-1], begin[1:]):
        at = int(offs[a]) + 16
        host[at:at + 2] = 0
        c = oracle().inet_checksum_chain([host[int(o):int(o) + int(n)].tobytes() for o, n in zip(offs[a:b], lens[a:b])],
                                         flow0[3], flow0[1], flow0[2])
        host[at], host[at + 1] = c >> 8, c & 0xFF
    damage(host, offs[begin[:-1]], lens[begin[:-1]], rng, variant)
    want = np.array([sc.chain_checksum(host, offs[a:b], lens[a:b], flow0) for a, b in zip(begin[:-1], begin[1:])],
                    dtype=np.uint16)
    return SimpleNamespace(host=host, offs=offs, lens=lens, begin=begin, n=len(begin) - 1, checksums=want,
                           total_lens=np.add.reduceat(lens, begin[:-1]))


def oracle_chain_checksums(b: SimpleNamespace) -> np.ndarray:
    flow0 = flows()[1][0]
    return np.array([oracle().inet_checksum_chain(
        [b.host[int(o):int(o) + int(n)].tobytes() for o, n in zip(b.offs[a:z], b.lens[a:z])], flow0[3], flow0[1],
        flow0[2]) for a, z in zip(b.begin[:-1], b.begin[1:])], dtype=np.uint16)


def check_chains(b: SimpleNamespace) -> None:
    zeros = int((b.checksums == 0).sum())
    assert zeros >= 8 and b.n - zeros >= 8, (zeros, b.n)


# ----------------------------------------------------------------------------
# RX and TX frames
# ----------------------------------------------------------------------------
def twin_frames(n: int, seed: int, checksummed: bool = True, l4_len: int = 0, stride: int = 0):
    """(bytes, starts, lens) of frames shaped as engine.gen_rx_frames makes them -- cfg4's Zipf L4
    lengths (or l4_len each) under an IPv4 (TCP, TCP, UDP) or IPv6 (TCP) header by a random kind,
    every other byte random -- back to back, or in the slots of a ring of `stride` (the rest of a
    slot zero, as engine.gen_rx_ring).  The generator's own random bytes come from the device, so
    these are other bytes in the same shape; `checksummed`: both fields by tx_reference.fill."""
    rng = np.random.default_rng([13, seed, l4_len, int(checksummed)])
    l4 = np.full(n, l4_len, dtype=np.int64) if l4_len else \
        oracle().zipf_lengths(workloads.cfg_seed(4), 0, n).astype(np.int64)
    kind = rng.integers(0, 4, n)
    lens = l4 + np.where(kind == 3, 40, 20)
    starts = np.arange(n, dtype=np.int64) * stride if stride else np.cumsum(lens) - lens
    total = n * stride if stride else (int(lens.sum()) + 16 + 127) // 128 * 128
    host = np.zeros(total, dtype=np.uint8) if stride else rng.integers(0, 256, total, dtype=np.uint8)
    for i in range(n):
        f = bytearray(rng.integers(0, 256, int(lens[i]), dtype=np.uint8).tobytes())
        if kind[i] == 3:
            f[0], f[4], f[5], f[6] = 0x60, int(l4[i]) >> 8, int(l4[i]) & 0xFF, 6
        else:
            f[0], f[2], f[3], f[6], f[7] = 0x45, int(lens[i]) >> 8, int(lens[i]) & 0xFF, 0, 0
            f[9] = 17 if kind[i] == 2 else 6
        frame = T.fill(bytes(f))[0] if checksummed else bytes(f)
        host[starts[i]:starts[i] + lens[i]] = np.frombuffer(frame, dtype=np.uint8)
    return host, starts, lens


def frames_batch(host, starts, lens, key, tx: bool = False, variant: int = 0) -> SimpleNamespace:
    """The frames host[start:start + len] with verify_sealing.damage applied over every frame's L4
    range (a flipped bit in one frame of eight, a sum-neutral swap in another, two bytes exchanged
    in a third).  RX: `verdicts`, rx_reference.verdict per frame.  TX: `filled`, the whole image
    with every frame replaced by tx_reference.fill's, and `done`, its PIPCK_TX_* bits.  `host` is
    copied, not modified."""
    rng = np.random.default_rng(variant_key(14, key, variant))
    host = np.array(host, dtype=np.uint8, copy=True)
    starts, lens = np.asarray(starts, dtype=np.int64), np.asarray(lens, dtype=np.int64)
    ranges = [R.l4_range(host[int(s):int(s) + int(n)].tobytes()) for s, n in zip(starts, lens)]
    damage(host, [int(s) + a for s, (a, _) in zip(starts, ranges)], [z - a for a, z in ranges], rng, variant)
    b = SimpleNamespace(host=host, starts=starts, lens=lens, n=len(lens))
    frames = [host[int(s):int(s) + int(n)].tobytes() for s, n in zip(starts, lens)]
    if not tx:
        b.verdicts = np.array([R.verdict(f) for f in frames], dtype=np.uint8)
        return b
    b.filled, b.done = host.copy(), np.zeros(b.n, dtype=np.uint8)
    for i, f in enumerate(frames):
        out, b.done[i] = T.fill(f, 0)
        b.filled[starts[i]:starts[i] + lens[i]] = np.frombuffer(out, dtype=np.uint8)
    return b


def check_rx(b: SimpleNamespace) -> None:
    """At least a tenth of the frames verify and at least a tenth fail their L4 checksum."""
    verifies = int((b.verdicts == R.VERIFIED).sum())
    fails = int(((b.verdicts & (R.L4_CHECKED | R.L4_OK)) == R.L4_CHECKED).sum())
    assert 10 * verifies >= b.n and 10 * fails >= b.n, (verifies, fails, b.n)


def check_tx(b: SimpleNamespace) -> None:
    """Each PIPCK_TX_* bit at least 8 times, and at least 8 frames whose bytes the fill changes."""
    for bit in (T.IP_FILLED, T.L4_FILLED):
        assert int(((b.done & bit) != 0).sum()) >= 8, bit
    assert int((b.filled != b.host).sum()) >= 8


# ----------------------------------------------------------------------------
# a mismatch, in words
# ----------------------------------------------------------------------------
def mismatch(group: str, knob: str, kernel: str, got, want, lens) -> str | None:
    """None where got equals want element for element; else the group, the knob, the kernel, how
    many packets are wrong, and the first eight with got / want and their lengths."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want):
        return None
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"{group} [{knob}] {kernel}: result {got.dtype}{got.shape}, reference {want.dtype}{want.shape}"
    bad = np.nonzero(got != want)[0]
    first = ", ".join(f"#{i}: got {int(got[i]):#x} want {int(want[i]):#x} len {int(np.asarray(lens)[i])}"
                      for i in map(int, bad[:8]))
    return f"{group} [{knob}] {kernel}: {bad.size} of {want.size} wrong; {first}"
