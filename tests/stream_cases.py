"""What tests/test_gpu_streams.py launches on and compares with, beyond the batches
of tests/dispatch_results.py: second contents for every replayed case, and the
ring frame sets of the forwarding graph and the alignment tests.  numpy and the
CPU references only (no torch, no GPU); tests/test_stream_cases.py pins all of
it on the CPU.  No reference arithmetic is written here.

Second contents.  A replayed graph must be shown to read its inputs again, so a
replayed case has contents A (variant 0, the batch of tests/dispatch_results.py)
and B (variant 1) on ONE layout -- the same offsets, lengths, flows, descriptors
and tile index, which steer the launch -- with other bytes and other packets
damaged (dispatch_results.damage), so that at least MIN_DIFFERENT of the
reference's elements differ between A and B: a replay that served stale results
cannot pass.  second(group, a) builds B from A's layout alone, so the GPU test,
whose layouts are the device generators', and the CPU test, on the oracle's twin
layouts, build it the same way.  B of an RX / TX frame batch is A's frames with
variant 1's damage on top: the headers, and so the lengths and the L4 ranges,
are A's.

B runs for one fixed group per kernel instantiation of the golden table's
default column and for every other group (second_groups); A runs for all.
"""
import functools
import random

import numpy as np

from tests import dispatch_cases as dc
from tests import dispatch_results as dr
from tests import rx_reference as R

MIN_DIFFERENT = 0.05  # of the reference's elements (tx_fill: of the frames of the filled image)


# ----------------------------------------------------------------------------
# second contents of the census groups
# ----------------------------------------------------------------------------
def default_kernel(golden: dict, group: str) -> str:
    rc, name = dc.decode(golden, group)["default"]
    assert rc == 0 and name
    return name


def second_groups(golden: dict) -> list[str]:
    """The groups replayed with contents B: the first fixed group of every default kernel, and
    every group that is not fixed."""
    seen, out = set(), []
    for g in dr.census_groups():
        if g.startswith("fixed_"):
            k = default_kernel(golden, g)
            if k in seen:
                continue
            seen.add(k)
        out.append(g)
    return out


def is_verify(group: str) -> bool:
    return group.startswith("fixed_verify") or group.endswith("_verify")


def second(group: str, a, variant: int = 1):
    """Contents `variant` on the layout of batch `a` (the group's batch of variant 0)."""
    if group.startswith("fixed_"):
        shape, mode = dr.fixed_shape(group)
        return dr.fixed_batch(shape, mode.endswith("_pseudo"), variant)
    if group.startswith("ragged_"):
        return dr.packets_batch(a.host.size, a.offs, a.lens, a.flow_idx, (2, 2), variant=variant)
    if group.startswith("packed_"):
        return dr.packets_batch(a.host.size, a.offs, a.lens, a.flow_idx, (2, int(group.startswith("packed_bytes_"))),
                                variant=variant)
    if group == "chains":
        return dr.chains_batch(a.host.size, a.offs, a.lens, (3,), variant=variant)
    stride = int(group[group.index("[") + 1:-1]) if group.startswith("rx_verify_ring") else 0
    tx = group == "tx_fill"
    return dr.frames_batch(a.host, a.starts, a.lens, (stride, int(tx)), tx=tx, variant=variant)


def check(group: str, b) -> None:
    """The condition of tests/dispatch_results.py that the group's batch meets."""
    if group == "chains":
        dr.check_chains(b)
    elif group == "tx_fill":
        dr.check_tx(b)
    elif group.startswith("rx_verify"):
        dr.check_rx(b)
    else:
        dr.check_packets(b)


def want(group: str, b) -> np.ndarray:
    """The reference of what the group's launch writes into its result buffer."""
    if group == "tx_fill":
        return b.done
    if group == "chains":
        return b.checksums
    return b.verdicts if group.startswith("rx_verify") or is_verify(group) else b.checksums


def same_layout(group: str, a, b) -> bool:
    names = ("starts", "lens") if group.startswith("rx_verify") or group == "tx_fill" else ("offs", "lens")
    return a.host.size == b.host.size and all(np.array_equal(getattr(a, k), getattr(b, k)) for k in names)


def different(group: str, a, b) -> float:
    """The share of the reference's elements that differ between a and b; tx_fill: the share of
    frames whose filled bytes differ."""
    if group == "tx_fill":
        return float(np.mean([not np.array_equal(a.filled[s:s + n], b.filled[s:s + n])
                              for s, n in zip(a.starts, a.lens)]))
    return float(np.mean(want(group, a) != want(group, b)))


# ----------------------------------------------------------------------------
# ring frame sets: the forwarding graph (stride 4,096) and the alignment tests
# ----------------------------------------------------------------------------
RING_SET_SEEDS = {"A": 401, "B": 402}


@functools.lru_cache(maxsize=None)
def _pool():
    """The frames tests/test_gpu_fwd_ring.py's _verified_frames draws on (all within 4,096
    bytes), split by rx_reference.verdict: (verified, not verified)."""
    from tests.test_fwd_reference import filled
    from tests.test_gpu_rx_reference import fuzz_frames

    frames = list(fuzz_frames()[:6000]) + list(filled("shaped")) + list(filled("corner"))
    assert max(map(len, frames)) <= 4096
    good = [f for f in frames if R.verdict(f) == R.VERIFIED]
    return good, [f for f in frames if R.verdict(f) != R.VERIFIED]


@functools.lru_cache(maxsize=None)
def ring_frames(which: str) -> tuple:
    """Frame set "A" or "B": 500 frames of 4,096 bytes or less, 250 that verify and 250 that do
    not, shuffled, so that verified and failing slots alternate irregularly within every wave."""
    good, bad = _pool()
    rng = random.Random(RING_SET_SEEDS[which])
    frames = rng.sample(good, 250) + rng.sample(bad, 250)
    rng.shuffle(frames)
    return tuple(frames)


def check_ring_frames(frames) -> None:
    v = np.array([R.verdict(f) for f in frames])
    assert 450 <= len(frames) <= 600 and max(map(len, frames)) <= 4096
    assert int((v == R.VERIFIED).sum()) >= 100 and int((v != R.VERIFIED).sum()) >= 100


@functools.lru_cache(maxsize=None)
def forward_reference(which: str):
    """The forwarding graph on frame set `which`, composed on the CPU: ok = rx_reference.verdict;
    verified slots take the tests' rule assignment, the others PIPCK_FWD_NO_RULE (untouched, done
    0); fwd_reference.rewrite with UDP_ZERO_AS_ONES; ok2 = the verdicts of the rewritten frames;
    ring2 = tx_reference.fill of them.  Returns a namespace of frames, ok, rule_of, rewritten,
    done, ok2, filled, tx_done."""
    from types import SimpleNamespace

    from tests import fwd_reference as F
    from tests.test_fwd_reference import assign, rule_table
    from tests.test_tx_ring_cases import reference_fill

    frames = list(ring_frames(which))
    ok = np.array([R.verdict(f) for f in frames], dtype=np.uint8)
    rules, rule_of = rule_table(), assign(frames)
    rewritten, done = [], np.zeros(len(frames), dtype=np.uint8)
    for i, f in enumerate(frames):
        out = (f, 0)
        if ok[i] == R.VERIFIED:
            out = F.rewrite(f, rules[int(rule_of[i])], F.UDP_ZERO_AS_ONES)
        rewritten.append(out[0])
        done[i] = out[1]
    ok2 = np.array([R.verdict(f) for f in rewritten], dtype=np.uint8)
    filled, tx_done = reference_fill(rewritten, 0)
    return SimpleNamespace(frames=frames, ok=ok, rule_of=rule_of, rewritten=rewritten, done=done, ok2=ok2,
                           filled=filled, tx_done=tx_done)


ALIGN_N = 130  # slots of the alignment rings: two full blocks of 64 and a partial one


@functools.lru_cache(maxsize=None)
def aligned_frames(stride: int) -> tuple:
    """130 frames for a ring of `stride` at every 16-byte phase: the filled shaped frames and the
    structured set's frames that fit the slot, the longest ones first in line (a jumbo stride
    gets its long frames), then a seeded sample of the rest."""
    from tests.test_fwd_reference import filled
    from tests.test_gpu_rx_reference import structured_set

    pool = [f for f in list(filled("shaped")) + list(structured_set()[0]) if 0 < len(f) <= stride]
    rng = random.Random(stride)
    longest = sorted(pool, key=len, reverse=True)[:24]
    frames = longest + rng.sample(pool, ALIGN_N - len(longest))
    rng.shuffle(frames)
    return tuple(frames)


# ----------------------------------------------------------------------------
# the calls outside the census: flow tables to prepare, an in-place update
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def flow_tables(family: int, variant: int):
    """verify_sealing.flow_table of dispatch_results.NF flows: (records as bytes, (family, src, dst, proto) per flow)."""
    from tests import verify_sealing as vs

    return vs.flow_table(np.random.default_rng([15, family, variant]), family, dr.NF, dr.PROTO)


PREPARE_SHAPE = (64, 64, dc.N)  # stride, length, packets of the batch checksummed with a freshly prepared table


@functools.lru_cache(maxsize=None)
def prepare_case(family: int, variant: int):
    """A flow table to prepare and a fixed batch of random bytes to checksum with the prepared
    table (implicit flows from `origin`): `checksums` by verify_reference.ones_sum with the
    table's pseudo-headers, so a table prepared from other records cannot give them."""
    from types import SimpleNamespace

    stride, length, n = PREPARE_SHAPE
    records, table = flow_tables(family, variant)
    host = np.random.default_rng([16, family, variant]).integers(0, 256, n * stride, dtype=np.uint8)
    origin = dr.NF * 1000 + family
    idx = dr.implicit_flows(origin, n)
    offs, lens = np.arange(n, dtype=np.int64) * stride, np.full(n, length, dtype=np.int64)
    return SimpleNamespace(records=np.frombuffer(records, dtype=np.uint8).copy(), host=host, origin=origin, n=n,
                           stride=stride, length=length, lens=lens,
                           checksums=dr.checksums(host, offs, lens, lambda i: table[int(idx[i])]))


UPDATE = dict(stride=96, length=80, n=dc.N, ck_off=16, edit_off=24, edit_len=8)


@functools.lru_cache(maxsize=None)
def update_case(with_pseudo: bool, variant: int):
    """An in-place update (pipck_update_fixed_n): `before`, packets of random bytes whose field at
    ck_off holds their checksum (verify_reference.ones_sum, with_pseudo: under flow_tables(4, 0));
    `new`, 8 bytes per packet for [edit_off, edit_off + edit_len); `after`, the arena pip's full
    recomputation leaves: the bytes replaced and the field recomputed (with_pseudo: under
    flow_tables(4, 1), a NAT of the addresses).  The stride padding is random and stays."""
    from types import SimpleNamespace

    from tests import verify_reference as vr

    u = SimpleNamespace(**UPDATE)
    rng = np.random.default_rng([17, int(with_pseudo), variant])
    before = rng.integers(0, 256, u.n * u.stride, dtype=np.uint8)
    new = rng.integers(0, 256, u.n * u.edit_len, dtype=np.uint8)
    new[:u.edit_len], new[u.edit_len:2 * u.edit_len] = 0, 0xFF
    origin = dr.NF * 2000 + 5
    idx = dr.implicit_flows(origin, u.n)
    old_t, new_t = (flow_tables(4, k)[1] for k in (0, 1)) if with_pseudo else (None, None)

    def seal(img, table):
        for i in range(u.n):
            p = img[i * u.stride:i * u.stride + u.length]
            p[u.ck_off:u.ck_off + 2] = 0
            c = 0xFFFF ^ vr.ones_sum(p, None if table is None else table[int(idx[i])])
            p[u.ck_off], p[u.ck_off + 1] = c >> 8, c & 0xFF

    seal(before, old_t)
    after = before.copy()
    after.reshape(u.n, u.stride)[:, u.edit_off:u.edit_off + u.edit_len] = new.reshape(u.n, u.edit_len)
    seal(after, new_t)
    return SimpleNamespace(before=before, new=new, after=after, origin=origin, with_pseudo=with_pseudo, **UPDATE)
