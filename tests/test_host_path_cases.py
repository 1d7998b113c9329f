"""CPU: tests/host_path_cases.py -- that its seam constants are the sources',
that every case lands on the seam it is named after, that a stale buffer, a
restarted implicit flow and chunk-relative result offsets would each change
nearly every result, that the table is deterministic, and that the composed
references give pip's compiled answers (tests/golden/kat.json)."""
import json
import re
from pathlib import Path

import numpy as np
import pytest

from tests import host_path_cases as hp
from tests import rx_reference as R
from tests import saturation_cases as sc

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "pip_amd" / "csrc"
T = hp.HOST_CHUNK_BYTES


def pattern_bytes(spec: dict) -> bytes:
    """The data of a kat.json case (as tests/golden/make_golden.py writes it)."""
    if "hex" in spec:
        return bytes.fromhex(spec["hex"])
    n = spec["len"]
    if spec["pattern"] == "const":
        return bytes([spec["byte"]]) * n
    assert spec["pattern"] == "affine", spec  # (i * mul + add) & 0xFF
    return ((np.arange(n, dtype=np.uint64) * spec["mul"] + spec["add"]) & 0xFF).astype(np.uint8).tobytes()


def _value(expr: str) -> int:
    expr = re.sub(r"\b(\d+)(?:ull|u)\b", r"\1", expr.strip())
    assert re.fullmatch(r"[\d\s<()]+", expr), expr
    return eval(expr, {"__builtins__": {}})


def _defined(source: str, pattern: str):
    """The values of the groups of `pattern` in the one line of `source` it matches."""
    hits = [m for m in (re.search(pattern, ln) for ln in (CSRC / source).read_text().splitlines()) if m]
    assert len(hits) == 1, (source, pattern, len(hits))
    return [_value(g) for g in hits[0].groups()]


def test_seam_constants_are_the_sources():
    assert _defined("pipck_host.hip", r"constexpr uint64_t kTarget = ([^,;]+), kMaxPkts = ([^,;]+);") == \
        [hp.HOST_CHUNK_BYTES, hp.HOST_CHUNK_PACKETS]
    assert _defined("pipck_host.hip", r"per_chunk = std::max<uint64_t>\(1, \(([^)]+)\) / stride\);") == \
        [hp.HOST_CHUNK_BYTES]
    assert _defined("pipck_rx.hip", r"constexpr uint32_t kRxFirstChunk = ([^,;]+), kRxChunk = ([^,;]+);") == \
        [hp.RX_FIRST_LAUNCH, hp.RX_LAUNCH]
    assert _defined("pipck_rx.hip", r"size_t nc = cap \? cap : \(([^)]+)\);") == [hp.RX_STAGE_BYTES]
    assert _defined("pipck_txq.hip", r"size_t nc = cap \? cap : \(([^)]+)\);") == [hp.TX_STAGE_BYTES]
    assert _defined("pipck_txq.hip", r"constexpr uint64_t kInPlaceFlushMax = ([^;]+);") == [hp.TX_INPLACE_MAX]
    assert (hp.HOST_CHUNK_BYTES, hp.HOST_CHUNK_PACKETS, hp.RX_FIRST_LAUNCH, hp.RX_LAUNCH, hp.RX_STAGE_BYTES,
            hp.TX_STAGE_BYTES, hp.TX_INPLACE_MAX) == (64 << 20, 1 << 20, 1024, 4096, 64 << 10, 1 << 20, 32 << 20)


# ---- fixed stride ------------------------------------------------------------------


def test_fixed_cases_land_on_their_seams():
    assert {n: (f.stride, f.length, f.per_chunk) for n, f in hp.FIXED.items()} == {
        "s65536": (65536, 65535, 1024), "s65521": (65521, 65521, 1024), "s9216": (9216, 8980, 7281),
        "s20": (20, 20, 3355443)}
    for f in hp.FIXED.values():
        assert f.per_chunk == max(1, T // f.stride)
        assert f.per_chunk % hp.NF and f.per_chunk % f.pool_size, f.name
        assert f.length <= f.stride
        if f.name == "s20":
            assert f.families == (0,) and f.prefixes == (f.per_chunk + 1,)
            assert hp.fixed_chunks(f, f.arena_packets) == [f.per_chunk, 1]
            continue
        assert f.arena_packets == 2 * f.per_chunk + 1  # a third chunk: the first reuse of buffer 0
        assert hp.fixed_chunks(f, f.arena_packets) == [f.per_chunk, f.per_chunk, 1]
        assert f.prefixes == (f.per_chunk - 1, f.per_chunk, f.per_chunk + 1, f.arena_packets)
        assert [len(hp.fixed_chunks(f, n)) for n in f.prefixes] == [1, 1, 2, 3]
        origins = hp.fixed_origins(f)
        assert origins[:3] == (0, 5, (1 << 32) - 3)
        wrap_at = (1 << 64) - origins[3]  # the first packet whose flow_origin + i passes 2^64
        assert f.per_chunk < wrap_at < 2 * f.per_chunk
        variants = hp.fixed_variants(f)
        assert {n for n, _, _ in variants} == set(f.prefixes) and {fam for _, fam, _ in variants} == {0, 4, 6}
        for fam in (4, 6):
            assert {o for n, a, o in variants if a == fam and n == f.arena_packets} == set(origins)
        assert {o for n, a, o in variants if a} == set(origins)
    assert hp.FIXED["s65521"].stride % 2 == 1 and hp.FIXED["s65536"].length < hp.FIXED["s65536"].stride


@pytest.mark.parametrize("name", list(hp.FIXED))
def test_fixed_cases_tell_the_wrong_models_apart(name):
    f = hp.FIXED[name]
    n = f.arena_packets
    chunks = hp.fixed_chunks(f, n)
    past = np.arange(n) >= chunks[0]
    for fam in f.families:
        for origin in (hp.fixed_origins(f) if fam else (0,)):
            want = hp.fixed_expected(name, n, fam, origin)
            assert hp.shifted_differs(want, chunks) >= 0.99, (fam, origin)
            moved = hp.chunk_relative(want, chunks, hp.POISON16)
            assert (moved != want)[past].mean() >= 0.90
            if fam:  # without a pseudo-header there is no flow to restart
                restarted = hp.fixed_expected(name, n, fam, origin, restart=tuple(chunks))
                assert (restarted != want)[past].mean() >= 0.90, (fam, origin)
                assert np.array_equal(restarted[:chunks[0]], want[:chunks[0]])


@pytest.mark.parametrize("name", list(hp.FIXED))
def test_fixed_expected_values_are_the_plain_reference(name):
    f = hp.FIXED[name]
    pool, _ = hp.fixed_pool(name)
    n, pc = f.arena_packets, f.per_chunk
    at = sorted({0, 1, 2, pc - 1, pc, pc + 1, pc + 2, pc + 3, 2 * pc - 1, 2 * pc, n - 1, n // 3} & set(range(n)))
    for fam in f.families:
        for origin in (hp.fixed_origins(f) if fam else (0,)):
            want = hp.fixed_expected(name, n, fam, origin)
            for i in at:
                ps = sc.flows(fam)[1][sc.implicit_flow(origin, i, hp.NF)] if fam else None
                assert int(want[i]) == sc.checksum(pool[i % f.pool_size, :f.length], ps), (fam, origin, i)
    # a table of 3 flows (tests/test_gpu_host_paths.py starts a context with one)
    want = hp.fixed_expected(name, 64, f.families[-1], 5, nf=3)
    for i in range(0, 64, 7):
        ps = sc.flows(f.families[-1])[1][(5 + i) % 3] if f.families[-1] else None
        assert int(want[i]) == sc.checksum(pool[i % f.pool_size, :f.length], ps)


def test_fixed_arena_is_the_pool_cycled():
    f = hp.FIXED["s9216"]
    arena, pool = hp.fixed_arena(f.name), hp.fixed_pool(f.name)[0]
    assert arena.size == f.arena_packets * f.stride > 2 * f.per_chunk * f.stride
    for i in (0, 1, f.pool_size - 1, f.pool_size, f.per_chunk, f.arena_packets - 1):
        assert np.array_equal(arena[i * f.stride:(i + 1) * f.stride], pool[i % f.pool_size])
    assert (pool[0] == 0xFF).all() and not pool[1].any()


# ---- frame pools --------------------------------------------------------------------


def test_pools_cycle_the_verdicts():
    for kind, (size, lo, hi) in hp.POOL_SHAPES.items():
        p = hp.pool(kind)
        assert len(p.frames) == size and size % 7 == 0
        assert p.verdicts.tolist() == [hp.VERDICT_CYCLE[k % 7] for k in range(size)]
        assert lo <= p.lens.min() and p.lens.max() <= hi
        assert [R.verdict(f) for f in p.frames] == p.verdicts.tolist()
        assert [sc.words(f) for f in p.frames] == p.wsums.tolist()
        assert len(set(p.frames)) >= size - 2  # distinct packets (two empty ones may coincide)
    assert len(set(hp.VERDICT_CYCLE)) == 7 and R.VERIFIED in hp.VERDICT_CYCLE and R.UNCHECKED in hp.VERDICT_CYCLE
    assert 0 in hp.pool("small").lens  # an empty packet in the small pool itself


# ---- byte-packed -------------------------------------------------------------------


def _cut_slowly(lens):
    """The cutter as the loop of its comment (short sequences only)."""
    out, first = [], 0
    while first < len(lens):
        m = b = 0
        while first + m < len(lens) and m < hp.HOST_CHUNK_PACKETS and b < T:
            b += int(lens[first + m])
            m += 1
        out.append(m)
        first += m
    return out


def test_cut_is_the_loop():
    rng = np.random.default_rng(5)
    for _ in range(3):
        lens = rng.integers(60000, 65536, 3000)
        assert hp.cut(lens) == _cut_slowly(lens)
    assert hp.cut(np.array([T // 1024] * 1024 + [0, 0, 7])) == [1024, 3]
    assert hp.cut(np.zeros(5, dtype=np.int64)) == [5]


def test_packed_cases_land_on_their_seams():
    ends = {}
    for name in hp.PACKED_NAMES:
        c = hp.packed(name)
        cum = np.cumsum(c.lens)
        ends[name] = (c.chunks, [int(cum[e - 1]) for e in np.cumsum(c.chunks)])
        assert sum(c.chunks) == c.count and len(c.chunks) >= 2
        for m in c.chunks[:-1]:  # no pool size (7 * 31, 7 * 43), no verdict cycle and no flow count divides a chunk
            assert m % 7 and m % hp.NF and m % len(hp.pool("big").frames) and m % len(hp.pool("small").frames)
    chunks, at = ends["bytes_exact"]
    assert at[0] == T and chunks[1] == 300                     # the cut IS the 64 MiB mark
    c = hp.packed("overshoot_max")
    chunks, at = ends["overshoot_max"]
    assert at[0] == T - 1 + 65535 and c.lens[chunks[0] - 1] == 65535 and chunks[1] == 300
    assert at[0] - T == 65534                                  # the largest overshoot there is
    chunks, at = ends["count_exact"]
    assert chunks == [1 << 20, 3] and at[0] < T
    assert hp.packed("count_exact").lens.max() <= 40 and hp.packed("count_exact").lens.min() == 0
    c = hp.packed("zeros_at_cut")
    chunks, at = ends["zeros_at_cut"]
    z = hp.ZERO_RUN
    a, b = chunks[0], chunks[0] + chunks[1]
    assert len(chunks) == 3 and chunks[1] == 1 << 20 and at[0] >= T and at[1] - at[0] < T
    assert not c.lens[a - 1 - z:a - 1].any() and c.lens[a - 1] > 0 and c.lens[a - 2 - z] > 0  # empty, then the crossing packet
    assert not c.lens[a:a + z].any() and c.lens[a + z] > 0     # empty right after the byte cut
    assert not c.lens[b - z:b].any() and c.lens[b - z - 1] > 0  # an empty run that ends ON the count cut
    assert not c.lens[b:b + z].any() and c.lens[b + z] > 0     # and one that starts right after it
    c = hp.packed("zero_tail")
    chunks, at = ends["zero_tail"]
    assert chunks[1] == 200 and not c.lens[chunks[0]:].any() and at[0] >= T and at[1] == at[0]


@pytest.mark.parametrize("name", hp.PACKED_NAMES)
def test_packed_cases_tell_the_wrong_models_apart(name):
    c = hp.packed(name)
    past = np.arange(c.count) >= c.chunks[0]
    verdicts = c.verdicts()
    assert hp.discriminates(c) and hp.shifted_differs(verdicts, c.chunks) >= 0.99
    assert (hp.chunk_relative(verdicts, c.chunks, hp.POISON) != verdicts)[past].mean() >= 0.90
    for fam, origin in hp.PACKED_FLOWS:
        want = c.checksums(fam, origin)
        assert hp.shifted_differs(want, c.chunks) >= 0.99, (fam, origin)
        assert (hp.chunk_relative(want, c.chunks, hp.POISON16) != want)[past].mean() >= 0.90
        if fam:
            restarted = c.checksums(fam, origin, restart=True)
            assert (restarted != want)[past].mean() >= 0.90, (fam, origin)


@pytest.mark.parametrize("name", hp.PACKED_NAMES)
def test_packed_expected_values_are_the_plain_reference(name):
    c = hp.packed(name)
    edges = np.cumsum(c.chunks)[:-1].tolist()
    at = sorted({0, 1, c.count - 1, c.count // 2} | {e + d for e in edges for d in (-2, -1, 0, 1)})
    verdicts = c.verdicts()
    for i in at:
        assert int(verdicts[i]) == R.verdict(c.packet(i)) and len(c.packet(i)) == c.lens[i]
    for fam, origin in hp.PACKED_FLOWS:
        want = c.checksums(fam, origin)
        for i in at:
            ps = sc.flows(fam)[1][sc.implicit_flow(origin, i, hp.NF)] if fam else None
            assert int(want[i]) == sc.checksum(c.packet(i), ps), (fam, origin, i)
    assert (1 << 64) - hp.PACKED_FLOWS[1][1] < c.chunks[0]  # the 2^64 wrap lies inside chunk 0


def test_packed_arena_is_the_packets_back_to_back():
    c = hp.packed("overshoot_max")
    arena = c.arena()
    assert arena.size == c.bytes + 64
    offs = np.concatenate([[0], np.cumsum(c.lens)[:-1]])
    for i in (0, 1, 216, 217, c.chunks[0] - 2, c.chunks[0] - 1, c.chunks[0], c.count - 1):
        assert arena[offs[i]:offs[i] + c.lens[i]].tobytes() == c.packet(i)


# ---- RX queue ----------------------------------------------------------------------


def test_rxq_cases_land_on_their_seams():
    first, later = hp.RX_FIRST_LAUNCH, hp.RX_FIRST_LAUNCH + hp.RX_LAUNCH
    assert hp.RXQ_COUNTS == (first - 1, first, first + 1, later - 1, later, later + 1)
    assert [hp.rxq_pinned(i) for i in range(8)] == [True, False, False, True] * 2
    # the copied bytes pass the first staging size before the first launch ...
    assert hp.rxq_copied_bounds(first - 1)[0] > hp.RX_STAGE_BYTES
    # ... which grows it to 1.5 times what was needed, rounded up to a doubling: twice its size.
    # They pass that again after the first launch and before the second
    assert 1.5 * (hp.RX_STAGE_BYTES + 16 + int(hp.pool("medium").lens.max())) < 2 * hp.RX_STAGE_BYTES
    assert hp.rxq_copied_bounds(first + 1)[1] < 2 * hp.RX_STAGE_BYTES
    assert hp.rxq_copied_bounds(later - 1)[0] > 2 * hp.RX_STAGE_BYTES
    p, seq = hp.rxq_sequence(later + 1)
    assert len(p.frames) % 4 and first % len(p.frames) and hp.RX_LAUNCH % len(p.frames)
    assert hp.shifted_differs(p.verdicts[seq], [first, hp.RX_LAUNCH, 1]) >= 0.99


# ---- TX queue scripts ----------------------------------------------------------------


def _ops(s, kind):
    return [op for op in s.ops if op[0] == kind]


def test_scripts_are_what_their_names_say():
    s = hp.script("rollback")
    refused = [op for op in _ops(s, "add") if op[6] != hp.PIPCK_OK]
    assert len(refused) == 1 and refused[0][5] and refused[0][6] == hp.PIPCK_EINVAL
    assert [seg[0] for seg in refused[0][3]] == [None, "B", "H"]
    at = s.ops.index(refused[0])
    before = s.ops[:at]
    assert len(before) == 5 and any(op[5] for op in before) and any(not op[5] for op in before)  # holds and staged bytes
    assert s.ops[at + 1:at + 3] == [("pending", 5), ("free", "B", hp.PIPCK_OK)]
    assert all(seg[0] != "B" for op in _ops(s, "add") if op[6] == hp.PIPCK_OK for seg in op[3])
    assert len(s.expect) == 10 and refused[0][4] not in s.expect and s.ops[-2:] == [("pending", 10), s.ops[-1]]
    assert s.ops[-1][0] == "flush" and sorted(s.ops[-1][1]) == sorted(s.expect)
    assert any(op[5] and op[3][0][0] == "A" for op in s.ops[at + 3:] if op[0] == "add")

    s = hp.script("erange_mid_batch")
    kinds = [(op[0], op[-1]) for op in s.ops if op[0] in ("add", "add_ip")]
    assert kinds[0][1] == 0 and kinds[-1][1] == 0 and [k for k in kinds if k[1]] == [("add", 2), ("add_ip", 2), ("add", 2)]
    lens = [n for op in _ops(s, "add") for _, _, n in op[3]] + [op[1][2] for op in _ops(s, "add_ip")]
    assert lens.count(65536) == 3 and lens.count(65535) == 2
    assert {op[2] for op in _ops(s, "add_ip") if op[3] == 0} | {op[4] for op in _ops(s, "add") if op[6] == 0} == set(s.expect)

    s = hp.script("ip_lengths")
    assert [op[1][2] for op in _ops(s, "add_ip")][:6] == [0, 20, 21, 24, 60, 65535]
    assert {op[1][1] % 2 for op in _ops(s, "add_ip")} == {0, 1}  # the headers at even and odd addresses
    assert s.expect[0] == 0xFFFF

    s = hp.script("empty_chains")
    adds = _ops(s, "add")
    assert {op[1] for op in adds if op[3] is None} == {4, 6} and adds[0][3] and adds[-1][3]
    for op in adds:
        if not op[3]:
            assert s.expect[op[4]] == sc.chain_checksum(s.mem, [], [], sc.flows(op[1])[1][op[2]])

    s = hp.script("sizes")
    assert [op[1] for op in _ops(s, "pending")] == list(hp.SIZES_BATCHES) == [3000, 1, 0, 7, 3000]
    assert [op[1] for op in _ops(s, "inplace")] == [0, None, 0, None, 0]
    staged = hp.script_staged_bytes(s)
    assert staged[0] > 2 * hp.TX_STAGE_BYTES and staged[4] > 2 * hp.TX_STAGE_BYTES  # grows past 1 MiB and 2 MiB
    assert 0 < staged[1] < 4096 and staged[2] == 0 and staged[4] < hp.TX_INPLACE_MAX
    assert {op[1] for op in _ops(s, "add")} == {4, 6} and len(_ops(s, "add_ip")) > 1000
    done = [op[1] for op in s.ops if op[0] in ("submit", "complete")]
    assert [len(d) for d in done] == [0, 3000, 1, 0, 7, 3000]  # every submit completes the batch before it
    assert len(s.expect) == sum(hp.SIZES_BATCHES) == s.slots

    s = hp.script("destroy_inflight")
    assert [op[0] for op in s.ops[-4:]] == ["submit", "inflight", "destroy", "free"] and not s.expect
    assert all(op[5] and all(seg[0] == "A" for seg in op[3]) for op in _ops(s, "add"))


def test_script_expectations_are_the_plain_reference():
    for name in hp.SCRIPT_NAMES:
        s = hp.script(name)
        for op in s.ops:
            if op[0] == "add" and op[6] == hp.PIPCK_OK and op[4] in s.expect and op[4] % 97 == 0:
                data = [s.mem[hp.REGION_AT[r] + o:hp.REGION_AT[r] + o + n] for r, o, n in op[3] or [] if r]
                want = sc.chain_replay([sc.words(d) for d in data] or [0], [len(d) for d in data],
                                       sc.flows(op[1])[1][op[2]])
                assert s.expect[op[4]] == want
    for t in range(hp.THREADS):
        rounds = hp.thread_rounds(t)
        assert len(rounds) == hp.ROUNDS and {m for m, _, _ in rounds} == set(hp.ROUND_MODES)
        for mode, pkts, want in rounds:
            assert len(pkts) == len(want) >= 1
            if mode == "zc":
                assert all(seg[0] != "heap" for _, _, segs, _ in pkts for seg in segs)
        used = {seg[0] for _, pkts, _ in rounds for _, _, segs, _ in pkts for seg in segs}
        assert used == {"own", "shared", "heap"}
    a = hp.THREAD_AT["shared"]
    shared = [hp.thread_memory(t)[a:a + hp.THREAD_REGIONS["shared"]] for t in range(hp.THREADS)]
    assert all(np.array_equal(shared[0], x) for x in shared[1:])
    assert not np.array_equal(hp.thread_memory(0)[:4096], hp.thread_memory(1)[:4096])


# ---- determinism and pip's answers --------------------------------------------------


def test_the_table_is_deterministic():
    before = (hp.fixed_pool("s9216")[1].copy(), hp.pool("medium").frames[:], hp.packed("zero_tail").seq.copy(),
              hp.packed("bytes_exact").checksums(6, 5).copy(), list(hp.script("rollback").ops),
              dict(hp.script("sizes").expect), hp.thread_rounds(2)[3])
    for fn in (hp.fixed_pool, hp.pool, hp.packed, hp.script, hp.thread_rounds, hp.thread_memory, hp.region_bytes):
        fn.cache_clear()
    after = (hp.fixed_pool("s9216")[1], hp.pool("medium").frames, hp.packed("zero_tail").seq,
             hp.packed("bytes_exact").checksums(6, 5), hp.script("rollback").ops, hp.script("sizes").expect,
             hp.thread_rounds(2)[3])
    assert np.array_equal(before[0], after[0]) and before[1] == after[1] and np.array_equal(before[2], after[2])
    assert np.array_equal(before[3], after[3]) and before[4] == after[4] and before[5] == after[5]
    assert before[6] == after[6]


def test_composed_references_give_pips_answers():
    """kat.json holds pip's compiled results: single packets through checksum() and through
    combine() (the vectorised step), chains through chain_checksum()."""
    cases = json.loads((ROOT / "tests" / "golden" / "kat.json").read_text())["cases"]
    seen = {"ip": 0, "inet": 0, "inet6": 0, "inet_chain": 0, "inet6_chain": 0}
    for c in cases:
        fn = c["fn"]
        if fn not in seen:
            continue
        seen[fn] += 1
        fam = 0 if fn == "ip" else (6 if "6" in fn else 4)
        ps = (fam, bytes.fromhex(c["src"]), bytes.fromhex(c["dst"]), c["proto"]) if fam else None
        if fn.endswith("_chain"):
            segs = [pattern_bytes(s) for s in c["segs"]]
            host = np.frombuffer(b"".join(segs) + b"\0", dtype=np.uint8)
            offs = np.concatenate([[0], np.cumsum([len(s) for s in segs])])[:len(segs)]
            assert sc.chain_checksum(host, offs, [len(s) for s in segs], ps) == c["expect"], c
        else:
            data = pattern_bytes(c["data"])
            if len(data) > hp.MAX_LEN:  # outside the batch ABI's domain (pip's u32 accumulator wraps there)
                seen[fn] -= 1
                continue
            assert sc.checksum(data, ps) == c["expect"], c
            terms = sc.pseudo_terms(ps, len(data))
            got = hp.combine(np.array([sc.words(data) + terms], dtype=np.uint64), np.array([len(data)]), 0, None)
            assert int(got[0]) == c["expect"], c
    assert min(seen.values()) >= 30, seen
