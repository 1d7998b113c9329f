"""CPU: tests/fwd_reference.py, the plain reference of pipck_fwd_rewrite_ring, held
to the two independent references already in the tree before the GPU tests
(tests/test_gpu_fwd_ring.py) hold the kernel to it:

  * rx_reference.verdict: an RFC 1624 update preserves a frame's one's-complement
    sums, so the RX verdict of a rewritten frame is the verdict it had;
  * tx_reference.fill: a rewritten frame whose checksums verified carries the
    checksums a full recomputation stores, apart from the two spellings of zero;

on hand-written frames with their bytes spelled out, and on the ABI.  The rule
table, the rule assignment and the frame sets of the GPU tests live here too."""
import ctypes as C
import functools
import re
from pathlib import Path

import numpy as np

from tests import fwd_reference as F
from tests import rx_reference as R
from tests import tx_reference as T
from tests.test_gpu_rx_reference import fuzz_frames, structured_set
from tests.test_tx_reference import corner_frames, pip_frames, shaped_frames

ROOT = Path(__file__).resolve().parents[1]

# the seven ops sets, cycled by frame index
OPS_SETS = (F.DEC_TTL, F.SET_SRC, F.SET_DST | F.SET_DPORT, F.ALL_OPS, F.SET_SPORT, F.SET_SRC | F.DEC_TTL, F.SET_DST)
SRC4, DST4 = bytes([203, 0, 113, 7]), bytes([198, 51, 100, 9])
SRC6, DST6 = bytes.fromhex("20010db885a3000000008a2e03707334"), bytes.fromhex("20010db8000000000000ff0000428329")
SPORT, DPORT = b"\xc0\x01", b"\x00\x35"


@functools.lru_cache(maxsize=None)
def rule_table():
    """The 14 rules of the tests: rule 7 * (family == 6) + k has ops OPS_SETS[k]."""
    return tuple(F.rule(ops, fam, *((SRC4, DST4) if fam == 4 else (SRC6, DST6)), SPORT, DPORT)
                 for fam in (4, 6) for ops in OPS_SETS)


def rule_index(frame, k):
    """Ops set k in the family of the frame's version nibble (4 where it is neither)."""
    return 7 * (len(frame) > 0 and frame[0] >> 4 == 6) + k


def assign(frames):
    """The tests' assignment: family by the version nibble, ops cycling by frame index."""
    return np.array([rule_index(f, i % 7) for i, f in enumerate(frames)], dtype=np.uint32)


def reference_rewrite(frames, rule_of, flags, rules=None):
    """([rewritten frames], done bytes) under rules[rule_of[i]]."""
    rules = rule_table() if rules is None else rules
    out = [F.rewrite(f, rules[int(r)], flags) for f, r in zip(frames, rule_of)]
    return [f for f, _ in out], np.array([d for _, d in out], dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def filled(which):
    """The shaped, corner or pip frames with both checksum fields filled (tx_reference.fill)."""
    frames = {"shaped": shaped_frames, "corner": lambda: [f for _, f, _ in corner_frames()], "pip": pip_frames}[which]()
    return tuple(T.fill(f, 0)[0] for f in frames)


@functools.lru_cache(maxsize=None)
def planted_ttl_frames():
    """The first 420 well-formed fuzz frames of each family, TTL / hop limit set to 0 and 1 in turn."""
    out = []
    for fam, at in ((4, 8), (6, 7)):
        pool = [f for f in fuzz_frames() if f and f[0] >> 4 == fam and F.rewrite(f, F.rule(0, fam))[1] == F.DONE][:420]
        assert len(pool) == 420
        for k, f in enumerate(pool):
            q = bytearray(f)
            q[at] = k & 1
            out.append(bytes(q))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def fuzz_ring_frames():
    """The 20,000 fuzz frames and the planted-TTL frames: the fuzz ring of the GPU tests."""
    return fuzz_frames() + planted_ttl_frames()


def _proto(f):
    up = T._upper(f)
    return None if up is None else up[0]


def _all_sets():
    return (("fuzz", fuzz_frames()), ("structured", structured_set()[0]), ("shaped", filled("shaped")),
            ("corner", filled("corner")), ("pip", pip_frames()))


@functools.lru_cache(maxsize=None)
def _every_ops(name):
    """[(frame, verdict before, [(ops index, flags, rewritten, done)])] for a frame set."""
    frames = dict(_all_sets())[name]
    out = []
    for f in frames:
        rows = []
        for k in range(7):
            for flags in (0, F.UDP_ZERO_AS_ONES):
                g, done = F.rewrite(f, rule_table()[rule_index(f, k)], flags)
                rows.append((k, flags, g, done))
        out.append((f, R.verdict(f), rows))
    return out


def test_verdict_is_preserved():
    """For every DONE frame under every ops set the RX verdict is the one it had with the flag
    set; with flags 0 the one allowed change is 7 -> 3, UDP over IPv4 whose field updated to 0."""
    done_frames = 0
    for name, _ in _all_sets():
        for f, before, rows in _every_ops(name):
            for k, flags, g, done in rows:
                if done != F.DONE:
                    assert g == f, (name, k, f.hex())
                    continue
                done_frames += 1
                after = R.verdict(g)
                if after == before:
                    continue
                at = T._upper(g)[1]
                assert flags == 0 and (before, after) == (7, 3) and g[0] >> 4 == 4 and _proto(g) == F.UDP and \
                    g[at + 6:at + 8] == b"\0\0" and f[at + 6:at + 8] != b"\0\0", (name, k, flags, before, after, f.hex())
    assert done_frames > 100000


def test_rewrite_equals_full_recomputation():
    """A DONE frame that verified before carries what tx_reference.fill stores, except where a
    field differs only as 0x0000 against 0xFFFF; such pairs occur, and nothing else does."""
    pairs = {}
    for name, _ in _all_sets():
        for f, before, rows in _every_ops(name):
            if before != R.VERIFIED:
                continue
            for k, flags, g, done in rows:
                if done != F.DONE:
                    continue
                full = T.fill(g, flags)[0]
                if full == g:
                    continue
                diff = [i for i in range(len(g)) if g[i] != full[i]]
                assert len(diff) == 2 and diff[1] == diff[0] + 1 and diff[0] % 2 == 0 and \
                    {g[diff[0]:diff[0] + 2], full[diff[0]:diff[0] + 2]} == {b"\0\0", b"\xff\xff"}, \
                    (name, k, flags, diff, f.hex())
                pairs.setdefault(name, set()).add(f)
    print("0x0000 / 0xFFFF pairs", {k: len(v) for k, v in pairs.items()})
    assert pairs, "no frame whose field differs as 0x0000 against 0xFFFF"


def test_fuzz_ring_census():
    frames = fuzz_frames()
    rule_of = assign(frames)
    out, done = reference_rewrite(frames, rule_of, 0)
    counts = {v: int((done == v).sum()) for v in (F.DONE, F.UNHANDLED, 0, F.EXPIRED)}
    print("fuzz census", counts)
    assert counts[F.DONE] >= 5000 and counts[F.UNHANDLED] >= 5000 and counts[0] >= 1000, counts
    assert counts == {F.DONE: 7474, F.UNHANDLED: 10059, 0: 2465, F.EXPIRED: 2}, counts
    by_pair = {}
    verified = 0
    for f, r, d in zip(frames, rule_of, done):
        if d == F.DONE:
            by_pair[(f[0] >> 4, _proto(f))] = by_pair.get((f[0] >> 4, _proto(f)), 0) + 1
            verified += R.verdict(f) == R.VERIFIED
    for pair in ((4, F.TCP), (4, F.UDP), (4, F.ICMP), (6, F.TCP), (6, F.UDP), (6, F.ICMP6)):
        assert by_pair.get(pair, 0) >= 100, (pair, by_pair)
    assert verified >= 1000, verified
    # EXPIRED does not come from the fuzz: the planted frames
    planted = planted_ttl_frames()
    assert sum(f[0] >> 4 == 4 for f in planted) >= 200 and sum(f[0] >> 4 == 6 for f in planted) >= 200
    ring = fuzz_ring_frames()
    done = reference_rewrite(ring, assign(ring), 0)[1][len(frames):]
    for fam in (4, 6):
        for ttl in (0, 1):
            hit = sum(1 for f, d in zip(planted, done)
                      if d == F.EXPIRED and f[0] >> 4 == fam and f[8 if fam == 4 else 7] == ttl)
            assert hit >= 50, (fam, ttl, hit)
    assert max(map(len, ring)) <= 1024


# (name, frame, rule, flags, the frame afterwards, done)
_ALL4 = F.rule(F.ALL_OPS, 4, SRC4, DST4, SPORT, DPORT)
HAND = (
    # RFC 1624 section 4: HC = 0xDD2F, m = 0x5555 becomes m' = 0x3285; eqn. 3 gives 0x0000 (eqn. 4 would
    # give 0xFFFF).  The second address word 0x0000 stays: ~0 + 0 = 0xFFFF changes nothing.
    ("rfc1624_section4",
     "4500001c1c4640004001dd2f555500000a0000010800f7ff00000000", F.rule(F.SET_SRC, 4, src=b"\x32\x85\0\0"), 0,
     "4500001c1c46400040010000328500000a0000010800f7ff00000000", F.DONE),
    # UDP over IPv4 with a zero field: TTL, addresses and ports rewritten, the header field updated, the zero kept
    ("udp4_zero_field_kept",
     "450000201c46400040119c6ec0a80001c0a800c704001f90000c000070696e67", _ALL4, 0,
     "450000201c4640003f11b942cb007107c6336409c0010035000c000070696e67", F.DONE),
    # a correct UDP checksum 0x7B5C and a new source port 0x7F5C = 0x7B5C + 0x0400: the field updates to 0x0000
    ("udp4_updates_to_zero",
     "450000201c46400040119c6ec0a80001c0a800c704001f90000c7b5c70696e67", F.rule(F.SET_SPORT, 0, sport=b"\x7f\x5c"), 0,
     "450000201c46400040119c6ec0a80001c0a800c77f5c1f90000c000070696e67", F.DONE),
    ("udp4_updates_to_zero_as_ones",
     "450000201c46400040119c6ec0a80001c0a800c704001f90000c7b5c70696e67", F.rule(F.SET_SPORT, 0, sport=b"\x7f\x5c"),
     F.UDP_ZERO_AS_ONES,
     "450000201c46400040119c6ec0a80001c0a800c77f5c1f90000cffff70696e67", F.DONE),
    ("udp6_updates_to_zero",
     "60000000000c114020010db800000000000000000000000120010db800000000000000000000000204001f90000ca20070696e67",
     F.rule(F.SET_SPORT, 0, sport=b"\xa6\x00"), 0,
     "60000000000c114020010db800000000000000000000000120010db8000000000000000000000002a6001f90000c000070696e67",
     F.DONE),
    ("udp6_updates_to_zero_as_ones",
     "60000000000c114020010db800000000000000000000000120010db800000000000000000000000204001f90000ca20070696e67",
     F.rule(F.SET_SPORT, 0, sport=b"\xa6\x00"), F.UDP_ZERO_AS_ONES,
     "60000000000c114020010db800000000000000000000000120010db8000000000000000000000002a6001f90000cffff70696e67",
     F.DONE),
    # HC = 0xFFFF (correct: the rest sums to 0xFFFF) and a destination port set to the value it has:
    # ~HC + ~m + m = 0xFFFF, so HC' = 0x0000 -- the other spelling of the same sum
    ("tcp4_ffff_unchanged_word",
     "450000281c46400040060a880a0000010a00000204001f90000076500000000050020200ffff0000",
     F.rule(F.SET_DPORT, 4, dport=b"\x1f\x90"), 0,
     "450000281c46400040060a880a0000010a00000204001f9000007650000000005002020000000000", F.DONE),
    # ICMP over IPv4 has no pseudo-header: the header field changes, the ICMP field does not
    ("icmp4_set_src",
     "4500001c1c46400040010a990a0000010a0000020800f7ff00000000", F.rule(F.SET_SRC, 4, src=SRC4), 0,
     "4500001c1c4640004001d891cb0071070a0000020800f7ff00000000", F.DONE),
    # IHL 15: the ports at 60, the TCP field at 76
    ("ipv4_40_option_bytes",
     "4f0000501c4640004006ec4c0a0000010a00000201010101010101010101010101010101010101010101010101010101010101010101"
     "01010101010004001f90000000010000000050020200764f0000", _ALL4, 0,
     "4f0000501c4640003f069b0acb007107c633640901010101010101010101010101010101010101010101010101010101010101010101"
     "010101010100c001003500000001000000005002020087660000", F.DONE),
    # what leaves a frame alone
    ("ttl_1_expires",
     "4500001c1c46400001010a990a0000010a0000020800f7ff00000000", F.rule(F.DEC_TTL), 0,
     "4500001c1c46400001010a990a0000010a0000020800f7ff00000000", F.EXPIRED),
    ("family_differs",
     "4500001c1c46400040010a990a0000010a0000020800f7ff00000000", F.rule(F.SET_SRC, 6, src=SRC6), 0,
     "4500001c1c46400040010a990a0000010a0000020800f7ff00000000", F.UNHANDLED),
    ("port_rule_on_icmp",
     "4500001c1c46400040010a990a0000010a0000020800f7ff00000000", F.rule(F.SET_SPORT, 0, sport=SPORT), 0,
     "4500001c1c46400040010a990a0000010a0000020800f7ff00000000", F.UNHANDLED),
    ("fragment_under_dec_ttl_alone",
     "4500001c1c46200040012a990a0000010a0000020800f7ff00000000", F.rule(F.DEC_TTL, 4), 0,
     "4500001c1c4620003f012b990a0000010a0000020800f7ff00000000", F.DONE),
    ("fragment_under_nat",
     "4500001c1c46200040012a990a0000010a0000020800f7ff00000000", F.rule(F.SET_SRC, 4, src=SRC4), 0,
     "4500001c1c46200040012a990a0000010a0000020800f7ff00000000", F.UNHANDLED),
    ("total_length_past_the_frame",
     "4500001d1c46400040010a990a0000010a0000020800f7ff00000000", F.rule(F.DEC_TTL), 0,
     "4500001d1c46400040010a990a0000010a0000020800f7ff00000000", 0),
)


def test_hand_written_cases():
    for name, before, rule, flags, after, done in HAND:
        got, got_done = F.rewrite(bytes.fromhex(before), rule, flags)
        assert (got.hex(), got_done) == (after, done), name
    # RFC 1624 section 4 in numbers
    assert F.update(0xDD2F, b"\x55\x55", b"\x32\x85") == 0x0000
    # an invalid rule leaves the frame alone
    f = bytes.fromhex(HAND[7][1])
    for bad in (F.rule(32), F.rule(F.DEC_TTL, 5), F.rule(F.SET_SRC, 0, src=SRC4), F.rule(F.SET_DST | F.DEC_TTL, 0)):
        assert not F.rule_valid(bad) and F.rewrite(f, bad) == (f, 0)
    assert F.rule_valid(F.rule(F.SET_SPORT | F.SET_DPORT | F.DEC_TTL, 0))


def far_tcp_frames():
    """The v6_ext_len_255 frames of the structured set whose TCP field lies past byte 96."""
    frames, names, _ = structured_set()
    return [f for f, n in zip(frames, names)
            if n == "v6_ext_len_255" and _proto(f) == F.TCP and T._upper(f)[1] + 16 >= 96 and
            T._upper(f)[2] - T._upper(f)[1] >= 20]


def test_ipv6_chain_past_the_window():
    far = far_tcp_frames()
    assert far
    for f in far:
        at = T._upper(f)[1]
        g, done = F.rewrite(f, rule_table()[7 + 3], 0)  # all five ops, family 6
        assert done == F.DONE
        changed = {i for i in range(len(f)) if f[i] != g[i]}
        assert changed <= {7} | set(range(8, 40)) | set(range(at, at + 4)) | {at + 16, at + 17} and 7 in changed
        assert g[8:40] == SRC6 + DST6 and g[at:at + 4] == SPORT + DPORT and g[7] == f[7] - 1
        assert R.verdict(g) == R.verdict(f)


def test_abi_declares_and_exports_fwd_rewrite_ring():
    from pip_amd import _lib

    raw = (ROOT / "include" / "pipck.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"\bint\s+pipck_fwd_rewrite_ring\s*\(([^)]*)\)\s*;", text)
    assert m, "include/pipck.h does not declare pipck_fwd_rewrite_ring"
    params = [p.strip() for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["d_arena", "slot_stride", "d_lens", "n_slots", "d_rules",
                                                           "n_rules", "d_rule_of", "flags", "d_done", "d_err", "stream"]
    assert int(re.search(r"#define PIPCK_VERSION_MINOR (\d+)", text).group(1)) >= 6
    assert "1.6: pipck_fwd_rewrite_ring" in re.sub(r"\s+", " ", raw)
    for name, value in (("SET_SRC", 1), ("SET_DST", 2), ("SET_SPORT", 4), ("SET_DPORT", 8), ("DEC_TTL", 16),
                        ("UDP_ZERO_AS_ONES", 1), ("DONE", 1), ("EXPIRED", 2), ("UNHANDLED", 4),
                        ("NO_RULE", 0xFFFFFFFF)):
        m = re.search(r"#define PIPCK_FWD_%s\s+(\w+)u\b" % name, text)
        assert m and int(m.group(1), 0) == value == getattr(_lib, "FWD_" + name), name
    assert C.sizeof(_lib.FwdRule) == 48
    assert [(n, getattr(_lib.FwdRule, n).offset) for n, _ in _lib.FwdRule._fields_] == [
        ("ops", 0), ("family", 4), ("pad", 5), ("src", 8), ("dst", 24), ("sport", 40), ("dport", 42), ("pad2", 44)]
    restype, argtypes = _lib.SIGNATURES["pipck_fwd_rewrite_ring"]
    assert restype is C.c_int and len(argtypes) == 11
    assert [argtypes[i] for i in (1, 3, 5, 7)] == [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32]
    lib = _lib.load()
    assert hasattr(lib, "pipck_fwd_rewrite_ring")
    assert lib.pipck_version() >> 16 == 1 and lib.pipck_version() & 0xFFFF >= 6
    # n_slots == 0 returns before any pointer check; argument errors carry the function's name
    p16 = C.c_void_p(16)
    assert lib.pipck_fwd_rewrite_ring(None, 0, None, 0, None, 0, None, 0, None, None, None) == _lib.PIPCK_OK
    for args in ((p16, 1024, p16, 1, p16, 1, None, 2, p16, None, None),  # an unknown flag bit
                 (p16, 1024, p16, 1, None, 1, None, 0, p16, None, None),  # no rule table
                 (p16, 1024, p16, 1, p16, 0, None, 0, p16, None, None),  # no rules
                 (p16, 1024, p16, 1, C.c_void_p(24), 1, None, 0, p16, None, None)):  # a misaligned rule table
        assert lib.pipck_fwd_rewrite_ring(*args) == _lib.PIPCK_EINVAL
        assert b"pipck_fwd_rewrite_ring" in lib.pipck_last_error()
