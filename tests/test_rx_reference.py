"""CPU: tests/rx_reference.py (the plain reference of the PIPCK_RX_* verdict
that tests/test_gpu_rx_reference.py holds every GPU path to) is itself pinned
-- to the packets pip's own stack emits, to every packet the suite's other
generators label by construction with the oracle's (pip's) checksums, to a
table of short frames labelled by hand, and to the properties a checksum
verdict must have.  The structured set and the fuzz of the GPU tests are
checked here for what they claim to contain, so a GPU run cannot pass on an
empty class."""
import random
from collections import Counter

import numpy as np

from tests import rx_reference as R
from tests import test_gpu_rx_reference as G
from tests.test_boundary import GOLDEN, _oracle_packets, _unchecked_and_walked_cases
from tests.test_gpu_rx import _device_edge_cases, _labelled_packets

IP_OK, L4_OK, L4_CHECKED = R.IP_OK, R.L4_OK, R.L4_CHECKED


def _mismatches(frames, want):
    return [(f[:64].hex(), len(f), w, R.verdict(f)) for f, w in zip(frames, want) if R.verdict(f) != w][:5]


def test_packets_of_pips_stack_verify():
    pkts = [bytes.fromhex(ln.strip()) for ln in GOLDEN.read_text().splitlines() if ln.strip() and
            not ln.startswith(("PACKETS", "VERIFY"))]
    assert len(pkts) >= 20
    assert not _mismatches(pkts, [R.VERIFIED] * len(pkts))


def test_labelled_packets_of_the_other_generators(oracle):
    """Every packet that tests/test_gpu_rx.py and tests/test_boundary.py label by
    construction (checksums by the oracle, pip's arithmetic) gets its label."""
    for seed, paddings in ((101, [0, 3]), (202, [0, 3, 17])):
        pkts, want = _labelled_packets(oracle, seed, paddings)
        assert len(pkts) == 5000 and not _mismatches(pkts, want)
    good, checked, broken = _oracle_packets(oracle)
    assert not _mismatches(good, [7 if c else 3 for c in checked])
    assert not _mismatches(broken, [5 if c else 3 for c in checked])
    assert sum(p[0] >> 4 == 4 and p[0] & 15 > 5 for p in good) > 200
    cases = [(p, w) for p, w in _device_edge_cases(oracle) if w is not None]
    assert len(cases) >= 16 and not _mismatches(*zip(*cases))
    cases, walked, bad, overlong, short = _unchecked_and_walked_cases(oracle)
    assert not _mismatches(*zip(*cases))
    assert not _mismatches(bad, [IP_OK | L4_CHECKED] * len(bad))
    assert not _mismatches([overlong] + short, [IP_OK] * 4)


def test_hand_labelled_table():
    rows = G.table()
    assert len(rows) >= 30
    for frame, want, why in rows:
        assert R.verdict(frame) == want, (frame.hex(), want, R.verdict(frame), why)
    assert {w for _, w, _ in rows} == {0, 1, 2, 3, 5, 6, 7}


def _built(n, seed):
    """n valid frames over both families, every checked protocol, options and
    extension headers, odd and even lengths."""
    rng = random.Random(seed)
    out = []
    for k in range(n):
        fam = rng.choice([4, 6])
        proto = rng.choice([R.TCP, R.UDP, R.ICMP if fam == 4 else R.ICMP6])
        options = rng.randbytes(4 * rng.randint(1, 10)) if fam == 4 and k % 2 else b""
        ext = None
        if fam == 6 and k % 2:
            chain = [(rng.choice([R.HOPOPTS, R.DSTOPTS, R.FRAGMENT]), rng.choice([0, 1, 5]))
                     for _ in range(rng.randint(1, 4))]
            ext = R.ext_chain([(t, 0 if t == R.FRAGMENT else a) for t, a in chain], proto)
        f = R.build(rng, fam, proto, rng.randint(R.MIN_L4[proto], 200), options=options, ext=ext)
        out.append(f + rng.randbytes(rng.choice([0, 0, 1, 18])))
    return out


def test_single_bit_properties():
    """Over 2,000 built frames (all verdict 7): any one bit of the L4 message
    flipped gives 5 -- but 3 where the flip zeroes a UDP-over-IPv4 checksum
    field; any one bit of IPv4 header bytes 1, 4, 5, 8, 10, 11 flipped clears
    exactly bit 0."""
    rng = random.Random(8)
    for f in _built(2000, 4):
        assert R.verdict(f) == R.VERIFIED, f.hex()
        a, b = R.l4_range(f)
        v4 = f[0] >> 4 == 4
        udp4 = v4 and f[9] == R.UDP
        picks = [(rng.randrange(a, b), rng.randrange(8)) for _ in range(4)]
        if udp4:
            c = f[a + 6] << 8 | f[a + 7]
            if bin(c).count("1") == 1:  # one bit away from "no checksum"
                picks.append((a + 6 if c >> 8 else a + 7, (c >> 8 or c).bit_length() - 1))
        for i, bit in picks:
            q = bytearray(f)
            q[i] ^= 1 << bit
            none_sent = udp4 and q[a + 6] == 0 and q[a + 7] == 0
            assert R.verdict(q) == (3 if none_sent else 5), (f.hex(), i, bit)
        if v4:
            for i in G.HDR_ONLY:
                q = bytearray(f)
                q[i] ^= 1 << rng.randrange(8)
                assert R.verdict(q) == R.VERIFIED & ~IP_OK, (f.hex(), i)
    # the exception itself, on a frame made for it
    # (a data word chosen so that the correct checksum field is 0x0100)
    f = bytearray(R.build(rng, 4, R.UDP, 0, l4=rng.randbytes(6) + bytes(6), fill=False))
    s0 = R.wsum(f[20:]) + R.wsum(f[12:20]) + R.UDP + 12
    f[28:30] = ((0xFFFF - 0x0100 - s0) % 0xFFFF).to_bytes(2, "big")
    f[26:28] = b"\x01\x00"
    assert R.verdict(f) == 7, f.hex()
    f[26] ^= 0x01
    assert R.verdict(f) == 3


def test_structured_set_holds_what_it_claims():
    """The GPU tests' structured set: about 3,000 frames, short but for the named
    long ones, every class at every start residue, every verdict the classes are
    built for; and the valid variant of every checkable class verifies."""
    frames, names, starts = G.structured_set()
    want = G.reference_verdicts()
    G.assert_alignment(names, starts)
    assert 2500 <= len(frames) <= 3600, len(frames)
    assert all(len(f) <= G.SHORT or n in ("long", "v6_ext_len_255") for f, n in zip(frames, names))
    per = {n: Counter() for n in names}
    for n, w in zip(names, want):
        per[n][int(w)] += 1
    assert set(per) >= {"v4_options", "v6_offsets", "v6_fragment_header", "v6_ext_len_255", "v6_chain_cap",
                        "link_padding", "sum_corners", "malformed_and_truncated", "table", "long", "tiny"}
    assert set(per["v4_options"]) >= {7, 5, 6, 3, 2} and per["v4_options"][7] == 120
    assert set(per["v6_offsets"]) == {7, 5} and per["v6_offsets"][7] >= 180
    assert set(per["v6_fragment_header"]) == {7, 5, 3}
    assert set(per["v6_ext_len_255"]) == {7, 5}
    assert set(per["v6_chain_cap"]) == {7, 5, 3}
    assert set(per["link_padding"]) >= {7, 5, 6} and per["link_padding"][7] >= 500
    assert set(per["sum_corners"]) >= {7, 5, 3}
    assert set(per["malformed_and_truncated"]) >= {0, 1}
    assert per["long"] == {7: 2} and set(per["tiny"]) == {0} and set(per["filler"]) == {0}
    assert R.verdict(G.host_only()) == 7 and len(G.host_only()) == 65545
    # IHL 6..15 each verify with every protocol it was built with
    ihl_ok = Counter((f[0] & 15, f[9]) for f, n, w in zip(frames, names, want) if n == "v4_options" and w == 7)
    assert all(ihl_ok[(ihl, p)] >= 4 for ihl in range(6, 16) for p in (R.TCP, R.UDP, R.ICMP))
    # upper-layer offsets 48..104 each verify; padding straddles byte 80
    offs = Counter(R.l4_range(f)[0] for f, n, w in zip(frames, names, want) if n == "v6_offsets" and w == 7)
    assert set(offs) == set(range(48, 105, 8))
    pads = {(len(f) - (R.l4_range(f)[1]), R.l4_range(f)[1]) for f, n in zip(frames, names) if n == "link_padding"}
    assert pads >= {(p, e) for p in G.PADDINGS for e in G.IP_ENDS}


def test_fuzz_reaches_every_verdict():
    frames = G.fuzz_frames()
    want = np.array([R.verdict(f) for f in frames], dtype=np.uint8)
    assert len(frames) == 20000
    G.assert_fuzz_condition(frames, want)
    v4 = [f for f in frames if len(f) >= 20 and f[0] >> 4 == 4]
    assert 0.3 < sum(f[0] & 15 > 5 for f in v4) / len(v4) < 0.5
