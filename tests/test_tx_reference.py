"""CPU: tests/tx_reference.py, the plain reference of pipck_tx_fill_device, pinned
three ways before the GPU tests (tests/test_gpu_tx_fill.py) hold the kernel to it:

  * against bytes pip's compiled stack wrote (tests/golden/stack_replay.txt);
  * against the oracle's pip_ip_checksum / pip_inet_checksum / pip_inet6_checksum
    (oracle/oracle.py) over every family, protocol, option and extension shape;
  * against the RX reference: what it fills, rx_reference.verdict accepts;

and on the 0x0000 / 0xFFFF corners of the sum, whose frames the GPU tests reuse."""
import functools
import random
import struct
from pathlib import Path

from tests import rx_reference as R
from tests import tx_reference as T

GOLDEN = Path(__file__).resolve().parent / "golden" / "stack_replay.txt"

CORNER_KINDS = ("tcp4_zero", "tcp6_zero", "udp4_zero", "udp6_zero", "icmp6_zero", "ip4_header_zero",
                "udp4_zero_flag", "udp6_zero_flag", "icmp4_all_zero")


def pip_frames():
    """The IP packets pip's real stack emitted (parsed as tests/test_boundary.py parses them)."""
    pkts = [bytes.fromhex(ln.strip()) for ln in GOLDEN.read_text().splitlines()
            if ln.strip() and not ln.startswith(("PACKETS", "VERIFY"))]
    assert len(pkts) >= 20
    return pkts


def preset(rng, frame, how):
    """The frame with every checksum field fill() writes overwritten: how =
    "zero", "random", or "correct" (the value fill() stores with flags 0)."""
    f = bytearray(frame)
    good, _ = T.fill(frame)
    for at, _ in T.fields(frame):
        f[at:at + 2] = {"zero": b"\0\0", "random": rng.randbytes(2), "correct": good[at:at + 2]}[how]
    return bytes(f)


def _zero_sum(rng, fam, proto, l4len, word_at, **kw):
    """A frame whose L4 sum (field zeroed, pseudo-header included) is a non-zero
    multiple of 0xFFFF: the two message bytes at word_at are adjusted."""
    f = bytearray(R.build(rng, fam, proto, l4len, fill=False, **kw))
    a, b = R.l4_range(f)
    c = a + R.CSUM_AT[proto]
    f[c:c + 2] = b"\0\0"
    f[a + word_at:a + word_at + 2] = b"\0\0"
    addresses = f[12:20] if fam == 4 else f[8:40]
    s = R.wsum(f[a:b]) + R.wsum(addresses) + proto + (b - a)
    f[a + word_at:a + word_at + 2] = struct.pack(">H", -s % 0xFFFF)
    s = R.wsum(f[a:b]) + R.wsum(addresses) + proto + (b - a)
    assert s > 0 and s % 0xFFFF == 0
    f[c:c + 2] = rng.randbytes(2)  # whatever the field holds
    if fam == 4:
        f[10:12] = rng.randbytes(2)
    return bytes(f)


def _zero_header(rng, options=b""):
    """An IPv4 frame whose header sum (field zeroed) is a multiple of 0xFFFF, by its ip_id."""
    f = bytearray(R.build(rng, 4, R.TCP, 33, options=options, fill=False))
    ihl = 20 + len(options)
    f[10:12] = b"\0\0"
    f[4:6] = b"\0\0"
    f[4:6] = struct.pack(">H", -R.wsum(f[:ihl]) % 0xFFFF)
    assert R.wsum(f[:ihl]) % 0xFFFF == 0
    f[10:12] = rng.randbytes(2)
    return bytes(f)


@functools.lru_cache(maxsize=None)
def corner_frames():
    """[(kind, frame, flags)]: the 0x0000 / 0xFFFF corners of every sum the call computes."""
    rng = random.Random(1624)
    out = []
    for k in range(3):
        odd = k & 1  # an odd message length: the last byte pads to a word
        out.append(("tcp4_zero", _zero_sum(rng, 4, R.TCP, 40 + odd, 24, options=rng.randbytes(4 * k)), 0))
        out.append(("tcp6_zero", _zero_sum(rng, 6, R.TCP, 44 + odd, 20), 0))
        out.append(("udp4_zero", _zero_sum(rng, 4, R.UDP, 18 + odd, 8), 0))
        out.append(("udp6_zero", _zero_sum(rng, 6, R.UDP, 30 + odd, 12), 0))
        out.append(("icmp6_zero", _zero_sum(rng, 6, R.ICMP6, 16 + odd, 8), 0))
        out.append(("ip4_header_zero", _zero_header(rng, rng.randbytes(8 * k)), 0))
        out.append(("udp4_zero_flag", _zero_sum(rng, 4, R.UDP, 21 + odd, 10), T.UDP_ZERO_AS_ONES))
        out.append(("udp6_zero_flag", _zero_sum(rng, 6, R.UDP, 12 + odd, 8, ext=R.ext_chain([(R.DSTOPTS, k)], R.UDP)),
                    T.UDP_ZERO_AS_ONES))
        out.append(("icmp4_all_zero", R.build(rng, 4, R.ICMP, 0, l4=bytes(2) + rng.randbytes(2) + bytes(4 + 7 * k),
                                              fill=False), 0))
    assert {k for k, _, _ in out} == set(CORNER_KINDS)
    return tuple(out)


def shaped_frames():
    """Frames of every family, protocol, IPv4 option length and IPv6 extension
    shape, their checksum fields left as random bytes (build(..., fill=False))."""
    rng = random.Random(42)
    out = []
    for proto in (R.TCP, R.UDP, R.ICMP, R.ICMP6, 47):
        for l4len in (R.MIN_L4.get(proto, 8), 21, 61, 300, 1461):
            for ihl in range(5, 16):
                out.append(R.build(rng, 4, proto, l4len, options=rng.randbytes(4 * (ihl - 5)), fill=False))
            out.append(R.build(rng, 4, proto, l4len, frag=0x2000, fill=False))
            for chain in ([], [(R.HOPOPTS, 0)], [(R.DSTOPTS, 3)], [(R.HOPOPTS, 1), (R.FRAGMENT, 0), (R.DSTOPTS, 0)],
                          [(R.DSTOPTS, 255)], [(R.HOPOPTS, 0), (R.DSTOPTS, 0), (R.FRAGMENT, 0), (R.DSTOPTS, 0)] * 2,
                          [(R.DSTOPTS, 0)] * 9, [(R.ROUTING, 0)], [(R.FRAGMENT, 8)]):
                out.append(R.build(rng, 6, proto, l4len, ext=R.ext_chain(chain, proto) if chain else None,
                                   fill=False))
            # link padding, short and past the 80-byte window
            out.append(R.build(rng, 6, proto, l4len, ext=R.ext_chain([(R.DSTOPTS, 1)], proto), fill=False) +
                       rng.randbytes(7))
            out.append(R.build(rng, 4, proto, l4len, options=rng.randbytes(12), fill=False) + b"\xff" * 100)
    return out


def test_fill_reproduces_pips_wire_bytes():
    """Every packet pip's compiled stack emitted, its checksum fields overwritten
    with zero, with random bytes and with their own value: fill() gives back
    the recorded bytes exactly."""
    rng = random.Random(5)
    pkts = pip_frames()
    fams = set()
    for p in pkts:
        where = T.fields(p)
        v4 = p[0] >> 4 == 4
        assert [b for _, b in where] == ([T.IP_FILLED] if v4 else []) + [T.L4_FILLED], p.hex()
        fams.add((p[0] >> 4, p[9] if v4 else p[6]))
        for how in ("zero", "random", "correct"):
            q = preset(rng, p, how)
            assert how == "correct" or q != p
            got, done = T.fill(q)
            assert got == p, (how, p.hex(), got.hex())
            assert done == (3 if v4 else 2)
    assert fams >= {(4, R.TCP), (4, R.UDP), (6, R.TCP), (6, R.UDP)}


def test_fill_equals_the_oracle(oracle):
    """The stored fields are htons of the oracle's pip_ip_checksum /
    pip_inet_checksum / pip_inet6_checksum over the same range with the field
    zeroed, for every family, protocol, option and extension shape."""
    seen = {}
    for f in shaped_frames() + [f for _, f, _ in corner_frames()]:
        got, done = T.fill(f)
        v4 = f[0] >> 4 == 4
        assert len(got) == len(f)
        changed = {i for i in range(len(f)) if got[i] != f[i]}
        allowed = set()
        if done & T.IP_FILLED:
            ihl = (f[0] & 15) * 4
            hdr = bytearray(f[:ihl])
            hdr[10:12] = b"\0\0"
            assert got[10:12] == struct.pack(">H", oracle.ip_checksum(bytes(hdr)))
            allowed |= {10, 11}
        if done & T.L4_FILLED:
            a, b = R.l4_range(f)
            proto = f[9] if v4 else _upper_proto(f)
            c = a + R.CSUM_AT[proto]
            msg = bytearray(f[a:b])
            msg[R.CSUM_AT[proto]:R.CSUM_AT[proto] + 2] = b"\0\0"
            if v4 and proto == R.ICMP:
                want = oracle.ip_checksum(bytes(msg))
            elif v4:
                want = oracle.inet_checksum(bytes(msg), proto, f[12:16], f[16:20])
            else:
                want = oracle.inet6_checksum(bytes(msg), proto, f[8:24], f[24:40])
            assert got[c:c + 2] == struct.pack(">H", want), (f[:80].hex(), proto)
            allowed |= {c, c + 1}
            seen[(f[0] >> 4, proto, a)] = seen.get((f[0] >> 4, proto, a), 0) + 1
        assert changed <= allowed
    assert {(v, p) for v, p, _ in seen} == {(4, R.TCP), (4, R.UDP), (4, R.ICMP), (6, R.TCP), (6, R.UDP), (6, R.ICMP6)}
    assert {a for v, _, a in seen if v == 4} == set(range(20, 64, 4))  # every IHL
    assert {a for v, _, a in seen if v == 6} >= {40, 48, 72, 104, 2088}  # up to 8 headers, and Hdr Ext Len 255


def _upper_proto(f):
    """Next-header value of the upper layer of an IPv6 frame R.l4_range walks."""
    nh, at = f[6], 40
    while nh in (R.HOPOPTS, R.DSTOPTS, R.FRAGMENT):
        nh, at = f[at], at + (8 if nh == R.FRAGMENT else 8 * (f[at + 1] + 1))
    return nh


def check_verdict_after_fill(frame, flags):
    """What fill() filled, the RX reference accepts."""
    got, done = T.fill(frame, flags)
    v = R.verdict(got)
    if done & T.IP_FILLED:
        assert v & R.IP_OK, frame[:64].hex()
    if done & T.L4_FILLED:
        v4 = frame[0] >> 4 == 4
        assert not v4 or done & T.IP_FILLED
        a, _ = R.l4_range(got)
        udp4_none = v4 and got[9] == R.UDP and got[a + 6:a + 8] == b"\0\0"
        assert not udp4_none or not flags & T.UDP_ZERO_AS_ONES
        assert v == (R.UNCHECKED if udp4_none else R.VERIFIED), (frame[:64].hex(), v, done)
    return got, done


def test_what_fill_fills_the_rx_reference_accepts():
    from tests.test_gpu_rx_reference import fuzz_frames

    counts = [0] * 4
    for flags in (0, 1):
        for f in shaped_frames() + [f for _, f, _ in corner_frames()] + list(fuzz_frames()[:4000]):
            counts[check_verdict_after_fill(f, flags)[1]] += 1
    assert min(counts) >= 100, counts


def test_corner_frames():
    """Sums that are a multiple of 0xFFFF store 0x0000 -- 0xFFFF for UDP under
    PIPCK_TX_UDP_ZERO_AS_ONES -- and the all-zero ICMPv4 message stores 0xFFFF."""
    corners = corner_frames()
    kinds = [k for k, _, _ in corners]
    for kind in CORNER_KINDS:
        assert kinds.count(kind) >= 1, kind
    for kind, f, flags in corners:
        got, done = T.fill(f, flags)
        if kind == "ip4_header_zero":
            assert done & T.IP_FILLED and got[10:12] == b"\0\0", kind
            continue
        assert done & T.L4_FILLED, kind
        a, _ = R.l4_range(f)
        proto = f[9] if f[0] >> 4 == 4 else _upper_proto(f)
        c = a + R.CSUM_AT[proto]
        want = b"\xff\xff" if kind in ("udp4_zero_flag", "udp6_zero_flag", "icmp4_all_zero") else b"\0\0"
        assert got[c:c + 2] == want, (kind, got[c:c + 2].hex())
        if kind.startswith("udp"):  # the same frame under the other flag value
            other, _ = T.fill(f, flags ^ T.UDP_ZERO_AS_ONES)
            assert other[c:c + 2] == (b"\0\0" if flags else b"\xff\xff"), kind
        check_verdict_after_fill(f, flags)


def test_fill_is_idempotent_and_leaves_unfilled_frames_alone():
    for f in shaped_frames()[:400] + [b"", bytes(19), bytes(20), b"\x45" + bytes(30), b"\x60" + bytes(38)]:
        for flags in (0, 1):
            once, done = T.fill(f, flags)
            assert T.fill(once, flags) == (once, done)
            if not done:
                assert once == bytes(f)
