"""tests/verify_reference.py held to pip, on the CPU, before any kernel is held
to it: its sum against the oracle restatement of pip's checksum functions and
against pip's own known answers (tests/golden/kat.json), and the sealing /
damage helpers of tests/verify_sealing.py against its verdict."""
import numpy as np
import pytest

from tests import verify_reference as vr
from tests import verify_sealing as vs
from tests.golden.make_golden import pattern_bytes

LENGTHS = list(range(71)) + [1480, 9001, 65535]
SRC4, DST4 = bytes([192, 168, 33, 2]), bytes([10, 0, 255, 1])
SRC6, DST6 = bytes(range(1, 17)), bytes(range(0xF0, 0x100))


def _ck(data, pseudo=None) -> int:
    return ~vr.ones_sum(data, pseudo) & 0xFFFF


@pytest.mark.parametrize("fill", ["random", "zero", "ff"])
def test_reference_sum_equals_the_oracle(oracle, fill):
    rng = np.random.default_rng(11)
    for n in LENGTHS:
        data = {"random": rng.integers(0, 256, n, dtype=np.uint8).tobytes(), "zero": bytes(n), "ff": b"\xff" * n}[fill]
        assert _ck(data) == oracle.ip_checksum(data), n
        for proto in (6, 17, 0, 255):
            assert _ck(data, (4, SRC4, DST4, proto)) == oracle.inet_checksum(data, proto, SRC4, DST4), (n, proto)
            assert _ck(data, (6, SRC6, DST6, proto)) == oracle.inet6_checksum(data, proto, SRC6, DST6), (n, proto)
        # the all-zero and all-0xFF flows of the GPU tests' tables
        for alen, fam, fn in ((4, 4, oracle.inet_checksum), (16, 6, oracle.inet6_checksum)):
            assert _ck(data, (fam, bytes(alen), bytes(alen), 0)) == fn(data, 0, bytes(alen), bytes(alen)), n
            ff = b"\xff" * alen
            assert _ck(data, (fam, ff, ff, 255)) == fn(data, 255, ff, ff), n


def test_reference_accepts_numpy_bytes():
    a = np.arange(37, dtype=np.uint8)
    assert vr.ones_sum(a) == vr.ones_sum(a.tobytes()) == vr.ones_sum(bytearray(a.tobytes()))
    assert vr.ones_sum(b"") == 0 and vr.verdict(b"") == 0
    assert vr.ones_sum(b"\xff\xff") == 0xFFFF and vr.verdict(b"\xff\xff") == 1
    assert vr.verdict(bytes(20)) == 0  # +0 is not "all ones"
    with pytest.raises(ValueError):
        vr.ones_sum(b"ab", (4, SRC6, DST6, 6))


def test_reference_sum_equals_pips_known_answers(kat):
    """Every single-buffer known answer of kat.json that carries a checksum (pip's
    compiled results): pip_ip_checksum, pip_inet_checksum, pip_inet6_checksum."""
    seen = {"ip": 0, "inet": 0, "inet6": 0}
    for c in kat:
        if c["fn"] not in seen:
            continue
        data = pattern_bytes(c["data"])
        if len(data) > 65535:
            # outside the batch domain (pipck.h: len <= 65535): pip's u32 accumulator wraps
            # there (the 131,076-byte known answers), which the exact-integer rule does not mirror
            continue
        pseudo = None
        if c["fn"] != "ip":
            pseudo = (4 if c["fn"] == "inet" else 6, bytes.fromhex(c["src"]), bytes.fromhex(c["dst"]), c["proto"])
        assert _ck(data, pseudo) == c["expect"], c
        seen[c["fn"]] += 1
    assert all(v >= 30 for v in seen.values()), seen


def _one_packet(rng, oracle, i, n, fam):
    """A sealed packet of n bytes at a random offset inside random bytes; returns
    (host, offset, pseudo)."""
    pseudo = None
    if fam:
        alen = 4 if fam == 4 else 16
        pseudo = (fam, rng.integers(0, 256, alen, dtype=np.uint8).tobytes(),
                  rng.integers(0, 256, alen, dtype=np.uint8).tobytes(), int(rng.integers(0, 256)))
    o = int(rng.integers(0, 16))
    host = rng.integers(0, 256, o + n + 16, dtype=np.uint8)
    offs, lens = np.array([o], dtype=np.uint64), np.array([n], dtype=np.uint32)
    fields = vs.seal(host, offs, lens, lambda _: pseudo, oracle, rng, rotate=i)  # field position i of the rotation
    assert (fields[0] >= 0) == (n >= 2)
    return host, o, pseudo


def test_sealing_makes_every_packet_verify(oracle):
    rng = np.random.default_rng(12)
    for n in LENGTHS:
        for fam in (0, 4, 6):
            for i in range(5):  # every field position of the rotation
                host, o, pseudo = _one_packet(rng, oracle, i, n, fam)
                assert vr.verdict(host[o:o + n], pseudo) == (1 if n >= 2 else 0), (n, fam, i)
    # all-zero and all-0xFF packets: the 0x0000 / 0xFFFF corners of the field
    for n in (2, 3, 20, 1480):
        for fill in (0, 0xFF):
            host = np.full(n, fill, dtype=np.uint8)
            offs, lens = np.array([0], dtype=np.uint64), np.array([n], dtype=np.uint32)
            for pseudo in (None, (4, bytes(4), bytes(4), 0), (6, b"\xff" * 16, b"\xff" * 16, 255)):
                vs.seal(host, offs, lens, lambda _: pseudo, oracle, rng)
                assert vr.verdict(host, pseudo) == 1, (n, fill, pseudo)


def test_one_flipped_bit_is_always_caught(oracle):
    rng = np.random.default_rng(13)
    for k in range(10_000):
        n = int(rng.integers(2, 200)) if k % 50 else int(rng.choice([1480, 9001, 65535]))
        fam = (0, 4, 6)[k % 3]
        host, o, pseudo = _one_packet(rng, oracle, 4, n, fam)
        assert vr.verdict(host[o:o + n], pseudo) == 1
        host[o + int(rng.integers(0, n))] ^= 1 << int(rng.integers(0, 8))
        assert vr.verdict(host[o:o + n], pseudo) == 0, (k, n, fam)


def test_damage_classes(oracle):
    """damage(): class 0 and 2 packets stop verifying (unless the swapped bytes
    are equal), class 1 (two whole words swapped) and 3..7 still verify; the
    batch meets check_mix()."""
    rng = np.random.default_rng(14)
    n = 4000
    lens = rng.integers(0, 120, n).astype(np.uint32)
    offs = (np.arange(n, dtype=np.uint64) * 128 + rng.integers(0, 8, n).astype(np.uint64))
    host = rng.integers(0, 256, n * 128 + 16, dtype=np.uint8)
    _, table = vs.flow_table(rng, 6, 97, 17)
    pseudo_of = lambda i: table[(5 + i) % 97]  # noqa: E731
    fields = vs.seal(host, offs, lens, pseudo_of, oracle, rng)
    sealed = host.copy()
    assert np.array_equal(vs.expected(host, offs, lens, pseudo_of), (lens >= 2).astype(np.uint8))
    vs.damage(host, offs, lens, rng)
    want = vs.expected(host, offs, lens, pseudo_of)
    vs.check_mix(want, lens, fields)
    for i in range(n):
        o, length, k = int(offs[i]), int(lens[i]), i % 8
        same = np.array_equal(host[o:o + length], sealed[o:o + length])
        if length < 2:
            assert want[i] == 0
        elif k in (0, 2) and not same:
            assert want[i] == 0, i
        else:
            assert want[i] == 1, i
        assert same == (k >= 3 or (k == 0 and length < 1) or (k == 1 and length < 4) or (k == 2 and length < 3)
                        or (k in (1, 2) and same)), i
    # nothing outside the packets was touched by seal() or damage()
    mask = np.ones(host.size, dtype=bool)
    for o, length in zip(offs, lens):
        mask[int(o):int(o) + int(length)] = False
    assert np.array_equal(host[mask], sealed[mask])
