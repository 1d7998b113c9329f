"""CPU: tests/fwd_classify_reference.py, the plain reference of pipck_fwd_classify_ring /
pipck_fwd_classify_device, held to the header's two hash vectors, to the census of the
frame sets and to fwd_reference.rewrite (a frame is keyed exactly when the all-ops rule
of its family rewrites it or finds it expired); then the three host functions of
libpipck.so -- pipck_fwd_key_hash, pipck_fwd_frame_key, pipck_fwd_table_build -- through
ctypes against it, the device calls' argument errors that need no device, and the ABI.
The frame sets, key sets and hand-made tables of the GPU tests
(tests/test_gpu_fwd_classify.py) live here too."""
import ctypes as C
import functools
import re
from pathlib import Path

import pytest

from tests import fwd_classify_reference as K
from tests import fwd_reference as F
from tests.test_fwd_device_cases import short_set
from tests.test_fwd_reference import fuzz_ring_frames, rule_index, rule_table
from tests.test_gpu_rx_reference import structured_set

ROOT = Path(__file__).resolve().parents[1]
PAIRS = ((4, K.ICMP), (4, K.UDP), (4, K.TCP), (6, K.UDP), (6, K.ICMP6), (6, K.TCP))
# set -> (frames, keyed, by PAIRS or None, unkeyed, malformed)
CENSUS = {"structured": (2983, 2596, (459, 585, 460, 381, 367, 344), 311, 76),
          "short": (192, 144, (24,) * 6, 20, 28),
          "fuzz": (20840, 7273, None, 11102, 2465)}
TABLE_SLOTS = (1, 2, 64, 4096)


@functools.lru_cache(maxsize=None)
def frame_set(name):
    return tuple({"structured": lambda: structured_set()[0], "short": short_set, "fuzz": fuzz_ring_frames}[name]())


@functools.lru_cache(maxsize=None)
def classes(name):
    """frame_class of every frame of a set, computed once."""
    return tuple(K.frame_class(f) for f in frame_set(name))


def binding_rule(key, i):
    """The rule a test binding carries: an index into test_fwd_reference.rule_table, of the key's family."""
    return 7 * (key[37] == 6) + i % 7


@functools.lru_cache(maxsize=None)
def ordinary_table(name, n_slots):
    """(keys, rules, table): every other distinct key of the set in order of first appearance, as
    many as a load of 0.5 allows (one key at least), so hits and misses both occur."""
    distinct = list(dict.fromkeys(c for c in classes(name) if isinstance(c, bytes)))
    keys = distinct[::2][:max(1, n_slots // 2)]
    rules = [binding_rule(k, i) for i, k in enumerate(keys)]
    status, table = K.build(keys, rules, n_slots)
    assert status == 0, (name, n_slots, status)
    return tuple(keys), tuple(rules), table


def udp4_key(k, sport=0):
    """A family-4 UDP key of the hand-made tables: 192.0.2.x -> 198.51.100.y, the numbers from k."""
    return K.key(4, K.UDP, bytes([192, 0, 2, k & 0xFF]), bytes([198, 51, 100, k >> 8 & 0xFF]), sport, 4000 + (k >> 16))


def frame_of_key(key, pad=b""):
    """The shortest frame with this key (its checksum fields are not looked at), then `pad` as link padding."""
    src, dst, ports, proto, family = key[:16], key[16:32], key[32:36], key[36], key[37]
    l4 = (ports if proto in (K.TCP, K.UDP) else bytes(4)) + bytes(K.MIN_L4[proto] - 4)
    if family == 4:
        f = bytes([0x45, 0]) + (20 + len(l4)).to_bytes(2, "big") + bytes([0, 0, 0x40, 0, 64, proto, 0, 0]) + src[:4] + dst[:4] + l4
    else:
        f = bytes([0x60, 0, 0, 0]) + len(l4).to_bytes(2, "big") + bytes([proto, 64]) + src + dst + l4
    assert K.frame_class(f + pad) == key
    return f + pad


@functools.lru_cache(maxsize=None)
def same_home_keys(n_slots, home, count):
    """`count` udp4 keys whose hash lands on slot `home` of n_slots, by brute force over the source port."""
    out, k = [], 0
    while len(out) < count:
        key = udp4_key(home, sport=k)
        if K.key_hash(key) & (n_slots - 1) == home:
            out.append(key)
        k += 1
        assert k < 1 << 16
    return tuple(out)


@functools.lru_cache(maxsize=None)
def chain_table():
    """(keys, absent, table): 64 slots filled by 64 keys of home slot 37 -- the last one sits at
    probe 64 -- and a 65th key of the same home that is absent: no empty entry anywhere, so its
    search ends at the bound."""
    keys = same_home_keys(64, 37, 65)
    status, table = K.build(keys[:64], [100 + i for i in range(64)], 64)
    assert status == 0 and all(e is not None for e in table)
    assert table[(37 + 63) & 63][0] == keys[63] and K.lookup(table, keys[63]) == 163 and K.lookup(table, keys[64]) is None
    return keys[:64], keys[64], table


@functools.lru_cache(maxsize=None)
def wrap_table():
    """(keys, table): three keys of home slot 7 in 8 slots: entries 7, 0 and 1."""
    keys = same_home_keys(8, 7, 3)
    status, table = K.build(keys, [5, 6, 7], 8)
    assert status == 0 and [i for i, e in enumerate(table) if e] == [0, 1, 7]
    assert [table[i][0] for i in (7, 0, 1)] == list(keys)
    return keys, table


NEAR_MISS_BYTES = {"src": 3, "dst": 16 + 2, "sport": 32, "dport": 35, "proto": 36, "family": 37, "pad": 39}


@functools.lru_cache(maxsize=None)
def near_miss_tables():
    """(key, {name: table}): 16-slot tables whose one entry sits at the key's home slot with the
    key's tag, its key differing in one byte of the named field (bit 0 flipped; proto 17 -> 6,
    family 4 -> 6, pad 0 -> 1) -- each a miss -- and "tag": the right key under a wrong tag."""
    key = udp4_key(0x0503, sport=777)
    h = K.key_hash(key)
    tables = {}
    for name, at in NEAR_MISS_BYTES.items():
        other = bytearray(key)
        other[at] = {"proto": K.TCP, "family": 6}.get(name, other[at] ^ 1)
        table = [None] * 16
        table[h & 15] = (bytes(other), 9, h | 0x80000000)
        tables[name] = table
    table = [None] * 16
    table[h & 15] = (key, 9, (h ^ 0x10) | 0x80000000)
    tables["tag"] = table
    for t in tables.values():
        assert K.lookup(t, key) is None
    exact = [None] * 16
    exact[h & 15] = (key, 9, h | 0x80000000)
    assert K.lookup(exact, key) == 9
    return key, tables


# ---------------------------------------------------------------------------- the reference
def test_hash_vectors():
    assert K.key_hash(bytes(40)) == 0x00000000
    assert K.key_hash(K.key(4, K.TCP, bytes([10, 0, 0, 1]), bytes([10, 0, 0, 2]), 1234, 80)) == 0x1C838748


@pytest.mark.parametrize("name", list(CENSUS))
def test_census(name):
    frames, keyed, by_pair, unkeyed, malformed = CENSUS[name]
    cs = classes(name)
    keys = [c for c in cs if isinstance(c, bytes)]
    assert (len(cs), len(keys), cs.count(K.NO_KEY), cs.count(K.MALFORMED)) == (frames, keyed, unkeyed, malformed)
    got = tuple(sum(1 for k in keys if (k[37], k[36]) == pair) for pair in PAIRS)
    print(name, "keyed by family / protocol", dict(zip(PAIRS, got)))
    assert sum(got) == keyed and min(got) >= 24
    if by_pair:
        assert got == by_pair
    assert all(K.key_valid(k) for k in keys)


@pytest.mark.parametrize("name", list(CENSUS))
def test_keyed_exactly_when_the_all_ops_rule_rewrites_or_expires(name):
    """Consistency with fwd_reference.rewrite.  A TCP or UDP frame is keyed exactly when the
    all-ops rule of its family gives DONE or EXPIRED.  That rule sets ports, which no ICMP / ICMPv6
    frame has (step 5 of the rewrite's list), and a TTL of 0 or 1 expires a well-formed frame before
    its upper layer is looked at (step 4).  So for every protocol the exact statement is made with
    the rule that sets both addresses and nothing else: keyed <=> DONE, unkeyed <=> UNHANDLED,
    malformed <=> 0; and the all-ops rule is held to it: a keyed TCP / UDP frame is DONE or EXPIRED,
    DONE only for such a frame, a malformed one 0."""
    done_all = 0
    for f, c in zip(frame_set(name), classes(name)):
        fam = 6 if len(f) and f[0] >> 4 == 6 else 4
        addr = F.rule(F.SET_SRC | F.SET_DST, fam, rule_table()[7 * (fam == 6)]["src"], rule_table()[7 * (fam == 6)]["dst"])
        want = {F.DONE: "keyed", F.UNHANDLED: K.NO_KEY, 0: K.MALFORMED}[F.rewrite(f, addr, 0)[1]]
        assert (c if isinstance(c, str) else "keyed") == want, f[:96].hex()
        done = F.rewrite(f, rule_table()[rule_index(f, 3)], 0)[1]  # all five ops
        tcpudp = isinstance(c, bytes) and c[36] in (K.TCP, K.UDP)
        if tcpudp:
            assert done in (F.DONE, F.EXPIRED), f[:96].hex()
        assert (done == F.DONE) <= tcpudp and (done == 0) == (c == K.MALFORMED), f[:96].hex()
        done_all += done == F.DONE
    assert done_all >= 90


def test_reference_tables_and_classify():
    keys, absent, table = chain_table()
    assert [K.lookup(table, k) for k in keys] == [100 + i for i in range(64)]
    wkeys, wtable = wrap_table()
    assert [K.lookup(wtable, k) for k in wkeys] == [5, 6, 7]
    assert K.table_from_bytes(K.table_bytes(wtable)) == wtable
    hit, miss = frame_of_key(wkeys[1]), frame_of_key(absent)
    unkeyed = bytes.fromhex("4500001c1c46200040012a990a0000010a0000020800f7ff00000000")  # a fragment
    assert K.classify(hit, wtable, 11, 12) == (6, K.HIT)
    assert K.classify(miss, wtable, 11, 12) == (11, K.MISS)
    assert K.classify(unkeyed, wtable, 11, 12) == (12, K.UNKEYED)
    assert K.classify(hit[:27], wtable, 11, 12) == (K.NO_RULE, 0)
    assert K.classify(hit, wtable, 11, 12, ok=3, ok_mask=7) == (K.NO_RULE, K.PASSED)
    assert K.classify(hit, wtable, 11, 12, ok=3, ok_mask=3) == (6, K.HIT)
    assert K.classify(hit, wtable, 11, 12, ok=0, ok_mask=0) == (6, K.HIT)
    assert K.classify(miss, wtable, K.NO_RULE, 12) == (K.NO_RULE, K.MISS)
    for n_slots in TABLE_SLOTS:
        for name in CENSUS:
            keys, rules, table = ordinary_table(name, n_slots)
            hits = sum(1 for c in classes(name) if isinstance(c, bytes) and K.lookup(table, c) is not None)
            misses = sum(1 for c in classes(name) if isinstance(c, bytes) and K.lookup(table, c) is None)
            assert hits >= 1 and misses >= 1, (name, n_slots)


# ---------------------------------------------------------------------------- the host functions
def _lib():
    from pip_amd import _lib

    return _lib, _lib.load()


def _c_build(keys, rules, n_slots, alloc=None):
    """(status, table bytes) of pipck_fwd_table_build."""
    _lib_, lib = _lib()
    raw = b"".join(keys)
    kbuf = (C.c_uint8 * max(len(raw), 1)).from_buffer_copy(raw or b"\0")
    rbuf = (C.c_uint32 * max(len(rules), 1))(*rules)
    table = (_lib_.FwdEntry * (n_slots if alloc is None else alloc))()
    rc = lib.pipck_fwd_table_build(kbuf, rbuf, len(keys), table, n_slots)
    return rc, bytes(table)


def test_c_hash_and_frame_key_on_every_frame():
    _lib_, lib = _lib()
    assert lib.pipck_fwd_key_hash(None) == 0
    key = _lib_.FwdKey()
    assert lib.pipck_fwd_frame_key(None, 40, C.byref(key)) == 0
    assert lib.pipck_fwd_frame_key(C.create_string_buffer(40), 40, None) == 0
    hashed = 0
    for name in CENSUS:
        for f, c in zip(frame_set(name), classes(name)):
            C.memset(C.byref(key), 0xA5, 40)
            got = lib.pipck_fwd_frame_key(C.create_string_buffer(f, max(len(f), 1)), len(f), C.byref(key))
            if isinstance(c, bytes):
                assert got == 1 and bytes(key) == c, f[:96].hex()
                assert lib.pipck_fwd_key_hash(C.byref(key)) == K.key_hash(c)
                hashed += 1
            else:
                assert got == 0 and bytes(key) == b"\xa5" * 40, f[:96].hex()
    assert hashed == 2596 + 144 + 7273
    vec = _lib_.FwdKey.from_buffer_copy(K.key(4, K.TCP, bytes([10, 0, 0, 1]), bytes([10, 0, 0, 2]), 1234, 80))
    assert lib.pipck_fwd_key_hash(C.byref(vec)) == 0x1C838748
    assert lib.pipck_fwd_key_hash(C.byref(_lib_.FwdKey())) == 0


def test_c_tables_are_byte_identical():
    for n_slots in TABLE_SLOTS:
        for name in CENSUS:
            keys, rules, table = ordinary_table(name, n_slots)
            assert _c_build(keys, rules, n_slots) == (0, K.table_bytes(table)), (name, n_slots)
    keys, _, table = chain_table()
    assert _c_build(keys, [100 + i for i in range(64)], 64) == (0, K.table_bytes(table))
    # the probe chain that wraps from the last slot to slot 0
    wkeys, wtable = wrap_table()
    rc, raw = _c_build(wkeys, [5, 6, 7], 8)
    assert (rc, raw) == (0, K.table_bytes(wtable))
    assert [raw[48 * i:48 * i + 40] for i in (7, 0, 1)] == list(wkeys)
    # no keys: a zeroed table, whatever it held; PIPCK_FWD_NO_RULE is a rule like any other
    assert _c_build([], [], 4) == (0, bytes(4 * 48))
    rc, raw = _c_build(wkeys[:1], [K.NO_RULE], 8)
    assert rc == 0 and K.table_from_bytes(raw)[7] == (wkeys[0], K.NO_RULE, K.key_hash(wkeys[0]) | 0x80000000)
    # the engine's wrapper gives the same bytes
    from pip_amd import engine

    assert engine.build_fwd_table(wkeys, [5, 6, 7], 8) == K.table_bytes(wtable)
    assert engine.fwd_key_bytes(4, K.UDP, wkeys[0][:4], wkeys[0][16:20], wkeys[0][32:34], wkeys[0][34:36]) == wkeys[0]
    assert engine.fwd_frame_key(frame_of_key(wkeys[2])) == wkeys[2] and engine.fwd_frame_key(b"\x45" * 19) is None


def test_c_build_refusals():
    _lib_, lib = _lib()
    good = udp4_key(1, 1)
    icmp4, icmp6 = K.key(4, K.ICMP, b"\1\2\3\4", b"\5\6\7\x08"), K.key(6, K.ICMP6, bytes(range(16)), bytes(range(16, 32)))
    assert _c_build([good, icmp4, icmp6], [1, 2, 3], 8)[0] == 0

    def mutate(key, at, value):
        k = bytearray(key)
        k[at] = value
        return bytes(k)

    bad = {"pad 0": mutate(good, 38, 1), "pad 1": mutate(good, 39, 0x80), "family 5": mutate(good, 37, 5),
           "family 0": mutate(good, 37, 0), "src byte 4": mutate(good, 4, 1), "src byte 15": mutate(good, 15, 1),
           "dst byte 4": mutate(good, 16 + 4, 1), "dst byte 15": mutate(good, 16 + 15, 1),
           "protocol 2": mutate(good, 36, 2), "ICMP with family 6": mutate(icmp6, 36, K.ICMP),
           "ICMPv6 with family 4": mutate(icmp4, 36, K.ICMP6), "ICMP with a source port": mutate(icmp4, 33, 1),
           "ICMPv6 with a destination port": mutate(icmp6, 34, 1)}
    for why, k in bad.items():
        assert not K.key_valid(k), why
        assert _c_build([icmp4, k], [1, 2], 8)[0] == _lib_.PIPCK_EINVAL, why
        assert K.build([icmp4, k], [1, 2], 8)[0] == K.EINVAL, why
        assert b"pipck_fwd_table_build" in lib.pipck_last_error()
    assert _c_build([good, icmp4, good], [1, 2, 3], 8)[0] == _lib_.PIPCK_EINVAL  # a duplicate key
    assert K.build([good, icmp4, good], [1, 2, 3], 8)[0] == K.EINVAL
    for n_slots in (0, 3, 6, 1 << 32, (1 << 31) + 1, 1 << 63):  # refused before the table is touched
        assert _c_build([good], [1], n_slots, alloc=1) == (_lib_.PIPCK_EINVAL, bytes(48)), n_slots
        assert K.build([good], [1], n_slots)[0] == K.EINVAL
    kbuf, rbuf, table = (C.c_uint8 * 40).from_buffer_copy(good), (C.c_uint32 * 1)(1), (_lib_.FwdEntry * 8)()
    assert lib.pipck_fwd_table_build(kbuf, rbuf, 1, None, 8) == _lib_.PIPCK_EINVAL
    assert lib.pipck_fwd_table_build(None, rbuf, 1, table, 8) == _lib_.PIPCK_EINVAL
    assert lib.pipck_fwd_table_build(kbuf, None, 1, table, 8) == _lib_.PIPCK_EINVAL
    assert lib.pipck_fwd_table_build(None, None, 0, table, 8) == _lib_.PIPCK_OK
    # PIPCK_ERANGE: 65 keys of one home slot in 128 slots
    keys = same_home_keys(128, 90, 65)
    assert _c_build(keys[:64], list(range(64)), 128)[0] == 0
    assert _c_build(keys, list(range(65)), 128)[0] == _lib_.PIPCK_ERANGE
    assert b"64 probes" in lib.pipck_last_error()
    assert K.build(keys, list(range(65)), 128)[0] == K.ERANGE and K.build(keys[:64], list(range(64)), 128)[0] == 0


# ---------------------------------------------------------------------------- the device calls, without a device
def test_classify_argument_errors_need_no_device():
    _lib_, lib = _lib()
    p16, p128, odd = C.c_void_p(1 << 20), C.c_void_p(1 << 21), C.c_void_p((1 << 20) + 8)
    ring, dev = lib.pipck_fwd_classify_ring, lib.pipck_fwd_classify_device
    # (arena, stride, lens, n, table, n_slots, miss, other, ok, ok_mask, rule_of, class, err, stream)
    assert ring(None, 0, None, 0, None, 0, 0, 0, None, 7, None, None, None, None) == _lib_.PIPCK_OK
    assert dev(None, 0, None, None, 0, None, 0, 0, 0, None, 0, None, None, None, None) == _lib_.PIPCK_OK
    assert ring(None, 0, None, 0, None, 0, 0, 0, None, 8, None, None, None, None) == _lib_.PIPCK_EINVAL
    assert b"pipck_fwd_classify_ring" in lib.pipck_last_error() and b"ok_mask" in lib.pipck_last_error()
    assert dev(None, 0, None, None, 0, None, 0, 0, 0, None, 8, None, None, None, None) == _lib_.PIPCK_EINVAL
    assert b"pipck_fwd_classify_device" in lib.pipck_last_error() and b"ok_mask" in lib.pipck_last_error()
    good = dict(arena=p16, stride=1024, lens=p16, n=1, table=p16, n_slots=64, ok=None, ok_mask=3, rule_of=p16)
    for change, why in ((dict(arena=None), "null arena"), (dict(lens=None), "null lengths"),
                        (dict(table=None), "null table"), (dict(rule_of=None), "null rule_of"),
                        (dict(n_slots=0), "no slots"), (dict(n_slots=3), "three slots"), (dict(n_slots=96), "96 slots"),
                        (dict(n_slots=1 << 32), "2^32 slots"), (dict(table=odd), "misaligned table"),
                        (dict(ok_mask=8), "ok_mask 8"), (dict(ok_mask=0xFFFFFFFF), "ok_mask all ones"),
                        (dict(arena=odd), "misaligned arena"), (dict(stride=1000), "stride 1000"),
                        (dict(stride=1016), "stride 1016"), (dict(stride=65552), "stride past 64 KiB")):
        a = {**good, **change}
        rc = ring(a["arena"], a["stride"], a["lens"], a["n"], a["table"], a["n_slots"], 0, 0, a["ok"], a["ok_mask"],
                  a["rule_of"], None, None, None)
        assert rc == _lib_.PIPCK_EINVAL, why
        assert b"pipck_fwd_classify_ring" in lib.pipck_last_error(), why
    good = dict(arena=p128, lens=p16, tile_off=p16, n=1, table=p16, n_slots=64, ok=None, ok_mask=3, rule_of=p16)
    for change, why in ((dict(arena=None), "null arena"), (dict(lens=None), "null lengths"),
                        (dict(tile_off=None), "null index"), (dict(table=None), "null table"),
                        (dict(rule_of=None), "null rule_of"), (dict(n_slots=0), "no slots"),
                        (dict(n_slots=12), "twelve slots"), (dict(n_slots=1 << 33), "2^33 slots"),
                        (dict(table=odd), "misaligned table"), (dict(ok_mask=9), "ok_mask 9"),
                        (dict(arena=C.c_void_p((1 << 21) + 64)), "arena 64 mod 128")):
        a = {**good, **change}
        rc = dev(a["arena"], 1 << 20, a["lens"], a["tile_off"], a["n"], a["table"], a["n_slots"], 0, 0, a["ok"],
                 a["ok_mask"], a["rule_of"], None, None, None)
        assert rc == _lib_.PIPCK_EINVAL, why
        assert b"pipck_fwd_classify_device" in lib.pipck_last_error(), why


# ---------------------------------------------------------------------------- the ABI
def test_abi_declares_and_exports_classification():
    _lib_, lib = _lib()
    raw = (ROOT / "include" / "pipck.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    want = {"pipck_fwd_key_hash": ["key"],
            "pipck_fwd_table_build": ["keys", "rules", "n_keys", "table", "n_slots"],
            "pipck_fwd_frame_key": ["frame", "len", "key"],
            "pipck_fwd_classify_ring": ["d_arena", "slot_stride", "d_lens", "n_slots_ring", "d_table", "n_slots",
                                        "miss_rule", "other_rule", "d_ok", "ok_mask", "d_rule_of", "d_class", "d_err",
                                        "stream"],
            "pipck_fwd_classify_device": ["d_arena", "arena_bytes", "d_lens", "d_tile_off", "n_packets", "d_table",
                                          "n_slots", "miss_rule", "other_rule", "d_ok", "ok_mask", "d_rule_of",
                                          "d_class", "d_err", "stream"]}
    for name, params in want.items():
        m = re.search(r"\b(?:int|uint32_t)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, "include/pipck.h does not declare " + name
        assert [p.split()[-1].lstrip("*") for p in m.group(1).split(",")] == params
        assert hasattr(lib, name) and len(_lib_.SIGNATURES[name][1]) == len(params)
    assert re.search(r"const\s+void\s*\*\s*d_arena[^;]*n_slots_ring", text), "the ring is const"
    p, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    assert _lib_.SIGNATURES["pipck_fwd_classify_ring"] == (C.c_int, [p, u64, p, u64, p, u64, u32, u32, p, u32, p, p, p, p])
    assert _lib_.SIGNATURES["pipck_fwd_classify_device"] == (C.c_int, [p, u64, p, p, u64, p, u64, u32, u32, p, u32, p, p,
                                                                       p, p])
    assert _lib_.SIGNATURES["pipck_fwd_key_hash"][0] is u32
    assert int(re.search(r"#define PIPCK_VERSION_MINOR (\d+)", text).group(1)) >= 8
    assert "1.8: pipck_fwd_classify_ring" in re.sub(r"\s+", " ", raw)
    assert lib.pipck_version() >> 16 == 1 and lib.pipck_version() & 0xFFFF >= 8
    for name, value in (("MAX_PROBE", 64), ("CLASS_HIT", 1), ("CLASS_MISS", 2), ("CLASS_UNKEYED", 4), ("CLASS_PASSED", 8)):
        m = re.search(r"#define PIPCK_FWD_%s\s+(\w+)u\b" % name, text)
        assert m and int(m.group(1), 0) == value == getattr(_lib_, "FWD_" + name), name
    assert (K.MAX_PROBE, K.HIT, K.MISS, K.UNKEYED, K.PASSED) == (64, 1, 2, 4, 8)
    assert C.sizeof(_lib_.FwdKey) == 40 and C.sizeof(_lib_.FwdEntry) == 48
    assert [(n, getattr(_lib_.FwdKey, n).offset) for n, _ in _lib_.FwdKey._fields_] == [
        ("src", 0), ("dst", 16), ("sport", 32), ("dport", 34), ("proto", 36), ("family", 37), ("pad", 38)]
    assert [(n, getattr(_lib_.FwdEntry, n).offset) for n, _ in _lib_.FwdEntry._fields_] == [
        ("key", 0), ("rule", 40), ("tag", 44)]
    capturable = re.sub(r"[\s*]+", " ", raw.split("NOT capturable")[0])
    assert "pipck_fwd_classify_ring and pipck_fwd_classify_device" in capturable
