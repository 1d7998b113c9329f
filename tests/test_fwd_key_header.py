"""pip_amd/csrc/pipck_fwdkey.hpp pinned on the CPU: a frame's key, the hash, the table
builder and the probe -- the text the classify kernels run and pipck_fwd_key_hash /
pipck_fwd_frame_key / pipck_fwd_table_build call.

The header is plain integer code that compiles without HIP; tests/fwd_key_main.cpp
includes it in that form, is built here with g++ -fsanitize=address,undefined as a
stand-alone program and answers queries on stdin; every frame and table sits in a heap
block of exactly its size, so a read past it ends the program.  Every expected value
comes from tests/fwd_classify_reference.py, never from a second copy of the C++."""
import shutil
import subprocess
from pathlib import Path

import pytest

from tests import fwd_classify_reference as K
from tests.test_fwd_classify_reference import (chain_table, classes, frame_of_key, frame_set, near_miss_tables,
                                               ordinary_table, same_home_keys, udp4_key, wrap_table)

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "pip_amd" / "csrc" / "pipck_fwdkey.hpp"


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    """ask(list of query lines) -> list of answer lines, split at blanks."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = tmp_path_factory.mktemp("fwd_key") / "fwd_key"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "fwd_key_main.cpp")], check=True)

    def run(queries):
        r = subprocess.run([str(exe)], input="".join(q + "\n" for q in queries), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        answers = [line.split() for line in r.stdout.splitlines()]
        assert len(answers) == len(queries)
        return answers

    return run


def _hex(b):
    return bytes(b).hex() or "-"


def test_header_has_no_hip_without_hipcc():
    """Nothing of HIP is included unless __HIPCC__ is defined (the g++ build above depends on it)."""
    text = HEADER.read_text()
    guarded = text.split("#ifdef __HIPCC__", 1)[1].split("#else", 1)[0]
    assert "#include <hip/" in guarded
    assert "#include <hip/" not in text.replace(guarded, "") and "hip_runtime" not in text.replace(guarded, "")
    for other in ("pipck_fwdparse.hpp", "pipck_rxparse.hpp", "pipck_txparse.hpp", "pipck_device.hpp"):
        assert '#include "%s"' % other not in text, other


def _want_key(frame):
    c = K.frame_class(frame)
    return ["0"] if c == K.MALFORMED else ["1"] if c == K.NO_KEY else ["2", c.hex()]


def test_keys_of_the_short_set_at_every_truncation(ask):
    """Every frame of the short set whole and cut at every length from 0 to its own: the parse
    answers as the reference does and reads nothing past the bytes it is given."""
    cuts = [f[:n] for f in frame_set("short") for n in range(len(f) + 1)]
    assert len(cuts) > 6000
    got = ask(["key " + _hex(f) for f in cuts])
    kinds = set()
    for f, g in zip(cuts, got):
        assert g == _want_key(f), f.hex()
        kinds.add(g[0])
    assert kinds == {"0", "1", "2"}


def test_keys_past_the_window_and_at_the_edges(ask):
    """The structured set's frames up to 2 KiB -- extension chains around and past byte 96 among
    them -- whole, and cut one byte short of each header the walk asks for."""
    frames = [f for f in frame_set("structured") if len(f) <= 2048]
    far = [f for f, c in zip(frame_set("structured"), classes("structured"))
           if isinstance(c, bytes) and c[37] == 6 and len(f) <= 2048 and f[6] in (0, 60, 44)]
    assert len(far) >= 50
    cuts = [f[:n] for f in far[::5] for n in range(40, min(len(f), 400))]
    batch = frames + cuts
    for f, g in zip(batch, ask(["key " + _hex(f) for f in batch])):
        assert g == _want_key(f), f[:96].hex()


def test_hashes(ask):
    keys = [c for c in classes("short") if isinstance(c, bytes)] + [bytes(40), bytes([0xFF]) * 40,
                                                                   K.key(4, K.TCP, bytes([10, 0, 0, 1]), bytes([10, 0, 0, 2]), 1234, 80)]
    got = ask(["hash " + k.hex() for k in keys])
    assert [int(g[0]) for g in got] == [K.key_hash(k) for k in keys]
    assert int(got[-3][0]) == 0 and int(got[-1][0]) == 0x1C838748


def _build_query(keys, rules, n_slots):
    return "build %d %s %s" % (n_slots, ",".join(map(str, rules)) or "-", _hex(b"".join(keys)))


def test_build_equals_the_reference(ask):
    cases = [(list(k), list(r), n) for name in ("short", "structured") for n in (1, 2, 64, 4096)
             for k, r, _ in [ordinary_table(name, n)]]
    ckeys, _, _ = chain_table()
    cases.append((list(ckeys), [100 + i for i in range(64)], 64))
    cases.append((list(wrap_table()[0]), [5, 6, 7], 8))
    cases.append(([], [], 4))
    over = same_home_keys(128, 90, 65)
    cases.append((list(over), list(range(65)), 128))  # PIPCK_ERANGE
    cases.append((list(over[:64]), list(range(64)), 128))
    good = udp4_key(1, 1)
    cases.append(([good, good], [1, 2], 8))  # a duplicate
    for at, value in ((38, 1), (39, 1), (37, 5), (4, 1), (31, 1), (36, 2), (36, K.ICMP6)):
        bad = bytearray(good)
        bad[at] = value
        cases.append(([good, bytes(bad)], [1, 2], 8))
    cases.append(([K.key(4, K.ICMP, b"\1\2\3\4", b"\5\6\7\x08", 1, 0)], [1], 8))  # ICMP with a port
    for n_slots in (0, 3, 1 << 32, (1 << 31) + 2):
        cases.append(([good], [1], n_slots))
    got = ask([_build_query(*c) for c in cases])
    seen = set()
    for (keys, rules, n_slots), g in zip(cases, got):
        status, table = K.build(keys, rules, n_slots)
        seen.add(status)
        assert int(g[0]) == status, (n_slots, len(keys))
        if status == 0:
            assert g[1] == K.table_bytes(table).hex(), (n_slots, len(keys))
    assert seen == {0, K.EINVAL, K.ERANGE}


def test_lookup_equals_the_reference(ask):
    queries, want = [], []

    def add(table, key):
        queries.append("lookup %d %s %s" % (len(table), K.table_bytes(table).hex(), key.hex()))
        rule = K.lookup(table, key)
        want.append(["0"] if rule is None else ["1", str(rule)])

    ckeys, absent, ctable = chain_table()
    for k in (ckeys[0], ckeys[31], ckeys[62], ckeys[63], absent):  # probes 1, 32, 63, 64, and the bound
        add(ctable, k)
    wkeys, wtable = wrap_table()
    for k in wkeys + (absent,):
        add(wtable, k)
    key, tables = near_miss_tables()
    for name, t in tables.items():
        add(t, key)
        assert want[-1] == ["0"], name
    exact = [None] * 16
    exact[K.key_hash(key) & 15] = (key, K.NO_RULE, K.key_hash(key) | 0x80000000)
    add(exact, key)
    assert want[-1] == ["1", str(K.NO_RULE)]
    keys, rules, table = ordinary_table("short", 64)
    for c in [c for c in classes("short") if isinstance(c, bytes)][:40]:
        add(table, c)
    add([None], key)  # one slot, empty
    add([(key, 3, K.key_hash(key) | 0x80000000)], key)  # one slot, the key's
    add([(absent, 3, K.key_hash(absent) | 0x80000000)], key)  # one slot, another's: 64 probes of it
    assert want[-3:] == [["0"], ["1", "3"], ["0"]]
    assert ask(queries) == want
    assert ["1", "163"] in want and sum(w == ["0"] for w in want) >= 12
    assert frame_of_key(key)  # the GPU tests build their frames from these keys
