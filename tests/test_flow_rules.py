"""pip_amd/csrc/pipck_flow.hpp pinned on the CPU: the one definition of a packet's
implicit flow, the three cheaper forms the kernels use in its place (stepping walk,
tile form, task form), the packet's result and the refusal report.

The header is plain integer code that compiles without HIP; tests/flow_rules_main.cpp
includes it in that form, is built here with g++ and answers queries on stdin.  Every
expected value is a Python integer from tests/saturation_cases.py (implicit_flow;
checksum / verdict through fold16), never a second copy of the C++.
"""
import shutil
import subprocess
from pathlib import Path

import pytest

from tests import saturation_cases as sc

ROOT = Path(__file__).resolve().parent.parent
WRAP = 1 << 64
NEAR_WRAP = tuple(o for o in sc.FLOW_ORIGINS if o >= WRAP - 200)  # the three origins near 2^64
K_FIXED_GRID_STEP = 4 * 304 * 256  # a k_fixed grid step of that order: blocks x packets per block


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    """ask(list of query lines) -> list of answer lines, as lists of ints."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    exe = tmp_path_factory.mktemp("flow_rules") / "flow_rules"
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", str(exe),
                    str(ROOT / "tests" / "flow_rules_main.cpp")], check=True)

    def run(queries):
        r = subprocess.run([str(exe)], input="".join(q + "\n" for q in queries), capture_output=True, text=True,
                           check=True)
        answers = [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
        assert len(answers) == len(queries)
        return answers

    return run


def test_header_has_no_hip_without_hipcc():
    """Nothing of HIP is included unless __HIPCC__ is defined (the g++ build above depends on it)."""
    text = (ROOT / "pip_amd" / "csrc" / "pipck_flow.hpp").read_text()
    guarded = text.split("#ifdef __HIPCC__", 1)[1].split("#else", 1)[0]
    assert "#include <hip/" in guarded
    assert "#include <hip/" not in text.replace(guarded, "")


def test_definition(ask):
    cases = [(o, i, nf) for o in sc.FLOW_ORIGINS for nf in sc.FLOW_COUNTS for i in range(256)]
    got = ask([f"def {o} {i} {nf}" for o, i, nf in cases])
    for (o, i, nf), (g,) in zip(cases, got):
        assert g == sc.implicit_flow(o, i, nf), (o, i, nf)


def _walk_parts(origin, first, step, count):
    """The walk first, first + step, ... (count indices) of a batch with this flow_origin, as
    launch_fixed runs it: whole where flow_origin + index never passes 2^64, else the part before
    the wrap (this origin) and the part from it on (origin 0, indices counted from the wrap).
    Yields (origin, first, k0, k1): walk indices k0 .. k1 - 1 start at `first` under `origin`."""
    to_wrap = (WRAP - origin) % WRAP
    if origin == 0 or first + (count - 1) * step < to_wrap:
        yield origin, first, 0, count
        return
    k0 = 0 if first >= to_wrap else -(-(to_wrap - first) // step)  # first k with first + k step >= to_wrap
    if k0:
        yield origin, first, 0, k0
    yield 0, first + k0 * step - to_wrap, k0, count


@pytest.mark.parametrize("step", (1, 64, 256, K_FIXED_GRID_STEP))
def test_stepping_walk(ask, step):
    count = 300
    queries, expect = [], []
    for o in sc.FLOW_ORIGINS:
        for nf in sc.FLOW_COUNTS:
            for start in (0, 1, 63):
                for po, pfirst, k0, k1 in _walk_parts(o, start, step, count):
                    assert po + pfirst + (k1 - k0 - 1) * step < WRAP  # the walk's precondition
                    queries.append(f"walk {po} {pfirst} {step} {nf} {k1 - k0}")
                    expect.append([sc.implicit_flow(o, start + k * step, nf) for k in range(k0, k1)])
    assert any(q.startswith("walk 0 ") for q in queries)  # some walk was split at the wrap
    for q, g, e in zip(queries, ask(queries), expect):
        assert g == e, q


def test_tile_form(ask):
    cases = []
    for o in NEAR_WRAP:
        for tile in sorted({0, 1, (WRAP - o) // 64}):  # the last: the tile holding the wrap
            cases += [(o, tile, nf) for nf in sc.FLOW_COUNTS]
    assert len(NEAR_WRAP) == 3
    got = ask([f"tile {o} {t} {nf}" for o, t, nf in cases])
    for (o, t, nf), g in zip(cases, got):
        assert g == [sc.implicit_flow(o, 64 * t + lane, nf) for lane in range(64)], (o, t, nf)


def test_task_form(ask):
    """f0 = flow_origin + p0 around the 32-bit remainder's bound 2^32 - 65, and near 2^64."""
    f0s = ((1 << 32) - 66, (1 << 32) - 65, (1 << 32) - 64, (1 << 32) - 1, 1 << 32) + NEAR_WRAP
    cases = []
    for f0 in f0s:
        for p0 in (0, 64, 1000):  # the same f0 as origin alone and as origin + p0
            cases += [(f0 - p0, p0, nf) for nf in sc.FLOW_COUNTS]
    got = ask([f"task {o} {p0} {nf}" for o, p0, nf in cases])
    for (o, p0, nf), g in zip(cases, got):
        assert g == [sc.implicit_flow(o, p0 + lane, nf) for lane in range(64)], (o, p0, nf)


def _bytes_with_word_sum(total: int) -> bytes:
    """Data whose big-endian 16-bit words add up to `total`: 0xFFFF words and one remainder word."""
    q, r = divmod(total, 0xFFFF)
    return b"\xff\xff" * q + r.to_bytes(2, "big")


def test_result(ask):
    sums = (0, 1, 0xFFFE, 0xFFFF, 0x10000, 0x1FFFE, 0x1FFFF)
    pf = []
    for s in sums:  # F is a folded sum (at most 0xFFFF); P carries the rest
        pf += [(s - f, f) for f in sorted({0, min(s, 1), min(s, 0xFFFF)})]
    pf += [(0xFFFF0000, 0xFFFF), ((1 << 32) - 1, 0)]
    cases = [(v, p, f, bad) for p, f in pf for v in (0, 1) for bad in (0, 1)]
    got = ask([f"res {v} {p} {f} {bad}" for v, p, f, bad in cases])
    got4 = ask([f"res4 {v} {p} {f} {bad}" for v, p, f, bad in cases])  # the form that also reports the refusal
    for (v, p, f, bad), (g,), g4 in zip(cases, got, got4):
        assert p + f < 1 << 32  # (no u32 wrap in these: the data below has exactly this sum)
        data = _bytes_with_word_sum(p + f)
        assert sc.words(data) == p + f
        want = 0 if bad else (sc.verdict(data) if v else sc.checksum(data))
        assert g == want, (v, hex(p), hex(f), bad)
        assert g4 == [want, (1 << 2) if bad else 0], (v, hex(p), hex(f), bad)  # 1 << PIPCK_ERANGE


def test_table_bound_and_refusal(ask):
    """An entry past the bound is refused without a table read (the program's table has 4 entries;
    a read past it would not return 0), and refuse() sets 1 << PIPCK_ERANGE only where asked."""
    got = ask(["tab 0 4", "tab 3 4", "tab 4 4", "tab 4000000000 4", "tab 2 2", f"tab 3 {(1 << 32) - 1}"])
    assert got == [[10, 0], [13, 0], [0, 1], [0, 1], [0, 1], [13, 0]]
    erange = 1 << 2  # PIPCK_ERANGE = 2 (include/pipck.h)
    text = (ROOT / "include" / "pipck.h").read_text()
    assert "#define PIPCK_ERANGE     2" in text
    got = ask(["err 0 1 1", "err 1 1 1", "err 0 0 1", "err 8 1 0", "err 8 1 1"])
    assert got == [[erange], [erange | 1], [0], [8], [8 | erange]]
