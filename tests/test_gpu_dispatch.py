"""GPU: which kernel runs.  For every entry point and batch shape in
tests/dispatch_cases.py, and every tuning knob moved from its default one at a
time, the return code and the kernel instantiation launched (pipck_last_launch,
cut at the closing '>' of its template arguments) equal tests/golden/dispatch.json,
which a build of the commit named in that file wrote.  No result is asserted here:
the parity, verify and RX suites do that for the same knobs."""
import json

import pytest

from tests import dispatch_cases as dc
from tests.conftest import GOLDEN


@pytest.fixture(scope="module")
def golden():
    return json.loads((GOLDEN / "dispatch.json").read_text())


@pytest.fixture(scope="module")
def device_batches():
    return dc.Batches()


def test_golden_covers_the_case_table(golden):  # (no GPU needed)
    assert sorted(golden["cases"]) == sorted(dc.groups())
    assert golden["knobs"] == {s: list(k) for s, k in dc.KNOB_SETS.items()}
    for g in dc.groups():
        assert list(dc.decode(golden, g)) == list(dc.knobs_of(g)), g
    assert len(golden["built_from"]) == 40


@pytest.mark.gpu
@pytest.mark.parametrize("group", dc.groups())
def test_launch_selection_equals_golden(golden, device_batches, group):
    want = dc.decode(golden, group)
    got = dc.run_group(device_batches, group)
    wrong = {k: (got.get(k), want[k]) for k in want if got.get(k) != want[k]}
    assert not wrong, wrong
