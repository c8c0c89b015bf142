"""The five synchronisers of waveforms_amd/sync/ against tests/golden/sync_recorded.json (tests/golden/make_sync_recorded.py:
recorded once, at the commit the file names): per case the ``waveforms_amd.device`` calls of one ``recover``, by name and in order,
the sequence of stage marks, ``launches``, the coarse choices and ``grid`` must be exactly what that commit's classes made.  The
case table and the runner are the generator's."""
import json
import sys
from pathlib import Path

import pytest

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
import make_sync_recorded as M  # noqa: E402

RECORDED = json.loads((GOLDEN / "sync_recorded.json").read_text())


def test_the_fixture_covers_the_case_table_and_is_not_vacuous():
    cases = RECORDED["cases"]
    assert sorted(cases) == sorted(M.CASES) and len(RECORDED["commit"]) == 40 and RECORDED["window"] == M.WINDOW
    for name, (cls, _kind, _key, n, _kw) in M.CASES.items():
        assert (cases[name]["class"], cases[name]["rows"]) == (cls, n), name
        assert ("launches" in cases[name]) == (cls == "JointAcquisition") and ("grid" in cases[name]) == (cls == "CPMTimingRecovery"), name
    M.check_recorded(cases)
    assert {len(c[k]) for c in cases.values() for k in c if k.endswith("choice")} == {5, 10}
    assert {cases[f"cpm_timing_{wf}_h{H}_{n}"]["grid"] for wf in M.SPECS for H in (4, 8) for n in M.LENGTHS} <= {0, 1}


def test_the_host_statements_of_the_smallest_cases_choose_and_unwrap():
    """The generator's ``check`` on the two quickest cases with a wrap, one carrier and one timing (all 22 cases:
    ``make_sync_recorded.py --check``): every choice array takes two values and each case unwraps a step that ``_wrap`` changes."""
    wraps = M.check(("carrier_600", "timing_300"))
    assert wraps["carrier_600"] >= 1 and wraps["timing_300"] >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(M.CASES))
def test_gpu_synchroniser_makes_the_recorded_calls_marks_and_choices(name):
    got, want = M.run_case(name), RECORDED["cases"][name]
    assert got["calls"] == want["calls"]
    assert got["marks"] == want["marks"]
    assert got == want
