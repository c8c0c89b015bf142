"""The synchroniser forms of tools/coded_ber.py against tests/golden/coded_ber_forms.json (tests/golden/make_coded_ber_forms.py:
recorded twice, at the commit the file names): per case the printed JSON - every key, the key order, every count and every derived
float; the times only as present and positive - and the ``waveforms_amd.device`` calls of the whole run, by name and in order, must
be exactly what that commit's tool printed and made.  Without a GPU: the tool's ``ap.error`` paths and its parser's options against
the same file.  The case table and the runner are the generator's."""
import json
import math
import sys
from pathlib import Path

import pytest

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
import make_coded_ber_forms as M  # noqa: E402

RECORDED = json.loads((GOLDEN / "coded_ber_forms.json").read_text())


def ordered(value):
    """Dicts as lists of pairs: equality then counts the key order."""
    if isinstance(value, dict):
        return [[k, ordered(v)] for k, v in value.items()]
    return [ordered(v) for v in value] if isinstance(value, list) else value


def test_the_fixture_covers_the_case_table_and_is_not_vacuous():
    cases = RECORDED["cases"]
    assert list(cases) == list(M.cases()) and len(RECORDED["commit"]) == 40 and int(RECORDED["commit"], 16) >= 0
    for name, argv in M.cases().items():
        assert cases[name]["argv"] == argv + M.ebn0(name), name
    M.check(cases)
    # what two recordings of the commit disagreed in: floats of the coarse estimates only, never a count
    for path in RECORDED["unstable"]:
        assert any(f"/{k}" in path for k in M.MAY_BE_UNSTABLE) and not path.endswith("/bursts"), path


def test_the_tool_refuses_what_the_recorded_tool_refused():
    assert list(RECORDED["errors"]) == list(M.ERRORS)
    for name, argv in M.ERRORS.items():
        assert M.run_error(argv) == RECORDED["errors"][name], name


def test_the_tool_has_the_recorded_options():
    assert M.options() == RECORDED["options"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(M.LOWER_DB))
def test_gpu_tool_form_prints_the_recorded_json_and_makes_the_recorded_calls(name):
    got, want = M.run_case(name), RECORDED["cases"][name]
    for path in RECORDED["unstable"]:
        case, kind, *rest = path.strip("/").split("/")[1:]
        if case == name and kind == "json":
            M.drop(got["json"], rest)
    assert got["argv"] == want["argv"]
    assert ordered(got["json"]) == ordered(want["json"])
    assert got["calls"] == M.unfold(want["calls"])
    assert got["times"] and all(isinstance(t, (int, float)) and math.isfinite(t) and t > 0 for t in got["times"]), got["times"]
