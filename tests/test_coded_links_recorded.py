"""The coded link classes against tests/golden/coded_links.json (tests/golden/make_coded_links.py: recorded once, at the commit
the file names): per case the ``waveforms_amd.device`` calls of a block, by name and in order, and every counter two small
blocks leave must be exactly what that commit's classes made and left.  The case table and the runner are the generator's."""
import json
import sys
from pathlib import Path

import pytest

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
import make_coded_links as M  # noqa: E402

RECORDED = json.loads((GOLDEN / "coded_links.json").read_text())


def test_the_fixture_covers_the_case_table_and_is_not_vacuous():
    cases = RECORDED["cases"]
    assert sorted(cases) == sorted(M.CASES) and len(RECORDED["commit"]) == 40
    for name, (cls, db, _make) in M.CASES.items():
        assert (cases[name]["class"], cases[name]["ebn0_db_x2"]) == (cls, 2 * db), name
    M.check(cases)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(M.CASES))
def test_gpu_link_makes_the_recorded_calls_and_counts(name):
    got, want = M.run_case(name), RECORDED["cases"][name]
    assert got["calls"] == want["calls"]
    assert got == want
