"""The refusals of the four code families' C entry points against tests/golden/code_refusals.json (recorded once by
tests/golden/make_code_refusals.py): the same tests make the same calls, and every call the library refuses must answer with the
recorded function, return code and message, in the recorded order.  The recorder is the generator's."""
import json
import sys
from pathlib import Path

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
import make_code_refusals as M  # noqa: E402

RECORDED = json.loads((GOLDEN / "code_refusals.json").read_text())


def test_the_fixture_names_every_family_and_only_refusals():
    assert len(RECORDED) > 100 and all(len(r) == 3 and r[1] < 0 and r[2].startswith(r[0] + ":") for r in RECORDED)
    for family in ("wf_ldpc_", "wf_conv_", "wf_turbo_", "wf_rs_"):
        assert any(r[0].startswith(family + "code_create") for r in RECORDED), family


def test_every_refusal_is_the_recorded_one():
    got = M.record()
    for i, (g, w) in enumerate(zip(got, RECORDED)):
        assert g == w, f"refusal {i}"
    assert len(got) == len(RECORDED)
