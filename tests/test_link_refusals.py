"""The refusals of the coded links' constructors against tests/golden/link_refusals.json (recorded once by
tests/golden/make_link_refusals.py): the same cases built from the same names, and every one must be refused with the recorded
exception type and the recorded message, word for word.  No case reaches a device.  The case table and the recorder are the
generator's."""
import json
import sys
from pathlib import Path

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
import make_link_refusals as M  # noqa: E402

RECORDED = json.loads((GOLDEN / "link_refusals.json").read_text())


def test_the_fixture_is_the_case_table_and_names_every_class_and_kind_of_refusal():
    assert list(RECORDED) == list(M.cases(M._names()))
    assert {r[0] for r in RECORDED.values()} == {"ValueError", "TypeError"} and all(r[1] for r in RECORDED.values())
    for cls in ("CodedSOQPSKLink", "IterativeSOQPSKLink", "CodedCPMLink multih", "CodedCPMLink pcmfm", "IterativeCPMLink multih",
                "IterativeCPMLink pcmfm"):
        assert sum(name.startswith(cls + ":") for name in RECORDED) > 40, cls


def test_every_refusal_is_the_recorded_one():
    got = M.record()
    for name, want in RECORDED.items():
        assert got[name] == want, name
    assert got == RECORDED
