"""The host halves of the uncoded links against tests/golden/link_geometry.json (recorded once by
tests/golden/make_link_geometry.py): the geometry entry points of the SOQPSK and CPM links and their streams must answer every
configuration of the sweep as recorded, and the run and stream-chunk entry points must refuse every recorded call with the
recorded return code and message.  No GPU: the refusals come before a device is touched.  The recorder is the generator's."""
import json
import sys
from pathlib import Path

GOLDEN = Path(__file__).resolve().parent / "golden"
sys.path.insert(0, str(GOLDEN))
import make_link_geometry as M  # noqa: E402

RECORDED = json.loads((GOLDEN / "link_geometry.json").read_text())
GEOMETRY = ("wf_link_workspace_bytes", "wf_link_layout", "wf_link_stream_workspace_bytes", "wf_link_stream_layout", "wf_link_stream_interior",
            "wf_cpm_link_workspace_bytes", "wf_cpm_link_layout", "wf_cpm_link_stream_workspace_bytes", "wf_cpm_link_stream_layout")
REFUSING = ("wf_link_run", "wf_cpm_link_run", "wf_link_stream_chunk", "wf_link_stream_chunk_phase", "wf_link_stream_steady",
            "wf_cpm_link_stream_chunk", "wf_cpm_link_stream_chunk_phase", "wf_link_stage_ms")


def test_the_fixture_covers_the_sweep_and_every_entry_point():
    geo, ref = RECORDED["geometry"], RECORDED["refusals"]
    assert len(geo) == 4 * 2 * 5 * 3 * 5 + 4 * 8 * 3 and sum(len(g[1]) for g in geo) > 15_000
    # (every kind of answer occurs: accepted and refused streams, interior and edge chunks)
    flat = [a for g in geo for a in g[1]]
    assert any(a == -1 for a in flat) and any(a == 1 for a in flat) and sum(isinstance(a, list) for a in flat) > 2_000
    assert {r[0] for r in ref} == set(REFUSING) and all(len(r) == 4 and r[2] < 0 and r[3] for r in ref)
    src = (GOLDEN / "make_link_geometry.py").read_text()
    assert all(f"lib.{fn}" in src for fn in GEOMETRY)


def test_every_geometry_answer_is_the_recorded_one():
    got = M.geometry()
    for g, w in zip(got, RECORDED["geometry"]):
        assert g == w, w[0]
    assert len(got) == len(RECORDED["geometry"])


def test_every_refusal_is_the_recorded_one():
    got = M.refusals()
    for g, w in zip(got, RECORDED["refusals"]):
        assert g == w, f"{w[0]}: {w[1]}"
    assert len(got) == len(RECORDED["refusals"])
