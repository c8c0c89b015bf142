"""tests/golden/coded_links.json: what every coded link class (waveforms_amd/encoding/coded.py, sccc.py, pccc.py, rsconv.py) does
on two small blocks, recorded at one commit: the names of the ``waveforms_amd.device`` calls of the second block, in order, and
every counter the block left on the device.  Names and integers only.  tests/test_coded_links_recorded.py runs the same cases with
the same runner and asserts equality, so a change of these classes that is meant to change nothing can show that it did.

    python3 tests/golden/make_coded_links.py --commit $(git rev-parse HEAD)        (on an MI355X; writes the JSON)
    python3 tests/golden/make_coded_links.py --scan                                (prints the Eb/N0 each case can use)

Eb/N0 per case is the operating point of the class's own tests, lowered in 0.5 dB steps where two such small blocks left no
information bit error in the first pass or the final result (``--scan`` does the lowering; the table holds the value used).
"""
import argparse
import json
import math
from pathlib import Path
from types import SimpleNamespace

OUT = Path(__file__).resolve().parent / "coded_links.json"
SEED = 7


def _names():
    from waveforms_amd.encoding import conv, framing, ldpc, rs, turbo
    from waveforms_amd.encoding.coded import CodedCPMLink, CodedSOQPSKLink, IterativeCPMLink, IterativeSOQPSKLink
    from waveforms_amd.encoding.pccc import TurboSOQPSKLink
    from waveforms_amd.encoding.rsconv import RSConvSOQPSKLink
    from waveforms_amd.encoding.sccc import ConvSOQPSKLink
    from waveforms_amd.sync import carrier

    code = ldpc.demo_code()
    rs_code = rs.RSCode.ccsds(16, 1)
    return SimpleNamespace(
        CodedSOQPSKLink=CodedSOQPSKLink, IterativeSOQPSKLink=IterativeSOQPSKLink, CodedCPMLink=CodedCPMLink, IterativeCPMLink=IterativeCPMLink,
        ConvSOQPSKLink=ConvSOQPSKLink, TurboSOQPSKLink=TurboSOQPSKLink, RSConvSOQPSKLink=RSConvSOQPSKLink,
        ldpc=code, framing=lambda: framing.Framing(code),
        # tests/test_carrier_link.py: 40 degrees and half the documented frequency limit
        carrier=(math.radians(40.0), 0.5 * carrier.MAX_DRIFT_TURNS / (8 * carrier.DEFAULT_WINDOW)), recovery=carrier.CarrierRecovery,
        conv=conv.nasa_k3(1022, tx_order=conv.qpp_order(2048, 31, 64)),                  # tests/test_sccc_link.py::sccc_code
        turbo=turbo.TurboCode.qpp(512, 31, 64),                                           # tests/test_pccc_link.py::link_code
        rs=rs_code, rs_inner=conv.ccsds_k7(8 * rs_code.n))                                # tests/test_rsconv_link.py::make(1)


IDD = dict(outer=3, inner=5, per_pass=True)
# name -> (class, information Eb/N0 in dB, constructor call on the names above)
CASES = {
    "coded_soqpsk_pt": ("CodedSOQPSKLink", 4.5, lambda n: n.CodedSOQPSKLink(n.ldpc, 5, detector="PT")),
    "coded_soqpsk_pam_framed": ("CodedSOQPSKLink", 4.5, lambda n: n.CodedSOQPSKLink(n.ldpc, 5, detector="PAM", framing=n.framing(), lead_bits=37)),
    "coded_soqpsk_carrier": ("CodedSOQPSKLink", 4.5, lambda n: n.CodedSOQPSKLink(n.ldpc, 5, framing=n.framing(), lead_bits=37, carrier=n.carrier,
                                                                                 recovery=n.recovery())),
    "idd_soqpsk": ("IterativeSOQPSKLink", 4.5, lambda n: n.IterativeSOQPSKLink(n.ldpc, 5, **IDD)),
    "idd_soqpsk_framed_live": ("IterativeSOQPSKLink", 4.5, lambda n: n.IterativeSOQPSKLink(n.ldpc, 5, framing=n.framing(), lead_bits=37, live_only=True,
                                                                                           **IDD)),
    "idd_soqpsk_framed_marker0": ("IterativeSOQPSKLink", 4.5, lambda n: n.IterativeSOQPSKLink(n.ldpc, 5, framing=n.framing(), lead_bits=37,
                                                                                              marker_prior=0.0, **IDD)),
    "coded_cpm_pcmfm": ("CodedCPMLink", 3.0, lambda n: n.CodedCPMLink(n.ldpc, 5, waveform="pcmfm")),
    "coded_cpm_multih_framed": ("CodedCPMLink", 7.0, lambda n: n.CodedCPMLink(n.ldpc, 5, waveform="multih", framing=n.framing(), lead_bits=37)),
    "idd_cpm_multih": ("IterativeCPMLink", 7.0, lambda n: n.IterativeCPMLink(n.ldpc, 5, waveform="multih", **IDD)),
    "idd_cpm_pcmfm_framed": ("IterativeCPMLink", 3.0, lambda n: n.IterativeCPMLink(n.ldpc, 5, waveform="pcmfm", framing=n.framing(), lead_bits=1, **IDD)),
    "idd_cpm_pcmfm_warmup0": ("IterativeCPMLink", 3.0, lambda n: n.IterativeCPMLink(n.ldpc, 5, waveform="pcmfm", prior_warmup=0, **IDD)),
    "conv_outer1": ("ConvSOQPSKLink", 4.0, lambda n: n.ConvSOQPSKLink(n.conv, 8, outer=1)),
    "conv_outer3": ("ConvSOQPSKLink", 4.0, lambda n: n.ConvSOQPSKLink(n.conv, 8, outer=3, per_pass=True)),
    "turbo_outer1": ("TurboSOQPSKLink", 5.0, lambda n: n.TurboSOQPSKLink(n.turbo, 8, outer=1)),
    "turbo_outer2": ("TurboSOQPSKLink", 5.0, lambda n: n.TurboSOQPSKLink(n.turbo, 8, outer=2, per_pass=True)),
    "turbo_no_early_stop": ("TurboSOQPSKLink", 5.0, lambda n: n.TurboSOQPSKLink(n.turbo, 8, outer=2, early_stop=False)),      # (no per-pass counts)
    "rsconv_outer1": ("RSConvSOQPSKLink", 6.0, lambda n: n.RSConvSOQPSKLink(n.rs, n.rs_inner, 2, erasures=0, outer=1)),
    "rsconv_erasures_outer2": ("RSConvSOQPSKLink", 6.0, lambda n: n.RSConvSOQPSKLink(n.rs, n.rs_inner, 2, erasures=8, outer=2)),
}


def _ints(value):
    """The integers of a result tuple (or of a list of them): its floats are ratios of the recorded counters."""
    if isinstance(value, (list, tuple)):
        return [_ints(v) for v in value if not isinstance(v, float)]
    return int(value)


def run_case(name: str, ebn0_db: float | None = None) -> dict:
    """Build the case's link, run blocks 0 and 1 with every public function of ``waveforms_amd.device`` recorded by name, and
    return the second block's call names and the link's counters and results."""
    from waveforms_amd import device as dev

    cls, table_db, make = CASES[name]
    ebn0_db = table_db if ebn0_db is None else ebn0_db
    link = make(_names())
    assert type(link).__name__ == cls
    calls = []

    def recorded(fname, fn):
        def call(*args, **kwargs):
            calls.append(fname)
            return fn(*args, **kwargs)
        return call

    real = {k: v for k, v in vars(dev).items() if not k.startswith("_") and callable(v) and not isinstance(v, type)}
    try:
        for k, fn in real.items():
            setattr(dev, k, recorded(k, fn))
        link.run_block(ebn0_db, seed=SEED, stream_id=0)
        del calls[:]
        link.run_block(ebn0_db, seed=SEED, stream_id=1)
    finally:
        for k, fn in real.items():
            setattr(dev, k, fn)
    out = {"class": cls, "ebn0_db_x2": int(round(2 * ebn0_db)), "calls": calls, "blocks": link.blocks, "result": _ints(link.result()),
           "uncoded_result": _ints(link.uncoded_result()), "counts": link.counts.cpu().tolist(), "uncoded": link.uncoded.cpu().tolist()}
    if getattr(link, "per_pass", False):
        out["pass_results"], out["pass_counts"] = _ints(link.pass_results()), link.pass_counts.cpu().tolist()
    if getattr(link, "live_only", False):
        out["live_results"] = _ints(link.live_results())
    if getattr(link, "framing", None) is not None:
        out["sync_result"] = _ints(link.sync_result()[:2])
    if hasattr(link, "rs_result"):
        out["rs_result"], out["rs_erasure_result"] = _ints(link.rs_result()), _ints(link.rs_erasure_result())
    if hasattr(link, "half_iterations"):
        out["half_iterations_sum"] = int(round(link.half_iterations() * link.blocks * link.ncw))
    return out


def info_errors(rec: dict) -> int:
    """Information bit errors of the first pass (where passes are counted) plus those of the final result."""
    return rec["result"][0] + (rec["pass_counts"][0][0] if "pass_counts" in rec else 0)


def check(records: dict) -> None:
    """The fixture must not pass vacuously: channel errors in every case, information bit errors in every class."""
    for name, rec in records.items():
        assert rec["uncoded_result"][0] > 0, f"{name}: no channel error"
    for cls in {rec["class"] for rec in records.values()}:
        assert any(info_errors(rec) for rec in records.values() if rec["class"] == cls), f"{cls}: no information bit error in any case"


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--commit", help="hash of the commit the fixture is recorded at")
    ap.add_argument("--out", type=Path, default=OUT)
    ap.add_argument("--scan", action="store_true", help="per case: lower Eb/N0 from the table's value in 0.5 dB steps until information bit errors show")
    args = ap.parse_args()
    if args.scan:
        for name, (_cls, db, _make) in CASES.items():
            rec = run_case(name, db)
            while not (info_errors(rec) and rec["uncoded_result"][0]) and db > -5.0:
                db -= 0.5
                rec = run_case(name, db)
            print(f"{name}: table {CASES[name][1]} dB, usable {db} dB, result {rec['result']} uncoded {rec['uncoded_result']}", flush=True)
        return
    if not args.commit:
        ap.error("--commit is needed to write the fixture")
    records = {name: run_case(name) for name in CASES}
    check(records)
    args.out.write_text(json.dumps({"commit": args.commit, "seed": SEED, "cases": records}, indent=1, sort_keys=True) + "\n")
    print("wrote", args.out, len(records), "cases")


if __name__ == "__main__":
    import sys

    sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))
    main()
