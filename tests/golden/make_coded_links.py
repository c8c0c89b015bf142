"""tests/golden/coded_links.json: what every coded link class (waveforms_amd/encoding/coded.py, sccc.py, pccc.py, rsconv.py) does
on two small blocks, recorded at one commit: the names of the ``waveforms_amd.device`` calls of the second block, in order, and
every counter the block left on the device.  Names and integers only.  tests/test_coded_links_recorded.py runs the same cases with
the same runner and asserts equality, so a change of these classes that is meant to change nothing can show that it did.

The cases with a synchroniser keyword (``SYNC``) also record the integers of the link's ``*_result()`` - the choices per window,
``grid``, the rejected windows of an anchored track - and the crc32 of the bytes of the rows the second block's first detector call
gets.  ``coarse_result`` is all floats, so its entry is the empty list: it records that the call answered, not a value.  A link that
does not count channel bits (its synchroniser leaves the rows shifted) records ``null`` for ``uncoded_result``.

    python3 tests/golden/make_coded_links.py --commit $(git rev-parse HEAD)        (on an MI355X; writes the JSON)
    python3 tests/golden/make_coded_links.py --scan [case ...]                     (prints the Eb/N0 each case can use)

Eb/N0 per case is the operating point of the class's own tests, lowered in 0.5 dB steps where two such small blocks left no
information bit error in the first pass or the final result (``--scan`` does the lowering; the table holds the value used).
"""
import argparse
import json
import math
import zlib
from pathlib import Path
from types import SimpleNamespace

OUT = Path(__file__).resolve().parent / "coded_links.json"
SEED = 7


def _names():
    from waveforms_amd.encoding import conv, framing, ldpc, rs, turbo
    from waveforms_amd.encoding.coded import PAD_BITS, CodedCPMLink, CodedSOQPSKLink, IterativeCPMLink, IterativeSOQPSKLink
    from waveforms_amd.encoding.pccc import TurboSOQPSKLink
    from waveforms_amd.encoding.rsconv import RSConvSOQPSKLink
    from waveforms_amd.encoding.sccc import ConvSOQPSKLink
    from waveforms_amd.sync import carrier, carrier_cpm, coarse, joint, joint_cpm, timing, timing_cpm
    from waveforms_amd.viterbi import cpm

    code = ldpc.demo_code()
    rs_code = rs.RSCode.ccsds(16, 1)
    per_window = 8 * carrier.DEFAULT_WINDOW
    spec = {"multih": cpm.ARTM_64, "pcmfm": cpm.PCMFM_20}

    def cpm_clock(w, limit):              # 6 samples late and half the documented drift
        return (6.0, 0.5 * limit[w] / (8 * timing_cpm.defaults(spec[w])["window"]))

    def cpm_carrier(w, limit, window):    # 40 degrees and half the documented drift
        return (math.radians(40.0), 0.5 * limit / (spec[w].p * 8 * window))

    return SimpleNamespace(
        # the synchroniser link tests' sizes and impairments (tests/test_{timing,joint,coarse,cpm_carrier,cpm_timing,joint_cpm}_link.py)
        spec=spec, T=timing.TimingRecovery, J=joint.JointAcquisition, K=lambda: coarse.CoarseFrequency(8, nfft=1024), CC=carrier_cpm.CPMCarrierRecovery,
        TC=timing_cpm.CPMTimingRecovery, JC=joint_cpm.CPMJointAcquisition,
        timing=(6.0, 0.5 * timing.MAX_DRIFT_SAMPLES / per_window),
        joint_carrier=(math.radians(40.0), 0.025 / per_window), joint_timing=(6.0, 0.8 / per_window),
        coarse_carrier=(math.radians(40.0), 0.02), coarse_joint_carrier=(math.radians(40.0), 0.02 + 0.025 / per_window),
        coarse_ncw=-(-(4 * 1024 - 37 - PAD_BITS) // framing.Framing(code).period),      # tests/test_coarse_link.py::_ncw
        cpm_carrier=lambda w: cpm_carrier(w, carrier_cpm.MAX_DRIFT_PERIODS, carrier_cpm.DEFAULT_WINDOW),
        cpm_clock=lambda w: cpm_clock(w, timing_cpm.MAX_DRIFT_SAMPLES),
        cpm_joint_carrier=lambda w: cpm_carrier(w, joint_cpm.MAX_DRIFT_PERIODS, 256), cpm_joint_clock=lambda w: cpm_clock(w, joint_cpm.MAX_DRIFT_SAMPLES),
        CodedSOQPSKLink=CodedSOQPSKLink, IterativeSOQPSKLink=IterativeSOQPSKLink, CodedCPMLink=CodedCPMLink, IterativeCPMLink=IterativeCPMLink,
        ConvSOQPSKLink=ConvSOQPSKLink, TurboSOQPSKLink=TurboSOQPSKLink, RSConvSOQPSKLink=RSConvSOQPSKLink,
        ldpc=code, framing=lambda: framing.Framing(code), framed=lambda: dict(framing=framing.Framing(code), lead_bits=37),
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
    # the synchroniser keywords: four codewords (the coarse cases: four segments of nfft bits), a handful of windows
    "coded_soqpsk_timing": ("CodedSOQPSKLink", 5.0, lambda n: n.CodedSOQPSKLink(n.ldpc, 4, **n.framed(), timing=n.timing, timing_recovery=n.T(8))),
    "coded_soqpsk_acquisition": ("CodedSOQPSKLink", 6.0, lambda n: n.CodedSOQPSKLink(n.ldpc, 4, **n.framed(), carrier=n.joint_carrier, timing=n.joint_timing,
                                                                                     acquisition=n.J(8))),
    "coded_soqpsk_acquisition_anchor": ("CodedSOQPSKLink", 5.0, lambda n: n.CodedSOQPSKLink(n.ldpc, 4, **n.framed(), carrier=n.joint_carrier,
                                                                                            timing=n.joint_timing, acquisition=n.J(8, anchor=3))),
    "coded_soqpsk_coarse_recovery": ("CodedSOQPSKLink", 5.0, lambda n: n.CodedSOQPSKLink(n.ldpc, n.coarse_ncw, **n.framed(), carrier=n.coarse_carrier,
                                                                                         recovery=n.recovery(), coarse=n.K())),
    "coded_soqpsk_coarse_acquisition": ("CodedSOQPSKLink", 5.0, lambda n: n.CodedSOQPSKLink(n.ldpc, n.coarse_ncw, **n.framed(), carrier=n.coarse_joint_carrier,
                                                                                            timing=n.joint_timing, acquisition=n.J(8, anchor=33),
                                                                                            coarse=n.K())),
    "idd_soqpsk_acquisition": ("IterativeSOQPSKLink", 6.0, lambda n: n.IterativeSOQPSKLink(n.ldpc, 4, **n.framed(), carrier=n.joint_carrier,
                                                                                           timing=n.joint_timing, acquisition=n.J(8), **IDD)),
    "coded_cpm_pcmfm_recovery": ("CodedCPMLink", 3.0, lambda n: n.CodedCPMLink(n.ldpc, 4, waveform="pcmfm", carrier=n.cpm_carrier("pcmfm"),
                                                                               recovery=n.CC(n.spec["pcmfm"]))),
    "coded_cpm_multih_clock": ("CodedCPMLink", 8.5, lambda n: n.CodedCPMLink(n.ldpc, 4, waveform="multih", **n.framed(), clock=n.cpm_clock("multih"),
                                                                              clock_recovery=n.TC(n.spec["multih"], 8))),
    "coded_cpm_pcmfm_joint": ("CodedCPMLink", 3.5, lambda n: n.CodedCPMLink(n.ldpc, 4, waveform="pcmfm", **n.framed(), carrier=n.cpm_joint_carrier("pcmfm"),
                                                                            clock=n.cpm_joint_clock("pcmfm"), joint=n.JC(n.spec["pcmfm"], 8))),
    "coded_cpm_multih_joint_anchor": ("CodedCPMLink", 7.5, lambda n: n.CodedCPMLink(n.ldpc, 4, waveform="multih", **n.framed(),
                                                                                     carrier=n.cpm_joint_carrier("multih"), clock=n.cpm_joint_clock("multih"),
                                                                                     joint=n.JC(n.spec["multih"], 8, anchor=3))),
    "idd_cpm_pcmfm_clock": ("IterativeCPMLink", 4.0, lambda n: n.IterativeCPMLink(n.ldpc, 4, waveform="pcmfm", **n.framed(), clock=n.cpm_clock("pcmfm"),
                                                                                  clock_recovery=n.TC(n.spec["pcmfm"], 8), **IDD)),
}
# For the synchroniser cases above: the ``*_result()`` methods whose integers are recorded too (choices, grid, rejected windows),
# beside the crc32 of the rows the detector gets in the second block.
SYNC = {
    "coded_soqpsk_timing": ("timing_result",), "coded_soqpsk_acquisition": ("acquisition_result",),
    "coded_soqpsk_acquisition_anchor": ("acquisition_result",), "coded_soqpsk_coarse_recovery": ("carrier_result", "coarse_result"),
    "coded_soqpsk_coarse_acquisition": ("acquisition_result", "coarse_result"), "idd_soqpsk_acquisition": ("acquisition_result",),
    "coded_cpm_pcmfm_recovery": ("carrier_result",), "coded_cpm_multih_clock": ("clock_result",), "coded_cpm_pcmfm_joint": ("joint_result",),
    "coded_cpm_multih_joint_anchor": ("joint_result",), "idd_cpm_pcmfm_clock": ("clock_result",),
}
DETECTORS = ("viterbi_soft", "viterbi_soft_apriori", "cpm_soft", "cpm_soft_apriori")


def _ints(value):
    """The integers of a result tuple (or of a list of them): its floats are ratios of the recorded counters."""
    if isinstance(value, (list, tuple)):
        return [_ints(v) for v in value if not isinstance(v, float) and getattr(v, "dtype", None) not in ("float32", "float64")]
    return value.tolist() if hasattr(value, "dtype") else int(value)


def run_case(name: str, ebn0_db: float | None = None) -> dict:
    """Build the case's link, run blocks 0 and 1 with every public function of ``waveforms_amd.device`` recorded by name, and
    return the second block's call names and the link's counters and results."""
    from waveforms_amd import device as dev

    cls, table_db, make = CASES[name]
    ebn0_db = table_db if ebn0_db is None else ebn0_db
    link = make(_names())
    assert type(link).__name__ == cls
    calls, crcs = [], []

    def recorded(fname, fn):
        def call(*args, **kwargs):
            calls.append(fname)
            if name in SYNC and fname in DETECTORS and link.blocks == 1 and not crcs:      # (the second block's first detector call)
                crcs.append(zlib.crc32(args[0].cpu().numpy().tobytes()))
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
    try:
        uncoded = _ints(link.uncoded_result())
    except RuntimeError:                                     # (a synchroniser that leaves the rows shifted: the link does not count them)
        uncoded = None
    out = {"class": cls, "ebn0_db_x2": int(round(2 * ebn0_db)), "calls": calls, "blocks": link.blocks, "result": _ints(link.result()),
           "uncoded_result": uncoded, "counts": link.counts.cpu().tolist(), "uncoded": link.uncoded.cpu().tolist()}
    if name in SYNC:
        out["sync_results"], out["rows_crc32"] = {method: _ints(getattr(link, method)()) for method in SYNC[name]}, crcs[0]
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
    """The fixture must not pass vacuously: channel errors in every case - information bit errors, in a case whose link does not
    count channel bits -, information bit errors in every class."""
    for name, rec in records.items():
        if rec["uncoded_result"] is None:
            assert name in SYNC and info_errors(rec) > 0, f"{name}: no information bit error"
        else:
            assert rec["uncoded_result"][0] > 0, f"{name}: no channel error"
    for cls in {rec["class"] for rec in records.values()}:
        assert any(info_errors(rec) for rec in records.values() if rec["class"] == cls), f"{cls}: no information bit error in any case"


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--commit", help="hash of the commit the fixture is recorded at")
    ap.add_argument("--out", type=Path, default=OUT)
    ap.add_argument("--scan", action="store_true", help="per case: lower Eb/N0 from the table's value in 0.5 dB steps until information bit errors show")
    ap.add_argument("cases", nargs="*", help="with --scan: these cases only")
    args = ap.parse_args()
    if args.scan:
        for name, (_cls, db, _make) in CASES.items():
            if args.cases and name not in args.cases:
                continue
            rec = run_case(name, db)
            while not (info_errors(rec) and (rec["uncoded_result"] is None or rec["uncoded_result"][0])) and db > -5.0:
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
