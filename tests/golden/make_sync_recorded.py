"""tests/golden/sync_recorded.json: what the five synchronisers of waveforms_amd/sync/ (CarrierRecovery, CPMCarrierRecovery,
TimingRecovery, CPMTimingRecovery, JointAcquisition) do on bursts of 300 and 600 rows at window 64, recorded at one commit: the
names of the ``waveforms_amd.device`` calls of one ``recover``, in order, the sequence of its stage marks, ``launches`` (joint),
the coarse choices and ``grid`` (CPM timing).  Names and integers only.  tests/test_sync_recorded.py runs the same cases with the
same runner and asserts equality, so a change of these classes that is meant to change nothing can show that it did.

    python3 tests/golden/make_sync_recorded.py --check                             (CPU: the cases are not vacuous)
    python3 tests/golden/make_sync_recorded.py --commit $(git rev-parse HEAD)      (on an MI355X; writes the JSON)
    python3 tests/golden/make_sync_recorded.py --values PATH [--host-only]         (every floating-point output as bit patterns)

300 rows are 5 windows (the rescale's ``nwin < 8`` branch, a short last window), 600 are 10 (``nwin >= 8``).  The bursts are the
existing tests' (test_timing._chain, test_cpm_timing._chain, test_carrier._pt_rows, test_cpm_carrier._oracle_rows), impaired at
the documented limits (``MAX_DRIFT_TURNS``, ``MAX_DRIFT_PERIODS``, ``MAX_DRIFT_SAMPLES``) for window 64.  ``check`` holds the
conditions under which the cases say anything, on the host statements: every choice array takes two values at least, and one
timing and one carrier case unwrap a step that ``_wrap`` changes.  Where a case did not at the first start offset tried, the
offset was moved (START below has the values used); no length was raised.

``--values`` writes an .npz (not committed) of uint64 bit patterns: the rows, trajectories and ``timing_refine`` corrections of
the same cases, the stage calls on seeded synthetic tables, and the five ``recover*_host`` statements on the 300-row bursts.
Two such files of two commits compared for equality say whether a rounding moved.
"""
import argparse
import functools
import json
import math
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
OUT = HERE / "sync_recorded.json"
SPS, WINDOW, SPAN, REFINE = 8, 64, 3, 1
LENGTHS = (300, 600)
# start offsets: degrees for the carrier cases, samples for the timing cases, (degrees, samples) for joint.  At 2.7 samples, the
# existing tests' offset, cpm_timing_pcmfm_h4_300 chose hypothesis 0 in all five windows and cpm_timing_multih_h4 hypothesis 1 in
# all five and all ten: 3.5 and 6.0 put a hypothesis boundary inside the 300 rows.
START = {"carrier": 40.0, "cpm_carrier_pcmfm": 40.0, "cpm_carrier_multih": 40.0, "timing": 2.7, "cpm_timing_pcmfm": 3.5,
         "cpm_timing_multih": 6.0, "joint": (130.0, 2.7)}
SPECS = {"pcmfm": "PCMFM_20", "multih": "ARTM_64"}


def _cases() -> dict:
    """name -> (class, kind, burst key, rows, constructor keywords)"""
    out = {}
    for n in LENGTHS:
        out[f"carrier_{n}"] = ("CarrierRecovery", "carrier", "carrier", n, dict(hypotheses=3))
        out[f"timing_{n}"] = ("TimingRecovery", "timing", "timing", n, dict(hypotheses=4))
        for wf in SPECS:
            out[f"cpm_carrier_{wf}_{n}"] = ("CPMCarrierRecovery", "carrier", f"cpm_carrier_{wf}", n, dict())
            for H in (4, 8):
                out[f"cpm_timing_{wf}_h{H}_{n}"] = ("CPMTimingRecovery", "timing", f"cpm_timing_{wf}", n, dict(hypotheses=H))
        for stack in (None, 1, 2):
            out[f"joint_stack{stack}_{n}"] = ("JointAcquisition", "joint", "joint", n,
                                              dict(timing_hypotheses=3, carrier_hypotheses=3, stack=stack))
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def _oracle():
    import oracle

    oracle.build_c_oracle()
    return oracle


def _spec(wf):
    from waveforms_amd.viterbi import cpm

    return getattr(cpm, SPECS[wf])


@functools.lru_cache(maxsize=None)
def burst(key: str, n: int) -> tuple:
    """The impaired burst of a case, on the host: what ``recover`` and the host statement take besides the settings."""
    import test_carrier
    import test_cpm_carrier
    import test_cpm_timing
    import test_timing
    from waveforms_amd.sync import carrier as C
    from waveforms_amd.sync import carrier_cpm as CC
    from waveforms_amd.sync import timing as T
    from waveforms_amd.sync import timing_cpm as TC

    orc, per_sample = _oracle(), 1.0 / (SPS * WINDOW)
    if key == "carrier":
        rows = test_carrier._pt_rows(orc, n + 12)[:n]
        return (test_carrier._rot(rows, START[key], C.MAX_DRIFT_TURNS, WINDOW),)
    if key.startswith("cpm_carrier_"):
        wf = key[len("cpm_carrier_"):]
        spec, rows = test_cpm_carrier._oracle_rows(orc, wf, n + 12)
        return (test_cpm_carrier._rot(rows[:n], START[key], test_cpm_carrier._drift(spec), WINDOW),)
    if key == "timing":
        sig, _noise, taps, first, have = test_timing._chain(orc, n + 12)
        assert have >= n
        return T.timing_offset_host(sig, START[key], T.MAX_DRIFT_SAMPLES * per_sample), taps, first, n
    if key.startswith("cpm_timing_"):
        wf = key[len("cpm_timing_"):]
        _s, sig, _noise, Tm, start0, have = test_cpm_timing._chain(orc, wf, n + 12)
        assert have >= n
        return T.timing_offset_host(sig, START[key], TC.MAX_DRIFT_SAMPLES[wf] * per_sample), Tm, start0, n
    assert key == "joint"
    sig, _noise, taps, first, have = test_timing._chain(orc, n + 12)
    assert have >= n
    deg, tau0 = START[key]
    bad = T.timing_offset_host(C.carrier_offset_host(sig, math.radians(deg), C.MAX_DRIFT_TURNS * per_sample), tau0, T.MAX_DRIFT_SAMPLES * per_sample)
    return bad, taps, first, n


def run_host(name: str) -> dict:
    """The case's host statement -> {output name: ndarray}; the choices under "choice" (joint: "tchoice", "cchoice")."""
    from waveforms_amd.sync import carrier as C
    from waveforms_amd.sync import carrier_cpm as CC
    from waveforms_amd.sync import joint as J
    from waveforms_amd.sync import timing as T
    from waveforms_amd.sync import timing_cpm as TC

    cls, _kind, key, n, kw = CASES[name]
    b = burst(key, n)
    if cls == "CarrierRecovery":
        return dict(zip(("rows", "phase", "choice"), C.recover_host(b[0], WINDOW, SPAN, kw["hypotheses"], REFINE)))
    if cls == "CPMCarrierRecovery":
        return dict(zip(("rows", "phase", "choice"), CC.recover_cpm_host(_spec(key.rsplit("_", 1)[1]), b[0], WINDOW, SPAN, refine=REFINE)))
    if cls == "TimingRecovery":
        return dict(zip(("rows", "tau", "choice"), T.recover_timing_host(b[0], b[1], b[2], n, SPS, WINDOW, SPAN, kw["hypotheses"], REFINE)))
    if cls == "CPMTimingRecovery":
        out = TC.recover_cpm_timing_host(_spec(key.rsplit("_", 1)[1]), b[0], b[1], b[2], SPS, n, WINDOW, SPAN, kw["hypotheses"], REFINE)
        return dict(zip(("rows", "tau", "choice"), out[:3]), grid=np.array(out[3]))
    out = J.recover_joint_host(b[0], b[1], b[2], n, SPS, WINDOW, SPAN, kw["timing_hypotheses"], kw["carrier_hypotheses"], REFINE)
    return dict(zip(("rows", "tau", "phase", "tchoice", "cchoice"), out))


def _wraps_of(fn) -> int:
    """``fn()`` with every ``_wrap`` of waveforms_amd.sync counting the steps it changes."""
    from waveforms_amd.sync import carrier_cpm, joint, timing_cpm  # noqa: F401  (every module of the package that may hold a _wrap)

    changed = [0]
    mods = [m for k, m in sys.modules.items() if k.startswith("waveforms_amd.sync.") and hasattr(m, "_wrap")]
    real = [m._wrap for m in mods]

    def counting(wrap):
        def _wrap(x, period):
            out = wrap(x, period)
            changed[0] += int(np.count_nonzero(np.asarray(out) != np.asarray(x)))
            return out
        return _wrap

    try:
        for m, w in zip(mods, real):
            m._wrap = counting(w)
        fn()
    finally:
        for m, w in zip(mods, real):
            m._wrap = w
    return changed[0]


def check(names=None) -> dict:
    """On the host statements: every case's choice arrays take at least two values; at least one timing case and one carrier
    case (of ``names``, default all) unwrap a step that ``_wrap`` changes.  -> name -> steps changed."""
    wraps = {}
    for name in (CASES if names is None else names):
        host = {}
        wraps[name] = _wraps_of(lambda: host.update(run_host(name)))
        for k, v in host.items():
            if k.endswith("choice"):
                assert np.unique(v).size >= 2, f"{name}: {k} = {v.tolist()} takes one value"
    for kind in ("timing", "carrier"):
        assert any(w for name, w in wraps.items() if CASES[name][1] == kind), f"no {kind} case unwraps a changed step: {wraps}"
    return wraps


def check_recorded(cases: dict) -> None:
    """The same on a recorded fixture, as far as names and integers say it."""
    for name, rec in cases.items():
        assert rec["calls"] and rec["marks"] and rec["marks"][0] == "start", name
        for k, v in rec.items():
            if k.endswith("choice"):
                assert len(set(v)) >= 2 and len(v) == -(-rec["rows"] // WINDOW), f"{name}: {k} = {v}"


def run_case(name: str, values: dict | None = None) -> dict:
    """Build the case's synchroniser, run ``recover`` once with every public function of ``waveforms_amd.device`` recorded by
    name, and return the call names, the marks and the integers.  ``values``: where the floating-point outputs go, as bits."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.sync import carrier as C
    from waveforms_amd.sync import carrier_cpm as CC
    from waveforms_amd.sync import joint as J
    from waveforms_amd.sync import timing as T
    from waveforms_amd.sync import timing_cpm as TC

    cls, _kind, key, n, kw = CASES[name]
    b = burst(key, n)
    common = dict(window=WINDOW, span=SPAN, refine=REFINE, **kw)
    if cls == "CarrierRecovery":
        rec, args, outs = C.CarrierRecovery(**common), (_hip.to_device(b[0]),), ("rows", "phase", "choice")
    elif cls == "CPMCarrierRecovery":
        rec, args, outs = CC.CPMCarrierRecovery(_spec(key.rsplit("_", 1)[1]), **common), (_hip.to_device(b[0]),), ("rows", "phase", "choice")
    elif cls == "TimingRecovery":
        rec, args, outs = T.TimingRecovery(SPS, **common), (_hip.to_device(b[0]), _hip.to_device(b[1]), b[2], n), ("rows", "tau", "choice")
    elif cls == "CPMTimingRecovery":
        rec = TC.CPMTimingRecovery(_spec(key.rsplit("_", 1)[1]), SPS, **common)
        args, outs = (_hip.to_device(b[0]), _hip.to_device(b[1]), b[2], n), ("rows", "tau", "choice", "grid")
    else:
        rec = J.JointAcquisition(SPS, **common)
        args, outs = (_hip.to_device(b[0]), _hip.to_device(b[1]), b[2], n), ("rows", "tau", "phase", "tchoice", "cchoice")
    assert type(rec).__name__ == cls
    rec.times = True
    calls, refined = [], []

    def recorded(fname, fn):
        def call(*args, **kwargs):
            calls.append(fname)
            out = fn(*args, **kwargs)
            if fname == "timing_refine":
                refined.append(out)
            return out
        return call

    real = {k: v for k, v in vars(dev).items() if not k.startswith("_") and callable(v) and not isinstance(v, type)}
    ctx = _hip.new_ctx()
    try:
        for k, fn in real.items():
            setattr(dev, k, recorded(k, fn))
        got = rec.recover(*args, ctx=ctx)
        got = [_hip.to_host(v) for v in got]
        refined = [_hip.to_host(v) for v in refined]
    finally:
        for k, fn in real.items():
            setattr(dev, k, fn)
        _hip.free_ctx(ctx)
    out = {"class": cls, "rows": n, "calls": calls, "marks": [m for m, _e in rec._events]}
    if cls == "JointAcquisition":
        out["launches"] = int(rec.launches)
    for k, v in zip(outs, got):
        if v.dtype == np.float64:
            if values is not None:
                values[f"case/{name}/{k}"] = _bits(v)
        else:
            out[k] = v.reshape(-1).astype(np.int64).tolist() if v.ndim else int(v)
    if values is not None:
        for i, v in enumerate(refined):
            values[f"case/{name}/refine{i}"] = _bits(v)
    return out


def _bits(a) -> np.ndarray:
    a = np.ascontiguousarray(a)
    if a.dtype == np.complex128:
        a = a.view(np.float64)
    return a.astype(np.float64, copy=False).view(np.uint64).copy() if a.dtype == np.float64 else a.copy()


def host_values(values: dict) -> None:
    """The five host statements on the 300-row bursts (CPU)."""
    for name in CASES:
        if CASES[name][3] == LENGTHS[0] and not name.startswith(("joint_stack1", "joint_stack2")):
            for k, v in run_host(name).items():
                values[f"host/{name}/{k}"] = _bits(v)


def stage_values(values: dict) -> None:
    """The stage calls on seeded synthetic tables (device)."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.sync import carrier as C
    from waveforms_amd.sync import timing as T

    ctx = _hip.new_ctx()
    period = 16.0

    def put(key, *tensors):
        for i, t in enumerate(tensors):
            values[f"stage/{key}/{i}"] = _bits(_hip.to_host(t))

    try:
        for nwin in (1, 2, 7, 8, 1025, 2049):
            for H in (3, 8):
                # tests/test_timing_edges.py::grid_case: exact parabolas about a drifting instant, wrapped modulo the period
                rng = np.random.Generator(np.random.PCG64(1000 * H + nwin))
                true = 3.0 - 1.6 * np.arange(nwin) + rng.uniform(-0.4, 0.4, nwin)
                stat = np.zeros((H, nwin, 2))
                stat[:, :, 0] = C._wrap(T.hypothesis_instants(period, H)[:, None] - true[None, :], period) ** 2 - 8000.0
                stat[:, :, 1] = rng.standard_normal((H, nwin)) * 40.0
                stat3 = rng.standard_normal((3, nwin, 2)) * 50.0 - 2000.0
                stat3[:, ::5, 0] = -2000.0
                stat3[1, 1::5, 0] = -1000.0
                d_stat, d_stat3 = _hip.to_device(stat), _hip.to_device(stat3)
                for span in (1, 5):
                    key = f"nwin{nwin}_H{H}_span{span}"
                    put("timing_track/" + key, *dev.timing_track(d_stat, period, span, ctx=ctx))
                    put("carrier_track/" + key, *dev.carrier_track(d_stat, span, ctx=ctx))
                    put("carrier_track_mod/" + key, *dev.carrier_track(d_stat, span, ctx=ctx, period=2.0 * math.pi / 16.0))
                    put("timing_refine/" + key, dev.timing_refine(d_stat3, 2.0, span, ctx=ctx))
        for ncalls in (1, 63, 64, 65, 257, 511):
            rng = np.random.Generator(np.random.PCG64(ncalls))
            rows = _hip.to_device(rng.standard_normal((ncalls, 3, 2)) * 30.0)
            branch = _hip.to_device(rng.integers(0, 8, ncalls).astype(np.uint8))
            term = _hip.to_device(rng.standard_normal((ncalls, 2)) * 30.0)
            llr = _hip.to_device(rng.standard_normal(2 * ncalls) * 30.0)
            for W in (64, 256):
                put(f"carrier_stat/n{ncalls}_W{W}", dev.carrier_stat(rows, branch, W, ctx=ctx))
                put(f"carrier_stat_terms/n{ncalls}_W{W}", dev.carrier_stat_terms(term, W, ctx=ctx))
                for bpc in (1, 2):
                    put(f"llr_stat/n{ncalls}_W{W}_bpc{bpc}", dev.llr_stat(llr, bpc, W, ctx=ctx))
        for ncalls in (1, 65, 300):
            rng = np.random.Generator(np.random.PCG64(7000 + ncalls))
            phases = {"none": None, "one": _hip.to_device(rng.uniform(-3.0, 3.0, 1)), "five": _hip.to_device(rng.uniform(-3.0, 3.0, 5))}
            for nvals in (3, 4, 16):
                rows = _hip.to_device(rng.standard_normal((ncalls, nvals, 2)) * 30.0)
                for pname, phase in phases.items():
                    put(f"rows_derotate_n/n{ncalls}_v{nvals}_{pname}", dev.rows_derotate_n(rows, nvals, WINDOW, phase, 0.3, ctx=ctx))
                    if nvals == 3:
                        put(f"rows_derotate/n{ncalls}_{pname}", dev.rows_derotate(rows, WINDOW, phase, 0.3, ctx=ctx))
        for ncalls in (1, 65):
            rows = _hip.to_device(np.random.Generator(np.random.PCG64(9000 + ncalls)).standard_normal((ncalls, 3, 2)) * 30.0)
            for H in (1, 3, 8):
                put(f"rows_derotate_hyp/n{ncalls}_H{H}", dev.rows_derotate_hyp(rows, H, ctx=ctx))
    finally:
        _hip.free_ctx(ctx)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--commit", help="hash of the commit the fixture is recorded at")
    ap.add_argument("--out", type=Path, default=OUT)
    ap.add_argument("--check", action="store_true", help="CPU: run check() on the host statements and print the steps each case's unwrapping changes")
    ap.add_argument("--values", type=Path, help="write every floating-point output of the cases, the stages and the host statements as bit patterns")
    ap.add_argument("--host-only", action="store_true", help="with --values: the host statements alone (CPU)")
    args = ap.parse_args()
    if args.check:
        for name, w in check().items():
            print(f"{name}: {w} steps changed by the unwrapping")
        return
    if args.values:
        values: dict = {}
        host_values(values)
        if not args.host_only:
            for name in CASES:
                run_case(name, values)
            stage_values(values)
        np.savez(args.values, **values)
        print("wrote", args.values, len(values), "arrays")
        return
    if not args.commit:
        ap.error("--commit is needed to write the fixture")
    check()
    records = {name: run_case(name) for name in CASES}
    check_recorded(records)
    args.out.write_text(json.dumps({"commit": args.commit, "window": WINDOW, "cases": records}, indent=1, sort_keys=True) + "\n")
    print("wrote", args.out, len(records), "cases")


sys.path[:0] = [p for p in (str(HERE.parent), str(HERE.parent.parent)) if p not in sys.path]
if __name__ == "__main__":
    main()
