"""The anchored unwrapping of both trackers on the host (waveforms_amd/sync/_stages.py: ``anchored_unwrap``; include/wfhip.h
states it; ``timing_track_host`` and ``carrier_track_host`` take it with ``anchor=K``).

The plain trackers unwrap the per-window estimates ψ_w modulo the period P BEFORE they smooth them, so one window whose estimate
errs by more than P/2 minus the drift leaves the trajectory a whole period off for the rest of the burst.  These tests pin that
defect on a deterministic table, and show that the anchored form - smooth on the circle, then unwrap - does not have it: on that
table, on seeded sequences with 2 % and 8 % of outlier windows, and at the edges of its definition (fewer windows than the
anchor, windows without an estimate, one window).  tests/test_anchored_track_gpu.py holds the device against these statements.

The ends of a burst.  The centred mean is clipped to the burst, so under a drift of d per window the trajectory's first and last
span // 2 windows lag the line by up to d whatever the unwrapping does (sync/timing.py says so where it sets
``MAX_DRIFT_SAMPLES``).  That lag is no slip.  The deterministic test therefore compares every window with the line AS THE MEAN
RENDERS IT (``centred_mean`` of the line itself), which is the line in the interior and the lagged line at the ends; the seeded
test leaves the first and last ``span`` windows out, as the issue that asked for it says.
"""
import math

import numpy as np
import pytest

from waveforms_amd.sync import _stages as S
from waveforms_amd.sync import carrier as C
from waveforms_amd.sync import timing as T

PERIODS = (math.pi, 2.0 * math.pi / 16.0)                  # SOQPSK-TG's and ARTM's carrier symmetry


# ------------------------------------------------------------------------------------------------ the tables
def timing_table(target, H: int, P: float, depth: float = 100.0):
    """float64[H, nwin, 2] whose X is a parabola (periodic in P) about ``target`` per window: ``timing_track_host`` reads ψ_w =
    target_w wrapped into [-P/2, P/2) back out of it exactly where the vertex is not clamped (a parabola's vertex is exact)."""
    s = T.hypothesis_instants(P, H)
    d = s[:, None] - np.asarray(target, dtype=np.float64)[None, :]
    d = d - P * np.round(d / P)
    X = np.zeros((H, d.shape[1], 2))
    X[:, :, 0] = d * d - depth
    return X


def carrier_table(target, H: int, P: float):
    """float64[H, nwin, 2]: hypothesis h sees the phase target - h P / H, and X is most negative at the hypothesis nearest to the
    target modulo P, so ψ_w = target_w modulo P."""
    t = np.asarray(target, dtype=np.float64)
    st = np.zeros((H, t.size, 2))
    for h in range(H):
        res = S._wrap(t - (h * P) / H, P)
        amp = 100.0 * np.cos(math.pi * res / P)            # largest where the residue is smallest
        st[h, :, 0], st[h, :, 1] = -amp * np.cos(res), -amp * np.sin(res)
    return st


def model(seed: int, nwin: int, drift: float, share: float, P: float = 8.0, sigma: float = 0.5):
    """The synthetic ψ of the issue's model -> (ψ wrapped into the period, the truth): a line of ``drift`` per window plus a slow
    sinusoidal wander, Gaussian error ``sigma``, and a ``share`` of the windows uniform over the period about the truth, a third of
    them followed by a second outlier (pairs).  In units of P / 8, so that the same sequences serve every period."""
    rng = np.random.default_rng(seed)
    w = np.arange(nwin)
    u = P / 8.0
    truth = u * (1.3 + drift * w + 0.6 * np.sin(2.0 * math.pi * 1.5 * w / max(nwin, 50)))
    psi = truth + u * sigma * rng.standard_normal(nwin)
    if nwin > 2 and share > 0.0:
        idx = rng.choice(nwin - 1, int(round(share * nwin)), replace=False)
        idx = np.unique(np.concatenate((idx, idx[: idx.size // 3] + 1)))
        psi[idx] = truth[idx] + rng.uniform(-0.5 * P, 0.5 * P, idx.size)
    return S._wrap(psi, P), truth


def steps(residual, P: float):
    """Whole periods by which a trajectory's residual moves between any two of its windows."""
    k = np.round((residual - residual[0]) / P)
    return int(k.max() - k.min())


# ------------------------------------------------------------------------------------------------ the deterministic table
H4, P8, NWIN, SPAN = 4, 8.0, 40, 5
LINE = 1.0 - 0.8 * np.arange(NWIN)


def _moved_table():
    target = LINE.copy()
    target[20] += 3.5                                       # more than P/2 - |drift| = 3.2: the step in wraps, the step out does not
    return timing_table(target, H4, P8)


def test_plain_tracker_slips_on_one_bad_window():
    """The defect, pinned: from window 23 on (behind the mean's reach of window 20) the plain trajectory is 8 ± 0.5 samples off
    the line as the mean renders it."""
    tau, _choice = T.timing_track_host(_moved_table(), P8, SPAN)
    off = tau - S.centred_mean(LINE, SPAN)
    print("plain: off the line by", np.round(off, 3))
    assert np.all(np.abs(off[:18]) < 1e-9)
    assert np.all(np.abs(off[23:] - P8) < 0.5)


def test_anchored_tracker_holds_the_line_and_rejects_the_bad_window():
    tau, choice, drift, marks = T.timing_track_host(_moved_table(), P8, SPAN, anchor=9)
    off = tau - S.centred_mean(LINE, SPAN)
    print("anchored: off the line by", np.round(off, 3), "drift", drift, "rejected", np.nonzero(marks)[0])
    assert np.all(np.abs(off) < 0.5)
    assert marks.dtype == np.uint8 and np.array_equal(np.nonzero(marks)[0], [20])
    assert abs(drift - (-0.8)) <= P8 / (4 * 9)
    assert np.array_equal(choice, T.timing_track_host(_moved_table(), P8, SPAN)[1])


@pytest.mark.parametrize("P", PERIODS)
def test_anchored_carrier_tracker_holds_the_line_and_rejects_the_bad_window(P):
    """The same table in the carrier's unit: a line of -P/10 per window, window 20 moved by 0.44 P (the timing table's 3.5 of 8)."""
    line = P * (0.125 - 0.1 * np.arange(NWIN))
    target = line.copy()
    target[20] += 0.4375 * P
    st = carrier_table(target, 4, P)
    plain = C.carrier_track_host(st, SPAN, P)[0] - S.centred_mean(line, SPAN)
    assert np.all(np.abs(plain[23:] - P) < P / 16.0)
    phase, _choice, drift, marks = C.carrier_track_host(st, SPAN, P, anchor=9, max_drift=0.25 * P)
    off = phase - S.centred_mean(line, SPAN)
    print(f"period {P:.4f}: off the line by at most {np.abs(off).max():.3g}, drift {drift:.4g}, rejected {np.nonzero(marks)[0]}")
    assert np.all(np.abs(off) < P / 16.0)
    assert np.array_equal(np.nonzero(marks)[0], [20]) and abs(drift - (-0.1 * P)) <= P / 36.0


# ------------------------------------------------------------------------------------------------ seeded sequences
@pytest.mark.parametrize("share", [0.02, 0.08])
@pytest.mark.parametrize("drift", [-0.8, 0.37])
def test_no_slip_on_seeded_sequences(drift, share):
    """826 windows, 20 seeds, K = 33: outside the first and last ``span`` windows no anchored trajectory's residual moves by a
    whole period between any two windows - asked as: by less than HALF a period, which a slip (a whole one) cannot meet and an
    error of 0.25 samples rms cannot miss.  The plain unwrapping slips in most of the same sequences, or the test showed nothing."""
    plain_slips, worst, rms = 0, 0.0, []
    for seed in range(20):
        psi, truth = model(seed, 826, drift, share)
        plain = (S.centred_mean(S.unwrap(psi, P8), SPAN) - truth)[SPAN:-SPAN]
        plain_slips += steps(plain, P8) > 0
        kept, found, marks = S.anchored_unwrap(psi, P8, 33, 1.25 * T.MAX_DRIFT_SAMPLES, 0.25 * P8)
        res = (S.centred_mean(kept, SPAN) - truth)[SPAN:-SPAN]
        worst = max(worst, float(res.max() - res.min()))
        rms.append(float(np.std(res)))
        assert res.max() - res.min() < 0.5 * P8, (seed, drift, share)
        assert abs(found - drift) <= P8 / (4 * 33) + 0.02 and 0 < marks.sum() < 0.3 * psi.size
    print(f"drift {drift}, outliers {share}: plain slips in {plain_slips} of 20, anchored in none (largest residual spread {worst:.3f}, rms {np.mean(rms):.3f})")
    assert plain_slips >= 10


@pytest.mark.parametrize("P", PERIODS)
def test_no_slip_on_seeded_carrier_sequences(P):
    """The same sequences in the carrier's unit (the model is in units of P / 8) through ``carrier_track_host`` with one
    hypothesis, which reads ψ = atan2(-Y, -X) back out of (-cos ψ, -sin ψ): the anchored trajectory never slips, the plain one does."""
    plain_slips = 0
    for seed in range(20):
        psi, truth = model(seed, 826, 0.37, 0.08, P)
        st = np.stack((-np.cos(psi), -np.sin(psi)), axis=1)[None]
        plain = (C.carrier_track_host(st, SPAN, P)[0] - truth)[SPAN:-SPAN]
        plain_slips += steps(plain, P) > 0
        phase, _c, found, marks = C.carrier_track_host(st, SPAN, P, anchor=33, max_drift=0.25 * P)
        res = (phase - truth)[SPAN:-SPAN]
        assert res.max() - res.min() < 0.5 * P, seed
        assert abs(found - 0.37 * P / 8.0) <= P / (4 * 33) + 0.0025 * P and 0 < marks.sum() < 0.3 * psi.size
    print(f"period {P:.4f}: plain slips in {plain_slips} of 20, anchored in none")
    assert plain_slips >= 10


# ------------------------------------------------------------------------------------------------ edges
K_EDGE = 9


@pytest.mark.parametrize("nwin", [1, 2, K_EDGE - 1, K_EDGE, K_EDGE + 1, 2 * K_EDGE + 1])
@pytest.mark.parametrize("P", (8.0,) + PERIODS)
def test_clean_sequences_come_back_as_the_plain_unwrap_at_every_length(nwin, P):
    """Without outliers the anchored ψ' is the plain unwrap's u up to a whole number of periods (the anchor's level is its own)
    at every length about the anchor - one window, two, a short segment, exactly one, one and a window, two and the gap between
    them - nothing is rejected and the drift found is the line's to a grid step."""
    drift = 0.11 * P
    psi = S._wrap(0.3 * P + drift * np.arange(nwin), P)
    kept, found, marks = S.anchored_unwrap(psi, P, K_EDGE, 0.25 * P, 0.25 * P)
    u = S.unwrap(psi, P)
    k = np.round((kept - u) / P)
    assert kept.shape == (nwin,) and not marks.any() and np.all(k == k[0])
    assert np.all(np.abs(kept - u - k[0] * P) < 1e-12 * P * max(nwin, 8))
    if nwin == 1:
        assert found == 0.0 and kept[0] == psi[0]
    elif nwin >= K_EDGE - 1:
        assert abs(found - drift) <= P / (4 * K_EDGE)
    for track, st in ((T.timing_track_host, timing_table(psi, 8, P)), (lambda s, p, n, **kw: C.carrier_track_host(s, n, p, **kw), carrier_table(psi, 8, P))):
        if P > 2.0 * math.pi and track is not T.timing_track_host:
            continue                                        # (the carrier's period is at most 2π)
        out = track(st, P, 3, anchor=K_EDGE, max_drift=0.25 * P)
        assert len(out) == 4 and out[0].shape == (nwin,) and out[3].shape == (nwin,) and not out[3].any()


@pytest.mark.parametrize("where", ["alone", "first", "last", "segment", "all"])
def test_windows_without_an_estimate_take_the_reference(where):
    """A ψ_w that is not finite has no phasor: it is marked and takes the reference's value - alone in mid-burst, at either end,
    a whole segment of the drift search (windows 2K .. 3K - 1), and a burst of nothing else (every score is 0, the first candidate
    is taken, and the reference is that candidate's line from 0).  A window
    with no phasor within K // 2 of it has a_w = 0 and so α_w = 0 by definition: the middle one of the empty segment is such a
    window, it is held to be finite and marked, not to be near the line."""
    P, K, nwin, drift = 8.0, K_EDGE, 5 * K_EDGE, -0.8
    line = 1.0 + drift * np.arange(nwin)
    bad = {"alone": [22], "first": [0], "last": [nwin - 1], "segment": list(range(2 * K, 3 * K)), "all": list(range(nwin))}[where]
    psi = S._wrap(line, P)
    psi[bad] = [np.nan, np.inf, -np.inf][len(bad) % 3]
    kept, found, marks = S.anchored_unwrap(psi, P, K, 2.0, 2.0)
    assert np.array_equal(np.nonzero(marks)[0], bad) and np.all(np.isfinite(kept)) and math.isfinite(found)
    if where == "all":
        assert found == -P * S.anchor_candidates(P, K, 2.0) / (4 * K) and np.array_equal(kept, found * np.arange(nwin))
        return
    off = kept - line
    k = np.round(off[0] / P) if where != "first" else np.round(off[1] / P)
    fin = np.isfinite(psi)
    anchored = np.array([fin[max(0, w - K // 2):w + K // 2 + 1].any() for w in range(nwin)])
    assert np.count_nonzero(~anchored) == (1 if where == "segment" else 0)
    assert np.all(np.abs(off - k * P)[anchored] < 0.5), off
    one = S.anchored_unwrap(np.array([np.nan]), P, K, 2.0, 2.0)
    assert one[0][0] == 0.0 and one[1] == 0.0 and one[2][0] == 1


def test_anchor_zero_is_the_present_functions_exactly():
    rng = np.random.default_rng(3)
    st = rng.standard_normal((4, 50, 2)) * 30.0 - 100.0
    for P in (8.0, 16.0):
        a, b = T.timing_track_host(st, P, 5), T.timing_track_host(st, P, 5, anchor=0, max_drift=99.0, reject=-1.0)
        assert len(a) == len(b) == 2 and np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1], b[1])
        X = st[:, :, 0]
        ch = np.argmin(X, axis=0)
        w = np.arange(50)
        psi = (ch * (P / 4) - 0.5 * P) + (P / 4) * T.vertex_host(X[(ch - 1) % 4, w], X[ch, w], X[(ch + 1) % 4, w], 0.5)
        assert np.array_equal(a[0], S.centred_mean(S.unwrap(psi, P), 5))
    for P in PERIODS:
        a, b = C.carrier_track_host(st, 5, P), C.carrier_track_host(st, 5, P, 0, None, None)
        assert len(a) == len(b) == 2 and np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1], b[1])


def test_argument_refusals():
    st = np.zeros((4, 10, 2))
    st[:, :, 0] = -1.0
    for kw in ({"anchor": 8}, {"anchor": 1}, {"anchor": 1025}, {"anchor": -3}, {"anchor": 9, "max_drift": 4.0}, {"anchor": 9, "max_drift": -0.1},
               {"anchor": 9, "max_drift": math.nan}, {"anchor": 9, "reject": 0.0}, {"anchor": 9, "reject": -1.0}, {"anchor": 9, "reject": 4.5},
               {"anchor": 9, "reject": math.inf}):
        with pytest.raises(ValueError):
            T.timing_track_host(st, 8.0, 3, **kw)
    for P in PERIODS:
        for kw in ({"anchor": 8}, {"anchor": 9, "max_drift": 0.5 * P}, {"anchor": 9, "max_drift": 0.1 * P, "reject": 0.0},
                   {"anchor": 9, "max_drift": 0.1 * P, "reject": 0.51 * P}):
            with pytest.raises(ValueError):
                C.carrier_track_host(st, 3, P, **kw)
    # the defaults: 1.25 times the documented drift, a quarter of the period
    assert S.anchor_args(9, None, None, 8.0, T.MAX_DRIFT_SAMPLES) == (9, 2.0, 2.0)
    assert S.anchor_args(0, 99.0, -1.0, 8.0, 1.6) == (0, 0.0, 0.0)
    assert S.anchor_candidates(8.0, 33, 2.0) == 33 and S.anchor_candidates(8.0, 9, 0.0) == 0


def test_classes_take_the_three_arguments_and_default_to_the_plain_trackers():
    from waveforms_amd.sync import carrier_cpm, joint, timing_cpm
    from waveforms_amd.viterbi import cpm as vc

    plain = (0, 0.0, 0.0)
    assert T.TimingRecovery(8).timing_anchor == plain and C.CarrierRecovery().carrier_anchor == plain
    assert joint.JointAcquisition(8).timing_anchor == plain and joint.JointAcquisition(8).carrier_anchor == plain
    assert T.TimingRecovery(8, anchor=33).timing_anchor == (33, 1.25 * T.MAX_DRIFT_SAMPLES, 4.0)          # period: two symbols
    acq = joint.JointAcquisition(8, anchor=33)
    assert acq.timing_anchor == (33, 1.25 * T.MAX_DRIFT_SAMPLES, 2.0)                                     # period: one symbol
    assert acq.carrier_anchor == (33, 1.25 * 2.0 * math.pi * C.MAX_DRIFT_TURNS, 0.25 * math.pi)
    assert joint.JointAcquisition(8, anchor=9, max_drift=1.0, reject=3.0).timing_anchor == (9, 1.0, 3.0)
    assert C.CarrierRecovery(anchor=5, max_drift=0.1, reject=1.0).carrier_anchor == (5, 0.1, 1.0)
    for spec, name in ((vc.ARTM_64, "multih"), (vc.PCMFM_20, "pcmfm")):
        P = carrier_cpm.period(spec)
        assert carrier_cpm.CPMCarrierRecovery(spec, anchor=33).carrier_anchor == (33, 1.25 * carrier_cpm.MAX_DRIFT_PERIODS * P, 0.25 * P)
        per = float(len(spec.K) * 8)
        assert timing_cpm.CPMTimingRecovery(spec, 8, anchor=33).timing_anchor == (33, 1.25 * timing_cpm.MAX_DRIFT_SAMPLES[name], 0.25 * per)
    for bad in ({"anchor": 4}, {"anchor": 9, "max_drift": 4.0}, {"anchor": 9, "reject": 0.0}):
        with pytest.raises(ValueError):
            joint.JointAcquisition(8, **bad)
        with pytest.raises(ValueError):
            T.TimingRecovery(8, **{**bad, "max_drift": 8.0} if "max_drift" in bad else bad)


def test_anchored_entry_points_exported_bound_and_declared():
    from pathlib import Path

    from waveforms_amd import _hip

    header = (Path(__file__).resolve().parent.parent / "include" / "wfhip.h").read_text()
    lib = _hip.lib()
    for name in ("wf_timing_track_anchored", "wf_carrier_track_anchored"):
        assert name in _hip.SIGNATURES and hasattr(lib, name) and f"int {name}(" in header, name


def test_anchored_entry_points_refuse_bad_arguments_without_a_gpu():
    """WF_ERR_VALUE before anything is launched (a fake context: no device exists here)."""
    import ctypes

    from waveforms_amd import _hip

    lib = _hip.lib()
    fake = ctypes.create_string_buffer(1 << 12)
    buf = ctypes.create_string_buffer(1 << 14)
    a = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    # (ctx, stat, H, nwin, span, period, anchor, max_drift, reject, out, choice, drift, marks)
    for fn, good in ((lib.wf_timing_track_anchored, (fake, a, 4, 10, 5, 8.0, 9, 2.0, 2.0, a + 1024, a + 2048, a + 3072, a + 4096)),
                     (lib.wf_carrier_track_anchored, (fake, a, 4, 10, 5, math.pi, 9, 0.3, 0.7, a + 1024, a + 2048, a + 3072, a + 4096))):
        P = good[5]
        for i, v in ((0, None), (1, None), (9, None), (10, None), (11, None), (12, None), (2, 0), (2, 257), (3, 0), (3, (1 << 31) + 1), (4, 4), (4, 0),
                     (5, 0.0), (5, math.inf), (6, 0), (6, 1), (6, 8), (6, 1025), (7, -0.1), (7, 0.5 * P), (7, math.nan), (8, 0.0), (8, 0.51 * P),
                     (8, math.nan), (1, a + 4), (9, a + 1028), (11, a + 3076)):
            args = good[:i] + (v,) + good[i + 1:]
            assert fn(*args, None) == _hip.WF_ERR_VALUE, (i, v)
