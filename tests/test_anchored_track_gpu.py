"""The anchored trackers on the device (``wf_timing_track_anchored``, ``wf_carrier_track_anchored``; include/wfhip.h) against the
host statements of tests/test_anchored_unwrap.py, and ``JointAcquisition(anchor=33)`` on the link.

Device against host.  The drift search's scores are sums of products of sincos values, which the device library and numpy round
differently, so the chosen candidate is the host's only where the host's best score LEADS: every test asserts on the host
first that the best score is 1e-9 (relative) above the second - six orders of magnitude above the rounding of a sum of 1023 unit
phasors - and that no |d_w| lies within 1e-9 P of the rejection threshold.  Then the candidate (through the drift) and the marks
must be the host's, the choices equal, and the trajectory within 1e-9 of the tracker's unit (the bound of
``test_cpm_timing_recover_*``).  Window counts: the deterministic 40, 826, and 1023 / 1024 / 1025 / 39 063 - one window short
of, at and past the tail's 1024 threads, and 38 windows per thread with a short last thread; K = 9 and 33 put segment edges (a
short last segment, a last gap) at every one of them.
"""
import math

import numpy as np
import pytest

from test_anchored_unwrap import H4, LINE, NWIN, P8, SPAN, _moved_table, carrier_table, model, timing_table
from waveforms_amd.sync import _stages as S
from waveforms_amd.sync import carrier as C
from waveforms_amd.sync import timing as T

pytestmark = pytest.mark.gpu


@pytest.fixture
def ctx():
    from waveforms_amd import _hip

    handle = _hip.new_ctx()
    yield handle
    _hip.free_ctx(handle)


def _against_host(kind, st, P, span, K, D, rho, ctx):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    if kind == "timing":
        want = T.timing_track_host(st, P, span, K, D, rho)
        got = dev.timing_track(_hip.to_device(st), P, span, ctx=ctx, anchor=K, max_drift=D, reject=rho)
    else:
        want = C.carrier_track_host(st, span, P, K, D, rho)
        got = dev.carrier_track(_hip.to_device(st), span, ctx=ctx, period=P, anchor=K, max_drift=D, reject=rho)
    traj, choice, drift, marks = (_hip.to_host(v) for v in got)
    nwin = st.shape[1]
    assert traj.shape == (nwin,) and choice.shape == (nwin,) and marks.shape == (nwin,) and drift.shape == (1,)
    assert np.array_equal(choice, want[1])
    if nwin > 1:                                            # the margins, on the host first
        psi = (T.timing_psi_host if kind == "timing" else C.carrier_psi_host)(st, P)[0]
        _z, _i, score = S.anchor_scores(psi, P, K, D)
        order = np.sort(score)
        lead = (order[-1] - order[-2]) / order[-1] if score.size > 1 else 1.0
        _ref, d, _f = S.anchor_reference(psi, P, K, D)
        edge = np.abs(np.abs(d) - rho).min() / P
        assert lead > 1e-9 and edge > 1e-9, (lead, edge)
    assert drift[0] == want[2]
    assert np.array_equal(marks, want[3])
    err = float(np.abs(traj - want[0]).max())
    print(f"{kind}, H {st.shape[0]}, {nwin} windows, K {K}: |device - host| <= {err:.3g}, drift {drift[0]:.6g}, {int(marks.sum())} rejected")
    assert err < 1e-9
    return err


def test_timing_track_anchored_on_the_deterministic_table(ctx):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    st = _moved_table()
    _against_host("timing", st, P8, SPAN, 9, 2.0, 2.0, ctx)
    tau, _c, drift, marks = (_hip.to_host(v) for v in dev.timing_track(_hip.to_device(st), P8, SPAN, ctx=ctx, anchor=9))
    assert np.all(np.abs(tau - S.centred_mean(LINE, SPAN)) < 0.5) and np.array_equal(np.nonzero(marks)[0], [20])
    # anchor=0 is the present entry point and its two outputs
    plain = dev.timing_track(_hip.to_device(st), P8, SPAN, ctx=ctx, anchor=0, max_drift=99.0, reject=-1.0)
    assert len(plain) == 2 and np.abs(_hip.to_host(plain[0])[23:] - S.centred_mean(LINE, SPAN)[23:] - P8).max() < 0.5


@pytest.mark.parametrize("P", (math.pi, 2.0 * math.pi / 16.0))
def test_carrier_track_anchored_on_the_deterministic_table(ctx, P):
    line = P * (0.125 - 0.1 * np.arange(NWIN))
    target = line.copy()
    target[20] += 0.4375 * P
    _against_host("carrier", carrier_table(target, H4, P), P, SPAN, 9, 0.25 * P, 0.25 * P, ctx)


@pytest.mark.parametrize("H", [3, 4, 64])
@pytest.mark.parametrize("nwin", [826, 1023, 1024, 1025, 39063])
def test_timing_track_anchored_against_the_host(ctx, nwin, H):
    """The model's sequences (8 % outliers) as tables of H hypotheses; K = 33 up to 1025 windows and 9 at 39 063 (4 341 segments)."""
    psi, _truth = model(nwin + H, nwin, -0.8 if H != 4 else 0.37, 0.08)
    K = 9 if nwin > 2000 else 33
    _against_host("timing", timing_table(psi, H, P8), P8, SPAN, K, 2.0, 2.0, ctx)


@pytest.mark.parametrize("H", [3, 4, 64])
@pytest.mark.parametrize("nwin", [826, 1023, 1024, 1025, 39063])
def test_carrier_track_anchored_against_the_host(ctx, nwin, H):
    P = math.pi if H != 4 else 2.0 * math.pi / 16.0
    psi, _truth = model(nwin + H, nwin, 0.37 if H != 4 else -0.8, 0.08, P)
    K = 33 if nwin > 2000 else 9
    _against_host("carrier", carrier_table(psi, H, P), P, SPAN, K, 0.25 * P, 0.25 * P, ctx)


@pytest.mark.parametrize("nwin", [1, 2, 8, 9, 10, 19])
def test_anchored_trackers_at_the_edges_of_the_anchor(ctx, nwin):
    """K = 9: one window, two, K - 1, K, K + 1 and 2K + 1; a window without an estimate (a NaN statistic) at either end."""
    psi = S._wrap(0.3 * P8 + 0.9 * np.arange(nwin), P8)
    st = timing_table(psi, 8, P8)
    _against_host("timing", st, P8, 3, 9, 2.0, 2.0, ctx)
    _against_host("carrier", carrier_table(psi * (math.pi / P8), 8, math.pi), math.pi, 3, 9, 0.25 * math.pi, 0.25 * math.pi, ctx)
    if nwin > 2:
        for w in (0, nwin - 1):
            bad = carrier_table(psi * (math.pi / P8), 1, math.pi)
            bad[0, w] = np.nan                              # ψ_w = atan2(NaN, NaN): no estimate
            _against_host("carrier", bad, math.pi, 3, 9, 0.25 * math.pi, 0.25 * math.pi, ctx)


def test_the_largest_anchor_and_every_candidate(ctx):
    """K = 1023 with D just under P / 2: 4 093 candidates over 16 workgroups of the drift search per segment."""
    psi, _truth = model(11, 2500, 0.37, 0.02)
    _against_host("timing", timing_table(psi, 4, P8), P8, SPAN, 1023, 3.99, 2.0, ctx)


# ------------------------------------------------------------------------------------------------ the link
NCW, LEAD, SPS, EBN0_DB, BLOCK = 100, 37, 8, 6.5, 0          # 100 codewords of the demo code: an 826-window burst
PER_WINDOW = SPS * C.DEFAULT_WINDOW
CARRIER = (math.radians(40.0), 0.025 / PER_WINDOW)          # tests/test_joint_link.py's impairment
TIMING = (6.0, 0.8 / PER_WINDOW)


def _excursion(tau):
    """The trajectory against the impairment, in samples, modulo the lattice: τ follows -(tau0 + eps n) / (1 + eps) at the
    window centres' samples n plus the statistic's own offset (``timing.BIAS_SAMPLES``); what is left, less the whole number of
    symbols it starts with (window 2: inside the clipped mean's lag).  (The rows start a few samples into the burst: eps times
    that is below 0.02 samples and is left out.)"""
    W = C.DEFAULT_WINDOW
    n = (np.arange(tau.size) * W + 0.5 * (W - 1)) * SPS
    e = tau + (TIMING[0] + TIMING[1] * n) / (1.0 + TIMING[1]) - T.BIAS_SAMPLES["PT"]
    return e - SPS * np.round(e[2] / SPS)


def test_anchored_acquisition_holds_the_burst_the_plain_one_loses():
    """One 826-window burst of the framed demo code at 6.5 dB under the link test's impairment (block 0 of seed 1, the first of
    the two bursts HISTORY.md followed): the plain acquisition leaves the impairment by at least one whole symbol, the anchored
    one stays within half a symbol of it over the whole burst and loses fewer codewords."""
    from waveforms_amd.encoding import framing as FR
    from waveforms_amd.encoding import ldpc
    from waveforms_amd.encoding.coded import CodedSOQPSKLink
    from waveforms_amd.sync import joint as J

    code = ldpc.demo_code()
    fr = FR.Framing(code)
    lost, exc = {}, {}
    for K in (0, 33):
        lk = CodedSOQPSKLink(code, NCW, framing=fr, lead_bits=LEAD, carrier=CARRIER, timing=TIMING, acquisition=J.JointAcquisition(SPS, anchor=K))
        lk.run_block(EBN0_DB, seed=1, stream_id=BLOCK)
        lost[K] = lk.result()[1]
        res = lk.acquisition_result()
        exc[K] = _excursion(res[0])
        assert len(res) == (8 if K else 4)
        if K:
            tdrift, trej, cdrift, crej = res[4:]
            print(f"anchored: timing drift {tdrift:+.4f} samples per window, {trej} windows rejected; carrier drift {cdrift / (2 * math.pi):+.5f} turns, {crej} rejected")
            assert abs(tdrift + 0.8) <= SPS / (4 * 33) + 0.05 and 0 <= trej < res[0].size // 2
    print(f"codewords lost of {NCW}: plain {lost[0]}, anchored {lost[33]}; largest excursion / symbol: plain {np.abs(exc[0]).max() / SPS:.2f}, "
          f"anchored {np.abs(exc[33]).max() / SPS:.2f}")
    assert np.abs(exc[0]).max() >= SPS
    assert np.abs(exc[33]).max() < 0.5 * SPS
    assert lost[33] < lost[0]


def test_anchored_acquisition_decides_as_the_plain_one_noiseless(oracle, ctx):
    """3 999 noiseless rows under tests/test_joint.py's first impairment: ``anchor=33`` (16 windows, one short segment) gives the
    plain acquisition's decisions outside one window at each end - at the plain one's rows or one row beside them, if the two
    trajectories start a whole symbol apart (the lattice)."""
    from test_joint import IMPAIRMENTS, W, _differ, _impair
    from test_timing import _chain
    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.sync import joint as J

    sig, _noise, taps, first, ncols = _chain(oracle, 4000)
    d_bad, d_taps = _hip.to_device(_impair(sig, IMPAIRMENTS[0])), _hip.to_device(taps)
    bits = {}
    for K in (0, 33):
        acq = J.JointAcquisition(SPS, anchor=K)
        rows = acq.recover(d_bad, d_taps, first, ncols, True, ctx=ctx)[0]
        bits[K] = _hip.to_host(dev.viterbi_soft_branch(rows, True, ctx=ctx)[1])
        assert (acq.timing_found is None) == (K == 0) and acq.launches == (76 if K == 0 else 76 + 2 + 2 * acq.refine)      # (a launch more per track)
    assert _differ(bits[33], bits[0], W, (0, 1, -1)) == 0
