"""Symbol timing recovery (waveforms_amd/sync/timing.py; include/wfhip.h: wf_timing_offset_c128, wf_mf_bank_resample_c128,
wf_timing_track, wf_timing_refine).

CPU: the host statements at their edges and ``recover_timing_host`` on the reference PT chain at the documented drift limit.
GPU: every device stage against its host statement within bounds that follow from the arithmetic (stated at each test), and
the whole recovery end to end.
"""
import ctypes
import math

import numpy as np
import pytest

from waveforms_amd.sync import carrier as C
from waveforms_amd.sync import timing as T

SPS = 8
U = 2.0 ** -53
NAMES = ("wf_timing_offset_c128", "wf_mf_bank_resample_c128", "wf_timing_track", "wf_timing_refine")


def _chain(oracle, n, detector="PT", ebn0=None, seed=3):
    """The reference chain up to the channel: (rotated signal, noise, taps complex128[3, ntaps], first, ncols) of n PN bits."""
    from waveforms_amd.filters.matched import pam_matched_filter_taps, pt_matched_filter_taps

    bits, _ = oracle.glfsr_bits(0x420000, 0x7FFFFF, n)
    g = oracle.freq_pulse_soqpsk_tg(SPS)
    symbols, _, _ = oracle.fsm_encode("SOQPSKTrellis4x2DiffEncoded", bits)
    _t, sig = oracle.cpm_modulate(symbols, 0.25, g, SPS)
    sig = sig * np.exp(-1j * np.pi / 4)
    noise = np.zeros(sig.size, dtype=np.complex128) if ebn0 is None else oracle.philox_awgn(oracle.sigma_for_ebn0(ebn0, SPS), 5, seed, 0, sig.size)
    taps = np.asarray((pt_matched_filter_taps if detector == "PT" else pam_matched_filter_taps)(g, 0.25, SPS), dtype=np.complex128)
    cols = oracle.decimate_columns(sig.size, SPS, 2, -1 if detector == "PT" else 0)
    return sig, noise, np.ascontiguousarray(taps), int(cols[0]), int(cols.size)


def _differ_up_to_two_rows(bits, genie, guard):
    """Decisions that differ from the genie's outside ``guard`` rows at each end, at the best of the shifts 0, +2, -2 rows."""
    want = genie[guard:genie.size - guard]
    return min(int(np.count_nonzero(bits[guard + sh:bits.size - guard + sh] != want)) for sh in (0, 2, -2))


# ------------------------------------------------------------------------------------------------ CPU
def test_timing_entry_points_exported_bound_and_declared():
    from pathlib import Path

    from waveforms_amd import _hip, device

    header = (Path(__file__).resolve().parent.parent / "include" / "wfhip.h").read_text()
    lib = _hip.lib()
    for name in NAMES:
        assert name in _hip.SIGNATURES and hasattr(lib, name) and f"int {name}(" in header, name
    for name in ("timing_offset", "mf_bank_resample", "timing_track", "timing_refine"):
        assert callable(getattr(device, name))
    for name in ("lagrange_host", "timing_offset_host", "mf_bank_resample_host", "timing_track_host", "timing_refine_host", "recover_timing_host"):
        assert callable(getattr(T, name))
    rec = T.TimingRecovery(SPS)
    assert (rec.sps, rec.window, rec.span, rec.hypotheses, rec.refine, rec.delta) == (8, 256, 5, 8, 1, 2.0)
    assert set(T.BIAS_SAMPLES) == {"PT", "PAM"} and 0.0 < T.MAX_DRIFT_SAMPLES < SPS


def test_timing_argument_validation_without_a_gpu():
    """Bad arguments return WF_ERR_VALUE before anything is launched (a fake context: no device exists here)."""
    from waveforms_amd import _hip

    lib = _hip.lib()
    fake = ctypes.create_string_buffer(1 << 16)
    buf = ctypes.create_string_buffer(1 << 14)
    a = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    b, c, d = a + 4096, a + 8192, a + 12288
    V = _hip.WF_ERR_VALUE
    nan, inf = float("nan"), float("inf")
    # wf_timing_offset_c128(ctx, in, n, tau0, eps, first_index, out, stream): out of place only
    for args in ((None, a, 10, 0.0, 0.0, 0, b), (fake, None, 10, 0.0, 0.0, 0, b), (fake, a, 10, 0.0, 0.0, 0, None), (fake, a, 0, 0.0, 0.0, 0, b),
                 (fake, a, 10, nan, 0.0, 0, b), (fake, a, 10, 0.0, inf, 0, b), (fake, a, 10, 0.0, 0.0, -1, b), (fake, a, 10, 0.0, 0.0, 1 << 53, b),
                 (fake, a + 8, 10, 0.0, 0.0, 0, b), (fake, a, 10, 0.0, 0.0, 0, b + 8), (fake, a, 10, 0.0, 0.0, 0, a), (fake, a, 10, 0.0, 0.0, 0, a + 144),
                 (fake, a + 16, 10, 0.0, 0.0, 0, a)):
        assert lib.wf_timing_offset_c128(*args, None) == V, args
    # wf_mf_bank_resample_c128(ctx, r, nsamp, taps, nfilt, ntaps, first, step, ncols, W, tau, nwin, tau0, out, stream)
    good = (fake, a, 100, b, 3, 9, 0, 8, 10, 64, c, 1, 0.0, d)
    for i, v in ((0, None), (1, None), (3, None), (13, None), (2, 0), (4, 2), (4, 4), (5, 8), (5, 0), (5, 257), (6, (1 << 40) + 1), (7, 0), (7, 65), (8, 0),
                 (9, 96), (9, 32), (11, 0), (12, nan), (12, inf), (1, a + 8), (3, b + 8), (13, d + 8), (10, c + 4)):
        args = good[:i] + (v,) + good[i + 1:]
        assert lib.wf_mf_bank_resample_c128(*args, None) == V, args
    # wf_timing_track(ctx, stat_h, H, nwin, span, period, tau, choice, stream)
    good = (fake, a, 8, 4, 1, 16.0, b, c)
    for i, v in ((0, None), (1, None), (6, None), (7, None), (2, 2), (2, 65), (3, 0), (4, 0), (4, 2), (5, 0.0), (5, -16.0), (5, nan), (5, inf), (1, a + 4),
                 (6, b + 4)):
        args = good[:i] + (v,) + good[i + 1:]
        assert lib.wf_timing_track(*args, None) == V, args
    # wf_timing_refine(ctx, stat3, nwin, span, delta, more, stream)
    good = (fake, a, 4, 1, 2.0, b)
    for i, v in ((0, None), (1, None), (5, None), (2, 0), (3, 0), (3, 4), (4, 0.0), (4, -1.0), (4, nan), (1, a + 4), (5, b + 4)):
        args = good[:i] + (v,) + good[i + 1:]
        assert lib.wf_timing_refine(*args, None) == V, args
    # ... and the Python layer's own
    for kw in ({"window": 96}, {"span": 4}, {"hypotheses": 2}, {"hypotheses": 65}, {"refine": -1}, {"delta": 0.0}, {"delta": float("nan")}, {"sps": 0}):
        with pytest.raises(ValueError):
            T.TimingRecovery(**{"sps": SPS, **kw})
    with pytest.raises(ValueError):
        T.timing_track_host(np.zeros((2, 4, 2)), 16.0)
    with pytest.raises(ValueError):
        T.timing_track_host(np.zeros((8, 4, 2)), 16.0, 2)


def test_lagrange_weights_sum_to_one_and_reproduce_a_cubic():
    mu = np.concatenate((np.linspace(0.0, 1.0, 1001)[:-1], [2.0 ** -60, 1.0 - 2.0 ** -53]))
    c = T.lagrange_host(mu)
    assert c.shape == (4, mu.size)
    # each weight carries a few roundings and the four are at most 1.25 in absolute sum
    assert np.abs(c.sum(axis=0) - 1.0).max() <= 8 * U
    assert (T.lagrange_host(0.0) == [0.0, 1.0, 0.0, 0.0]).all()
    rng = np.random.default_rng(1)
    for coef in rng.standard_normal((20, 4)) * [1.0, 3.0, 0.5, 0.25]:
        p = np.polynomial.Polynomial(coef)
        terms = c * p(np.array([-1.0, 0.0, 1.0, 2.0]))[:, None]
        got = terms[0] + terms[1] + terms[2] + terms[3]
        assert (np.abs(got - p(mu)) <= 16 * (2.0 * U) * np.abs(terms).max(axis=0)).all(), coef


def test_host_statements_at_their_edges():
    rng = np.random.default_rng(2)
    x = rng.standard_normal(257) + 1j * rng.standard_normal(257)
    assert (T.timing_offset_host(x, 0.0, 0.0) == x).all()
    # a whole number of samples is a shift, zeros coming in at the end
    assert (T.timing_offset_host(x, 3.0, 0.0)[:-3] == x[3:]).all() and not T.timing_offset_host(x, 3.0, 0.0)[-3:].any()
    # a trajectory that climbs 10 samples per window is read as -6 per window at period 16: modulo two symbols, the nearest
    H, period = 8, 16.0
    s = T.hypothesis_instants(period, H)
    assert (s == -8.0 + 2.0 * np.arange(8)).all()
    stat = np.zeros((H, 6, 2))
    for w in range(6):
        stat[:, w, 0] = C._wrap(s - 10.0 * w, period) ** 2 - 100.0
    tau, choice = T.timing_track_host(stat, period, 1)
    assert (np.diff(tau) == -6.0).all() and tau[0] == 0.0 and choice.tolist() == [4, 1, 6, 3, 0, 5]
    sm, _ = T.timing_track_host(stat, period, 3)
    np.testing.assert_allclose(sm, [(tau[0] + tau[1]) / 2] + [tau[j - 1:j + 2].sum() / 3 for j in range(1, 5)] + [(tau[4] + tau[5]) / 2], atol=1e-12)
    # a minimum between two hypotheses: the vertex of a true parabola is exact
    stat[:, :, 0] = ((s - 0.5) ** 2)[:, None]
    assert np.abs(T.timing_track_host(stat, period, 1)[0] - 0.5).max() < 1e-12
    # ties between hypotheses go to the smallest h; three equal points are not convex: vertex 0, the hypothesis's own instant
    tie = np.zeros((5, 2, 2))
    tie[:, :, 0] = -1.0
    tau, choice = T.timing_track_host(tie, 20.0, 1)
    assert not choice.any() and (tau == -10.0).all()
    # a non-convex triple gives vertex 0, a convex one is clamped
    assert T.vertex_host(1.0, 2.0, 1.0, 0.5) == 0.0 and T.vertex_host(3.0, 2.0, 1.0, 0.5) == 0.0 and T.vertex_host(np.nan, 2.0, 1.0, 0.5) == 0.0
    assert T.vertex_host(2.0, 0.0, 1.0, 0.5) == 1.0 / 6.0 and T.vertex_host(100.0, 0.0, -50.0, 0.5) == 0.5 and T.vertex_host(-50.0, 0.0, 100.0, 1.0) == -1.0
    st3 = np.zeros((3, 4, 2))
    st3[:, :, 0] = [[3.0, 1.0, 5.0, 1.0], [1.0, 2.0, 1.0, 1.0], [2.0, 1.0, -1.0, 1.0]]
    more = T.timing_refine_host(st3, 2.0, 1)
    assert more[0] == 2.0 * (0.5 / 3.0) and more[1] == 0.0 and more[2] == 2.0 and more[3] == 0.0
    assert T.timing_refine_host(st3, 2.0, 3)[0] == (more[0] + more[1]) / 2.0


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_trajectory_over_many_wraps_keeps_the_period_of_the_received_samples(sign):
    """3 000 windows at the documented drift limit: 4 800 samples, 300 wraps.  The statistic's aliases lie 16 / (1 + eps) RECEIVED
    samples apart (the drifting signal's symbols are 8 / (1 + eps) apart there) and ``timing_track_host`` unwraps modulo 16, so
    its trajectory leaves the instants that keep row k on symbol k by eps² n / (1 + eps): 3.7 samples at the end, beyond the
    refinement's ±2.  ``rescale_host`` takes that out.  Synthetic statistics: exact parabolas about the true instants, so the
    vertex is exact wherever a minimum and its neighbours lie on one branch; 0.05 covers the windows where they do not."""
    H, period, sps, W, nwin = 8, 16.0, SPS, C.DEFAULT_WINDOW, 3000
    eps = sign * T.MAX_DRIFT_SAMPLES / (sps * W)
    alias = period / (1.0 + eps)
    centre = 1.0 + sps * (W * np.arange(nwin) + 0.5 * (W - 1))
    true = -(6.0 + eps * centre) / (1.0 + eps) + T.BIAS_SAMPLES["PT"]
    s = T.hypothesis_instants(period, H)
    stat = np.zeros((H, nwin, 2))
    stat[:, :, 0] = C._wrap(s[:, None] - true[None, :], alias) ** 2 - 8000.0
    tau, _choice = T.timing_track_host(stat, period, 5)
    off = tau - true
    fixed = T.rescale_host(tau, sps * W) - true
    k = round(float(fixed[2]) / alias)                     # the alias the first windows settled on: a whole number of periods
    print(f"drift {sign * T.MAX_DRIFT_SAMPLES:+.1f}: unwrapped modulo 16 the trajectory leaves by {np.abs(off[2:-2] - off[2]).max():.3f} samples, rescaled by {np.abs(fixed[2:-2] - k * alias).max():.4f}")
    assert np.abs(off[2:-2] - off[2]).max() > 3.0
    assert np.abs(fixed[2:-2] - k * alias).max() < 0.05
    assert (T.rescale_host(np.array([1.5]), 2048.0) == [1.5]).all() and (T.rescale_host(np.full(9, -3.25), 2048.0) == -3.25).all()


def test_resample_host_with_no_trajectory_is_the_decimated_bank(oracle):
    sig, _noise, taps, first, ncols = _chain(oracle, 400)
    rows, mag = T.mf_bank_resample_host(sig, taps, first, SPS, ncols)
    want = oracle.pt_bank(sig, oracle.freq_pulse_soqpsk_tg(SPS), 0.25, SPS)[:, first::SPS][:, :ncols].T
    assert np.array_equal(rows, want) and (mag >= np.abs(rows) * (1 - 1e-12)).all()
    assert not T.mf_bank_resample_host(sig, taps, first, SPS, 5, 64, np.array([np.nan]))[0].any()


@pytest.fixture(scope="module")
def pt_burst(oracle):
    """3 999 noiseless PT rows' worth of samples and the genie's decisions."""
    sig, _noise, taps, first, ncols = _chain(oracle, 4000)
    genie = C.map_branch_host(T.mf_bank_resample_host(sig, taps, first, SPS, ncols)[0])[1]
    return sig, taps, first, ncols, genie


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("tau0", [-5.3, 2.7, 6.0])
def test_recover_timing_host_at_the_documented_drift_limit(pt_burst, tau0, sign):
    """Defaults (H = 8, W = 256, span 5, one refinement at ±2): the decisions after recovery are the unimpaired burst's, up to a
    shift of two rows (the instant is recovered modulo two symbols), outside a guard of one window at each end."""
    sig, taps, first, ncols, genie = pt_burst
    eps = sign * T.MAX_DRIFT_SAMPLES / (SPS * C.DEFAULT_WINDOW)
    bad = T.timing_offset_host(sig, tau0, eps)
    rows, tau, choice = T.recover_timing_host(bad, taps, first, ncols, SPS)
    assert tau.shape == choice.shape == (-(-ncols // C.DEFAULT_WINDOW),)
    assert _differ_up_to_two_rows(C.map_branch_host(rows)[1], genie, C.DEFAULT_WINDOW) == 0
    # without the recovery the burst is lost: otherwise the line above shows nothing
    lost = _differ_up_to_two_rows(C.map_branch_host(T.mf_bank_resample_host(bad, taps, first, SPS, ncols)[0])[1], genie, C.DEFAULT_WINDOW)
    print(f"tau0 {tau0}, drift {sign * T.MAX_DRIFT_SAMPLES:+.1f} per window: {lost} decisions lost without the recovery")
    assert lost > 300
    # the trajectory is the impairment's, seen from the statistic's minimum and modulo two symbols: -(tau0 + eps n) + bias at
    # the window centres.  A window's own estimate scatters by 0.02 to 0.03 samples (BIAS_SAMPLES' measurement) and by 0.05 under
    # this drift: 0.15 is three times that.  The clipped mean lags by up to one window's drift at the burst's two ends, and the
    # refinement's own mean spreads what it takes back over the two windows next to them: those four are held to the drift only.
    centre = first + SPS * (C.DEFAULT_WINDOW * np.arange(tau.size) + 0.5 * (C.DEFAULT_WINDOW - 1))
    resid = C._wrap(tau + tau0 + eps * centre - T.BIAS_SAMPLES["PT"], 2.0 * SPS)
    print(f"   residual against the impairment: windows 4 .. -5 {np.abs(resid[4:-4]).max():.3f} samples, all {np.abs(resid).max():.3f}")
    assert np.abs(resid[4:-4]).max() < 0.15 and np.abs(resid).max() < T.MAX_DRIFT_SAMPLES


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture
def ctx():
    from waveforms_amd import _hip

    handle = _hip.new_ctx()
    yield handle
    _hip.free_ctx(handle)


@pytest.mark.gpu
def test_timing_offset_against_the_host_statement():
    """n = 4099 (17 workgroups, the last one partial).  |device - host| <= 8 * 2^-53 * Σ |c_i| |x|: four products and three sums on
    either side, each within 2^-53 of its exact value relative to the sum of absolute terms; the weights themselves are the
    same roundings on both sides."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    rng = np.random.default_rng(11)
    n = 4099
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    d_x = _hip.to_device(x)
    for tau0, eps in ((0.0, 0.0), (0.3, 0.0), (-2.75, 1e-4), (5.0, -1e-4)):
        for first_index in (0, 10 ** 6):
            want = T.timing_offset_host(x, tau0, eps, first_index)
            got = _hip.to_host(dev.timing_offset(d_x, tau0, eps, first_index), True)
            ok, fl, mu = T._split(tau0 + eps * (np.arange(n) + first_index).astype(np.float64))
            bound = 8.0 * U * T._interpolated(np.abs(x), np.arange(n) + fl, ok, np.abs(T.lagrange_host(mu)))
            err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag))
            print(f"tau0 {tau0}, eps {eps}, first {first_index}: max error / bound = {(err[bound > 0] / bound[bound > 0]).max():.3f}")
            assert (err <= bound).all(), (tau0, eps, err.max())
            if (tau0, eps) == (0.0, 0.0):
                assert (got == x).all()
    # out of place only: the same buffer, and an overlapping view of it, are refused before anything is launched
    with pytest.raises(ValueError, match="out of place"):
        dev.timing_offset(d_x, 0.3, 0.0, out=d_x)
    big = _hip.to_device(np.concatenate((x, x)))
    with pytest.raises(ValueError, match="out of place"):
        dev.timing_offset(big[:n], 0.3, 0.0, out=big[8:n + 8])
    with pytest.raises(ValueError):
        dev.timing_offset(d_x, float("nan"), 0.0)
    assert (_hip.to_host(d_x, True) == x).all()


def _trajectories(ncols, window, nsamp, first):
    """name -> (first, window, tau or None, tau0): what the resampling bank must serve."""
    nwin = -(-ncols // window)
    w = np.arange(nwin, dtype=np.float64)
    nan = 3.0 + 0.25 * w
    nan[nwin // 2] = np.nan
    return {
        "none": (first, 64, None, 0.0),
        "constant": (first, 64, None, -3.625),
        "one window": (first, 8192, np.array([2.3]), 0.5),
        "ramp": (first, window, -1.7 + 0.9 * w, 0.125),                          # crosses an integer in every tile, and inside windows
        "sawtooth": (first, window, 20.0 * (-1.0) ** w + 0.3, 0.0),             # ±20 samples between neighbouring windows
        "jumps": (first, window, 150.0 * (-1.0) ** w - 40.25, 0.0),             # wider than any tile's staged span: the path through global memory
        "before 0": (-5 * SPS - 3, window, 0.4 * w, 0.75),                       # the first rows lie before sample 0
        "past the end": (nsamp - (ncols // 2) * SPS, window, 0.4 * w, 0.75),     # the last rows lie behind the last sample
        "far away": (first, window, np.full(nwin, 1e7), 0.0),                    # every row outside the burst
        "nan": (first, window, nan, 0.0),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("ncols", [1, 63, 257, 1000])
@pytest.mark.parametrize("detector", ["PT", "PAM"])
def test_mf_bank_resample_against_the_host_statement(oracle, ctx, detector, ncols):
    """PT (9 taps) and PAM (73 taps) at sps 8 on noisy samples.  Per component |device - host| <= (ntaps + 12) * 2^-53 * the host
    statement's absolute-value sum: the running-error bound of a sum of ntaps + 4 terms, with room for the weights' own roundings.
    The rows in front of and behind the requested ones keep their sentinel."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    sig, noise, taps, first, have = _chain(oracle, 1003, detector, 6.0)
    assert have >= 1000 and taps.shape == (3, 9 if detector == "PT" else 73)
    r = sig + noise
    d_r, d_taps = _hip.to_device(r), _hip.to_device(taps)
    window, guard, sentinel = 64, 4, -7.5
    plain = _hip.to_host(dev.mf_bank(d_r, d_taps, first, SPS, ncols), True)
    for name, (f0, W, tau, tau0) in _trajectories(ncols, window, r.size, first).items():
        want, mag = T.mf_bank_resample_host(r, taps, f0, SPS, ncols, W, tau, tau0)
        buf = _hip.to_device(np.full((ncols + 2 * guard, 3, 2), sentinel))
        out = dev.mf_bank_resample(d_r, d_taps, f0, SPS, ncols, W, None if tau is None else _hip.to_device(tau), tau0, out=buf[guard:guard + ncols], ctx=ctx)
        assert out.data_ptr() == buf[guard:].data_ptr()
        full = _hip.to_host(buf)
        assert (full[:guard] == sentinel).all() and (full[guard + ncols:] == sentinel).all(), name
        got = _hip.to_host(out, True)
        bound = (taps.shape[1] + 12) * U * mag
        err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag))
        live = bound > 0
        print(f"{detector} {ncols} {name}: max error / bound = {(err[live] / bound[live]).max() if live.any() else 0.0:.3f}, {int((~want.any(axis=1)).sum())} zero rows")
        assert (err <= bound).all(), (name, err.max())
        if name == "none":
            assert (np.maximum(np.abs(got.real - plain.real), np.abs(got.imag - plain.imag)) <= bound).all()
        if name == "nan":
            dead = np.isnan(T.instants_host(ncols, W, tau, tau0))
            assert dead.any() and not got[dead].any() and (ncols < 3 * window or got[~dead].any())
        if name == "far away":
            assert not got.any()
        if name in ("before 0", "past the end") and ncols >= 63:
            assert want.any() and not want[0 if name == "before 0" else -1].any()
    # a fresh output buffer when none is given
    got = _hip.to_host(dev.mf_bank_resample(d_r, d_taps, first, SPS, ncols, tau0=0.5, ctx=ctx), True)
    want, mag = T.mf_bank_resample_host(r, taps, first, SPS, ncols, tau0=0.5)
    assert got.shape == (ncols, 3) and (np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag)) <= (taps.shape[1] + 12) * U * mag).all()


@pytest.mark.gpu
@pytest.mark.parametrize("step,ntaps", [(1, 1), (3, 129), (10, 91), (64, 9), (7, 255)])
def test_mf_bank_resample_other_steps_and_bank_lengths(ctx, step, ntaps):
    """Odd steps (no pad slots), the longest banks and the widest step, where a tile is 32 rows: the same bound."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    rng = np.random.default_rng(100 * step + ntaps)
    ncols, window = 700, 64
    r = rng.standard_normal(ncols * step + 50) + 1j * rng.standard_normal(ncols * step + 50)
    taps = rng.standard_normal((3, ntaps)) + 1j * rng.standard_normal((3, ntaps))
    tau = np.cumsum(rng.uniform(-3.0, 3.0, -(-ncols // window)))
    want, mag = T.mf_bank_resample_host(r, taps, 2, step, ncols, window, tau, 0.3)
    got = _hip.to_host(dev.mf_bank_resample(_hip.to_device(r), _hip.to_device(taps), 2, step, ncols, window, _hip.to_device(tau), 0.3, ctx=ctx), True)
    err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag))
    assert (err <= (ntaps + 12) * U * mag).all(), err.max()


@pytest.mark.gpu
def test_mf_bank_resample_more_tiles_than_workgroups(ctx):
    """4096 workgroups of 256 rows are launched at most: from 1 048 577 rows on a workgroup walks more than one tile, restaging
    its window and taking the tile's span again.  PT-length taps, a drifting trajectory with a jump near the end."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    rng = np.random.default_rng(77)
    ncols, window = 4096 * 256 + 4096 + 300, 256
    nwin = -(-ncols // window)
    r = rng.standard_normal(ncols * SPS + 900) + 1j * rng.standard_normal(ncols * SPS + 900)
    taps = rng.standard_normal((3, 9)) + 1j * rng.standard_normal((3, 9))
    tau = -0.8 * np.arange(nwin, dtype=np.float64)
    tau[-3:] += 300.0
    first = int(0.8 * nwin) + 5
    want, mag = T.mf_bank_resample_host(r, taps, first, SPS, ncols, window, tau, 0.3)
    got = _hip.to_host(dev.mf_bank_resample(_hip.to_device(r), _hip.to_device(taps), first, SPS, ncols, window, _hip.to_device(tau), 0.3, ctx=ctx), True)
    err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag))
    worst = int(np.argmax(err - (9 + 12) * U * mag))
    assert (err <= (9 + 12) * U * mag).all(), (worst, err[worst // 3], want[worst // 3], got[worst // 3])


def _track_bound(psi_like, nwin, span, period=None):
    """(nwin + span + 8) * 2^-53 * (|ψ_0| + Σ |steps|): the recursive-summation bound of the running sum and the mean."""
    steps = np.diff(psi_like)
    if period is not None:
        steps = C._wrap(steps, period)
    return (nwin + span + 8) * U * (abs(psi_like[0]) + np.abs(steps).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("nwin", [1, 2, 1500])
@pytest.mark.parametrize("H", [3, 8, 64])
def test_timing_track_on_synthetic_tables(ctx, H, nwin):
    """Random tables with exact ties between hypotheses, windows whose triple is flat and a window whose vertex sits at
    the clamp: choice bitwise, tau within the recursive-summation bound.  1500 windows: the tracker's 1024 threads own up to two."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    rng = np.random.default_rng(1000 * H + nwin)
    period = 16.0
    stat = rng.standard_normal((H, nwin, 2)) * 50.0 - 2000.0
    stat[:, ::7, 0] = np.round(stat[:, ::7, 0] / 40.0) * 40.0            # exact ties, also between the two smallest
    stat[:, 3::11, 0] = -2000.0                                          # all equal: den = 0, vertex 0, choice 0
    if nwin > 5:
        stat[:, 5, 0] = -1.0
        stat[1, 5, 0] = -1000.0                                          # a lone spike: a convex triple with a = c, vertex 0
        stat[0, 4, 0], stat[1, 4, 0], stat[2, 4, 0] = -3000.0, -3000.0 - 1e-9, 0.0      # a vertex next to the clamp: V = -0.5 to rounding
    d_stat = _hip.to_device(stat)
    for span in (1, 5):
        want_tau, want_choice = T.timing_track_host(stat, period, span)
        tau, choice = dev.timing_track(d_stat, period, span, ctx=ctx)
        assert np.array_equal(_hip.to_host(choice), want_choice)
        bound = _track_bound(T.timing_track_host(stat, period, 1)[0], nwin, span)
        err = np.abs(_hip.to_host(tau) - want_tau).max()
        print(f"H {H}, nwin {nwin}, span {span}: max |device - host| = {err:.3g}, bound {bound:.3g}")
        assert err <= bound
    assert (want_choice[3::11] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("nwin", [1, 2, 1500])
def test_timing_refine_on_synthetic_tables(ctx, nwin):
    """No running sum here: the device's values are the host's to the rounding of the span's mean."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    rng = np.random.default_rng(nwin)
    stat3 = rng.standard_normal((3, nwin, 2)) * 50.0 - 2000.0
    stat3[:, ::5, 0] = -2000.0                                           # flat: den = 0
    stat3[1, 1::5, 0] = -1000.0                                          # concave: den < 0
    d_stat3 = _hip.to_device(stat3)
    for span, delta in ((1, 2.0), (5, 2.0), (3, 0.75)):
        want = T.timing_refine_host(stat3, delta, span)
        got = _hip.to_host(dev.timing_refine(d_stat3, delta, span, ctx=ctx))
        one = T.timing_refine_host(stat3, delta, 1)
        assert not one[::5].any() and not one[1::5].any() and np.abs(one).max() <= delta
        assert np.abs(got - want).max() <= (span + 8) * U * delta, (span, np.abs(got - want).max())
        if span == 1:
            assert np.array_equal(got, want)


@pytest.fixture(scope="module")
def bursts(oracle):
    """About 2 100 PT rows' worth of samples, noiseless and at 8 dB, read at n + 6.0 + eps n with half the documented drift."""
    out = {}
    eps = 0.5 * T.MAX_DRIFT_SAMPLES / (SPS * C.DEFAULT_WINDOW)
    for ebn0 in (None, 8.0):
        sig, noise, taps, first, ncols = _chain(oracle, 2101, "PT", ebn0)
        genie = C.map_branch_host(T.mf_bank_resample_host(sig + noise, taps, first, SPS, ncols)[0])[1]
        bad = T.timing_offset_host(sig, 6.0, eps) + noise
        out[ebn0] = (bad, taps, first, ncols, genie, T.recover_timing_host(bad, taps, first, ncols, SPS))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("ebn0", [None, 8.0])
def test_recover_end_to_end(bursts, ctx, ebn0):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    bad, taps, first, ncols, genie, (host_rows, host_tau, host_choice) = bursts[ebn0]
    rec = T.TimingRecovery(SPS)
    rec.times = True
    rows, tau, choice = rec.recover(_hip.to_device(bad), _hip.to_device(taps), first, ncols, True, ctx=ctx)
    assert np.array_equal(_hip.to_host(choice), host_choice)
    np.testing.assert_allclose(_hip.to_host(tau), host_tau, rtol=0, atol=1e-9)      # (the stages' own tests hold the bounds)
    bits = _hip.to_host(dev.viterbi_soft_branch(rows, True, ctx=ctx)[1])
    assert np.array_equal(bits, C.map_branch_host(host_rows)[1])
    errs = _differ_up_to_two_rows(bits, genie, rec.window)
    lost = _differ_up_to_two_rows(C.map_branch_host(T.mf_bank_resample_host(bad, taps, first, SPS, ncols)[0])[1], genie, rec.window)
    print(f"Eb/N0 {ebn0}: {errs} decisions differ from the genie's outside the guard, {lost} without the recovery; stages {rec.stage_times()}")
    assert set(rec.stage_times()) == {"resample", "soft_branch", "stat", "track", "rescale", "add"}
    if ebn0 is None:
        assert errs == 0 and lost > 100
