"""Symbol timing recovery for the SOQPSK-TG receiver: feed-forward and decision-directed, over windows of detector rows, with
no sequential loop filter (include/wfhip.h states the device operations: ``wf_timing_offset_c128``,
``wf_mf_bank_resample_c128``, ``wf_timing_track``, ``wf_timing_refine``; the statistic is ``wf_carrier_stat``'s).  The reference
has no synchroniser; every definition here is this package's own.

The ``*_host`` functions are the HOST statements of the definitions, written straight from them in numpy: the device agrees
with them to rounding (the resampling bank sums in another order, the tracker scans in blocks).  ``TimingRecovery`` is the
device-resident composition, ``recover_timing_host`` the same on the host.

How it works.  Along a maximum-likelihood path the decided branches' metric terms add up to X_w, the first component of
``carrier_stat`` (waveforms_amd/sync/carrier.py), which is most negative when the matched filters are sampled where the eye is
widest.  As a function of the sampling instant X_w is smooth with a period of TWO symbols (a shift by one symbol swaps the
trellis's column parity) and has one minimum per period.  So: ``hypotheses`` passes over the noisy samples, pass h sampling the
bank at the reference's instants moved by s_h = -sps + h 2 sps / H (``mf_bank_resample``), per window the pass with the
smallest X and the guarded vertex of the parabola through it and its two neighbours; the per-window instants are unwrapped
modulo two symbols and smoothed over ``span`` windows; ``refine`` rounds then sample at τ - δ, τ, τ + δ and move τ to the
vertex of those three.  A vertex is taken only where the three points are strictly convex, and is clamped: a window without a
minimum to offer leaves the estimate where it was.  The last pass samples the bank along τ.

The period in received samples.  The rows are taken in the RECEIVED sample domain, where a signal read at n + tau0 + eps n has
its symbols sps / (1 + eps) samples apart: the statistic's aliases lie 2 sps / (1 + eps) apart, while ``timing_track`` unwraps
modulo exactly 2 sps (the receiver does not know eps).  Every wrap therefore leaves the unwrapped trajectory u short by
2 sps eps / (1 + eps) samples; u follows -(tau0 + eps n) where the instants that keep row k on symbol k follow
-(tau0 + eps n) / (1 + eps), and after n samples the two are eps² n / (1 + eps) apart: 12 samples on a 1e7-row burst at
eps = 3.9e-4, more than half a period.  The trajectory's own slope s (samples per received sample, which is -eps) says by how
much: ``rescale_host`` stretches the trajectory about its first window by 1 / (1 - s) before the refinement.

The estimate is modulo two symbols: the rows may come out two rows early or late, which a framed link's frame search absorbs
as it absorbs the carrier recovery's π.

Limits.  The instant must stay within the pull-in of one hypothesis across a window: the supported drift is
|eps| sps W <= ``MAX_DRIFT_SAMPLES`` samples per window.  The statistic's minimum is not the reference's hand-tuned offset
(``BIAS_SAMPLES``); the recovery goes to the minimum.  The drift is taken as ONE rate over the burst (``rescale_host`` below).
No carrier recovery at the same time here: the two-dimensional search is ``waveforms_amd.sync.joint.JointAcquisition``.
SOQPSK-TG only, and the interpolation is a pass of its own over the samples per hypothesis (not fused into the detector's row load).
"""
from __future__ import annotations

import math

import numpy as np

from . import _stages
from ._stages import centred_mean as _centred_mean
from .carrier import DEFAULT_SPAN, DEFAULT_WINDOW, _check_window, carrier_stat_host, interpolate_phase_host, map_branch_host

DEFAULT_HYPOTHESES = 8
DEFAULT_REFINE = 1
DEFAULT_DELTA = 2.0
_HUGE = 2.0 ** 62                         # an instant at or beyond it has no sample near it: a zero row

# Where the noiseless statistic's minimum sits relative to the reference's sample offset (encoding.coded.TIMING_OFFSET: -1 for
# PT, 0 for PAM), in samples at sps 8: the mean of recover_timing_host's trajectory on an unimpaired noiseless burst of 3 999
# rows of the reference chain (W 256, span 5, H 8, one refinement at ±2), windows 2 .. nwin - 3; its standard deviation over
# those windows is 0.017 (PT) and 0.031 (PAM).  The recovered rows are sampled there, not at the hand-tuned offset.
BIAS_SAMPLES = {"PT": -1.17, "PAM": -0.85}
# |eps| sps W: the drift of the instant across one window, in samples, that the recovery is documented for.  On a burst of
# 3 999 rows (16 windows, at most seven wraps) with tau0 in {-5.3, 2.7, 6.0} and either sign the noiseless host statement decides
# every bit as the genie (outside one window at each end, up to a shift of two rows) up to 7.0 samples per window and loses the
# burst at 8.0, half the period, where the unwrapping turns the other way (PT and PAM alike).  The limit does not depend on the
# burst's length as long as eps is one rate: rescale_host takes the eps² n term out (tests/test_timing.py follows 3 000 windows
# and 300 wraps at this limit on synthetic statistics; INTEGRATION.md has the device's 1e7-row bursts).  The documented limit
# stays far inside 7.0: the clipped mean at the burst's two ends lags a drift d by up to d samples in the first and last
# window, which the refinement (clamped to ±δ) must pull back.
MAX_DRIFT_SAMPLES = 1.6


def lagrange_host(mu) -> np.ndarray:
    """The cubic Lagrange weights of the nodes -1, 0, 1, 2 at the fraction ``mu`` -> float64[4, ...]: the products left to
    right, then the division (include/wfhip.h)."""
    mu = np.asarray(mu, dtype=np.float64)
    p1, m1, m2 = mu + 1.0, mu - 1.0, mu - 2.0
    return np.stack((-(mu * m1 * m2) / 6.0, (p1 * m1 * m2) / 2.0, -(p1 * mu * m2) / 2.0, (p1 * mu * m1) / 6.0))


def _split(t):
    """t -> (usable, floor as int64, fraction); an instant that is not finite or at or beyond 2^62 is not usable."""
    t = np.asarray(t, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.abs(t) < _HUGE
    fl = np.floor(np.where(ok, t, 0.0))
    return ok, fl.astype(np.int64), np.where(ok, t, 0.0) - fl


def _interpolated(values, index, ok, weights):
    """Σ_i weights[i] values[index + i - 1], i = 0 .. 3 in this order; an index outside ``values`` (or a row not ``ok``) gives 0."""
    n = values.shape[-1]
    acc = np.zeros(values.shape[:-1] + index.shape, dtype=values.dtype)
    for i in range(4):
        s = index + (i - 1)
        use = ok & (s >= 0) & (s < n)
        acc = acc + np.where(use, weights[i], 0.0) * values[..., np.clip(s, 0, n - 1)]
    return acc


def timing_offset_host(signal, tau0: float, eps: float, first_index: int = 0) -> np.ndarray:
    """``wf_timing_offset_c128``: out_n = Σ_i c_i(μ_n) in[n + b_n + i] with t_n = tau0 + eps (first_index + n), complex128."""
    x = np.asarray(signal, dtype=np.complex128).reshape(-1)
    n = np.arange(x.size, dtype=np.int64)
    pr = float(eps) * (n + int(first_index)).astype(np.float64)
    ok, fl, mu = _split(float(tau0) + pr)
    return _interpolated(x, n + fl, ok, lagrange_host(mu))


def _full_rate(r, taps):
    """v_f(n), 0 <= n < nsamp: np.convolve(r, taps[f], "same") for a burst at least as long as the filter."""
    c = (taps.shape[1] - 1) // 2
    return np.stack([np.convolve(r, tp)[c:c + r.size] for tp in taps])


def instants_host(ncols: int, window: int = 64, tau=None, tau0: float = 0.0) -> np.ndarray:
    """t_k = tau0 + τ_k of ``wf_mf_bank_resample_c128``, τ interpolated as ``wf_rows_derotate`` interpolates its phase."""
    tk = 0.0 if tau is None else interpolate_phase_host(ncols, window, tau)
    return float(tau0) + tk + np.zeros(int(ncols))


def mf_bank_resample_host(received, taps, first: int, step: int, ncols: int, window: int = 64, tau=None, tau0: float = 0.0):
    """``wf_mf_bank_resample_c128`` from its definition: the full-rate bank, then four of its values per row ->
    (rows complex128[ncols, 3], the same sum over absolute values float64[ncols, 3]: Σ_i |c_i| Σ_t |r| |taps|)."""
    r = np.asarray(received, dtype=np.complex128).reshape(-1)
    taps = np.asarray(taps, dtype=np.complex128)
    if taps.ndim != 2 or taps.shape[0] != 3 or taps.shape[1] % 2 == 0:
        raise ValueError("taps must be complex128[3, ntaps], ntaps odd")
    ok, fl, mu = _split(instants_host(ncols, window, tau, tau0))
    B = int(first) + np.arange(int(ncols), dtype=np.int64) * int(step) + fl
    c = lagrange_host(mu)
    rows = _interpolated(_full_rate(r, taps), B, ok, c)
    mag = _interpolated(_full_rate(np.abs(r), np.abs(taps)).real, B, ok, np.abs(c))
    return np.ascontiguousarray(rows.T), np.ascontiguousarray(mag.T)


def vertex_host(a, b, c, lim: float) -> np.ndarray:
    """The guarded vertex of the parabola through (-1, a), (0, b), (1, c): 0.5 (a - c) / den where den = (a - b) + (c - b) > 0,
    otherwise 0; clamped to ±lim."""
    a, b, c = (np.asarray(v, dtype=np.float64) for v in (a, b, c))
    den = (a - b) + (c - b)
    with np.errstate(invalid="ignore"):
        good = den > 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.where(good, (0.5 * (a - c)) / np.where(good, den, 1.0), 0.0)
    return np.where(v > lim, lim, np.where(v < -lim, -lim, v))


def hypothesis_instants(period: float, H: int) -> np.ndarray:
    """s_h = (h * (period / H)) - period / 2, h < H: where pass h of the coarse search samples."""
    dh = float(period) / float(H)
    return np.arange(int(H), dtype=np.float64) * dh - 0.5 * float(period)


def timing_psi_host(stat, period: float):
    """What ``wf_timing_track`` forms per window before it unwraps: float64[H, nwin, 2] -> (ψ f64[nwin] in [-period/2, period/2),
    choice u8[nwin])."""
    period = float(period)
    if not (math.isfinite(period) and period > 0.0):
        raise ValueError(f"period = {period} must be finite and positive")
    X = np.asarray(stat, dtype=np.float64)[:, :, 0]
    H, nwin = X.shape
    if not 3 <= H <= 64:
        raise ValueError(f"H = {H} outside 3 .. 64")
    choice = np.argmin(X, axis=0)                          # the first of equal minima
    w = np.arange(nwin)
    v = vertex_host(X[(choice - 1) % H, w], X[choice, w], X[(choice + 1) % H, w], 0.5)
    dh = period / float(H)
    return (choice.astype(np.float64) * dh - 0.5 * period) + dh * v, choice.astype(np.uint8)


def timing_track_host(stat, period: float, span: int = 1, anchor: int = 0, max_drift=None, reject=None):
    """``wf_timing_track``: float64[H, nwin, 2] -> (tau f64[nwin] in samples, choice u8[nwin]).  ``anchor`` = K > 0:
    ``wf_timing_track_anchored``, the anchored unwrapping of ``_stages.anchored_unwrap`` in place of the running one ->
    (tau, choice, the drift found in samples per window, the rejected windows u8[nwin]); ``max_drift`` in samples per window
    (None: 1.25 ``MAX_DRIFT_SAMPLES``), ``reject`` in samples (None: period / 4)."""
    psi, choice = timing_psi_host(stat, period)
    period = float(period)
    K, D, rho = _stages.anchor_args(anchor, max_drift, reject, period, MAX_DRIFT_SAMPLES)
    if K:
        kept, drift, marks = _stages.anchored_unwrap(psi, period, K, D, rho)
        return _centred_mean(kept, span), choice, drift, marks
    return _centred_mean(_stages.unwrap(psi, period), span), choice


def rescale_host(tau, samples_per_window: float) -> np.ndarray:
    """The unwrapped trajectory in the period of the RECEIVED samples (the module's docstring says why):
    τ'_w = τ_0 + (τ_w - τ_0) / (1 - s),  s = (τ_b - τ_a) / ((b - a) samples_per_window)
    with a = 2, b = nwin - 3 (inside the clipped mean's lag at the two ends) for nwin >= 8 and a = 0, b = nwin - 1 otherwise; one
    window: unchanged.  s is ONE rate for the burst: the impairment's model, a constant eps."""
    tau = np.asarray(tau, dtype=np.float64).reshape(-1)
    out = _stages.rescale(tau, tau.size, samples_per_window)
    return tau.copy() if out is tau else out


def timing_refine_host(stat3, delta: float, span: int = 1) -> np.ndarray:
    """``wf_timing_refine``: float64[3, nwin, 2] taken at τ - δ, τ, τ + δ -> the correction to τ, f64[nwin]."""
    X = np.asarray(stat3, dtype=np.float64)[:, :, 0]
    if X.shape[0] != 3:
        raise ValueError("stat3 must be float64[3, nwin, 2]")
    return _centred_mean(float(delta) * vertex_host(X[0], X[1], X[2], 1.0), span)


def recover_timing_host(received, taps, first: int, ncols: int, sps: int, window: int = DEFAULT_WINDOW, span: int = DEFAULT_SPAN,
                        hypotheses: int = DEFAULT_HYPOTHESES, refine: int = DEFAULT_REFINE, delta: float = DEFAULT_DELTA,
                        differential: bool = True):
    """``TimingRecovery.recover`` on the host -> (rows complex128[ncols, 3], tau f64[nwin], choice u8[nwin])."""
    period = 2.0 * float(sps)

    def stat_at(tau, tau0):
        rows = mf_bank_resample_host(received, taps, first, sps, ncols, window, tau, tau0)[0]
        return carrier_stat_host(rows, map_branch_host(rows, differential)[2], window)

    tau, choice = _stages.timing_recover_host(stat_at, period, float(sps) * float(window), span, hypotheses, refine, float(delta))
    return mf_bank_resample_host(received, taps, first, sps, ncols, window, tau)[0], tau, choice


class TimingRecovery(_stages.Synchroniser):
    """Symbol timing recovery of a burst of noisy samples at ``sps`` samples per symbol, everything on the device:

    1. ``hypotheses`` passes of ``mf_bank_resample`` at tau0 = s_h -> ``viterbi_soft_branch`` -> ``carrier_stat``,
    2. ``timing_track`` with period 2 sps: per window the best hypothesis and its guarded vertex, unwrapped and smoothed, and the
       trajectory stretched by 1 / (1 - its own slope) to the period of the received samples (``rescale_host``: four tensor
       operations on nwin values),
    3. ``refine`` rounds of three such passes along τ at -δ, 0, +δ and ``timing_refine``; τ += its output,
    4. ``mf_bank_resample`` along τ: the rows the detector gets.

    ``recover`` returns those rows, the trajectory (samples per window, modulo two symbols) and the coarse choices; nothing
    comes back to the host.  ``times=True`` keeps device events around every stage of the last call (``stage_times``).

    ``anchor`` = K > 0 (odd, 3 .. 1023): the tracks use the anchored unwrapping of include/wfhip.h in place of the running one -
    no cycle slips behind a bad window; ``max_drift`` and ``reject`` in samples (per window) (None: 1.25 times the documented drift limit and a
    quarter of the period).  The last ``recover``'s coarse track leaves the drift found and the rejected windows on the device in
    ``timing_found``."""

    def __init__(self, sps: int, window: int = DEFAULT_WINDOW, span: int = DEFAULT_SPAN, hypotheses: int = DEFAULT_HYPOTHESES,
                 refine: int = DEFAULT_REFINE, delta: float = DEFAULT_DELTA, anchor: int = 0, max_drift=None, reject=None) -> None:
        super().__init__()
        self._anchor_init("timing", anchor, max_drift, reject, 2.0 * float(sps), MAX_DRIFT_SAMPLES)
        self.window = _check_window(window)
        self.sps = _stages.check_range("sps", sps, 1, 64)
        self.span = _stages.check_span(span)
        self.hypotheses = _stages.check_range("hypotheses", hypotheses, 3, 64)
        self.refine = _stages.check_refine(refine)
        self.delta = _stages.check_delta(delta)

    def recover(self, received, taps, first: int, ncols: int, differential: bool = True, ctx=None):
        from .. import _hip
        from .. import device as dev

        W, ncols = self.window, int(ncols)
        nwin = -(-ncols // W)
        period = 2.0 * float(self.sps)
        work = _hip.empty((ncols, 3, 2), "float64")
        self._events = []
        self._mark("start")

        def stat_at(tau, tau0, out):
            dev.mf_bank_resample(received, taps, first, self.sps, ncols, W, tau, tau0, out=work, ctx=ctx)
            self._mark("resample")
            _llr, _bits, branch = dev.viterbi_soft_branch(work, differential, ctx=ctx)
            self._mark("soft_branch")
            dev.carrier_stat(work, branch, W, out=out, ctx=ctx)
            self._mark("stat")

        tau, choice = _stages.timing_recover(self, stat_at, period, nwin, ctx)
        dev.mf_bank_resample(received, taps, first, self.sps, ncols, W, tau, 0.0, out=work, ctx=ctx)
        self._mark("resample")
        return work, tau, choice
