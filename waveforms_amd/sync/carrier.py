"""Carrier phase and frequency recovery for the SOQPSK-TG receiver: feed-forward and decision-directed, over windows of
detector rows, with no sequential loop filter (include/wfhip.h states the device operations: ``wf_carrier_offset_c128``,
``wf_viterbi4_soft_branch``, ``wf_carrier_stat``, ``wf_carrier_track``, ``wf_rows_derotate``).  The reference has no
synchroniser; every definition here is this package's own.

The ``*_host`` functions are the HOST statements of the definitions, written straight from them in numpy: the device's
branches and statistics equal them bit for bit, the trajectory and the derotation to rounding (the device's ``atan2`` and
``sincos`` are not numpy's).  ``CarrierRecovery`` is the device-resident composition, ``recover_host`` the same on the host.

How it works.  Along a maximum-likelihood path the decided branch's term q_k = state_exp_term[start] z_k[idx(out)] has a
large negative real part (metrics are minimised); rotating the rows by θ rotates every q_k by θ, so the angle of -Σ q_k
over a window estimates θ - as long as the decisions are mostly right, which holds up to about 20 degrees.  Beyond that a
coarse search takes over: ``hypotheses`` passes over the whole burst, pass h on rows derotated by h π / H, and per window
the pass whose Σ Re q is most negative.  The trellis is symmetric under a rotation by π (not by π/2), so H hypotheses span
[0, π) and the estimate is modulo π; the frame search's polarity σ absorbs the rest.

Limits.  The phase must stay within the decision-directed pull-in across one window: the supported frequency offset is
|nu| sps W <= ``MAX_DRIFT_TURNS`` turns per window (nu in cycles per sample), measured on ``recover_host``
(tests/test_carrier.py).  No timing recovery here (both at once: ``waveforms_amd.sync.joint.JointAcquisition``); the hypothesis rotation is a pass of its own over the rows (not fused into
the detector's row load); the recovery passes carry no prior.  H hypotheses cost H detections: the price of needing no
sequential loop.  The CPM detectors (ARTM, PCM/FM) have the same scheme in ``waveforms_amd.sync.carrier_cpm``, which shares
``carrier_track_host`` (with its period) and ``interpolate_phase_host`` with this module.
"""
from __future__ import annotations

import math

import numpy as np

from . import _stages
from ._stages import _wrap, check_window as _check_window

DEFAULT_WINDOW = 256
DEFAULT_SPAN = 5
DEFAULT_HYPOTHESES = 8
DEFAULT_REFINE = 1
MAX_DRIFT_TURNS = 0.05                    # |nu| sps W: phase drift across one window, in turns (18 degrees); the noiseless host
                                          # statement decides every bit as the genie up to 0.08 and makes its first error at 0.12

# Branch b of column c in list order: start = b >> 1, end, index of the output symbol (0: -2, 1: 0, 2: +2)
_OUT_IDX = ((1, 2, 1, 0, 0, 1, 2, 1), (1, 0, 2, 1, 1, 2, 0, 1))
_STATE_EXP = (1j, -1.0, 1.0, -1j)


def _branches(differential: bool):
    cols = []
    for c in range(2):
        brs = []
        for b in range(8):
            s, lsb = b >> 1, b & 1
            e = (s & 1) + 2 * lsb if c == 0 else (s & 2) + lsb
            flip = ((s >> 1) if c == 0 else (s & 1)) if differential else 0
            brs.append((b, s, e, lsb ^ flip, _OUT_IDX[c][b]))
        cols.append(brs)
    return cols


def _rows3(rows) -> np.ndarray:
    z = np.asarray(rows)
    if z.dtype != np.complex128:
        z = np.ascontiguousarray(z, dtype=np.float64).reshape(-1, 3, 2).view(np.complex128)
    return np.ascontiguousarray(z).reshape(-1, 3)


def carrier_phase_host(n: int, theta0: float, nu: float, first_index: int = 0) -> np.ndarray:
    """φ_k of ``wf_carrier_offset_c128``, k < n: theta0 + 2π frac(nu (first_index + k)), each operation rounded once."""
    t = float(nu) * (np.arange(int(n), dtype=np.int64) + int(first_index)).astype(np.float64)
    fr = t - np.floor(t)
    return float(theta0) + (2.0 * math.pi) * fr


def carrier_offset_host(signal, theta0: float, nu: float, first_index: int = 0) -> np.ndarray:
    """``wf_carrier_offset_c128``: signal_k exp(j φ_k) with φ_k of ``carrier_phase_host``, complex128 in and out."""
    x = np.asarray(signal, dtype=np.complex128).reshape(-1)
    phi = carrier_phase_host(x.size, theta0, nu, first_index)
    return x * (np.cos(phi) + 1j * np.sin(phi))


def map_branch_host(rows, differential: bool = True):
    """``wf_viterbi4_soft_branch``, one section at a time -> (llr f64[n], bits u8[n], branch u8[n]).

    llr and bits are the max-log-MAP detector's (include/wfhip.h, wf_viterbi4_soft); branch[k] is the b of column k % 2 that
    minimises T_k(b) = (ã_k(start b) + inc_k(b)) + b̃_{k+1}(end b), ties to the smallest b."""
    z = _rows3(rows)
    brs = _branches(bool(differential))
    n = z.shape[0]
    inc = np.empty((n, 8))
    for c in range(2):
        for (b, s, _e, _i, idx) in brs[c]:
            inc[c::2, b] = (_STATE_EXP[s] * z[c::2, idx]).real
    inc = inc.tolist()
    inf = math.inf
    alpha = [None] * (n + 1)
    a = [0.0, 0.0, 0.0, 0.0]
    alpha[0] = a
    for k in range(n):
        ik, new = inc[k], [inf, inf, inf, inf]
        for (b, s, e, _i, _x) in brs[k & 1]:
            v = a[s] + ik[b]
            if v < new[e]:
                new[e] = v
        mn = min(new)
        a = [v - mn for v in new]
        alpha[k + 1] = a
    llr = np.empty(n)
    branch = np.empty(n, dtype=np.uint8)
    bt = [0.0, 0.0, 0.0, 0.0]
    for k in range(n - 1, -1, -1):
        ik, a, new = inc[k], alpha[k], [inf, inf, inf, inf]
        m = [inf, inf]
        best, tv = 0, inf
        for (b, s, e, i, _x) in brs[k & 1]:
            t = (a[s] + ik[b]) + bt[e]
            if t < m[i]:
                m[i] = t
            if t < tv:
                best, tv = b, t
            v = ik[b] + bt[e]
            if v < new[s]:
                new[s] = v
        llr[k] = m[1] - m[0]
        branch[k] = best
        mn = min(new)
        bt = [v - mn for v in new]
    return llr, (llr < 0).astype(np.uint8), branch


def branch_terms_host(rows, branch):
    """q_k = state_exp_term[start b_k] z_k[idx(out b_k)] as its signed components (x, y): no product is rounded."""
    z = _rows3(rows)
    b = np.asarray(branch, dtype=np.int64).reshape(-1) & 7
    k = np.arange(z.shape[0])
    idx = np.asarray(_OUT_IDX, dtype=np.int64)[k & 1, b]
    v = z[k, idx]
    re, im = v.real, v.imag
    start = b >> 1
    x = np.choose(start, (-im, -re, re, im))
    y = np.choose(start, (re, -im, im, -re))
    return x, y


def carrier_stat_host(rows, branch, window: int = DEFAULT_WINDOW) -> np.ndarray:
    """``wf_carrier_stat`` -> float64[nwin, 2] = (X_w, Y_w), in the header's order of additions: 64 lane partials per window
    (rows w W + 64 i + l, i increasing, from +0), then p_l += p_{l+d} for d = 32 .. 1."""
    return stat_terms_host(*branch_terms_host(rows, branch), window)


def stat_terms_host(x, y, window: int = DEFAULT_WINDOW) -> np.ndarray:
    """(X_w, Y_w) from the terms themselves, in ``wf_carrier_stat``'s order of additions (``wf_carrier_stat_terms``)."""
    window = _check_window(window)
    x, y = np.asarray(x, dtype=np.float64).reshape(-1), np.asarray(y, dtype=np.float64).reshape(-1)
    return np.stack((_stages.window_sum(x, window), _stages.window_sum(y, window)), axis=1)


def _wrap_pi(x):
    return _wrap(x, math.pi)


def carrier_psi_host(stat, period: float = math.pi):
    """What ``wf_carrier_track`` forms per window before it unwraps: float64[H, nwin, 2] -> (ψ f64[nwin], choice u8[nwin])."""
    period = float(period)
    if not (math.isfinite(period) and 0.0 < period <= 2.0 * math.pi):
        raise ValueError(f"period = {period} outside (0, 2π]")
    stat = np.asarray(stat, dtype=np.float64)
    if stat.ndim == 2:
        stat = stat[None]
    H, nwin = stat.shape[0], stat.shape[1]
    choice = np.argmin(stat[:, :, 0], axis=0)              # the first of equal minima
    w = np.arange(nwin)
    bx, by = stat[choice, w, 0], stat[choice, w, 1]
    return (choice.astype(np.float64) * period) / float(H) + np.arctan2(-by, -bx), choice.astype(np.uint8)


def carrier_track_host(stat, span: int = DEFAULT_SPAN, period: float = math.pi, anchor: int = 0, max_drift=None, reject=None):
    """``wf_carrier_track``: float64[H, nwin, 2] -> (phase f64[nwin], choice u8[nwin]).  ``period``: the symmetry of the
    trellis in place of π (``wf_carrier_track_mod``).  ``anchor`` = K > 0: ``wf_carrier_track_anchored``, the anchored unwrapping
    of ``_stages.anchored_unwrap`` in place of the running one -> (phase, choice, the drift found in radians per window, the
    rejected windows u8[nwin]); ``max_drift`` in radians per window (None: 1.25 * 2π ``MAX_DRIFT_TURNS``), ``reject`` in radians
    (None: period / 4)."""
    psi, choice = carrier_psi_host(stat, period)
    period, span = float(period), _stages.check_span(span)
    K, D, rho = _stages.anchor_args(anchor, max_drift, reject, period, 2.0 * math.pi * MAX_DRIFT_TURNS)
    if K:
        kept, drift, marks = _stages.anchored_unwrap(psi, period, K, D, rho)
        return _stages.centred_mean(kept, span), choice, drift, marks
    return _stages.centred_mean(_stages.unwrap(psi, period), span), choice


def interpolate_phase_host(ncalls: int, window: int, phase) -> np.ndarray:
    """φ_k of ``wf_rows_derotate``: linear between the window centres w W + (W - 1) / 2, flat outside the first and last."""
    window = _check_window(window)
    phase = np.asarray(phase, dtype=np.float64).reshape(-1)
    nwin = phase.size
    t = (np.arange(int(ncalls), dtype=np.float64) - 0.5 * float(window - 1)) / float(window)
    fl = np.floor(t)
    w = np.clip(fl.astype(np.int64), 0, max(nwin - 2, 0))
    f = t - fl
    p0 = phase[w]
    d = phase[np.minimum(w + 1, nwin - 1)] - p0
    fd = f * d
    phi = p0 + fd
    phi = np.where(t <= 0.0, phase[0], phi)
    return np.where(t >= float(nwin - 1), phase[nwin - 1], phi)


def derotate_host(rows, window: int = 64, phase=None, phase0: float = 0.0) -> np.ndarray:
    """``wf_rows_derotate``: complex128[n, 3] times exp(-j (phase0 + φ_k)); ``phase=None``: φ = 0."""
    return _stages.derotate(_rows3(rows), window, phase, phase0)


def estimate_host(rows, differential: bool = True) -> float:
    """The whole-burst decision-directed estimate of the rows' rotation, in radians: the angle of -Σ q_k along the
    max-log-MAP path (no hypothesis search: valid where the decisions are mostly right)."""
    _llr, _bits, branch = map_branch_host(rows, differential)
    x, y = branch_terms_host(rows, branch)
    return math.atan2(-float(np.sum(y)), -float(np.sum(x)))


def recover_host(rows, window: int = DEFAULT_WINDOW, span: int = DEFAULT_SPAN, hypotheses: int = DEFAULT_HYPOTHESES,
                 refine: int = DEFAULT_REFINE, differential: bool = True):
    """``CarrierRecovery.recover`` on the host -> (rows_out complex128[n, 3], phase f64[nwin], choice u8[nwin])."""
    z = _rows3(rows)
    H = int(hypotheses)
    stats = []
    for h in range(H):
        zh = derotate_host(z, phase0=(float(h) * math.pi) / float(H))
        stats.append(carrier_stat_host(zh, map_branch_host(zh, differential)[2], window))
    return _stages.carrier_recover_host(np.stack(stats), lambda out: carrier_stat_host(out, map_branch_host(out, differential)[2], window),
                                        lambda phase: derotate_host(z, window, phase), span, refine, math.pi)


class CarrierRecovery(_stages.Synchroniser):
    """Carrier phase and frequency recovery of a burst of 48-byte detector rows, everything on the device:

    1. ``hypotheses`` passes of ``rows_derotate`` by h π / H -> ``viterbi_soft_branch`` -> ``carrier_stat``,
    2. ``carrier_track``: per window the best hypothesis and its phase, unwrapped modulo π and smoothed over ``span`` windows,
    3. ``rows_derotate`` by that trajectory,
    4. ``refine`` further passes with one hypothesis on the derotated rows; each adds its trajectory to the one before it,
       and the input rows are derotated by the sum.

    ``recover`` returns the derotated rows, the trajectory (radians per window, modulo π) and the coarse choices; nothing
    comes back to the host.  ``times=True`` keeps device events around every stage of the last call (``stage_times``).

    ``anchor`` = K > 0 (odd, 3 .. 1023): the tracks use the anchored unwrapping of include/wfhip.h in place of the running one -
    no cycle slips behind a bad window; ``max_drift`` and ``reject`` in radians (per window) (None: 1.25 times the documented drift limit and a
    quarter of the period).  The last ``recover``'s coarse track leaves the drift found and the rejected windows on the device in
    ``carrier_found``."""

    def __init__(self, window: int = DEFAULT_WINDOW, span: int = DEFAULT_SPAN, hypotheses: int = DEFAULT_HYPOTHESES,
                 refine: int = DEFAULT_REFINE, anchor: int = 0, max_drift=None, reject=None) -> None:
        super().__init__()
        self._anchor_init("carrier", anchor, max_drift, reject, math.pi, 2.0 * math.pi * MAX_DRIFT_TURNS)
        self.window = _check_window(window)
        self.span = _stages.check_span(span)
        self.hypotheses = _stages.check_range("hypotheses", hypotheses, 1, 256)
        self.refine = _stages.check_refine(refine)

    def recover(self, rows, differential: bool = True, ctx=None):
        from .. import _hip
        from .. import device as dev

        H, W = self.hypotheses, self.window
        n = rows.numel() * rows.element_size() // 48
        nwin = -(-n // W)
        stat = _hip.empty((H, nwin, 2), "float64")
        work = _hip.empty(tuple(rows.shape), "float64")
        self._events = []
        self._mark("start")
        for h in range(H):
            dev.rows_derotate(rows, phase0=(float(h) * math.pi) / float(H), out=work, ctx=ctx)
            self._mark("derotate")
            _llr, _bits, branch = dev.viterbi_soft_branch(work, differential, ctx=ctx)
            self._mark("soft_branch")
            dev.carrier_stat(work, branch, W, out=stat[h], ctx=ctx)
            self._mark("stat")

        def statistic():
            _llr, _bits, branch = dev.viterbi_soft_branch(work, differential, ctx=ctx)
            self._mark("soft_branch")
            one = dev.carrier_stat(work, branch, W, ctx=ctx)
            self._mark("stat")
            return one

        def derotate_by(phase):
            dev.rows_derotate(rows, W, phase, out=work, ctx=ctx)
            self._mark("derotate")

        phase, choice = _stages.carrier_recover(self, stat, statistic, derotate_by, nwin, ctx)
        return work, phase, choice
