"""What the five synchronisers of this package share, stated once: the device classes' stage marks and argument checks, the
host statements' wrap, unwrapping (the running one and the anchored one), centred mean and window sum, the rescale of a
timing trajectory, and the compositions - coarse search, track, refinement - of the timing and of the carrier recoveries, on
the device and on the host.  The modules beside this one hold what is their own: the statistics, the stages' host statements
and the limits.

The host and the device compositions stay two texts: one works on stacked numpy tables, the other writes into preallocated
device tables and takes marks.
"""
from __future__ import annotations

import math

import numpy as np


# ------------------------------------------------------------------------------------------------ the device classes
class Synchroniser:
    """The stage marks of a device-resident synchroniser: ``times=True`` keeps device events around every stage of the last
    ``recover`` (``stage_times``)."""

    def __init__(self) -> None:
        self.times = False
        self._events: list = []
        self.timing_anchor = self.carrier_anchor = (0, 0.0, 0.0)
        self.timing_found = self.carrier_found = None

    def _anchor_init(self, which: str, anchor, max_drift, reject, period: float, limit: float) -> None:
        """``which`` = "timing" or "carrier": that tracker's (K, D, ρ) of ``anchor_args`` (K = 0: the plain unwrapping).  The last
        ``recover``'s coarse track leaves (the drift found: a device float64[1], the rejected windows: device uint8[nwin]) in
        ``timing_found`` / ``carrier_found``; None without an anchor."""
        setattr(self, which + "_anchor", anchor_args(anchor, max_drift, reject, period, limit))

    def _mark(self, name: str) -> None:
        if self.times:
            from .. import _hip

            ev = _hip.torch().cuda.Event(enable_timing=True)
            ev.record()
            self._events.append((name, ev))

    def stage_times(self) -> dict[str, float]:
        """Milliseconds per stage of the last ``recover`` (``times=True``), summed over its passes - synchronises."""
        out: dict[str, float] = {}
        for (_n0, e0), (name, e1) in zip(self._events, self._events[1:]):
            e1.synchronize()
            out[name] = out.get(name, 0.0) + e0.elapsed_time(e1)
        return out


def check_window(window: int) -> int:
    window = int(window)
    if not (64 <= window <= 8192 and window % 64 == 0):
        raise ValueError(f"window = {window} must be a multiple of 64 from 64 to 8192")
    return window


def check_span(span) -> int:
    if int(span) < 1 or int(span) % 2 == 0:
        raise ValueError(f"span = {span} must be odd and at least 1")
    return int(span)


def check_refine(refine) -> int:
    if int(refine) < 0:
        raise ValueError(f"refine = {refine} must not be negative")
    return int(refine)


def check_delta(delta) -> float:
    if not (math.isfinite(float(delta)) and float(delta) > 0.0):
        raise ValueError(f"delta = {delta} must be finite and positive")
    return float(delta)


def check_range(name: str, value, lo: int, hi: int) -> int:
    """``hypotheses`` and ``sps``: the bounds are the class's own (the device stages')."""
    if not lo <= int(value) <= hi:
        raise ValueError(f"{name} = {value} outside {lo} .. {hi}")
    return int(value)


# ------------------------------------------------------------------------------------------------ host statements
def _wrap(x, period):
    return x - period * np.ceil(x / period - 0.5)


def unwrap(psi, period: float) -> np.ndarray:
    """u_0 = ψ_0, u_j = u_{j-1} + wrap(ψ_j - ψ_{j-1}): the running sum both trackers smooth."""
    u = np.empty(psi.size)
    u[0] = psi[0]
    step = _wrap(psi[1:] - psi[:-1], period)
    for j in range(1, psi.size):
        u[j] = u[j - 1] + step[j - 1]
    return u


def anchor_args(anchor, max_drift, reject, period: float, limit: float):
    """The anchored unwrapping's arguments checked -> (K, D, ρ).  ``anchor`` = K: 0 (the plain unwrapping; D and ρ come back as
    0) or odd, 3 .. 1023; ``max_drift`` = D in ψ's unit per window, 0 <= D < period / 2 (None: 1.25 ``limit``, the caller's
    documented drift); ``reject`` = ρ, 0 < ρ <= period / 2 (None: period / 4)."""
    K, P = int(anchor), float(period)
    if K == 0:
        return 0, 0.0, 0.0
    if not (3 <= K <= 1023 and K % 2 == 1):
        raise ValueError(f"anchor = {anchor} must be 0 or odd, 3 .. 1023")
    D = 1.25 * float(limit) if max_drift is None else float(max_drift)
    if not (math.isfinite(D) and 0.0 <= D < 0.5 * P):
        raise ValueError(f"max_drift = {D} outside [0, period / 2 = {0.5 * P})")
    rho = 0.25 * P if reject is None else float(reject)
    if not (math.isfinite(rho) and 0.0 < rho <= 0.5 * P):
        raise ValueError(f"reject = {rho} outside (0, period / 2 = {0.5 * P}]")
    return K, D, rho


def anchor_candidates(period: float, anchor: int, max_drift: float) -> int:
    """n = ceil((4K D) / P): the drift search tries f_i = i / (4K) cycles per window, |i| <= n (the product, the division, ceil)."""
    return int(math.ceil((float(4 * int(anchor)) * float(max_drift)) / float(period)))


def _turn(m, q: int):
    """exp(-j 2π m / q) for integers 0 <= m < q: the quotient, the product with 2π, then cos and sin."""
    a = (2.0 * math.pi) * (np.asarray(m, dtype=np.float64) / float(q))
    return np.cos(a) - 1j * np.sin(a)


def anchor_scores(psi, period: float, anchor: int, max_drift: float):
    """Steps 1 and 2 of ``anchored_unwrap`` -> (z complex128[nwin], the candidates i int64[2n + 1], their scores float64[2n + 1])."""
    psi = np.asarray(psi, dtype=np.float64).reshape(-1)
    P, K = float(period), int(anchor)
    q, nwin = 4 * K, psi.size
    ok = np.isfinite(psi)
    t = np.where(ok, psi, 0.0) / P
    ang = (2.0 * math.pi) * (t - np.floor(t))
    z = np.where(ok, np.cos(ang) + 1j * np.sin(ang), 0.0)
    n = anchor_candidates(P, K, max_drift)
    i = np.arange(-n, n + 1, dtype=np.int64)
    score = np.zeros(i.size)
    for s in range(0, nwin, 2 * K):
        acc = np.zeros(i.size, dtype=np.complex128)
        for j in range(min(K, nwin - s)):
            acc = acc + z[s + j] * _turn((i * j) % q, q)
        score = score + (acc.real * acc.real + acc.imag * acc.imag)
    return z, i, score


def anchored_unwrap(psi, period: float, anchor: int, max_drift: float, reject: float):
    """The anchored unwrapping of include/wfhip.h: ψ[nwin] -> (ψ' float64[nwin], the drift found f̂ P in ψ's unit per window,
    the rejected windows uint8[nwin]).  Smooth on the circle first, unwrap second:

    1. z_w = exp(j 2π frac(ψ_w / P)); a ψ_w that is not finite has z_w = 0,
    2. f̂ = i / (4K), the first |i| <= n of the largest Σ_segments |Σ_{j < K} z_{s+j} exp(-j 2π frac(i j / (4K)))|², the segments
       starting at s = 0, 2K, ..,
    3. y_w = z_w exp(-j 2π frac(f̂ w)); a_w = Σ y over the windows within K // 2 of w; α = atan2(Im a, Re a); u = ``unwrap``(α, 2π);
       r_w = (P / 2π) u_w + (P f̂) w,
    4. d_w = wrap(ψ_w - r_w, P); ψ'_w = r_w + d_w, or r_w (and a mark) where ψ_w is not finite or |d_w| > ρ.

    i j and i w are reduced modulo 4K as integers: no angle grows with the burst.  One window: (ψ_0 or 0, 0, the mark)."""
    psi = np.asarray(psi, dtype=np.float64).reshape(-1)
    ok = np.isfinite(psi)
    if psi.size == 1:
        return np.where(ok, psi, 0.0), 0.0, (~ok).astype(np.uint8)
    ref, d, drift = anchor_reference(psi, period, anchor, max_drift)
    marks = ~ok | (np.abs(d) > float(reject))
    return np.where(marks, ref, ref + d), drift, marks.astype(np.uint8)


def anchor_reference(psi, period: float, anchor: int, max_drift: float):
    """Steps 2 to 4 of ``anchored_unwrap`` up to the decision, for two windows or more -> (r float64[nwin], d float64[nwin] (of
    0 where ψ_w is not finite), f̂ P)."""
    psi = np.asarray(psi, dtype=np.float64).reshape(-1)
    P, K = float(period), int(anchor)
    q, nwin = 4 * K, psi.size
    ok = np.isfinite(psi)
    z, i, score = anchor_scores(psi, P, K, max_drift)
    best = int(i[int(np.argmax(score))])                   # the first of equal maxima
    w = np.arange(nwin, dtype=np.int64)
    y = z * _turn((best * w) % q, q)
    a = np.zeros(nwin, dtype=np.complex128)
    for k in range(-(K // 2), K // 2 + 1):                 # a_w += y_{w+k}: every w's terms in increasing order
        lo, hi = max(0, -k), min(nwin, nwin - k)
        if lo < hi:
            a[lo:hi] = a[lo:hi] + y[lo + k:hi + k]
    u = unwrap(np.arctan2(a.imag, a.real), 2.0 * math.pi)
    fhat = float(best) / float(q)
    ref = (P / (2.0 * math.pi)) * u + (P * fhat) * w.astype(np.float64)
    return ref, _wrap(np.where(ok, psi, 0.0) - ref, P), fhat * P


def centred_mean(u, span: int) -> np.ndarray:
    """The mean of u over the windows within span // 2 of each, clipped to the burst, added in increasing order."""
    span = check_span(span)
    nwin, r = u.size, span // 2
    out = np.empty(nwin)
    for j in range(nwin):
        lo, hi = max(0, j - r), min(nwin - 1, j + r)
        s = 0.0
        for i in range(lo, hi + 1):
            s += u[i]
        out[j] = s / float(hi - lo + 1)
    return out


def window_sum(values, per: int) -> np.ndarray:
    """float64[nwin]: the sums over windows of ``per`` values (a multiple of 64) in ``wf_carrier_stat``'s order of additions - 64
    lane partials per window (values w per + 64 i + l, i increasing, from +0), then p_l += p_{l+d} for d = 32 .. 1."""
    n = values.size
    nwin = -(-n // per)
    pad = np.zeros(nwin * per)                             # a partial that starts from +0 is never -0: adding +0 adds nothing
    pad[:n] = values
    pad = pad.reshape(nwin, per // 64, 64)
    p = np.zeros((nwin, 64))
    for i in range(per // 64):
        p = p + pad[:, i, :]
    d = 32
    while d >= 1:
        p[:, :d] = p[:, :d] + p[:, d:2 * d]
        d //= 2
    return p[:, 0]


def rescale(tau, nwin: int, samples_per_window: float):
    """``timing.rescale_host``'s stretch of tau[nwin] - a numpy array or a device tensor: only indexing, -, / and + - about its
    first window by 1 / (1 - its own slope); fewer than two windows: ``tau`` itself."""
    if nwin < 2:
        return tau
    a, b = (2, nwin - 3) if nwin >= 8 else (0, nwin - 1)
    s = (tau[b] - tau[a]) / (float(b - a) * float(samples_per_window))
    return tau[0] + (tau - tau[0]) / (1.0 - s)


def derotate(z, window: int, phase, phase0: float) -> np.ndarray:
    """complex128[n, nvals] times exp(-j (phase0 + φ_k)); ``phase=None``: φ = 0."""
    from .carrier import interpolate_phase_host

    phi = 0.0 if phase is None else interpolate_phase_host(z.shape[0], window, phase)
    tot = -(float(phase0) + phi) + np.zeros(z.shape[0])
    return z * (np.cos(tot) + 1j * np.sin(tot))[:, None]


# ------------------------------------------------------------------------------------------------ the timing composition
def timing_recover(rec, stat_at, period: float, nwin: int, ctx):
    """The device composition of a timing recovery -> (tau, choice): ``rec.hypotheses`` coarse passes ``stat_at(None, s_h,
    stat[h])``, ``timing_track``, the rescale, ``rec.refine`` rounds of three passes ``stat_at(tau, d, stat3[j])`` at -δ, 0, +δ
    and ``timing_refine``.  ``stat_at(tau, tau0, out)`` is the class's own statistic; it takes its marks itself."""
    from .. import _hip
    from .. import device as dev
    from .timing import hypothesis_instants

    stat = _hip.empty((rec.hypotheses, nwin, 2), "float64")
    for h, s in enumerate(hypothesis_instants(period, rec.hypotheses)):
        stat_at(None, float(s), stat[h])
    K, D, rho = rec.timing_anchor
    tau, choice, *found = dev.timing_track(stat, period, rec.span, ctx=ctx, anchor=K, max_drift=D, reject=rho)
    rec.timing_found = tuple(found) if K else None
    rec._mark("track")
    tau = rescale(tau, nwin, float(rec.sps) * float(rec.window))
    rec._mark("rescale")
    for _ in range(rec.refine):
        stat3 = _hip.empty((3, nwin, 2), "float64")
        for j, d in enumerate((-rec.delta, 0.0, rec.delta)):
            stat_at(tau, d, stat3[j])
        more = dev.timing_refine(stat3, rec.delta, rec.span, ctx=ctx)
        rec._mark("track")
        tau = tau + more
        rec._mark("add")
    return tau, choice


def timing_recover_host(stat_at, period: float, samples_per_window: float, span: int, hypotheses: int, refine: int, delta: float,
                        anchor: int = 0, max_drift=None, reject=None):
    """The same on the host statements -> (tau, choice); ``stat_at(tau, tau0)`` returns float64[nwin, 2]."""
    from .timing import hypothesis_instants, rescale_host, timing_refine_host, timing_track_host

    tau, choice = timing_track_host(np.stack([stat_at(None, s) for s in hypothesis_instants(period, hypotheses)]), period, span,
                                    anchor, max_drift, reject)[:2]
    tau = rescale_host(tau, samples_per_window)
    for _ in range(int(refine)):
        tau = tau + timing_refine_host(np.stack([stat_at(tau, d) for d in (-delta, 0.0, delta)]), delta, span)
    return tau, choice


# ------------------------------------------------------------------------------------------------ the carrier composition
def carrier_round(rec, phase, statistic, derotate_by, nwin: int, ctx, period=None):
    """One decision-directed round on the device -> the phase moved by its trajectory: ``statistic()`` of the work rows
    (float64[nwin, 2]), ``carrier_track`` with one hypothesis, the add, ``derotate_by(phase)``."""
    from .. import device as dev

    K, D, rho = rec.carrier_anchor
    more = dev.carrier_track(statistic().view(1, nwin, 2), rec.span, ctx=ctx, period=period, anchor=K, max_drift=D, reject=rho)[0]
    rec._mark("track")
    phase = phase + more
    rec._mark("add")
    derotate_by(phase)
    return phase


def carrier_recover(rec, coarse, statistic, derotate_by, nwin: int, ctx, period=None):
    """The device composition of a carrier recovery from its coarse table on -> (phase, choice): ``carrier_track`` of
    ``coarse`` (modulo ``period``; None: π), ``derotate_by`` that trajectory, ``rec.refine`` rounds of ``carrier_round``.
    ``statistic`` and ``derotate_by`` are the class's own; they take their marks themselves."""
    from .. import device as dev

    K, D, rho = rec.carrier_anchor
    phase, choice, *found = dev.carrier_track(coarse, rec.span, ctx=ctx, period=period, anchor=K, max_drift=D, reject=rho)
    rec.carrier_found = tuple(found) if K else None
    rec._mark("track")
    derotate_by(phase)
    for _ in range(rec.refine):
        phase = carrier_round(rec, phase, statistic, derotate_by, nwin, ctx, period)
    return phase, choice


def carrier_recover_host(coarse, statistic, derotate_by, span: int, refine: int, period: float, anchor: int = 0, max_drift=None,
                         reject=None):
    """The same on the host statements -> (rows, phase, choice): ``statistic(rows)`` returns float64[nwin, 2],
    ``derotate_by(phase)`` the input rows derotated."""
    from .carrier import carrier_track_host

    phase, choice = carrier_track_host(coarse, span, period, anchor, max_drift, reject)[:2]
    out = derotate_by(phase)
    for _ in range(int(refine)):
        more = carrier_track_host(statistic(out)[None], span, period, anchor, max_drift, reject)[0]
        phase = phase + more
        out = derotate_by(phase)
    return out, phase, choice
