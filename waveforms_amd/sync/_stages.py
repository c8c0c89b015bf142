"""What the five synchronisers of this package share, stated once: the device classes' stage marks and argument checks, the
host statements' wrap, unwrapping, centred mean and window sum, the rescale of a timing trajectory, and the compositions - coarse
search, track, refinement - of the timing and of the carrier recoveries, on the device and on the host.  The modules beside
this one hold what is their own: the statistics, the stages' host statements and the limits.

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
    tau, choice = dev.timing_track(stat, period, rec.span, ctx=ctx)
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


def timing_recover_host(stat_at, period: float, samples_per_window: float, span: int, hypotheses: int, refine: int, delta: float):
    """The same on the host statements -> (tau, choice); ``stat_at(tau, tau0)`` returns float64[nwin, 2]."""
    from .timing import hypothesis_instants, rescale_host, timing_refine_host, timing_track_host

    tau, choice = timing_track_host(np.stack([stat_at(None, s) for s in hypothesis_instants(period, hypotheses)]), period, span)
    tau = rescale_host(tau, samples_per_window)
    for _ in range(int(refine)):
        tau = tau + timing_refine_host(np.stack([stat_at(tau, d) for d in (-delta, 0.0, delta)]), delta, span)
    return tau, choice


# ------------------------------------------------------------------------------------------------ the carrier composition
def carrier_round(rec, phase, statistic, derotate_by, nwin: int, ctx, period=None):
    """One decision-directed round on the device -> the phase moved by its trajectory: ``statistic()`` of the work rows
    (float64[nwin, 2]), ``carrier_track`` with one hypothesis, the add, ``derotate_by(phase)``."""
    from .. import device as dev

    more, _c = dev.carrier_track(statistic().view(1, nwin, 2), rec.span, ctx=ctx, period=period)
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

    phase, choice = dev.carrier_track(coarse, rec.span, ctx=ctx, period=period)
    rec._mark("track")
    derotate_by(phase)
    for _ in range(rec.refine):
        phase = carrier_round(rec, phase, statistic, derotate_by, nwin, ctx, period)
    return phase, choice


def carrier_recover_host(coarse, statistic, derotate_by, span: int, refine: int, period: float):
    """The same on the host statements -> (rows, phase, choice): ``statistic(rows)`` returns float64[nwin, 2],
    ``derotate_by(phase)`` the input rows derotated."""
    from .carrier import carrier_track_host

    phase, choice = carrier_track_host(coarse, span, period)
    out = derotate_by(phase)
    for _ in range(int(refine)):
        more, _c = carrier_track_host(statistic(out)[None], span, period)
        phase = phase + more
        out = derotate_by(phase)
    return out, phase, choice
