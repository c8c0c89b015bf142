"""Carrier phase and frequency recovery for the generic CPM detectors (ARTM multi-h, PCM/FM): the feed-forward,
decision-directed scheme of ``waveforms_amd.sync.carrier`` on the full-phase trellis (include/wfhip.h states the device
operations: ``wf_cpm_soft_branch``, ``wf_carrier_stat_terms``, ``wf_carrier_track_mod``, ``wf_rows_derotate_n``).  The
reference has no synchroniser; every definition here is this package's own.

What differs from SOQPSK-TG.  The full-phase trellis is exactly symmetric under a rotation of the rows by P = 2π / p (22.5
degrees for ARTM, 36 for PCM/FM): it moves the phase index v of every state by one and leaves the input symbols alone.  The
estimate is therefore modulo P and the ambiguity never reaches the data: no framing is needed to resolve it.  The detector
takes its rotation table as an argument, so a coarse hypothesis is a rotated table of 2p entries (``hypothesis_table``), not
a pass over the rows: ``hypotheses`` = H passes span [0, P) in steps of P / H.  Two are enough (one locks to either
neighbour near the midpoints and fails under drift, four are no better than two); with one refinement that is three
detector passes.

The ``*_host`` functions are the HOST statements, in numpy.  ``cpm_map_branch_host`` forms its increments without fma, so
its branches equal the device's except at near-ties of T (none within 1e-9 on link rows); the statistics are bitwise given
the terms, the trajectory and the derotation agree to rounding.  ``carrier_track_host`` and ``interpolate_phase_host`` are
carrier.py's.  The noiseless estimate is not the injected rotation: the two-symbol matched filters leave a constant offset
of a few degrees (0.9 to 2.6 for ARTM, 2.9 for PCM/FM at 8 samples per symbol), harmless to the detector that follows - so
a trajectory is compared with the host statement's, not with the injected phase.

Limits.  The phase must stay within the decision-directed pull-in across one window: the supported frequency offset is
|nu| sps W <= ``MAX_DRIFT_PERIODS`` / p turns per window (nu in cycles per sample) - 0.0078 turns for ARTM, 0.0125 for
PCM/FM - measured on ``recover_cpm_host`` at the default window, 40 degrees of start phase, both signs, 5 seeds of random
symbols (tests/test_cpm_carrier.py holds the noiseless case):
  noiseless, 4096 calls: no decision differs from the genie's at 0.125, 0.1875, 0.25, 0.3 and 0.4 of P per window; at 0.5
      every burst fails (26 .. 63 symbol errors for ARTM, 15 .. 27 for PCM/FM);
  ARTM at 8 dB, 8192 calls, the same noise as the genie's: 550 symbol errors against the genie's 544 at 0.125, 620 at 0.25,
      1474 at 0.4;   PCM/FM at 6 dB: 104 against 104 at 0.125 and at 0.25, 134 at 0.4.
No timing recovery; the time-varying derotation is a pass of its own over the rows; the recovery passes carry no prior; specs
whose full-phase trellis has more than 64 states (ARTM_256) are refused.
"""
from __future__ import annotations

import math

import numpy as np

from . import _stages
from .carrier import DEFAULT_SPAN, DEFAULT_WINDOW, _check_window, stat_terms_host

DEFAULT_HYPOTHESES = 2
DEFAULT_REFINE = 1
MAX_DRIFT_PERIODS = 0.125                 # drift across one window as a fraction of P = 2π / p; the noiseless host statement decides
                                          # every symbol as the genie up to 0.4 and fails at 0.5; at 8 dB ARTM loses from 0.25 on


def period(spec) -> float:
    """P = 2π / p: the rotation of the rows under which the full-phase trellis of ``spec`` is symmetric."""
    return (2.0 * math.pi) / float(spec.p)


def hypothesis_table(spec, phase0: float = 0.0) -> np.ndarray:
    """float64[2p][2] = (cos, sin)(π r / p + phase0): ``rotation_table(spec)`` turned by ``phase0``, the table with which
    the detector sees the rows derotated by ``phase0`` (bitwise ``rotation_table`` at 0)."""
    ang = np.pi * np.arange(2 * spec.p) / spec.p + float(phase0)
    return np.ascontiguousarray(np.stack([np.cos(ang), np.sin(ang)], axis=1))


def _check_spec(spec) -> None:
    if spec.NC != spec.p:
        raise ValueError(f"the recovery runs on the full-phase trellis: NC = {spec.NC}, p = {spec.p} (viterbi.cpm.full_phase)")
    if spec.nstates > 64:
        raise ValueError(f"{spec.nstates} states: the soft detector behind the recovery stops at 64")


def _rows(spec, rows) -> np.ndarray:
    z = np.asarray(rows)
    if z.dtype != np.complex128:
        z = np.ascontiguousarray(z, dtype=np.float64).reshape(-1, spec.nfilt, 2).view(np.complex128)
    return np.ascontiguousarray(z).reshape(-1, spec.nfilt)


def _trellis(spec):
    """Per variant kv (0 / 1: the leaving symbol's K[0] / K[1], 2: pre-start): end[kv][s, u] and, per end state, the flat
    indices s M + u of its M entering branches; dt[kv] = the tilt's step."""
    M, p, Lp, S = spec.M, spec.p, spec.Lp, spec.nstates
    msub = M ** max(Lp - 2, 0)
    Ks = (spec.K[0], spec.K[-1], 0)
    ends, srcs = [], []
    s = np.arange(S)
    v, corr = s % p, s // p
    for K_old in Ks:
        end = np.empty((S, M), dtype=np.int64)
        for u in range(M):
            u_old = np.full(S, u) if Lp == 1 else corr // msub
            corr2 = np.zeros(S, dtype=np.int64) if Lp == 1 else u + M * (corr % msub)
            end[:, u] = (v + K_old * u_old) % p + p * corr2
        ends.append(end)
        srcs.append(np.argsort(end.reshape(-1), kind="stable").reshape(S, M))
    return ends, srcs


def _call_tables(spec, n: int, first_call: int):
    """kv and tilt of the calls first_call .. first_call + n - 1 (cpm_oracle.c: tilt = (M - 1) Σ K over the symbols that left)."""
    Lp, nh, p2 = spec.Lp, len(spec.K), 2 * spec.p
    g = np.arange(n, dtype=np.int64) + int(first_call)
    m_old = g - Lp + 1
    kv = np.where(m_old < 0, 2, m_old % nh if nh == 2 else 0)
    m = np.maximum(m_old, 0)
    per = sum(spec.K)
    acc = (m // nh) % p2 * per
    for i in range(nh - 1):
        acc = acc + np.where(m % nh > i, spec.K[i], 0)
    tilt = ((spec.M - 1) * (acc % p2)) % p2
    return kv, tilt


def cpm_map_branch_host(spec, rows, first_call: int = 0, rot=None, margins: bool = False):
    """``wf_cpm_soft_branch`` on the host -> (llr f64[n lgM], bits u8[n lgM], branch u8[n], x f64[n], y f64[n]).

    The recursions of ``wf_cpm_soft`` (include/wfhip.h) with, per call, b* = M s + u of the smallest
    T = (ã_k(s) + inc) + b̃_{k+1}(end), ties to the smallest b, and the components of q_k on it.  ``rot``: the rotation table
    (default ``hypothesis_table(spec)``).  Increments are formed as -(cos Re Z + sin Im Z) with two roundings where the
    device has one fma.  ``margins=True`` appends the gap between the smallest and the second smallest T of every call
    (f64[n]): where it is tiny, the two roundings may pick another branch than the fma does."""
    _check_spec(spec)
    z = _rows(spec, rows)
    n, M, p, S, lg = z.shape[0], spec.M, spec.p, spec.nstates, spec.bits_per_symbol
    rot = hypothesis_table(spec) if rot is None else np.asarray(rot, dtype=np.float64).reshape(2 * p, 2)
    ends, srcs = _trellis(spec)
    kv, tilt = _call_tables(spec, n, first_call)
    s = np.arange(S)
    v2, f = 2 * (s % p), (np.arange(M)[None, :] + M * (s // p)[:, None])           # f[s, u]
    r = (v2[None, :] - tilt[:, None]) % (2 * p)                                     # r[k, s]
    cr, sr = rot[r, 0][:, :, None], rot[r, 1][:, :, None]
    zf = z[:, f]                                                                    # [k, s, u]
    inc = -(cr * zf.real + sr * zf.imag)
    quad = -(cr * zf.imag - sr * zf.real)
    alpha = np.empty((n + 1, S))
    a = np.zeros(S)
    alpha[0] = a
    for k in range(n):
        new = (a[:, None] + inc[k]).reshape(-1)[srcs[kv[k]]].min(axis=1)
        a = new - new.min()
        alpha[k + 1] = a
    llr = np.empty((n, lg))
    branch = np.empty(n, dtype=np.uint8)
    x, y, gap = np.empty(n), np.empty(n), np.empty(n)
    sel = [[(np.arange(M) >> (lg - 1 - i)) & 1 == bit for bit in (0, 1)] for i in range(lg)]
    b = np.zeros(S)
    for k in range(n - 1, -1, -1):
        g = b[ends[kv[k]]]
        t = (alpha[k][:, None] + inc[k]) + g
        for i in range(lg):
            llr[k, i] = t[:, sel[i][1]].min() - t[:, sel[i][0]].min()
        best = int(np.argmin(t))                                                    # the first of equal minima: the smallest b
        branch[k] = best
        x[k], y[k] = inc[k].reshape(-1)[best], quad[k].reshape(-1)[best]
        if margins:
            two = np.partition(t.reshape(-1), 1)[:2]
            gap[k] = two[1] - two[0]
        new = (inc[k] + g).min(axis=1)
        b = new - new.min()
    llr = llr.reshape(-1)
    out = (llr, (llr < 0).astype(np.uint8), branch, x, y)
    return out + (gap,) if margins else out


def carrier_stat_terms_host(x, y, window: int = DEFAULT_WINDOW) -> np.ndarray:
    """``wf_carrier_stat_terms`` -> float64[nwin, 2] = (X_w, Y_w), in ``wf_carrier_stat``'s order of additions."""
    return stat_terms_host(x, y, window)


def derotate_n_host(spec, rows, window: int = 64, phase=None, phase0: float = 0.0) -> np.ndarray:
    """``wf_rows_derotate_n``: complex128[n, nfilt] times exp(-j (phase0 + φ_k)); ``phase=None``: φ = 0."""
    return _stages.derotate(_rows(spec, rows), window, phase, phase0)


def recover_cpm_host(spec, rows, window: int = DEFAULT_WINDOW, span: int = DEFAULT_SPAN, hypotheses: int = DEFAULT_HYPOTHESES,
                     refine: int = DEFAULT_REFINE, first_call: int = 0):
    """``CPMCarrierRecovery.recover`` on the host -> (rows_out complex128[n, nfilt], phase f64[nwin], choice u8[nwin])."""
    z = _rows(spec, rows)
    H, P = int(hypotheses), period(spec)
    stats = []
    for h in range(H):
        _l, _b, _br, x, y = cpm_map_branch_host(spec, z, first_call, hypothesis_table(spec, (float(h) * P) / float(H)))
        stats.append(carrier_stat_terms_host(x, y, window))

    def statistic(out):
        _l, _b, _br, x, y = cpm_map_branch_host(spec, out, first_call)
        return carrier_stat_terms_host(x, y, window)

    return _stages.carrier_recover_host(np.stack(stats), statistic, lambda phase: derotate_n_host(spec, z, window, phase), span, refine, P)


class CPMCarrierRecovery(_stages.Synchroniser):
    """Carrier phase and frequency recovery of a burst of CPM detector rows (float64[ncalls, nfilt, 2], what ``cpm_mf_rows``
    writes), everything on the device:

    1. ``hypotheses`` passes of ``cpm_soft_branch`` on the rows AS THEY ARE, pass h with the table turned by h P / H
       (``hypothesis_table``, uploaded once) -> ``carrier_stat_terms``,
    2. ``carrier_track`` with period P: per window the best hypothesis and its phase, unwrapped modulo P, smoothed over ``span``,
    3. ``rows_derotate_n`` by that trajectory,
    4. ``refine`` further passes with the plain table on the derotated rows; each adds its trajectory to the one before it,
       and the input rows are derotated by the sum.

    ``recover`` returns the derotated rows, the trajectory (radians per window, modulo P = 2π / p) and the coarse choices;
    nothing comes back to the host.  ``times=True`` keeps device events around every stage of the last call (``stage_times``).
    ``spec``: a full-phase design with at most 64 states (``viterbi.cpm.full_phase``: ARTM_64, PCMFM_20).

    ``anchor`` = K > 0 (odd, 3 .. 1023): the tracks use the anchored unwrapping of include/wfhip.h in place of the running one -
    no cycle slips behind a bad window; ``max_drift`` and ``reject`` in radians (per window) (None: 1.25 times the documented drift limit and a
    quarter of the period).  The last ``recover``'s coarse track leaves the drift found and the rejected windows on the device in
    ``carrier_found``."""

    def __init__(self, spec, window: int = DEFAULT_WINDOW, span: int = DEFAULT_SPAN, hypotheses: int = DEFAULT_HYPOTHESES,
                 refine: int = DEFAULT_REFINE, anchor: int = 0, max_drift=None, reject=None) -> None:
        super().__init__()
        _check_spec(spec)
        self._anchor_init("carrier", anchor, max_drift, reject, period(spec), MAX_DRIFT_PERIODS * period(spec))
        self.spec = spec
        self.window = _check_window(window)
        self.span = _stages.check_span(span)
        self.hypotheses = _stages.check_range("hypotheses", hypotheses, 1, 256)
        self.refine = _stages.check_refine(refine)
        self._tables = None

    def recover(self, rows, ctx=None, first_call: int = 0):
        from .. import _hip
        from .. import device as dev

        spec, H, W, P = self.spec, self.hypotheses, self.window, period(self.spec)
        if self._tables is None:
            self._tables = [_hip.to_device(hypothesis_table(spec, (float(h) * P) / float(H))) for h in range(H)]
        n = rows.numel() // (2 * spec.nfilt)
        nwin = -(-n // W)
        stat = _hip.empty((H, nwin, 2), "float64")
        self._events = []
        self._mark("start")
        for h in range(H):
            _llr, _bits, _branch, term = dev.cpm_soft_branch(rows, spec, first_call, 0, ctx=ctx, d_rot=self._tables[h])
            self._mark("soft_branch")
            dev.carrier_stat_terms(term, W, out=stat[h], ctx=ctx)
            self._mark("stat")
        work = None                                              # the first derotation makes it, the later ones write into it

        def statistic():
            _llr, _bits, _branch, term = dev.cpm_soft_branch(work, spec, first_call, 0, ctx=ctx, d_rot=self._tables[0])
            self._mark("soft_branch")
            one = dev.carrier_stat_terms(term, W, ctx=ctx)
            self._mark("stat")
            return one

        def derotate_by(phase):
            nonlocal work
            work = dev.rows_derotate_n(rows, spec.nfilt, W, phase, out=work, ctx=ctx)
            self._mark("derotate")

        phase, choice = _stages.carrier_recover(self, stat, statistic, derotate_by, nwin, ctx, P)
        return work, phase, choice
