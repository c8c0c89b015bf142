"""Symbol timing recovery for the generic CPM chains (ARTM multi-h, PCM/FM): the feed-forward scheme of
``waveforms_amd.sync.timing`` on the full-phase trellis (include/wfhip.h states the device operations:
``wf_cpm_mf_rows_resample_c128`` and ``wf_llr_stat``; the trajectory stages are ``wf_timing_track`` and ``wf_timing_refine``,
untouched).  The reference has no synchroniser; every definition here is this package's own.

What differs from SOQPSK-TG.

The statistic.  The summed decided-branch metric X of timing.py has no usable minimum for ARTM: on its 64-state trellis the
maximum-likelihood path fits almost as well at a wrong instant.  A wrong instant makes AMBIGUOUS decisions, so the statistic
here is the summed LLR magnitude S_w = -Σ |λ| over a window's bits, from the plain soft detector (``cpm_soft``), for both
waveforms (``llr_stat``).  It goes into the X slot of the table the trajectory stages read.

The period.  S repeats every nh symbols (PCM/FM: one symbol, ARTM: two, where template column k % nh fits again), and the
tracker unwraps modulo nh sps samples.  The trellis does not repeat with that period: over nh symbols the tilt advances by
(M - 1) ΣK units of π/p, an odd number (7, 27), while the trellis's symmetry is two units, P = 2π/p.  One period late the rows
match the detector's call index on a phase grid turned by P/2; two periods late everything is as at 0.  So after the
trajectory one GRID decision per burst follows: two passes along τ, one with the link's rotation table and one with the
table turned by P/2 (``carrier_cpm.hypothesis_table``); ``grid`` = 1 if Σ_w S_w is smaller on the turned grid (ties to 0).
The final rows are made with the templates multiplied by e^{j grid P/2}, which derotates them by grid P/2 at no cost.

The defaults.  ARTM's well is a third as wide as PCM/FM's (±1.5 samples on a floor): its hypotheses lie one sample apart
(H = 16 over 16 samples) and its refinement samples at ±1; PCM/FM takes H = 8 over 8 samples and ±2, as SOQPSK-TG.

The ``*_host`` functions are the HOST statements.  ``cpm_mf_rows_resample_host`` forms every fused multiply-add of the
definition exactly (``_fma``: error-free transformations and one rounding to odd), so it is bitwise the device's and, with no
trajectory, bitwise the reference chain's ``cpm_mf_rows``; ``llr_stat_host`` is bitwise; the detector behind the statistic is
``carrier_cpm.cpm_map_branch_host``, whose λ agree with the device's to rounding.

The estimate is modulo nh symbols: the rows may come out a whole number of periods early or late, which a framed link's
frame search absorbs.

Limits.  The instant must stay within the pull-in of one hypothesis across a window: the supported drift is
|eps| sps W <= ``MAX_DRIFT_SAMPLES[waveform]`` samples per window.  Measured on ``recover_cpm_timing_host`` at sps 8 on the
reference chain on random symbols, noiseless, tau0 in {-2.7, 2.7, 6.0}, both signs; a case holds when every decision is the
genie's up to a shift of the rows by one period, outside one window at each end:
  PCM/FM (W 256, 2100 calls): all six cases hold at 0.4, 0.8, 1.2, 1.6, 2.0 and 2.5 samples per window; 2 fail at 3.0, 5 at 3.5,
      all at 4.0 (half the period).  Documented: 0.6, the margin timing.py took (1.6 where 7.0 held).
  ARTM (W 512, 4148 calls, and W 1024, 8244 calls): all hold at 0.1 .. 2.0; all six fail at 3.0.  Documented: 0.25, the drift
      the window study below was run at.  In samples per window the limit is PCM/FM's: the well is narrower but the
      hypotheses lie twice as close.
The ARTM window.  At 5.0 dB channel Eb/N0 (the demo-code link's waterfall less 3.01 dB), 5 seeds, unimpaired and at ±0.25
samples per window, bursts of 8 WHOLE windows: a coarse choice further than one hypothesis from the true one occurs in 7 of
15 bursts at W 256, in 1 of 15 at W 512 and in none at W 1024, the default.  The criterion is met for whole windows ONLY: with
100 calls behind the eight windows the short last window's choice was off by 4 to 7 hypotheses in 4 of 15 bursts at W 1024,
and in 7 and 4 of 15 at W 256 and 512 (HISTORY.md has the tables).  The links' own bursts end in such a window (the demo link's 4 251
calls are four windows and 155 calls), and the framed ARTM link is 0.81 dB from the genie at FER 1e-2 with lost codewords up to
9.5 dB.  On the host statement, 24 such bursts at 5.74 dB channel Eb/N0 (8.75 dB information), 6 samples late at half the
documented drift: the grid decision is right in all 24 (and the link's frame search locks at the lead in every block from
7.5 dB on, so no period is slipped); the short window's choice is off by 3 in one burst, whose trajectory is then 0.4 to 0.8
samples out over the last three windows; elsewhere the trajectory is 0.1 to 0.3 samples from the impairment.  So the grid
decision is not the cause; the short window accounts for bursts at the rate the tail shows; how much of the 0.81 dB is the
trajectory's own noise has not been separated.
The drift is ONE rate over the burst (``timing.rescale_host``).  No carrier recovery at the same time; specs whose full-phase
trellis has more than 64 states are refused; every hypothesis is a pass of the resampling front end AND of the soft detector.
"""
from __future__ import annotations

import math

import numpy as np

from . import _stages
from .carrier import DEFAULT_SPAN, _check_window
from .carrier_cpm import _check_spec, cpm_map_branch_host, hypothesis_table, period as grid_period
from .timing import _split, instants_host, lagrange_host

DEFAULT_REFINE = 1
# per waveform (by nh: 1 = PCM/FM, 2 = ARTM): hypotheses over one period of nh sps samples, the refinement's δ, the window
DEFAULTS = {1: {"hypotheses": 8, "delta": 2.0, "window": 256},
            2: {"hypotheses": 16, "delta": 1.0, "window": 1024}}
# |eps| sps W in samples (the module's docstring has the measurement)
MAX_DRIFT_SAMPLES = {"pcmfm": 0.6, "multih": 0.25}

def defaults(spec) -> dict:
    """{"hypotheses", "delta", "window"} for ``spec``'s waveform."""
    return dict(DEFAULTS[len(spec.K)])


# ------------------------------------------------------------------------------------------------ exact fma in numpy
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _fma(a, b, c):
    """Correctly rounded a b + c on float64 arrays: the product and the two sums error-free (Dekker, Knuth), the two error terms
    added with rounding to odd, one last rounding (Boldo and Melquiond, "Emulation of a FMA and correctly rounded sums", 2008).
    Exact for finite operands whose product neither overflows nor falls into the subnormals."""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (a, b, c)))
    uh, ul = _two_prod(a, b)
    th, tl = _two_sum(c, ul)
    vh, vl = _two_sum(uh, th)
    s, e = _two_sum(tl, vl)
    bits = np.ascontiguousarray(s).view(np.int64)
    fix = (e != 0.0) & (bits & 1 == 0)                       # inexact and even: the neighbour on e's side is odd
    bits = np.where(fix, bits + np.where((e > 0.0) == (s > 0.0), 1, -1), bits)
    return vh + bits.view(np.float64)


# ------------------------------------------------------------------------------------------------ host statements
def cpm_mf_rows_resample_host(received, templates, start0: int, sps: int, ncalls: int, window: int = 64, tau=None, tau0: float = 0.0):
    """``wf_cpm_mf_rows_resample_c128`` from its definition, every fma exact -> (rows complex128[ncalls, nfilt], the same sum over
    absolute values float64[ncalls, nfilt]: Σ_k (Σ_i |c_i| |r|) |T|)."""
    r = np.asarray(received, dtype=np.complex128).reshape(-1)
    T = np.asarray(templates, dtype=np.complex128)
    if T.ndim != 3 or T.shape[0] not in (1, 2):
        raise ValueError("templates must be complex128[nh, nfilt, ntm], nh 1 or 2")
    nh, nfilt, ntm = T.shape
    ncalls, nsamp = int(ncalls), r.size
    ok, fl, mu = _split(instants_host(ncalls, window, tau, tau0))
    n = np.arange(ncalls, dtype=np.int64)
    g = (int(start0) + n * int(sps) + fl)[:, None] + np.arange(ntm, dtype=np.int64)[None, :]          # [n, k]
    c = lagrange_host(mu)[:, :, None]                                                                  # [4, n, 1]

    def sample(i):
        s = g + (i - 1)
        use = ok[:, None] & (s >= 0) & (s < nsamp)
        return np.where(use, r[np.clip(s, 0, nsamp - 1)], 0.0)

    ra, rb, rc, rd = (sample(i) for i in range(4))
    x_re = _fma(c[3], rd.real, _fma(c[2], rc.real, _fma(c[1], rb.real, c[0] * ra.real)))
    x_im = _fma(c[3], rd.imag, _fma(c[2], rc.imag, _fma(c[1], rb.imag, c[0] * ra.imag)))
    ax = sum(np.abs(c[i]) * np.abs(v) for i, v in enumerate((ra, rb, rc, rd)))
    Tn = T[n % nh]                                                                                     # [n, f, k]
    zr, zi = np.zeros((ncalls, nfilt)), np.zeros((ncalls, nfilt))
    mag = np.zeros((ncalls, nfilt))
    for k in range(ntm):
        xr, xi, tr, ti = x_re[:, k, None], x_im[:, k, None], Tn[:, :, k].real, Tn[:, :, k].imag
        zr = _fma(xr, tr, _fma(xi, ti, zr))
        zi = _fma(-xr, ti, _fma(xi, tr, zi))
        mag = mag + ax[:, k, None] * np.abs(Tn[:, :, k])
    dead = ~(ok & (g[:, -1] + 2 >= 0) & (g[:, 0] - 1 < nsamp))                                         # a zero row, +0 in both components
    zr[dead], zi[dead], mag[dead] = 0.0, 0.0, 0.0
    return zr + 1j * zi, mag


def llr_stat_host(llr, bits_per_call: int, window: int) -> np.ndarray:
    """``wf_llr_stat`` -> float64[nwin, 2] = (-Σ |λ|, +0) per window of ``window`` calls, in ``wf_carrier_stat``'s order of
    additions: bitwise."""
    lam = np.abs(np.asarray(llr, dtype=np.float64).reshape(-1))
    per = int(bits_per_call) * _check_window(window)
    if not 1 <= int(bits_per_call) <= 8 or lam.size == 0 or lam.size % int(bits_per_call):
        raise ValueError("llr must hold bits_per_call (1 .. 8) values for each of at least one call")
    total = _stages.window_sum(lam, per)
    out = np.zeros((total.size, 2))
    out[:, 0] = -total
    return out


def turned_templates_host(spec, templates, grid: int) -> np.ndarray:
    """The templates times e^{j grid P/2} (the real products and sums one at a time, as the device composition forms them);
    ``grid`` 0: the templates themselves."""
    T = np.asarray(templates, dtype=np.complex128)
    if not grid:
        return T
    ang = 0.5 * grid_period(spec)
    cs, sn = math.cos(ang), math.sin(ang)
    return (T.real * cs - T.imag * sn) + 1j * (T.real * sn + T.imag * cs)


def recover_cpm_timing_host(spec, received, templates, start0: int, sps: int, ncalls: int, window: int | None = None,
                            span: int = DEFAULT_SPAN, hypotheses: int | None = None, refine: int = DEFAULT_REFINE,
                            delta: float | None = None, soft=None):
    """``CPMTimingRecovery.recover`` on the host -> (rows complex128[ncalls, nfilt], tau f64[nwin], choice u8[nwin], grid 0 / 1).
    ``soft(rows, rot)`` -> λ replaces ``cpm_map_branch_host`` (a faster restatement of the same detector)."""
    _check_spec(spec)
    dflt = defaults(spec)
    W = int(dflt["window"] if window is None else window)
    H = int(dflt["hypotheses"] if hypotheses is None else hypotheses)
    delta = float(dflt["delta"] if delta is None else delta)
    per = float(len(spec.K) * int(sps))
    lg = spec.bits_per_symbol
    if soft is None:
        def soft(rows, rot):
            return cpm_map_branch_host(spec, rows, 0, rot)[0]

    def stat_at(tau, tau0, rot=None):
        rows = cpm_mf_rows_resample_host(received, templates, start0, sps, ncalls, W, tau, tau0)[0]
        return llr_stat_host(soft(rows, rot), lg, W)

    tau, choice = _stages.timing_recover_host(stat_at, per, float(sps) * float(W), span, H, refine, delta)
    plain = stat_at(tau, 0.0)[:, 0].sum()
    turned = stat_at(tau, 0.0, hypothesis_table(spec, 0.5 * grid_period(spec)))[:, 0].sum()
    grid = 1 if turned < plain else 0
    rows = cpm_mf_rows_resample_host(received, turned_templates_host(spec, templates, grid), start0, sps, ncalls, W, tau)[0]
    return rows, tau, choice, grid


class CPMTimingRecovery(_stages.Synchroniser):
    """Symbol timing recovery of a burst of noisy CPM samples at ``sps`` samples per symbol, everything on the device:

    1. ``hypotheses`` passes of ``cpm_mf_rows_resample`` at tau0 = s_h = h period / H - period / 2 -> ``cpm_soft`` ->
       ``llr_stat``; the period is nh sps samples,
    2. ``timing_track`` with that period, and ``timing.rescale_host``'s stretch (samples per window = sps W),
    3. ``refine`` rounds of three such passes along τ at -δ, 0, +δ and ``timing_refine``; τ += its output,
    4. the grid decision: two passes along τ, with the rotation table as it is and turned by P/2; ``grid`` = 1 if Σ_w S_w is
       smaller on the turned grid,
    5. ``cpm_mf_rows_resample`` along τ with the templates times e^{j grid P/2}: the rows the detector gets.

    ``recover`` returns those rows, the trajectory (samples per window, modulo nh symbols), the coarse choices and the grid
    (a device int64 scalar tensor); nothing comes back to the host.  ``times=True`` keeps device events around every stage of the
    last call (``stage_times``).  ``spec``: a full-phase design with at most 64 states (``viterbi.cpm.full_phase``: ARTM_64,
    PCMFM_20); ``window``, ``hypotheses`` and ``delta`` default per waveform (``defaults``).

    ``anchor`` = K > 0 (odd, 3 .. 1023): the tracks use the anchored unwrapping of include/wfhip.h in place of the running one -
    no cycle slips behind a bad window; ``max_drift`` and ``reject`` in samples (per window) (None: 1.25 times the documented drift limit and a
    quarter of the period).  The last ``recover``'s coarse track leaves the drift found and the rejected windows on the device in
    ``timing_found``."""

    def __init__(self, spec, sps: int, window: int | None = None, span: int = DEFAULT_SPAN, hypotheses: int | None = None,
                 refine: int = DEFAULT_REFINE, delta: float | None = None, anchor: int = 0, max_drift=None, reject=None) -> None:
        super().__init__()
        _check_spec(spec)
        self._anchor_init("timing", anchor, max_drift, reject, float(len(spec.K) * int(sps)), MAX_DRIFT_SAMPLES["multih" if len(spec.K) == 2 else "pcmfm"])
        dflt = defaults(spec)
        self.spec = spec
        self.window = _check_window(dflt["window"] if window is None else window)
        self.sps = _stages.check_range("sps", sps, 1, 256)
        self.span = _stages.check_span(span)
        self.hypotheses = _stages.check_range("hypotheses", dflt["hypotheses"] if hypotheses is None else hypotheses, 3, 64)
        self.refine = _stages.check_refine(refine)
        self.delta = _stages.check_delta(dflt["delta"] if delta is None else delta)
        self._tables = None

    def recover(self, received, templates, start0: int, ncalls: int, ctx=None):
        """``received``: device float64[nsamp, 2]; ``templates``: device float64[nh, nfilt, ntm, 2] of ``spec`` ->
        (rows float64[ncalls, nfilt, 2], tau f64[nwin], choice u8[nwin], grid int64[])."""
        from .. import _hip
        from .. import device as dev

        spec, W, ncalls = self.spec, self.window, int(ncalls)
        lg, nwin = spec.bits_per_symbol, -(-ncalls // W)
        per = float(len(spec.K) * self.sps)
        half = 0.5 * grid_period(spec)
        if self._tables is None:
            self._tables = [_hip.to_device(hypothesis_table(spec)), _hip.to_device(hypothesis_table(spec, half))]
        work = _hip.empty((ncalls, spec.nfilt, 2), "float64")
        self._events = []
        self._mark("start")

        def stat_at(tau, tau0, out, table=0):
            dev.cpm_mf_rows_resample(received, templates, start0, self.sps, ncalls, W, tau, tau0, out=work, ctx=ctx)
            self._mark("resample")
            llr, _bits = dev.cpm_soft(work, spec, 0, 0, ctx=ctx, d_rot=self._tables[table])
            self._mark("soft")
            dev.llr_stat(llr, lg, W, out=out, ctx=ctx)
            self._mark("stat")

        tau, choice = _stages.timing_recover(self, stat_at, per, nwin, ctx)
        both = _hip.empty((2, nwin, 2), "float64")
        for table in (0, 1):
            stat_at(tau, 0.0, both[table], table)
        total = both[:, :, 0].sum(dim=1)
        grid = (total[1] < total[0]).to(_hip.torch().int64)
        cs, sn = math.cos(half), math.sin(half)
        tr, ti = templates[..., 0], templates[..., 1]
        turned = _hip.torch().stack((tr * cs - ti * sn, tr * sn + ti * cs), dim=-1)
        final = _hip.torch().where(grid.bool(), turned, templates).contiguous()
        self._mark("grid")
        dev.cpm_mf_rows_resample(received, final, start0, self.sps, ncalls, W, tau, 0.0, out=work, ctx=ctx)
        self._mark("resample")
        return work, tau, choice, grid
