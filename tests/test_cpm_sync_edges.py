"""The CPM timing and carrier stages at the tile, lookup and tie edges that tests/test_cpm_timing.py and
tests/test_cpm_carrier.py do not reach (include/wfhip.h: wf_cpm_mf_rows_resample_c128, wf_llr_stat, wf_carrier_track_mod; the
compositions ``CPMTimingRecovery.recover`` and ``CPMCarrierRecovery.recover``).

``cpm_mf_rows_resample_kernel`` walks tiles of ``syms`` rows in three phases behind four barriers and keeps a tile's samples in
LDS iff the span its rows read, ``need``, is at most the staged ``region``.  Here a later tile sits at need = region - 1, region
and region + 1 for seven launch geometries, rising and falling; all ten instantiations run, the nine-tap register path at sps 1,
64 and 256 and the two shapes next to the LDS ceiling among them; a workgroup's successive tiles come in every order of LDS,
global memory and dead; rows die one by one at the burst's two ends, under NaN and ±inf windows and beside ±2^62; a sample of
+inf and one of NaN sit in a staged tile and in one read from global memory; and the window lookup runs at 1, 2 and 3 windows.
``llr_stat_kernel`` takes a second step of its grid-stride loop and sees ±inf and NaN.  ``carrier_track_kernel`` runs with the
periods 2π/16 and 2π/10 on its segment grid, with exact ties between hypotheses and with steps of exactly ±P/2.  The two
compositions run at 1, 2, 7, 8 and 9 windows, the last one a few calls long.

CPU: the tile restated (geometry, ``need``, phases B and C on the staged span alone, with two seeded defects) and pinned to the
kernel's ``#define``s, and the preconditions that make the device comparisons sound.  GPU: the resampler and the statistic BITWISE
(uint64 views: -0 is not +0) against tests/cpm_timing_ref.c and ``llr_stat_host``; the tracker and the compositions against the
host statements within the header's bounds.
"""
import functools
import math
import re
from pathlib import Path

import numpy as np
import pytest

import test_carrier_edges as CE
from test_cpm_carrier import _rot
from test_cpm_timing import SPS, _chain, ref, restate, soft_c  # noqa: F401  (ref: the fixture of the two C restatements)
from test_timing_edges import _complex, _freeze
from waveforms_amd.sync import carrier as C
from waveforms_amd.sync import carrier_cpm as CC
from waveforms_amd.sync import timing as T
from waveforms_amd.sync import timing_cpm as TCM

EPS = 2.0 ** -52
CSRC = Path(__file__).resolve().parent.parent / "waveforms_amd" / "csrc"

# ---- A1. the launch geometry of wf_cpm_mf_rows_resample_c128, restated (test_kernel_constants_are_the_restated_ones pins it)
CRS_THREADS, CRS_EXTRA, CRS_GRID_CAP, CRS_TARGET_SLOTS, CRS_MAX_SLOTS, CRS_MIN_SYMS, LSTAT_THREADS = 256, 64, 2048, 2560, 9984, 32, 256
LSTAT_GRID = 1 << 16                  # llr_stat_kernel: blocks launched at most, LSTAT_THREADS / 64 windows each
# (nh, nfilt, ntm, sps) -> (syms, region, LDS bytes), worked out by hand from crs_geometry
GEOMETRY = {(1, 4, 9, 8): (127, 1084, 40720), (1, 4, 9, 1): (198, 273, 40800), (2, 16, 9, 64): (33, 2124, 40064),
            (1, 4, 9, 256): (32, 8012, 134080), (1, 2, 3, 2): (256, 580, 31904), (2, 64, 60, 8): (30, 359, 158624),
            (1, 2, 257, 256): (18, 4676, 157776)}


def geometry(nh, nfilt, ntm, sps):
    """(syms, region, LDS bytes) as crs_geometry chooses them: the most rows (<= 256) whose window, interpolated samples,
    weights, instants and template copy (none for nine taps: registers) fit the target; under 32 rows, 32 or as many as fit the
    ceiling."""
    tmpl = 0 if ntm == 9 else nh * nfilt * ntm

    def total(S):
        return (S - 1) * sps + ntm + 3 + CRS_EXTRA + S * ntm + 2 * S + (S + 1) // 2 + tmpl

    S = CRS_THREADS
    while S > 1 and total(S) > CRS_TARGET_SLOTS:
        S -= 1
    if S < CRS_MIN_SYMS:
        S = CRS_MIN_SYMS
        while S > 1 and total(S) > CRS_MAX_SLOTS:
            S -= 1
    assert total(S) <= CRS_MAX_SLOTS
    return S, (S - 1) * sps + ntm + 3 + CRS_EXTRA, 16 * total(S)


# ---- A2. phase A restated
def rows_B(start0, sps, ncalls, W, tau, tau0, ntm, nsamp):
    """(B_n, live_n, μ_n, usable_n) of every row as phase A forms them from the host statement's instants: usable iff |t| < 2^62,
    live iff usable and B + ntm + 1 >= 0 and B - 1 < nsamp (otherwise every sample the row reads lies outside the burst)."""
    with np.errstate(invalid="ignore"):
        ok, fl, mu = T._split(T.instants_host(ncalls, W, tau, tau0))
    B = int(start0) + np.arange(int(ncalls), dtype=np.int64) * int(sps) + fl
    return B, ok & (B + ntm + 1 >= 0) & (B - 1 < nsamp), mu, ok


def tile_needs(start0, sps, ncalls, W, tau, tau0, ntm, nsamp, syms, region):
    """Per tile of ``syms`` rows (any row live, lo, need, fits): lo = min B - 1 over the live rows, the first sample any of them
    reads, need = (max B + ntm + 1) - lo + 1, the samples from there to the last one, fits = any and need <= region."""
    B, live, _mu, _ok = rows_B(start0, sps, ncalls, W, tau, tau0, ntm, nsamp)
    starts = np.arange(0, int(ncalls), int(syms))
    big = np.iinfo(np.int64).max
    mn = np.minimum.reduceat(np.where(live, B, big), starts)
    mx = np.maximum.reduceat(np.where(live, B, -big), starts)
    some = mn <= mx
    lo = np.where(some, mn, 1) - 1
    need = np.where(some, (np.where(some, mx, 0) + ntm + 1) - lo + 1, 0)
    return some, lo, need, some & (need <= region)


def tile_kinds(*args):
    """0: staged in LDS, 1: read from global memory, 2: dead, per tile."""
    some, _lo, _need, fits = tile_needs(*args)
    return np.where(~some, 2, np.where(fits, 0, 1))


# ---- A3. phases B and C of one tile restated, reading the staged span alone
def tile_restatement(r, Tm, start0, sps, ncalls, W, tau, tau0, tile, short=False, strict=False):
    """rows complex128[rows of the tile, nfilt] as the kernel forms them: a tile that fits reads ``s_r``, here an array of
    ``region`` slots of which the first ``need`` are staged (zeros outside the burst; a slot nobody staged reads as zero, the
    mildest content a previous trip can leave); a tile that does not reads the burst, bounds-checked; every fma exact.
    Seeded defects: ``short`` - the staging loop stops one sample early; ``strict`` - the staging is decided by need < region
    while phase B goes by need <= region, so at need = region a span is read that nobody staged."""
    nh, nfilt, ntm = Tm.shape
    syms, region, _lds = geometry(nh, nfilt, ntm, sps)
    nsamp = r.size
    B, live, mu, _ok = rows_B(start0, sps, ncalls, W, tau, tau0, ntm, nsamp)
    a, e = tile * syms, min(tile * syms + syms, ncalls)
    B, live, mu = B[a:e], live[a:e], mu[a:e]
    out = np.zeros((e - a, nfilt), dtype=np.complex128)
    if not live.any():
        return out
    lo = int(B[live].min()) - 1
    need = int(B[live].max()) + ntm + 1 - lo + 1
    k = np.arange(ntm, dtype=np.int64)

    def burst(s):
        return np.where((s >= 0) & (s < nsamp), r[np.clip(s, 0, nsamp - 1)], 0.0)

    if need <= region:
        s_r = np.zeros(region, dtype=np.complex128)
        if need < region or not strict:
            staged = need - 1 if short else need
            s_r[:staged] = burst(lo + np.arange(staged, dtype=np.int64))
        at = np.where(live[:, None], (B - 1 - lo)[:, None] + k[None, :], 0)
        xs = [s_r[at + i] for i in range(4)]
    else:
        xs = [burst((B - 1)[:, None] + k[None, :] + i) for i in range(4)]
    c = T.lagrange_host(mu)[:, :, None]
    f = TCM._fma
    xr = f(c[3], xs[3].real, f(c[2], xs[2].real, f(c[1], xs[1].real, c[0] * xs[0].real)))
    xi = f(c[3], xs[3].imag, f(c[2], xs[2].imag, f(c[1], xs[1].imag, c[0] * xs[0].imag)))
    Tn = Tm[np.arange(a, e) % nh]
    zr, zi = np.zeros((e - a, nfilt)), np.zeros((e - a, nfilt))
    for j in range(ntm):
        tr, ti = Tn[:, :, j].real, Tn[:, :, j].imag
        zr = f(xr[:, j, None], tr, f(xi[:, j, None], ti, zr))
        zi = f(-xr[:, j, None], ti, f(xi[:, j, None], tr, zi))
    zr[~live], zi[~live] = 0.0, 0.0
    out.real, out.imag = zr, zi
    return out


def same_bits(got, want):
    """Bit for bit, so that -0 is not +0."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))


def same_bits_off_nan(got, want):
    """The NaNs where the restatement has them (per component), everything else bit for bit."""
    g, w = np.ascontiguousarray(got).view(np.float64), np.ascontiguousarray(want).view(np.float64)
    nan = np.isnan(w)
    return g.shape == w.shape and np.array_equal(np.isnan(g), nan) and np.array_equal(g.view(np.uint64)[~nan], w.view(np.uint64)[~nan])


def all_plus_zero(rows):
    return not np.ascontiguousarray(rows).view(np.uint64).any()


# ---- B1. a later tile at, one under and one over the staged span
BOUNDARY = [(1, 4, 9, 8), (2, 16, 9, 8), (1, 2, 3, 2), (2, 8, 4, 3), (1, 64, 11, 10), (2, 4, 65, 64), (1, 4, 9, 256)]
BOUNDARY_TAU0, BOUNDARY_TILE, BOUNDARY_W = 0.25, 1, 64


@functools.lru_cache(maxsize=None)
def boundary_case(shape, fall):
    """2.5 tiles of rows in windows of 64 under a trajectory that is zero up to the last window centre at or in front of tile
    1's first row and has ONE slope of X samples per window from there to the burst's end, for the three X that put tile 1's need
    at region - 1, region and region + 1.  Rising, tile 1's first row holds the smallest B and its last row the largest; falling
    by more than sps a row (X > 64 sps) the other way round: the whole tile lies on the slope.  Tile 0 is flat in front of the
    knee and tile 2, half a tile on the same slope, stays inside its region.

    Both ends of the tile move with X, so need(X) climbs with a wobble of one: each X is searched on the CPU from the middle of
    the bracket [least X that reaches the wanted need, least X that exceeds it] outwards until need is the wanted value AND the
    two extreme rows' fractions are at least 0.05 from 0 and 1, so that the first and the last sample of the span carry a weight.
    No geometry of the seven needed another construction: the smallest tiles here are 32 rows, half a window, and tile 1 of
    them lies on the slope between the first two centres.  Everything is built once and read-only."""
    nh, nfilt, ntm, sps = shape
    syms, region, _lds = geometry(*shape)
    ncalls, W, tile = 2 * syms + syms // 2, BOUNDARY_W, BOUNDARY_TILE
    nwin = -(-ncalls // W)
    knee = int((tile * syms - 0.5 * (W - 1)) // W)
    assert 0 <= knee < nwin - 1
    sign = -1.0 if fall else 1.0
    far, rows = 1 << 40, slice(tile * syms, tile * syms + syms)

    def trajectory(X):
        return sign * X * np.maximum(np.arange(nwin, dtype=np.float64) - knee, 0.0)

    def need(X):
        return int(tile_needs(far, sps, ncalls, W, trajectory(X), BOUNDARY_TAU0, ntm, 2 * far, syms, region)[2][tile])

    def weighted(X):
        B, _live, mu, _ok = rows_B(far, sps, ncalls, W, trajectory(X), BOUNDARY_TAU0, ntm, 2 * far)
        ends = mu[rows][[int(np.argmin(B[rows])), int(np.argmax(B[rows]))]]
        return bool((np.minimum(ends, 1.0 - ends) >= 0.05).all())

    def least(target):
        lo = 64.0 * sps if fall else 0.0
        assert need(lo) < target
        hi = lo + 64.0
        while need(hi) < target:
            hi = lo + 2.0 * (hi - lo)
        for _ in range(50):
            mid = 0.5 * (lo + hi)
            lo, hi = (lo, mid) if need(mid) >= target else (mid, hi)
        return hi

    def pick(target):
        x0, x1 = least(target), least(target + 1)
        mid, step = 0.5 * (x0 + x1), max(abs(x1 - x0), 1.0 / syms) / 1000.0
        for j in range(4000):
            for X in (mid + j * step, mid - j * step):
                if need(X) == target and weighted(X):
                    return X
        raise AssertionError((shape, fall, target))

    heights = [pick(region + d) for d in (-1, 0, 1)]
    reach = int(math.ceil(max(heights) * (nwin - 1 - knee))) + 1
    start0 = 5 + (reach if fall else 0)
    nsamp = start0 + ncalls * sps + (0 if fall else reach) + ntm + 8
    rng = np.random.default_rng(sum(shape) + 1000 * sps + (500000 if fall else 0))
    r, Tm = _complex(rng, nsamp), _complex(rng, nh, nfilt, ntm)
    runs = tuple((X, trajectory(X)) for X in heights)
    _freeze(r, Tm, *(tau for _X, tau in runs))
    return {"syms": syms, "region": region, "ncalls": ncalls, "W": W, "tile": tile, "start0": start0, "nsamp": nsamp, "r": r, "Tm": Tm,
            "runs": runs}


_RESTATED: dict = {}


def restated(ref, key, *args):
    """tests/cpm_timing_ref.c on a shared case, once: read-only."""
    if key not in _RESTATED:
        _RESTATED[key] = restate(ref, *args)
        _freeze(_RESTATED[key])
    return _RESTATED[key]


def boundary_want(ref, shape, fall, i):
    case = boundary_case(shape, fall)
    _X, tau = case["runs"][i]
    return restated(ref, ("boundary", shape, fall, i), case["r"], case["Tm"], case["start0"], shape[3], case["ncalls"], case["W"], tau, BOUNDARY_TAU0)


# ---- B2. every instantiation
INSTANCES = [(nh, nfilt) for nh in (1, 2) for nfilt in (2, 4, 8, 16, 64)]
NINE_TAP_SPS = [(1, 4, 9, 1), (2, 16, 9, 1), (1, 4, 9, 64), (2, 16, 9, 64), (1, 4, 9, 256), (2, 16, 9, 256)]
CEILING = [(2, 64, 60, 8), (1, 2, 257, 256)]
# per instantiation a shape beyond 48 KiB of LDS (the attribute is set) and one within (it is not): small, LARGE, small
LDS_ORDER = [((1, 2, 3, 2), (1, 2, 257, 256)), ((1, 64, 11, 10), (2, 64, 60, 8)), ((1, 4, 9, 8), (1, 4, 9, 256))]


RAMP_RUNS = [((nh, nfilt, ntm, 8), 300) for nh, nfilt in INSTANCES for ntm in (9, 5)] + [(shape, None) for shape in NINE_TAP_SPS + CEILING]


@functools.lru_cache(maxsize=None)
def ramp_case(shape, ncalls=None):
    """Random samples and templates under the ramp tau_w = 0.3 + (70 / syms + 0.9) w, which climbs by more than one sample per
    tile between the first and the last window centre (in front of the first and behind the last it is flat), with window 2 NaN
    where there are more than three windows: the rows between the centres of windows 1 and 3 are dead.  ``ncalls`` None: two
    tiles and five rows, but at least two windows and five rows -> (r, Tm, start0, ncalls, W, tau, tau0)."""
    nh, nfilt, ntm, sps = shape
    syms, _region, _lds = geometry(*shape)
    ncalls, W = max(2 * syms, 128) + 5 if ncalls is None else ncalls, 64
    nwin = -(-ncalls // W)
    tau = 0.3 + (70.0 / syms + 0.9) * np.arange(nwin)
    if nwin > 3:
        tau[2] = np.nan
    start0 = 3
    rng = np.random.default_rng(7000 + sum(shape) + ncalls)
    r, Tm = _complex(rng, start0 + ncalls * sps + ntm + int(tau[-1]) + 6), _complex(rng, nh, nfilt, ntm)
    _freeze(r, Tm, tau)
    return r, Tm, start0, ncalls, W, tau, -0.375


# ---- B3. a workgroup's successive tiles in every order
WALK_SHAPE, WALK_W, WALK_TAU0, WALK_START0 = (1, 2, 3, 2), 64, 0.3, 8
WALK_NCALLS = 3 * CRS_GRID_CAP * 256 + 1


@functools.lru_cache(maxsize=None)
def walk_case():
    """-> (tau f64[24577], nsamp, kind per tile: 0 LDS, 1 global, 2 dead - by ``tile_kinds``, not by intent).  A tile of 256 rows is
    four windows.  Each tile draws one of three forms: flat at the running level (its rows span 516 samples of the staged 580);
    a step of +300 samples between its second and its third window (616 samples and more even with 32 dead rows at either end: out
    of LDS), the level staying up; all four windows NaN (dead; the level starts again at 0 behind it, and the 32 rows on either
    side of it, which interpolate towards a NaN, are dead rows of live tiles).  A jitter of ±0.3 per window moves the fractions.
    Tile 0 and the last tile, one row, are flat."""
    syms, region, _lds = geometry(*WALK_SHAPE)
    assert (syms, region) == (256, 580)
    ntiles, nwin = 3 * CRS_GRID_CAP + 1, -(-WALK_NCALLS // WALK_W)
    rng = np.random.default_rng(33)
    form = rng.integers(0, 3, ntiles)
    form[0] = form[-1] = 0
    tau, level = np.empty(nwin), 0.0
    for k in range(ntiles):
        w = 4 * k
        if form[k] == 2:
            tau[w:w + 4], level = np.nan, 0.0
        elif form[k] == 1:
            tau[w:w + 2] = level
            level += 300.0
            tau[w + 2:w + 4] = level
        else:
            tau[w:w + 4] = level
    tau += rng.uniform(-0.3, 0.3, nwin)
    nsamp = WALK_START0 + 2 * WALK_NCALLS + int(np.nanmax(tau)) + 16
    kind = tile_kinds(WALK_START0, 2, WALK_NCALLS, WALK_W, tau, WALK_TAU0, 3, nsamp, syms, region)
    _freeze(tau, kind)
    return tau, nsamp, kind


# ---- B4. dead and half-dead rows
DEAD_SHAPE, DEAD_NCALLS, DEAD_TAU0 = (1, 4, 9, 8), 600, 0.25
DEAD_START0 = -(8 * 126 + 10)         # row 126, the last of tile 0, has B + ntm + 1 = 0: the one live row of its tile
DEAD_NSAMP = DEAD_START0 + 8 * DEAD_NCALLS + 30
DEAD_TAU = np.array([np.inf, 0.5, 0.5, 1.9, np.nan, np.inf, -2.2, 0.8, 3.1, -np.inf])
_freeze(DEAD_TAU)
# (start0, nsamp, which row, live) at tau0 in (0.0, 0.5), five calls of sps 8: the first row's B + ntm + 1 = v through -2 .. 1 and
# the last row's B - 1 = nsamp + e through nsamp - 2 .. nsamp + 1
END_BURSTS = [(v - 10, 200, 0, v >= 0) for v in (-2, -1, 0, 1)] + [(3, 34 - e, 4, e < 0) for e in (-2, -1, 0, 1)]
HUGE_TAU0 = float(2 ** 62 - 1024)


@functools.lru_cache(maxsize=None)
def nonfinite_case():
    """(1, 4, 9, 8), 400 calls: tile 0 flat (staged), tile 1 with a step of +150 samples over rows 160 .. 223 (1170 samples against
    the staged 1084: global memory), tiles 2 and 3 flat again -> (r, Tm, start0, tau, the sample in tile 0's span, the one in tile 1's)."""
    rng = np.random.default_rng(77)
    start0, ncalls = 6, 400
    tau = np.array([0.3, 0.3, 0.3, 150.3, 150.3, 150.3, 150.3])
    r, Tm = _complex(rng, start0 + 8 * ncalls + 180), _complex(rng, 1, 4, 9)
    B, _live, _mu, _ok = rows_B(start0, 8, ncalls, 64, tau, 0.0, 9, r.size)
    _freeze(r, Tm, tau)
    return r, Tm, start0, ncalls, tau, int(B[60]) + 4, int(B[200]) + 3


# ---- D. wf_carrier_track_mod on synthetic statistics
PERIODS = [2.0 * math.pi / 16, 2.0 * math.pi / 10]
MOD_GRID = [(1, 1023, 1), (2, 1024, 5), (2, 1025, 5), (4, 2047, 1), (3, 2049, 5), (2, 5000, 101), (2, 3, 5), (1, 1, 1)]
WRAP_MARGIN = 0.25                    # of P/π rad: test_carrier_edges.WRAP_MARGIN in the units of the period


def synthetic_stat_mod(H, nwin, period, seed=0):
    """``test_carrier_edges.synthetic_stat`` with π replaced by ``period``: θ_w = (P/π) (1 + 2π 0.04 w + U(-0.2, 0.2)), a step of
    (P/π) (0.25 ± 0.4) rad, at least 0.92 P/π from ±P/2.  Hypothesis h sees r = θ_w - h P / H reduced into [-P/2, P/2] and
    (X, Y) = -a (cos r, sin r) with a = 100 (1 + cos(π r / P)): the smaller |r|, the lower X, and ψ = h P / H + r = θ modulo P."""
    rng = np.random.default_rng(1000 * H + nwin + seed)
    theta = (period / math.pi) * (1.0 + 2.0 * math.pi * 0.04 * np.arange(nwin) + rng.uniform(-0.2, 0.2, nwin))
    r = theta[None, :] - (np.arange(H, dtype=np.float64) * period / H)[:, None]
    r = r - period * np.round(r / period)
    a = 100.0 * (1.0 + np.cos(math.pi * r / period))
    return theta, np.ascontiguousarray(np.stack([-a * np.cos(r), -a * np.sin(r)], axis=-1))


def wrap_margin_mod(stat, period):
    """(P/2 - the largest |wrapped step| of the host statement at span 1) in units of P/π."""
    u, _choice = C.carrier_track_host(stat, 1, period)
    return (0.5 * period - (float(np.abs(np.diff(u)).max()) if u.size > 1 else 0.0)) * math.pi / period


@functools.lru_cache(maxsize=None)
def mod_grid_case(H, nwin, span, period):
    theta, stat = synthetic_stat_mod(H, nwin, period)
    phase, choice = C.carrier_track_host(stat, span, period)
    _freeze(theta, stat, phase, choice)
    return theta, stat, phase, choice, wrap_margin_mod(stat, period)


@functools.lru_cache(maxsize=None)
def mod_tie_case(period):
    """H = 4, 2049 windows, span 5: on every third window the winning hypothesis m's statistics stand in m - 1 and m + 1 (modulo
    4) as well.  The smallest of the three indices wins, at most one hypothesis from m, so ψ moves by ±P/4 at most on those
    windows and the steps, (P/π) (0.25 ± 0.4 ± π/4), keep 0.13 P/π from ±P/2."""
    _theta, stat = synthetic_stat_mod(4, 2049, period, seed=1)
    stat = stat.copy()
    w = np.arange(0, 2049, 3)
    m = np.argmin(stat[:, w, 0], axis=0)
    stat[(m + 1) % 4, w] = stat[m, w]
    stat[(m + 3) % 4, w] = stat[m, w]
    phase, choice = C.carrier_track_host(stat, 5, period)
    _freeze(stat, phase, choice, m)
    return stat, phase, choice, wrap_margin_mod(stat, period), m


HALF_NWIN = 2100


@functools.lru_cache(maxsize=None)
def half_step_case(period):
    """H = 2, span 1: (X, Y) = (-1, +0) in both hypotheses' slots, and 2^-40 less in X for the one a random bit names.  atan2(-0, +x)
    is -0, so ψ_w = (h_w P) / 2 - 0 is 0 or P/2 exactly and every step is 0, +P/2 or -P/2 exactly."""
    h = np.random.default_rng(5).integers(0, 2, HALF_NWIN)
    stat = np.zeros((2, HALF_NWIN, 2))
    stat[:, :, 0] = -1.0
    stat[h, np.arange(HALF_NWIN), 0] = -1.0 - 2.0 ** -40
    phase, choice = C.carrier_track_host(stat, 1, period)
    _freeze(stat, phase, choice, h)
    return stat, phase, choice, h


header_bound = CE.header_bound         # include/wfhip.h, wf_carrier_track (and _mod): 8 * 2^-52 * max(1, |phase|) * nwin


# ---- E. the compositions at 1, 2, 7, 8 windows and a short last one
WAVEFORMS = ["pcmfm", "multih"]
SHORT_WINDOW, SHORT_LATE, SHORT_SEED = 64, 2.7, 8
TIMING_NCALLS = [60, 128, 448, 512, 512 + 5]
CARRIER_NROWS = [64, 65, 128, 448, 512, 517]
CHOICE_GAP = 2.0 ** -40               # of |X|: what the winning hypothesis must lead by


@pytest.fixture(scope="module")
def short_bursts(oracle, ref):
    """waveform -> (spec, samples 2.7 late, templates, start0, soft, unimpaired rows): one noiseless burst of the reference chain (seed 8)."""
    out = {}
    for waveform in WAVEFORMS:
        spec, sig, _noise, Tm, start0, have = _chain(oracle, waveform, 560, None, seed=SHORT_SEED)
        assert have >= max(TIMING_NCALLS + CARRIER_NROWS)
        bad = T.timing_offset_host(sig, SHORT_LATE, 0.0)
        rows = TCM.cpm_mf_rows_resample_host(sig, Tm, start0, SPS, max(CARRIER_NROWS))[0]
        _freeze(bad, Tm, rows)
        out[waveform] = (spec, bad, Tm, start0, soft_c(ref, spec), rows)
    return out


_TIMING_HOST: dict = {}


def timing_host(short_bursts, waveform, ncalls):
    """(coarse table f64[H, nwin, 2], Σ_w S_w on the plain and on the turned grid, what ``recover_cpm_timing_host`` returns), once."""
    key = (waveform, ncalls)
    if key not in _TIMING_HOST:
        spec, bad, Tm, start0, soft, _rows = short_bursts[waveform]
        lg, W = spec.bits_per_symbol, SHORT_WINDOW

        def stat_at(tau, tau0, rot=None):
            return TCM.llr_stat_host(soft(TCM.cpm_mf_rows_resample_host(bad, Tm, start0, SPS, ncalls, W, tau, tau0)[0], rot), lg, W)

        H = TCM.defaults(spec)["hypotheses"]
        coarse = np.stack([stat_at(None, s) for s in T.hypothesis_instants(float(len(spec.K) * SPS), H)])
        result = TCM.recover_cpm_timing_host(spec, bad, Tm, start0, SPS, ncalls, window=W, soft=soft)
        tau = result[1]
        plain = stat_at(tau, 0.0)[:, 0].sum()
        turned = stat_at(tau, 0.0, CC.hypothesis_table(spec, 0.5 * CC.period(spec)))[:, 0].sum()
        _TIMING_HOST[key] = (coarse, float(plain), float(turned), result)
    return _TIMING_HOST[key]


_CARRIER_HOST: dict = {}


def carrier_host(short_bursts, waveform, nrows):
    """(rows turned by 40 degrees, coarse table f64[2, nwin, 2], smallest gap between the two best T of a call over the coarse
    passes, what ``recover_cpm_host`` returns), once."""
    key = (waveform, nrows)
    if key not in _CARRIER_HOST:
        spec, _bad, _Tm, _start0, _soft, rows = short_bursts[waveform]
        bad = _rot(rows[:nrows], 40.0)
        P, stats, gap = CC.period(spec), [], math.inf
        for h in range(CC.DEFAULT_HYPOTHESES):
            _l, _b, _br, x, y, g = CC.cpm_map_branch_host(spec, bad, 0, CC.hypothesis_table(spec, (float(h) * P) / float(CC.DEFAULT_HYPOTHESES)), margins=True)
            stats.append(CC.carrier_stat_terms_host(x, y, SHORT_WINDOW))
            gap = min(gap, float(g.min()))
        _CARRIER_HOST[key] = (bad, np.stack(stats), gap, CC.recover_cpm_host(spec, bad, window=SHORT_WINDOW))
    return _CARRIER_HOST[key]


def _lead(table):
    """Per window (runner-up - winner) / |winner| of the X column over the hypotheses."""
    xs = np.sort(table[:, :, 0], axis=0)
    return (xs[1] - xs[0]) / np.abs(xs[0])


# ------------------------------------------------------------------------------------------------ CPU
def _defines(path, names):
    src = (CSRC / path).read_text()
    return {name: int(re.search(rf"^#define\s+{name}\s+(\d+)\b", src, re.M).group(1)) for name in names}


def test_kernel_constants_are_the_restated_ones():
    """The boundary cases below sit on the kernel's own thresholds.  A retuned kernel fails here instead of moving them off."""
    want = {"CRS_THREADS": CRS_THREADS, "CRS_EXTRA": CRS_EXTRA, "CRS_GRID_CAP": CRS_GRID_CAP, "CRS_TARGET_SLOTS": CRS_TARGET_SLOTS,
            "CRS_MAX_SLOTS": CRS_MAX_SLOTS, "CRS_MIN_SYMS": CRS_MIN_SYMS}
    assert _defines("wf_cpm_timing.hip", want) == want


def test_llr_stat_constants_are_the_restated_ones():
    """One wave per window, LSTAT_THREADS / 64 windows a block, at most 2^16 blocks: what sizes the second grid-stride step."""
    assert _defines("wf_cpm_timing.hip", ["LSTAT_THREADS"]) == {"LSTAT_THREADS": LSTAT_THREADS}
    src = (CSRC / "wf_cpm_timing.hip").read_text()
    assert re.search(r"wf_grid_for\(nwin, LSTAT_WAVES, 1 << 16\)", src) and re.search(r"#define\s+LSTAT_WAVES\s+\(LSTAT_THREADS / WF_WAVE\)", src)
    assert STAT_NCALLS == 64 * (LSTAT_GRID * (LSTAT_THREADS // 64)) + 65


def test_geometry_restated_is_the_librarys():
    from waveforms_amd import device

    for shape, want in GEOMETRY.items():
        assert geometry(*shape) == want, shape
    shapes = set(GEOMETRY) | set(BOUNDARY) | set(NINE_TAP_SPS) | set(CEILING) | {s for pair in LDS_ORDER for s in pair}
    shapes |= {(nh, nfilt, ntm, 8) for nh, nfilt in INSTANCES for ntm in (9, 5)} | {WALK_SHAPE, DEAD_SHAPE}
    for shape in sorted(shapes):
        syms, region, lds = geometry(*shape)
        assert device.cpm_mf_rows_resample_geometry(*shape) == (syms, CRS_GRID_CAP, lds), shape
        assert region == (syms - 1) * shape[3] + shape[2] + 3 + CRS_EXTRA
    # the tiles the cases below are about: the reduced ones and the two ceilings of LDS
    assert {geometry(*s)[0] for s in BOUNDARY} == {127, 256, 255, 76, 32}
    assert all(geometry(*large)[2] > 48 * 1024 >= geometry(*small)[2] for small, large in LDS_ORDER)


@pytest.mark.parametrize("fall", [False, True])
@pytest.mark.parametrize("shape", BOUNDARY)
def test_boundary_tiles_need_exactly_what_they_claim(shape, fall):
    """Tile 1's need is region - 1, region and region + 1 with every row of the burst live and every sample any row reads inside
    the burst (random, non-zero); the other two tiles are staged; the rows that hold the smallest and the largest B have
    fractions off 0, so c_0 on the span's first sample and c_3 on its last are not 0."""
    case = boundary_case(shape, fall)
    nh, nfilt, ntm, sps = shape
    syms, region, ncalls, W, tile, start0, nsamp = (case[k] for k in ("syms", "region", "ncalls", "W", "tile", "start0", "nsamp"))
    assert tile != 0 and len({X for X, _tau in case["runs"]}) == 3 and case["r"].all() and case["Tm"].all()
    for d, (X, tau) in zip((-1, 0, 1), case["runs"]):
        some, lo, need, fits = tile_needs(start0, sps, ncalls, W, tau, BOUNDARY_TAU0, ntm, nsamp, syms, region)
        B, live, mu, _ok = rows_B(start0, sps, ncalls, W, tau, BOUNDARY_TAU0, ntm, nsamp)
        print(f"{shape} {'fall' if fall else 'rise'} {X:.6f} a window: needs {need.tolist()}, region {region}")
        assert live.all() and B.min() - 1 >= 0 and B.max() + ntm + 1 < nsamp
        assert need.size == 3 and need[tile] == region + d and fits.tolist() == [True, d <= 0, True]
        rows = slice(tile * syms, tile * syms + syms)
        k_min, k_max = rows.start + int(np.argmin(B[rows])), rows.start + int(np.argmax(B[rows]))
        assert (k_min, k_max) == ((rows.stop - 1, rows.start) if fall else (rows.start, rows.stop - 1))
        assert lo[tile] == B[k_min] - 1 and lo[tile] + need[tile] - 1 == B[k_max] + ntm + 1
        c = T.lagrange_host(mu[[k_min, k_max]])
        assert c[0, 0] != 0.0 and c[3, 1] != 0.0 and 0.05 <= mu[k_min] <= 0.95 and 0.05 <= mu[k_max] <= 0.95


@pytest.mark.parametrize("fall", [False, True])
@pytest.mark.parametrize("shape", BOUNDARY)
def test_tile_restatement_and_its_seeded_defects(ref, shape, fall):
    """Phases B and C restated on the staged span alone are tests/cpm_timing_ref.c bit for bit on the boundary tile of every case.
    A staging loop one sample short differs wherever the tile is staged (region - 1, region), and a staging decided by
    need < region differs at need = region and nowhere else: the cases can tell both."""
    case = boundary_case(shape, fall)
    syms, tile = case["syms"], case["tile"]
    rows = slice(tile * syms, tile * syms + syms)
    for i, d in enumerate((-1, 0, 1)):
        _X, tau = case["runs"][i]
        want = boundary_want(ref, shape, fall, i)[rows]
        args = (case["r"], case["Tm"], case["start0"], shape[3], case["ncalls"], case["W"], tau, BOUNDARY_TAU0, tile)
        assert want.all() and same_bits(tile_restatement(*args), want), d
        assert same_bits(tile_restatement(*args, short=True), want) == (d == 1), d
        assert same_bits(tile_restatement(*args, strict=True), want) == (d != 0), d


def test_tile_restatement_on_the_other_tiles_and_on_dead_rows(ref):
    """... and on tiles 0 and 2 of one case, and on every tile of the burst of dead windows (+0 rows included)."""
    case = boundary_case((1, 4, 9, 8), False)
    want = boundary_want(ref, (1, 4, 9, 8), False, 1)
    for tile in (0, 2):
        got = tile_restatement(case["r"], case["Tm"], case["start0"], 8, case["ncalls"], case["W"], case["runs"][1][1], BOUNDARY_TAU0, tile)
        assert same_bits(got, want[tile * 127:tile * 127 + 127]), tile
    r, Tm = dead_burst()
    want = restated(ref, "dead", r, Tm, DEAD_START0, 8, DEAD_NCALLS, 64, DEAD_TAU, DEAD_TAU0)
    for tile in range(5):
        got = tile_restatement(r, Tm, DEAD_START0, 8, DEAD_NCALLS, 64, DEAD_TAU, DEAD_TAU0, tile)
        assert same_bits(got, want[tile * 127:tile * 127 + 127]), tile


@pytest.mark.parametrize("shape,ncalls", RAMP_RUNS)
def test_ramp_crosses_an_integer_in_every_tile(shape, ncalls):
    """At least two tiles, all staged; every live tile of at least 8 rows that lies between the first and
    the last window centre sees ⌊t⌋ change (tiles in front of the first centre and behind the last are flat: 18 .. 33 rows are
    less than half a window); where there are more than three windows, window 2 is dead."""
    r, Tm, start0, ncalls, W, tau, tau0 = ramp_case(shape, ncalls)
    syms, region, _lds = geometry(*shape)
    B, live, _mu, ok = rows_B(start0, shape[3], ncalls, W, tau, tau0, shape[2], r.size)
    fl = B - start0 - np.arange(ncalls) * shape[3]
    some, _lo, need, fits = tile_needs(start0, shape[3], ncalls, W, tau, tau0, shape[2], r.size, syms, region)
    nwin = tau.size
    assert some.size >= 2 and np.array_equal(live, ok) and B[live].min() >= 1 and B[live].max() + shape[2] + 1 < r.size
    crossing = 0
    for t in range(some.size):
        rows = slice(t * syms, min(t * syms + syms, ncalls))
        changes = live[rows].any() and np.unique(fl[rows][live[rows]]).size >= 2
        crossing += bool(changes)
        inside = rows.start >= 32 and rows.stop <= 64 * (nwin - 1) + 32 and live[rows].all() and rows.stop - rows.start >= 8
        assert changes or not inside, (shape, t)
    assert crossing >= 2 and fits[some].all()
    if nwin > 3:
        assert (~live).nonzero()[0].tolist() == list(range(96, 224))


def test_walk_reaches_every_ordered_pair_of_lds_global_and_dead():
    """Workgroup b walks the tiles b, b + 2048 and b + 4096 (workgroup 0 also 6144): every ordered pair of (LDS, global, dead)
    occurs at least 100 times between a workgroup's successive tiles."""
    tau, nsamp, kind = walk_case()
    G = CRS_GRID_CAP
    assert kind.size == 3 * G + 1 and tau.size == 4 * 3 * G + 1 and kind[0] == 0 and kind[-1] == 0
    pairs = list(zip(kind[:G], kind[G:2 * G])) + list(zip(kind[G:2 * G], kind[2 * G:3 * G])) + [(kind[2 * G], kind[3 * G])]
    counts = {(x, y): sum(1 for p in pairs if p == (x, y)) for x in range(3) for y in range(3)}
    print(f"(tile, next tile of the workgroup) over 0 LDS, 1 global, 2 dead: {counts}; tiles of each kind {np.bincount(kind).tolist()}")
    assert min(counts.values()) >= 100, counts
    B, live, _mu, _ok = rows_B(WALK_START0, 2, WALK_NCALLS, WALK_W, tau, WALK_TAU0, 3, nsamp)
    assert B[live].min() >= 2 and B[live].max() + 8 < nsamp and 0.2 < live.mean() < 0.8


def dead_burst():
    rng = np.random.default_rng(66)
    return _complex(rng, DEAD_NSAMP), _complex(rng, 1, 4, 9)


def test_dead_windows_leave_one_live_row_and_a_dead_tile():
    """(1, 4, 9, 8), 600 calls, tiles of 127 rows: tile 0 has ONE live row, its last (B + ntm + 1 = 0: it reads sample 0 alone);
    tile 2 lies between the centres of windows 3 and 6 with windows 4 (NaN) and 5 (+inf) dead, so it is dead as a whole between
    two live tiles; the -inf in the last window kills the rows behind the centre of window 8, and the +inf in the first one
    lies over rows the burst's start has killed already.  The instants there are +inf, -inf and NaN (inf - inf, 0 * inf)."""
    syms, region, _lds = geometry(*DEAD_SHAPE)
    B, live, mu, ok = rows_B(DEAD_START0, 8, DEAD_NCALLS, 64, DEAD_TAU, DEAD_TAU0, 9, DEAD_NSAMP)
    some, _lo, need, fits = tile_needs(DEAD_START0, 8, DEAD_NCALLS, 64, DEAD_TAU, DEAD_TAU0, 9, DEAD_NSAMP, syms, region)
    per_tile = [int(live[t * syms:t * syms + syms].sum()) for t in range(5)]
    print(f"live rows per tile {per_tile}, needs {need.tolist()}")
    assert per_tile == [1, 97, 0, 92, 36] and some.tolist() == [True, True, False, True, True] and fits[some].all()
    assert live[126] and B[126] + 9 + 1 == 0 and mu[126] == 0.75 and need[0] == 12
    assert (~ok).nonzero()[0].tolist() == list(range(96)) + list(range(224, 416)) + list(range(544, 600))
    with np.errstate(invalid="ignore"):
        t = T.instants_host(DEAD_NCALLS, 64, DEAD_TAU, DEAD_TAU0)
    assert np.isposinf(t[:32]).all() and np.isnan(t[32:96]).all() and np.isnan(t[224:416]).all() and np.isneginf(t[544:]).all()


def test_end_bursts_and_huge_instants_on_the_restatement(ref):
    """The two closed ends of the zero-row rule on tests/cpm_timing_ref.c, which has no such rule: a row the rule calls dead comes
    out +0 in both components, a live one non-zero when μ != 0."""
    rng = np.random.default_rng(70)
    r_all, Tm = _complex(rng, 200), _complex(rng, 1, 4, 9)
    for tau0 in (0.0, 0.5):
        for start0, nsamp, row, want_live in END_BURSTS:
            B, live, mu, _ok = rows_B(start0, 8, 5, 64, None, tau0, 9, nsamp)
            assert bool(live[row]) == want_live and mu[row] == tau0 and live.sum() == 4 + want_live
            assert (B[0] + 10 in (-2, -1, 0, 1)) if row == 0 else (B[4] - 1 - nsamp in (-2, -1, 0, 1))
            want = restate(ref, r_all[:nsamp], Tm, start0, 8, 5, 64, None, tau0)
            assert all_plus_zero(want[~live]) and (tau0 == 0.0 or want[live].all())
    for tau0 in (HUGE_TAU0, -HUGE_TAU0):
        _B, live, _mu, ok = rows_B(3, 8, 130, 64, None, tau0, 9, 200)
        assert ok.all() and not live.any() and abs(tau0) < 2.0 ** 62 and all_plus_zero(restate(ref, r_all, Tm, 3, 8, 130, 64, None, tau0))


def test_nonfinite_samples_sit_where_they_should():
    r, Tm, start0, ncalls, tau, s_lds, s_glob = nonfinite_case()
    kind = tile_kinds(start0, 8, ncalls, 64, tau, 0.0, 9, r.size, 127, 1084)
    B, live, _mu, _ok = rows_B(start0, 8, ncalls, 64, tau, 0.0, 9, r.size)
    assert kind.tolist() == [0, 1, 0, 0] and live.all()
    for s, tile in ((s_lds, 0), (s_glob, 1)):
        touched = ((B - 1 <= s) & (s <= B + 10)).nonzero()[0]
        assert touched.size >= 1 and (touched // 127 == tile).all(), (s, touched)


@pytest.mark.parametrize("nwin", [1, 2, 3])
@pytest.mark.parametrize("W", [64, 8192])
def test_window_lookup_rows_either_side_of_a_centre(W, nwin):
    """No row lies ON a centre for even W: the rows next to centre w are half a row either side of it, their τ 1/(2W) of the way
    to the neighbouring entry; the first and the last row take the end entries as they are."""
    tau, tau0 = lookup_tau(nwin), 0.3
    t = T.instants_host(nwin * W, W, tau, tau0)
    assert t[0] == tau0 + tau[0] and t[-1] == tau0 + tau[-1]
    for w in range(nwin):
        below, above = t[w * W + W // 2 - 1], t[w * W + W // 2]
        left = tau[w] if w == 0 else tau[w - 1] + (1.0 - 0.5 / W) * (tau[w] - tau[w - 1])
        right = tau[w] if w == nwin - 1 else tau[w] + (0.5 / W) * (tau[w + 1] - tau[w])
        np.testing.assert_allclose([below, above], [tau0 + left, tau0 + right], rtol=0, atol=1e-12)


def lookup_tau(nwin):
    return np.array([1.7, -2.6, 4.2])[:nwin]


@pytest.mark.parametrize("period", PERIODS)
def test_mod_grid_keeps_clear_of_the_wrap(period):
    """``test_carrier_edges``' preconditions with the period in place of π: every wrapped step at least WRAP_MARGIN P/π from ±P/2,
    ψ on θ modulo P to 1e-9, no two hypotheses tied."""
    for H, nwin, span in MOD_GRID:
        theta, stat, _phase, choice, margin = mod_grid_case(H, nwin, span, period)
        xs = np.sort(stat[:, :, 0], axis=0)
        gap = float((xs[1] - xs[0]).min()) if H > 1 else math.inf
        print(f"P 2π/{round(2 * math.pi / period)}, H {H}, nwin {nwin}: wrap margin {margin:.3f} P/π, smallest gap between the two best X {gap:.3g}")
        assert margin >= WRAP_MARGIN and gap > 0.0
        follow, _c = C.carrier_track_host(stat, 1, period)
        off = follow - theta
        assert np.abs(off - period * np.round(off / period)).max() <= 1e-9
        assert nwin < 100 or len(set(choice.tolist())) == H
    stat, _phase, choice, margin, m = mod_tie_case(period)
    xs = stat[:, :, 0]
    tied = (xs == xs.min(axis=0)).sum(axis=0)
    w = np.arange(0, 2049, 3)
    print(f"ties: {int((tied == 3).sum())} windows with three equal minima, wrap margin {margin:.3f} P/π")
    assert (tied[w] == 3).all() and (tied[1::3] == 1).all() and (tied[2::3] == 1).all() and margin >= 0.1
    assert np.array_equal(choice[w], np.minimum(np.minimum(m, (m + 1) % 4), (m + 3) % 4)) and len(set(m.tolist())) == 4 and (choice[w] != m).sum() > 100


@pytest.mark.parametrize("period", PERIODS)
def test_half_period_steps_are_exact_and_go_up(period):
    stat, phase, choice, h = half_step_case(period)
    half = (1.0 * period) / 2.0
    assert half + half == period and half / period == 0.5
    psi = (choice.astype(np.float64) * period) / 2.0 + np.arctan2(-stat[choice, np.arange(HALF_NWIN), 1], -stat[choice, np.arange(HALF_NWIN), 0])
    raw = np.diff(psi)
    assert np.array_equal(choice, h) and set(np.unique(psi).tolist()) == {0.0, half} and set(np.unique(raw).tolist()) == {-half, 0.0, half}
    print(f"P 2π/{round(2 * math.pi / period)}: {int((raw == half).sum())} steps of exactly +P/2, {int((raw == -half).sum())} of exactly -P/2")
    assert (raw == half).sum() >= 40 and (raw == -half).sum() >= 40
    assert C._wrap(np.array([half, -half]), period).tolist() == [half, half]
    steps = np.diff(phase)
    assert np.array_equal(steps != 0.0, raw != 0.0) and np.abs(steps[raw != 0.0] - half).max() <= 64 * EPS * phase[-1] and phase[0] == 0.0 + psi[0]


@pytest.mark.parametrize("ncalls", TIMING_NCALLS)
@pytest.mark.parametrize("waveform", WAVEFORMS)
def test_short_timing_bursts_leave_no_decision_to_a_rounding(short_bursts, waveform, ncalls):
    """Seed 8, 2.7 samples late, W = 64: in every window of the coarse table the winning hypothesis leads by more than 2^-40 |S|, and
    the two grid totals differ by more than nwin 2^-50 (|plain| + |turned|) (the device adds them in another order)."""
    coarse, plain, turned, (rows, tau, choice, grid) = timing_host(short_bursts, waveform, ncalls)
    nwin = -(-ncalls // SHORT_WINDOW)
    assert nwin == {60: 1, 128: 2, 448: 7, 512: 8, 517: 9}[ncalls] and coarse.shape[1:] == (nwin, 2) and tau.shape == (nwin,)
    lead = _lead(coarse)
    split = abs(plain - turned) / (abs(plain) + abs(turned))
    print(f"{waveform} {ncalls}: smallest lead {lead.min():.3g}, grid {grid}, |plain - turned| / (|plain| + |turned|) = {split:.3g}, tau {np.round(tau, 3).tolist()}")
    assert (lead > CHOICE_GAP).all() and np.array_equal(np.argmin(coarse[:, :, 0], axis=0), choice)
    assert split > nwin * 2.0 ** -50 and grid == (1 if turned < plain else 0)


@pytest.mark.parametrize("nrows", CARRIER_NROWS)
@pytest.mark.parametrize("waveform", WAVEFORMS)
def test_short_carrier_bursts_leave_no_decision_to_a_rounding(short_bursts, waveform, nrows):
    """The same margin on the two hypotheses of the carrier search, and no call of the coarse passes whose two best T lie within
    1e-9 (where the host statement's two roundings could pick another branch than the device's fma)."""
    bad, coarse, gap, (out, phase, choice) = carrier_host(short_bursts, waveform, nrows)
    nwin = -(-nrows // SHORT_WINDOW)
    lead = _lead(coarse)
    print(f"{waveform} {nrows}: smallest lead {lead.min():.3g}, smallest gap between the two best T {gap:.3g}, phase {np.round(phase, 4).tolist()}")
    assert phase.shape == choice.shape == (nwin,) and (lead > CHOICE_GAP).all() and np.array_equal(np.argmin(coarse[:, :, 0], axis=0), choice)
    assert gap >= 1e-9


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture
def ctx():
    from waveforms_amd import _hip

    handle = _hip.new_ctx()
    yield handle
    _hip.free_ctx(handle)


GUARD, SENTINEL = 3, -7.5


def _resample(ctx, d_r, d_T, nfilt, start0, sps, ncalls, W, tau, tau0):
    """The device's rows as complex128[ncalls, nfilt], written between sentinel rows that must stay as they are
    (test_cpm_timing._check_resample's guard)."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    buf = _hip.to_device(np.full((ncalls + 2 * GUARD, nfilt, 2), SENTINEL))
    out = dev.cpm_mf_rows_resample(d_r, d_T, start0, sps, ncalls, W, None if tau is None else _hip.to_device(np.array(tau, dtype=np.float64)), tau0,
                                   out=buf[GUARD:GUARD + ncalls], ctx=ctx)
    assert out.data_ptr() == buf[GUARD:].data_ptr()
    full = _hip.to_host(buf)
    assert (full[:GUARD] == SENTINEL).all() and (full[GUARD + ncalls:] == SENTINEL).all()
    return _hip.to_host(out, True)


def _where(got, want):
    """For a failure message: how many rows differ, the first of them."""
    bad = (np.ascontiguousarray(got).view(np.uint64) != np.ascontiguousarray(want).view(np.uint64)).reshape(got.shape[0], -1).any(axis=1)
    return f"{int(bad.sum())} rows differ, the first at {int(np.argmax(bad))}"


@pytest.mark.gpu
@pytest.mark.parametrize("fall", [False, True])
@pytest.mark.parametrize("shape", BOUNDARY)
def test_cpm_mf_rows_resample_at_the_staged_span(ref, ctx, shape, fall):
    """need = region - 1 and region: tile 1 is staged, to its last slot; region + 1: it reads global memory.  Bit for bit
    tests/cpm_timing_ref.c."""
    from waveforms_amd import _hip

    case = boundary_case(shape, fall)
    d_r, d_T = _hip.to_device(np.array(case["r"])), _hip.to_device(np.array(case["Tm"]))
    for i, d in enumerate((-1, 0, 1)):
        _X, tau = case["runs"][i]
        want = boundary_want(ref, shape, fall, i)
        got = _resample(ctx, d_r, d_T, shape[1], case["start0"], shape[3], case["ncalls"], case["W"], tau, BOUNDARY_TAU0)
        assert want.all() and same_bits(got, want), (d, _where(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("nh,nfilt", INSTANCES)
def test_cpm_mf_rows_resample_every_instantiation(ref, ctx, nh, nfilt):
    """<NF, 9> and <NF, 0> at both nh: sps 8, 300 calls, random templates, a ramp that crosses an integer in every tile and a NaN window."""
    from waveforms_amd import _hip

    for ntm in (9, 5):
        r, Tm, start0, ncalls, W, tau, tau0 = ramp_case((nh, nfilt, ntm, 8), 300)
        want = restate(ref, r, Tm, start0, 8, ncalls, W, tau, tau0)
        got = _resample(ctx, _hip.to_device(np.array(r)), _hip.to_device(np.array(Tm)), nfilt, start0, 8, ncalls, W, tau, tau0)
        assert same_bits(got, want), (ntm, _where(got, want))
        assert all_plus_zero(got[96:224]) and got[:96].all() and got[224:].all()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", NINE_TAP_SPS + CEILING)
def test_cpm_mf_rows_resample_other_sps_and_the_lds_ceiling(ref, ctx, shape):
    """The nine-tap register path at sps 1, 64 (33-row tiles) and 256 (the 32-row fallback tile in 134 080 B) with one and two
    template columns, and the two shapes next to the 156 KiB ceiling: two tiles and five rows each."""
    from waveforms_amd import _hip

    r, Tm, start0, ncalls, W, tau, tau0 = ramp_case(shape)
    want = restate(ref, r, Tm, start0, shape[3], ncalls, W, tau, tau0)
    got = _resample(ctx, _hip.to_device(np.array(r)), _hip.to_device(np.array(Tm)), shape[1], start0, shape[3], ncalls, W, tau, tau0)
    assert want.any() and same_bits(got, want), _where(got, want)


@pytest.mark.gpu
def test_cpm_mf_rows_resample_small_lds_after_and_before_large(ref, ctx):
    """One instantiation with a tile within 48 KiB, then one beyond it (the launch raises the kernel's dynamic-LDS limit), then
    the small one again: <2, 0>, <64, 0> and <4, 9>."""
    from waveforms_amd import _hip

    for small, large in LDS_ORDER:
        for shape in (small, large, small):
            r, Tm, start0, ncalls, W, tau, tau0 = ramp_case(shape)
            want = restated(ref, ("ramp", shape), r, Tm, start0, shape[3], ncalls, W, tau, tau0)
            got = _resample(ctx, _hip.to_device(np.array(r)), _hip.to_device(np.array(Tm)), shape[1], start0, shape[3], ncalls, W, tau, tau0)
            assert same_bits(got, want), (shape, _where(got, want))


@pytest.mark.gpu
def test_cpm_mf_rows_resample_successive_tiles_in_every_order(ref, ctx):
    """1 572 865 rows of two filters of three taps at sps 2: every workgroup walks three tiles and workgroup 0 a fourth, over LDS
    that holds the previous trip's span, rows and instants (the CPU test counts the orders).  The whole output, bit for bit."""
    from waveforms_amd import _hip

    torch = _hip.torch()
    tau, nsamp, kind = walk_case()
    rng = np.random.default_rng(34)
    r, Tm = _complex(rng, nsamp), _complex(rng, 1, 2, 3)
    want = restate(ref, r, Tm, WALK_START0, 2, WALK_NCALLS, WALK_W, tau, WALK_TAU0)
    d_r = _hip.to_device(r)
    try:
        got = _resample(ctx, d_r, _hip.to_device(Tm), 2, WALK_START0, 2, WALK_NCALLS, WALK_W, tau, WALK_TAU0)
    finally:
        del d_r
        torch.cuda.empty_cache()
    if not same_bits(got, want):
        bad = (got.view(np.uint64) != want.view(np.uint64)).reshape(WALK_NCALLS, -1).any(axis=1)
        row = int(np.argmax(bad))
        tile = row // 256
        raise AssertionError(f"{int(bad.sum())} rows differ, the first at {row}: tile {tile} (workgroup {tile % CRS_GRID_CAP}, its trip "
                             f"{tile // CRS_GRID_CAP}, kind {int(kind[tile])} after {int(kind[tile - CRS_GRID_CAP]) if tile >= CRS_GRID_CAP else None})")
    dead = np.repeat(kind == 2, 256)[:WALK_NCALLS]
    assert all_plus_zero(got[dead]) and got[~dead].any()


@pytest.mark.gpu
def test_cpm_mf_rows_resample_dead_and_half_dead_rows(ref, ctx):
    """The burst of NaN, +inf and -inf windows (one live row in tile 0, tile 2 dead between live tiles); five-call bursts whose
    first and last rows step across the two closed ends of the zero-row rule at μ = 0 and 1/2; tau0 = ±(2^62 - 1024) and -0."""
    from waveforms_amd import _hip

    r, Tm = dead_burst()
    d_T = _hip.to_device(Tm)
    want = restated(ref, "dead", r, Tm, DEAD_START0, 8, DEAD_NCALLS, 64, DEAD_TAU, DEAD_TAU0)
    got = _resample(ctx, _hip.to_device(r), d_T, 4, DEAD_START0, 8, DEAD_NCALLS, 64, DEAD_TAU, DEAD_TAU0)
    _B, live, _mu, _ok = rows_B(DEAD_START0, 8, DEAD_NCALLS, 64, DEAD_TAU, DEAD_TAU0, 9, DEAD_NSAMP)
    assert same_bits(got, want), _where(got, want)
    assert all_plus_zero(got[~live]) and got[live].all() and live[126] and not live[:126].any()
    rng = np.random.default_rng(70)
    r_all, Tm = _complex(rng, 200), _complex(rng, 1, 4, 9)
    d_T = _hip.to_device(Tm)
    for tau0 in (0.0, 0.5):
        for start0, nsamp, row, want_live in END_BURSTS:
            _B, live, _mu, _ok = rows_B(start0, 8, 5, 64, None, tau0, 9, nsamp)
            want = restate(ref, r_all[:nsamp], Tm, start0, 8, 5, 64, None, tau0)
            got = _resample(ctx, _hip.to_device(r_all[:nsamp]), d_T, 4, start0, 8, 5, 64, None, tau0)
            assert same_bits(got, want), (tau0, start0, nsamp, got[row], want[row])
            assert all_plus_zero(got[~live]) and bool(live[row]) == want_live and (tau0 == 0.0 or got[live].all())
    d_r = _hip.to_device(r_all)
    for tau0 in (HUGE_TAU0, -HUGE_TAU0):
        assert all_plus_zero(_resample(ctx, d_r, d_T, 4, 3, 8, 130, 64, None, tau0)), tau0
        got = _resample(ctx, d_r, d_T, 4, 3, 8, 130, 64, np.array([tau0, 0.0]), 0.0)   # ... as a trajectory's entry, and on the way down from it
        assert all_plus_zero(got[:32]) and same_bits(got, restate(ref, r_all, Tm, 3, 8, 130, 64, np.array([tau0, 0.0]), 0.0)), tau0
    got = _resample(ctx, d_r, d_T, 4, 3, 8, 20, 64, None, -0.0)
    assert same_bits(got, restate(ref, r_all, Tm, 3, 8, 20, 64, None, -0.0)) and same_bits(got, _resample(ctx, d_r, d_T, 4, 3, 8, 20, 64, None, 0.0)) and got.all()


@pytest.mark.gpu
@pytest.mark.parametrize("first", ["inf", "nan"])
def test_cpm_mf_rows_resample_nonfinite_samples(ref, ctx, first):
    """A sample of +inf (real part) and one of NaN, one in the staged tile 0 and one in tile 1, which reads global memory (and the
    other way round): the rows whose footprints miss them are those of the clean run bit for bit, the others have their NaNs
    where tests/cpm_timing_ref.c has them and are bitwise its values elsewhere (0 weights times inf included)."""
    from waveforms_amd import _hip

    r, Tm, start0, ncalls, tau, s_lds, s_glob = nonfinite_case()
    d_T = _hip.to_device(np.array(Tm))
    clean = _resample(ctx, _hip.to_device(np.array(r)), d_T, 4, start0, 8, ncalls, 64, tau, 0.0)
    assert same_bits(clean, restate(ref, r, Tm, start0, 8, ncalls, 64, tau, 0.0))
    bad = np.array(r)
    values = (complex(np.inf, 1.5), complex(np.nan, -0.5))
    bad[s_lds], bad[s_glob] = values if first == "inf" else values[::-1]
    want = restate(ref, bad, Tm, start0, 8, ncalls, 64, tau, 0.0)
    got = _resample(ctx, _hip.to_device(bad), d_T, 4, start0, 8, ncalls, 64, tau, 0.0)
    B, _live, _mu, _ok = rows_B(start0, 8, ncalls, 64, tau, 0.0, 9, r.size)
    touched = ((B - 1 <= s_lds) & (s_lds <= B + 10)) | ((B - 1 <= s_glob) & (s_glob <= B + 10))
    assert same_bits(got[~touched], clean[~touched]) and same_bits_off_nan(got, want), _where(got, want)
    finite = np.isfinite(want.view(np.float64)).reshape(ncalls, -1)
    assert not finite[touched].all(axis=1).any() and finite[~touched].all() and np.isnan(want.view(np.float64)).any() and touched.sum() >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("nwin", [1, 2, 3])
@pytest.mark.parametrize("W", [64, 8192])
def test_cpm_mf_rows_resample_window_lookup(ref, ctx, W, nwin):
    """The inlined ``timing_tau_at`` from this kernel: a trajectory of 1, 2 and 3 entries over nwin W rows, the whole output bit
    for bit (the rows next to every centre and the burst's first and last row among them), and with more entries than windows."""
    from waveforms_amd import _hip

    rng = np.random.default_rng(50 + nwin)
    ncalls, start0 = nwin * W, 12
    r, Tm = _complex(rng, start0 + 8 * ncalls + 40), _complex(rng, 1, 4, 9)
    d_r, d_T = _hip.to_device(r), _hip.to_device(Tm)
    tau = lookup_tau(nwin)
    want = restate(ref, r, Tm, start0, 8, ncalls, W, tau, 0.3)
    got = _resample(ctx, d_r, d_T, 4, start0, 8, ncalls, W, tau, 0.3)
    assert want.all() and same_bits(got, want), _where(got, want)
    more = np.concatenate([tau, [9.5, -7.25]])
    short = ncalls - W // 2                                       # ends half a row in front of the last centre: the two further entries are not read
    want = restate(ref, r, Tm, start0, 8, short, W, more, 0.3)
    got = _resample(ctx, d_r, d_T, 4, start0, 8, short, W, more, 0.3)
    assert same_bits(got, want) and same_bits(got, _resample(ctx, d_r, d_T, 4, start0, 8, short, W, tau, 0.3)), _where(got, want)


STAT_NCALLS = 64 * (65536 * 4) + 65


@pytest.mark.gpu
def test_llr_stat_takes_a_second_grid_stride_step(ctx):
    """262 146 windows of 64 values on 65 536 blocks of four waves: the last two windows are a second trip, the last one holds
    one value.  Bit for bit ``llr_stat_host`` on the host copy of values drawn on the device."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    torch = _hip.torch()
    nwin = -(-STAT_NCALLS // 64)
    assert nwin == LSTAT_GRID * (LSTAT_THREADS // 64) + 2
    lam = torch.randn(STAT_NCALLS, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(13)) * 10.0
    buf = _hip.to_device(np.full((nwin + 2, 2), SENTINEL))
    try:
        got = _hip.to_host(dev.llr_stat(lam, 1, 64, out=buf[1:-1], ctx=ctx))
        want = TCM.llr_stat_host(_hip.to_host(lam), 1, 64)
    finally:
        del lam
        torch.cuda.empty_cache()
    full = _hip.to_host(buf)
    assert (full[0] == SENTINEL).all() and (full[-1] == SENTINEL).all()
    assert same_bits(got, want), int(np.argmax((got != want).any(axis=1)))
    assert (want[:, 0] < 0).all() and all_plus_zero(got[:, 1])


@pytest.mark.gpu
def test_llr_stat_nonfinite_values(ctx):
    """bits_per_call 8 at W = 8192, the largest window (65 536 values a wave): +inf gives -inf, +inf and -inf give -inf (|λ| comes
    before the sum), a NaN gives the host statement's NaN and leaves the other windows alone."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    rng = np.random.default_rng(14)
    ncalls = 2 * 8192 + 5
    lam = rng.standard_normal(ncalls * 8) * 10.0
    lam[12345] = np.inf
    lam[65536 + 777], lam[65536 + 60000] = np.inf, -np.inf
    want = TCM.llr_stat_host(lam, 8, 8192)
    got = _hip.to_host(dev.llr_stat(_hip.to_device(lam), 8, 8192, ctx=ctx))
    assert want[:, 0].tolist()[:2] == [-np.inf, -np.inf] and np.isfinite(want[2, 0]) and same_bits(got, want)
    lam[2 * 65536 + 3] = np.nan
    lam[777] = -np.inf
    want = TCM.llr_stat_host(lam, 8, 8192)
    buf = _hip.to_device(np.full((3 + 2, 2), SENTINEL))
    got = _hip.to_host(dev.llr_stat(_hip.to_device(lam), 8, 8192, out=buf[1:-1], ctx=ctx))
    full = _hip.to_host(buf)
    assert (full[0] == SENTINEL).all() and (full[-1] == SENTINEL).all()
    assert np.isnan(want[:, 0]).tolist() == [False, False, True] and same_bits_off_nan(got, want) and all_plus_zero(got[:, 1])


def _track(stat, span, period, ctx):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    phase, choice = dev.carrier_track(_hip.to_device(np.array(stat, dtype=np.float64)), span, ctx=ctx, period=period)      # a copy: the shared inputs are read-only
    return _hip.to_host(phase), _hip.to_host(choice)


@pytest.mark.gpu
@pytest.mark.parametrize("period", PERIODS)
@pytest.mark.parametrize("H,nwin,span", MOD_GRID)
def test_carrier_track_mod_on_the_segment_grid(ctx, H, nwin, span, period):
    """phase within the header's bound of the host statement, choice equal.  The CPU test above holds the preconditions."""
    _theta, stat, want, want_choice, margin = mod_grid_case(H, nwin, span, period)
    assert margin >= WRAP_MARGIN
    phase, choice = _track(stat, span, period, ctx)
    assert phase.shape == want.shape and choice.shape == want_choice.shape and choice.dtype == np.uint8
    ratio = np.abs(phase - want) / header_bound(want)
    print(f"P 2π/{round(2 * math.pi / period)}, H {H}, nwin {nwin}, span {span}: max |device - host| / bound = {ratio.max():.3g}")
    assert np.array_equal(choice, want_choice), int(np.count_nonzero(choice != want_choice))
    assert (ratio <= 1.0).all(), (ratio.max(), int(np.argmax(ratio)))


@pytest.mark.gpu
@pytest.mark.parametrize("period", PERIODS)
def test_carrier_track_mod_ties_and_half_period_steps(ctx, period):
    """Three equal minima: the smallest index.  Steps of exactly ±P/2: both taken as +P/2, through a division by a period that
    is not π; the unwrapped trajectory rises by P/2 at every step and never falls."""
    stat, want, want_choice, margin, _m = mod_tie_case(period)
    assert margin >= 0.1
    phase, choice = _track(stat, 5, period, ctx)
    ratio = np.abs(phase - want) / header_bound(want)
    print(f"P 2π/{round(2 * math.pi / period)} ties: max |device - host| / bound = {ratio.max():.3g}")
    assert np.array_equal(choice, want_choice), int(np.count_nonzero(choice != want_choice))
    assert (ratio <= 1.0).all(), ratio.max()
    stat, want, want_choice, _h = half_step_case(period)
    phase, choice = _track(stat, 1, period, ctx)
    ratio = np.abs(phase - want) / header_bound(want)
    steps = np.diff(phase)
    print(f"P 2π/{round(2 * math.pi / period)} half steps: max |device - host| / bound = {ratio.max():.3g}, smallest device step {steps.min():.3g}")
    assert np.array_equal(choice, want_choice)
    assert (ratio <= 1.0).all(), ratio.max()
    stepping = np.diff(want) != 0.0
    assert steps.min() >= 0.0 and not steps[~stepping].any() and np.abs(steps[stepping] - 0.5 * period).max() <= 2.0 * header_bound(want).max()


@pytest.mark.gpu
@pytest.mark.parametrize("ncalls", TIMING_NCALLS)
@pytest.mark.parametrize("waveform", WAVEFORMS)
def test_cpm_timing_recover_at_one_two_seven_eight_and_nine_windows(short_bursts, ctx, waveform, ncalls):
    """``CPMTimingRecovery.recover`` restates ``rescale_host`` as tensor operations: skipped at one window, anchored at
    (0, nwin - 1) below eight and at (2, nwin - 3) from eight on; 517 calls end in a window of five."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    spec, bad, Tm, start0, soft, _rows = short_bursts[waveform]
    _coarse, _plain, _turned, (host_rows, host_tau, host_choice, host_grid) = timing_host(short_bursts, waveform, ncalls)
    rec = TCM.CPMTimingRecovery(spec, SPS, window=SHORT_WINDOW)
    rows, tau, choice, grid = rec.recover(_hip.to_device(np.array(bad)), _hip.to_device(np.array(Tm)), start0, ncalls, ctx=ctx)
    got = _hip.to_host(tau)
    err = np.abs(got - host_tau).max()
    print(f"{waveform} {ncalls}: {got.size} windows, max |device tau - host tau| = {err:.3g} samples (/ 1e-9 = {err / 1e-9:.3g}), grid {host_grid}")
    assert np.array_equal(_hip.to_host(choice), host_choice) and int(grid.cpu()) == host_grid
    assert got.shape == host_tau.shape and err < 1e-9
    assert np.array_equal(_hip.to_host(dev.cpm_soft(rows, spec, ctx=ctx)[1]).astype(bool), soft(host_rows) < 0)


@pytest.mark.gpu
@pytest.mark.parametrize("nrows", CARRIER_NROWS)
@pytest.mark.parametrize("waveform", WAVEFORMS)
def test_cpm_carrier_recover_at_one_two_seven_eight_and_nine_windows(short_bursts, ctx, waveform, nrows):
    """``CPMCarrierRecovery.recover`` at W = 64 on 64 .. 517 rows turned by 40 degrees: choice exact, phase within the tracker's
    bound of ``recover_cpm_host``, the decisions after the recovery the host's."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    spec, _bad, _Tm, _start0, soft, _rows = short_bursts[waveform]
    bad, _coarse, _gap, (host_out, host_phase, host_choice) = carrier_host(short_bursts, waveform, nrows)
    rec = CC.CPMCarrierRecovery(spec, window=SHORT_WINDOW)
    out, phase, choice = rec.recover(_hip.to_device(bad), ctx=ctx)
    ratio = np.abs(_hip.to_host(phase) - host_phase) / header_bound(host_phase)
    print(f"{waveform} {nrows}: {host_phase.size} windows, max |device - host| / bound = {ratio.max():.3g}")
    assert np.array_equal(_hip.to_host(choice), host_choice)
    assert (ratio <= 1.0).all(), ratio.max()
    assert np.array_equal(_hip.to_host(dev.cpm_soft(out, spec, ctx=ctx)[1]).astype(bool), soft(host_out) < 0)
