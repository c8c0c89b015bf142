"""The timing stages at the tile, segment and wrap edges that tests/test_timing.py does not reach (include/wfhip.h:
wf_timing_offset_c128, wf_mf_bank_resample_c128, wf_timing_track, wf_timing_refine).

``mf_resample_kernel`` walks tiles of ``ob`` rows and keeps a tile in LDS iff the span of samples its rows read, ``need``, is at
most the staged ``region``; here a tile sits at need = region - 1, region and region + 1 for every launch geometry (padded and
unpadded windows, the reduced tiles of 224, 32 and 16 rows), rising and falling; workgroups walk a second and a third tile in
every order of LDS and global memory; a row takes every integer instant across the burst's two ends; and the window lookup
runs with windows that are no multiple of a tile, with the longest window, and with trajectories shorter and longer than the
burst.  ``timing_track_kernel`` is one workgroup of 1024 threads with the blocked scan of ``carrier_track_kernel``: it is fed
1023 .. 5000 windows, tables whose ψ is exact so that steps of exactly half a period occur (wrap is closed at the top), exact
ties between neighbouring hypotheses, and a window of NaNs.  ``timing_offset_kernel`` runs at 2^24 + 3 elements, the first
size at which its grid-stride loop takes a second step, and ``TimingRecovery.recover`` at 1, 2, 7 and 8 windows.

CPU: the launch geometry restated and pinned to the kernel's constants, and the preconditions that make the device
comparisons sound (exact ``need`` values, transition counts, wrap margins, counts of half-period steps, a seeded defect of the
blocked scan).  GPU: the device against the host statements of waveforms_amd/sync/timing.py within the header's bounds.
"""
import functools
import math
import re
from pathlib import Path

import numpy as np
import pytest

from test_timing import SPS, U, _chain, _track_bound
from waveforms_amd.sync import carrier as C
from waveforms_amd.sync import timing as T

# ---- the launch geometry of wf_mf_bank_resample_c128, restated (test_kernel_constants_are_the_restated_ones pins it)
RS_THREADS, RS_LDS_SLOTS, RS_EXTRA, RS_MAX_TAPS, TTRACK_THREADS = 256, 3072, 64, 255, 1024
RS_GRID = 4096                        # workgroups launched at most: tile b + 4096 is workgroup b's second tile
GEOMETRY = {(8, 9): (256, 2116), (8, 73): (256, 2180), (1, 255): (256, 577), (3, 129): (256, 961), (10, 91): (224, 2388),
            (64, 9): (32, 2060), (64, 255): (16, 1282), (7, 255): (256, 2107)}


def geometry(step, ntaps):
    """(ob, region) as the host side of wf_mf_bank_resample_c128 chooses them."""
    pad = step % 2 == 0
    ob = RS_THREADS
    while True:
        region = (ob - 1) * step + ntaps + 3 + RS_EXTRA
        slots = region + (region // step + 1 if pad else 0)
        if slots + 3 * ntaps <= RS_LDS_SLOTS:
            return ob, region
        assert ob > 1
        ob = ob - 16 if ob > 16 else ob - 1


def tile_B(first, step, ncols, W, tau, tau0, nsamp=None):
    """(B_k, live_k) of every row as the kernel forms them: live iff the instant is usable and one of the four nodes can lie in
    the burst (nsamp None: every usable row)."""
    ok, fl, _mu = T._split(T.instants_host(ncols, W, tau, tau0))
    B = int(first) + np.arange(int(ncols), dtype=np.int64) * int(step) + fl
    return B, (ok if nsamp is None else ok & (B + 2 >= 0) & (B - 1 < nsamp))


def tile_needs(first, step, ncols, W, tau, tau0, ntaps, ob, nsamp=None):
    """need = max B - min B + 2 c + 4 over the live rows of every tile of ``ob`` rows (0 for a tile without one): the number of
    samples from the first one any row of the tile reads, B - 1 - c, to the last one, B + 2 + c."""
    B, live = tile_B(first, step, ncols, W, tau, tau0, nsamp)
    starts = np.arange(0, int(ncols), int(ob))
    big = np.iinfo(np.int64).max
    mn = np.minimum.reduceat(np.where(live, B, big), starts)
    mx = np.maximum.reduceat(np.where(live, B, -big), starts)
    return np.where(mn <= mx, mx - mn + (ntaps - 1) + 4, 0)


def _rows_error(got, want):
    return np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag))


def _complex(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


# ---- 1. a tile at, one under and one over the staged span
BOUNDARY = [(8, 9), (8, 73), (1, 255), (3, 129), (10, 91), (64, 9), (64, 255)]
BOUNDARY_TAU0 = 0.25


@functools.lru_cache(maxsize=None)
def boundary_case(step, ntaps, fall):
    """ncols = 2.5 ob rows in windows of 64 under a trajectory that is zero except for one final slope of height X, for the
    three X that put the boundary tile's need at region - 1, region and region + 1.

    The slope lies between two window centres, 64 rows apart.  Tiles of 224 and 256 rows: tau = [0, 0, 0, X] rises over rows
    160 .. 223 of tile 0, whose first row then holds the smallest B and whose last row the largest.  Mirrored, X < 0 beyond
    the fall that turns the rows' order round: the largest B is row 159's, the last one in front of the slope, and the smallest
    that of the row at the slope's foot (223 or 224; the rows in front of the first window centre, 31.5, and behind the last
    one take the end values, so B climbs again by ``step`` per row there, and a slope one window later would put tile 1 on the
    same boundary).  The reduced tiles (32 and 16 rows) are shorter than half a window and tile 0 lies in front of the first
    centre: it cannot see a slope at any W >= 64.  There tau = [0, X] and the boundary tile is the first one on the slope, tile
    1 of 32 rows and tile 2 of 16 (ncols = 40: its 8 rows); rising, its first row holds the smallest B and its last row the
    largest, and falling the other way round.

    From the bracket's lower end on (rising: 0; falling: 64 step, where the slope's rows share one B) need lies under the wanted
    values until it reaches them and does not come back; each X is the middle between the least |X| that reaches the wanted need and the least that exceeds it (bisection),
    so that the extreme rows' fractions are not 0 and their outermost weights count.  Everything is built once and read-only."""
    ob, region = geometry(step, ntaps)
    ncols, W, c = 2 * ob + ob // 2, 64, (ntaps - 1) // 2
    if ob >= 224:
        zeros, tile = 3, 0
    else:
        zeros, tile = 1, 32 // ob
    sign = -1.0 if fall else 1.0

    def trajectory(X):
        return np.array([0.0] * zeros + [sign * X])

    def need(X):
        return int(tile_needs(0, step, ncols, W, trajectory(X), BOUNDARY_TAU0, ntaps, ob)[tile])

    def least(target):
        lo = 64.0 * step if fall else 0.0
        assert need(lo) < target
        hi = lo + 64.0
        while need(hi) < target:
            hi = lo + 2.0 * (hi - lo)
        for _ in range(50):
            mid = 0.5 * (lo + hi)
            lo, hi = (lo, mid) if need(mid) >= target else (mid, hi)
        return hi

    heights = [0.5 * (least(region + d) + least(region + d + 1)) for d in (-1, 0, 1)]
    reach = int(math.ceil(max(heights))) + 1
    first = 5 + (reach if fall else 0)
    nsamp = first + ncols * step + (0 if fall else reach) + c + 8
    rng = np.random.default_rng(1000 * step + ntaps + (500000 if fall else 0))
    r, taps = _complex(rng, nsamp), _complex(rng, 3, ntaps)
    runs = []
    for X in heights:
        tau = trajectory(X)
        want, mag = T.mf_bank_resample_host(r, taps, first, step, ncols, W, tau, BOUNDARY_TAU0)
        _freeze(tau, want, mag)
        runs.append((X, tau, want, mag))
    _freeze(r, taps)
    return {"ob": ob, "region": region, "ncols": ncols, "W": W, "c": c, "tile": tile, "first": first, "nsamp": nsamp, "r": r, "taps": taps,
            "runs": tuple(runs)}


# ---- 2. a workgroup's later tiles
WALK_STEP, WALK_NTAPS, WALK_W, WALK_NCOLS, WALK_TAU0 = 1, 9, 256, 2 * RS_GRID * 256 + 300, 0.3


@functools.lru_cache(maxsize=None)
def walk_case():
    """-> (tau f64[8194], first, nsamp, fits bool[8194]).  A random walk over the windows: steps of U(-3, 3), a third of them
    ±200 instead.  A window is a tile long, so a tile sees half of the step into its window and half of the step out of it:
    +100 samples on top of its 255 leave the staged 331, -100 only crowd its rows.  The steps around workgroup 1's three tiles
    and around the third tiles are set: tile 1 small steps, tile 4097 +200, tile 8192 (workgroup 0's third) half of +200, tile
    8193 (44 rows, workgroup 1's third) a small step."""
    rng = np.random.default_rng(31)
    nwin = -(-WALK_NCOLS // WALK_W)
    steps = rng.uniform(-3.0, 3.0, nwin)
    jump = rng.random(nwin) < 1.0 / 3.0
    steps[jump] = np.where(rng.random(nwin) < 0.5, -200.0, 200.0)[jump]
    steps[0], steps[1], steps[2], steps[RS_GRID + 1] = 0.0, 1.0, -2.0, 200.0
    steps[2 * RS_GRID], steps[2 * RS_GRID + 1] = 200.0, 1.5
    tau = np.cumsum(steps)
    first = int(-tau.min()) + 20
    nsamp = first + WALK_NCOLS + int(tau.max()) + 20
    ob, region = geometry(WALK_STEP, WALK_NTAPS)
    fits = tile_needs(first, WALK_STEP, WALK_NCOLS, WALK_W, tau, WALK_TAU0, WALK_NTAPS, ob, nsamp) <= region
    _freeze(tau, fits)
    return tau, first, nsamp, fits


# ---- 4. the tracker's segment grid
# (H, nwin, span): around one and two windows per segment, clipped segments (2049: seg = 3, the last 341 threads own nothing),
# a span wider than the burst, H = 5, and the two smallest bursts
GRID = [(3, 1023, 1), (8, 1024, 5), (8, 1025, 5), (5, 2047, 1), (3, 2049, 5), (8, 5000, 101), (64, 1500, 3001), (8, 3, 5), (3, 1, 1)]
PERIOD = 16.0
WRAP_MARGIN = 1.0                     # samples: the least distance of a wrapped step from ±8 the comparisons below rely on


@functools.lru_cache(maxsize=None)
def grid_case(H, nwin, span):
    """One grid entry, computed once: (true, stat, host tau, host choice, host tau at span 1).  Exact parabolas about a
    drifting instant: true_w = 3 - 1.6 w + U(-0.4, 0.4), X_{h,w} = wrap(s_h - true_w)^2 - 8000, Y = 0."""
    rng = np.random.default_rng(1000 * H + nwin)
    true = 3.0 - 1.6 * np.arange(nwin) + rng.uniform(-0.4, 0.4, nwin)
    stat = np.zeros((H, nwin, 2))
    stat[:, :, 0] = C._wrap(T.hypothesis_instants(PERIOD, H)[:, None] - true[None, :], PERIOD) ** 2 - 8000.0
    tau, choice = T.timing_track_host(stat, PERIOD, span)
    one, _c = T.timing_track_host(stat, PERIOD, 1)
    _freeze(true, stat, tau, choice, one)
    return true, stat, tau, choice, one


def blocked_scan_restatement(stat, period, span, advance_prev=True):
    """``timing_track_host`` with the running sum u taken as the kernel's blocked scan: seg = ceil(nwin / 1024), segment
    t = [min(t seg, nwin), min(t seg + seg, nwin)); each segment adds its own wrapped steps from +0 (the first one starts with
    ψ_0), the 1024 segment sums are added in order into offsets, and u_w = offset + running sum; then the centred mean.
    ``advance_prev=False`` seeds the defect the grid must catch: the previous ψ is not advanced inside a segment."""
    X = np.asarray(stat, dtype=np.float64)[:, :, 0]
    H, nwin = X.shape
    choice = np.argmin(X, axis=0)
    w = np.arange(nwin)
    dh = period / float(H)
    psi = (choice.astype(np.float64) * dh - 0.5 * period) + dh * T.vertex_host(X[(choice - 1) % H, w], X[choice, w], X[(choice + 1) % H, w], 0.5)
    seg = -(-nwin // TTRACK_THREADS)
    sums, run = np.zeros(TTRACK_THREADS), np.empty(nwin)
    for t in range(TTRACK_THREADS):
        a = min(t * seg, nwin)
        e = min(a + seg, nwin)
        s, prev = 0.0, (psi[a - 1] if 0 < a < nwin else 0.0)
        for j in range(a, e):
            s += psi[j] if j == 0 else float(C._wrap(psi[j] - prev, period))
            if advance_prev:
                prev = psi[j]
            run[j] = s
        sums[t] = s
    off, u = 0.0, np.empty(nwin)
    for t in range(TTRACK_THREADS):
        a = min(t * seg, nwin)
        e = min(a + seg, nwin)
        u[a:e] = off + run[a:e]
        off += sums[t]
    return T._centred_mean(u, span), choice.astype(np.uint8)


# ---- 5. exact ties
SPIKE_TABLES = [(8, 16.0), (64, 16.0), (4, 20.0), (6, 12.0)]
SPIKE_NWIN = 2100


@functools.lru_cache(maxsize=None)
def spike_table(H, period):
    """X = -1 everywhere and -1000 at one random hypothesis per window: a = c, so every vertex is exactly 0, ψ = s_h exactly and
    every step a multiple of period / H -> (stat, ψ, host tau at span 1, host choice)."""
    rng = np.random.default_rng(3000 + 100 * H + int(period))      # (a seed that gives H = 64, where one step in 64 is a tie, its 40)
    h = rng.integers(0, H, SPIKE_NWIN)
    stat = np.zeros((H, SPIKE_NWIN, 2))
    stat[:, :, 0] = -1.0
    stat[h, np.arange(SPIKE_NWIN), 0] = -1000.0
    psi = T.hypothesis_instants(period, H)[h]
    tau, choice = T.timing_track_host(stat, period, 1)
    _freeze(stat, psi, tau, choice)
    return stat, psi, tau, choice


def _table(H, columns):
    """float64[H, nwin, 2] with X = -1 and -1000 at the listed hypotheses of every window (None: the whole window NaN)."""
    stat = np.zeros((H, len(columns), 2))
    stat[:, :, 0] = -1.0
    for w, hs in enumerate(columns):
        if hs is None:
            stat[:, w, 0] = np.nan
        else:
            stat[list(hs), w, 0] = -1000.0
    return stat


# Two equal minima next to each other, (h, h + 1): c = b, V = +1/2 exactly, the choice is h.  (H - 1, 0): a = b at choice 0,
# V = -1/2 exactly, ψ = -P/2 - P/(2H).  Every ψ and every sum below is a small multiple of 1/2: exact on either side.
# name -> (H, period, the minima per window, ψ, tau at span 1, choice)
NEIGHBOUR_TABLES = {
    # ψ -4 (V = +1/2 at h = 1) -> 6 (a lone spike at h = 4): a step of exactly +P/2 through the clamp with H odd; ... -> -4: -P/2, taken as +P/2
    "H 5, P 20": (5, 20.0, [(1, 2), (4,), (4, 0), (1,), (1, 2), (4,), (1, 2)], [-4.0, 6.0, -12.0, -6.0, -4.0, 6.0, -4.0],
                  [-4.0, 6.0, 8.0, 14.0, 16.0, 26.0, 36.0], [1, 4, 0, 1, 1, 4, 1]),
    # H even: ±P/2 between two half vertices, -7 -> 1 -> -7 and -9 -> -1
    "H 8, P 16": (8, 16.0, [(0, 1), (4, 5), (0, 1), (7, 0), (3, 4), (7,)], [-7.0, 1.0, -7.0, -9.0, -1.0, 6.0], [-7.0, 1.0, 9.0, 7.0, 15.0, 22.0],
                  [0, 4, 0, 0, 3, 7]),
    # every hypothesis of window 2 NaN: choice 0, vertex 0, ψ = s_0 = -8, and the windows after it go on from there
    "a NaN window": (8, 16.0, [(5,), (6,), None, (3,), (4,), (2,)], [2.0, 4.0, -8.0, -2.0, 0.0, -4.0], [2.0, 4.0, 8.0, 14.0, 16.0, 12.0],
                     [5, 6, 0, 3, 4, 2]),
}


# ---- 7. recover at 1, 2, 7 and 8 windows
RECOVER_NCOLS = [60, 128, 448, 512]
RECOVER_WINDOW = 64
RECOVER_TAU0 = 2.7


@pytest.fixture(scope="module")
def short_bursts(oracle):
    """ncols -> (samples read at n + 2.7 + eps n with half the documented drift for W = 64, taps, first, the coarse table
    float64[8, nwin, 2] of ``recover_timing_host``, its result).  Noiseless PT rows of the reference chain."""
    sig, _noise, taps, first, have = _chain(oracle, 520)
    assert have >= max(RECOVER_NCOLS)
    eps = 0.5 * T.MAX_DRIFT_SAMPLES / (SPS * RECOVER_WINDOW)
    bad = T.timing_offset_host(sig, RECOVER_TAU0, eps)
    out = {}
    for ncols in RECOVER_NCOLS:
        coarse = []
        for s in T.hypothesis_instants(2.0 * SPS, T.DEFAULT_HYPOTHESES):
            rows = T.mf_bank_resample_host(bad, taps, first, SPS, ncols, RECOVER_WINDOW, None, s)[0]
            coarse.append(C.carrier_stat_host(rows, C.map_branch_host(rows)[2], RECOVER_WINDOW))
        out[ncols] = (bad, taps, first, np.stack(coarse), T.recover_timing_host(bad, taps, first, ncols, SPS, RECOVER_WINDOW))
    return out


# ------------------------------------------------------------------------------------------------ CPU
def test_kernel_constants_are_the_restated_ones():
    """The boundary cases below sit on the kernel's own thresholds.  A retuned kernel fails here instead of moving them off."""
    src = (Path(__file__).resolve().parent.parent / "waveforms_amd" / "csrc" / "wf_timing.hip").read_text()
    got = {name: int(re.search(rf"^#define\s+{name}\s+(\d+)\b", src, re.M).group(1)) for name in ("RS_THREADS", "RS_LDS_SLOTS", "RS_EXTRA", "RS_MAX_TAPS", "TTRACK_THREADS")}
    assert got == {"RS_THREADS": RS_THREADS, "RS_LDS_SLOTS": RS_LDS_SLOTS, "RS_EXTRA": RS_EXTRA, "RS_MAX_TAPS": RS_MAX_TAPS, "TTRACK_THREADS": TTRACK_THREADS}
    assert int(re.search(r"P\.nblk < (\d+) \? P\.nblk : \1", src).group(1)) == RS_GRID
    for (step, ntaps), want in GEOMETRY.items():
        assert geometry(step, ntaps) == want, (step, ntaps)
    assert {geometry(*k) for k in BOUNDARY} >= {(256, 2116), (224, 2388), (32, 2060), (16, 1282)}
    # the worked example: first 5, tau0 0.25, tau = [0, 0, 0, X] at (8, 9)
    for X, want in ((63.74, 2115), (63.75, 2116), (64.999, 2117)):
        assert tile_needs(5, 8, 640, 64, np.array([0.0, 0.0, 0.0, X]), 0.25, 9, 256).tolist() == [want, 2052, 1028], X


@pytest.mark.parametrize("fall", [False, True])
@pytest.mark.parametrize("step,ntaps", BOUNDARY)
def test_boundary_tiles_need_exactly_what_they_claim(step, ntaps, fall):
    """The boundary tile's need is region - 1, region and region + 1, with every row live and the other tiles inside their
    region.  At region + 1 the farthest sample a row of the tile reads lies ``region`` slots from the window's first one: one
    past what would have been staged.  And the comparison can tell: without the outermost sample at either end of the tile's
    span the host statement itself leaves the bound (the extreme rows' outer weights are not 0)."""
    case = boundary_case(step, ntaps, fall)
    ob, region, ncols, W, c, tile = (case[k] for k in ("ob", "region", "ncols", "W", "c", "tile"))
    first, nsamp, r, taps = (case[k] for k in ("first", "nsamp", "r", "taps"))
    assert len({X for X, *_ in case["runs"]}) == 3
    for d, (X, tau, want, mag) in zip((-1, 0, 1), case["runs"]):
        needs = tile_needs(first, step, ncols, W, tau, BOUNDARY_TAU0, ntaps, ob, nsamp)
        B, live = tile_B(first, step, ncols, W, tau, BOUNDARY_TAU0, nsamp)
        rows = slice(tile * ob, min(tile * ob + ob, ncols))
        print(f"step {step}, ntaps {ntaps}, {'fall' if fall else 'rise'} {X:.4f}: needs {needs.tolist()}, region {region}")
        assert live.all() and B.min() >= 0 and B.max() + 2 + c < nsamp
        assert needs.size == 3 and needs[tile] == region + d and all(needs[i] <= region for i in range(3) if i != tile), (needs, region)
        lo = int(B[rows].min()) - 1 - c
        top = int(B[rows].max()) + 2 + c
        assert top - lo + 1 == needs[tile]
        if d == 1:
            assert (B[rows] + 2 + c - lo).max() == region
        k_min, k_max = tile * ob + int(np.argmin(B[rows])), tile * ob + int(np.argmax(B[rows]))
        if not fall or ob < 224:
            assert (k_min, k_max) == ((rows.stop - 1, rows.start) if fall else (rows.start, rows.stop - 1))
        else:
            assert k_max == 159 and k_min in (223, 224)
        bound = (ntaps + 12) * U * mag
        for s, k in ((top, k_max), (lo, k_min)):
            if s < 0:
                continue                                             # (rising from first = 5, the window starts before the burst: zeros either way)
            r2 = np.array(r)
            r2[s] = 0.0
            other = T.mf_bank_resample_host(r2, taps, first, step, ncols, W, tau, BOUNDARY_TAU0)[0]
            assert (_rows_error(other[k], want[k]) > 1e6 * bound[k]).any(), (s, k)


def test_walk_reaches_every_order_of_lds_and_global():
    tau, first, nsamp, fits = walk_case()
    ob, region = geometry(WALK_STEP, WALK_NTAPS)
    assert (ob, region) == (256, 331) and fits.size == 2 * RS_GRID + 2 and fits.size == tau.size
    B, live = tile_B(first, WALK_STEP, WALK_NCOLS, WALK_W, tau, WALK_TAU0, nsamp)
    assert live.all() and B.min() >= 8 and B.max() + 8 < nsamp
    a, b = fits[:RS_GRID], fits[RS_GRID:2 * RS_GRID]
    counts = {(x, y): int(np.count_nonzero((a == x) & (b == y))) for x in (True, False) for y in (True, False)}
    print(f"(first tile fits, second tile fits) -> workgroups: {counts}; third tiles fit: {fits[2 * RS_GRID:].tolist()}")
    assert min(counts.values()) >= 100, counts
    assert fits[2 * RS_GRID:].tolist() == [False, True]
    # workgroup 1 stages, reads global memory, then stages again over its first window
    assert [bool(fits[1 + i * RS_GRID]) for i in range(3)] == [True, False, True]


def test_burst_end_rows_on_the_host_statement():
    """step 1, 40 samples, first -6, tau0 1/2: B runs through every integer from -6 to 45.  Rows 0 .. 3 and 47 .. 51 are zero, row 4
    (B = -2) lives on its last node alone and row 46 (B = nsamp) on its first."""
    rng = np.random.default_rng(40)
    r = _complex(rng, 40)
    c = T.lagrange_host(0.5)
    for ntaps in (1, 5):
        taps = _complex(rng, 3, ntaps)
        v = T._full_rate(r, taps)
        want, mag = T.mf_bank_resample_host(r, taps, -6, 1, 52, tau0=0.5)
        B, live = tile_B(-6, 1, 52, 64, None, 0.5, 40)
        assert B.tolist() == list(range(-6, 46)) and (~live).nonzero()[0].tolist() == [0, 1, 2, 3, 47, 48, 49, 50, 51]
        assert (~want.any(axis=1)).nonzero()[0].tolist() == [0, 1, 2, 3, 47, 48, 49, 50, 51] and np.array_equal(mag == 0.0, want == 0.0)
        assert np.array_equal(want[4], c[3] * v[:, 0]) and np.array_equal(want[46], c[0] * v[:, 39])
        assert np.array_equal(want[5], c[2] * v[:, 0] + c[3] * v[:, 1])


@pytest.mark.parametrize("H,nwin,span", GRID)
def test_blocked_scan_restatement_against_the_host_statement(H, nwin, span):
    """The blocked scan is the definition's running sum to rounding: within the header's bound at every grid entry.  The inputs
    keep every wrapped step at least WRAP_MARGIN from ±8 and the trajectory on the true instants modulo 16 to 1e-9, so that a
    rounding cannot flip a wrap.  The seeded defect - the previous ψ not advanced inside a segment - stays within the bound
    wherever a segment holds one window and breaks it at every nwin > 1024: what the device comparison at these sizes adds."""
    true, stat, want, want_choice, one = grid_case(H, nwin, span)
    got, choice = blocked_scan_restatement(stat, PERIOD, span)
    bound = _track_bound(one, nwin, span)
    ratio = float(np.abs(got - want).max() / bound)
    margin = 0.5 * PERIOD - (float(np.abs(np.diff(one)).max()) if nwin > 1 else 0.0)
    xs = np.sort(stat[:, :, 0], axis=0)
    bad, _c = blocked_scan_restatement(stat, PERIOD, span, advance_prev=False)
    bad_ratio = float(np.abs(bad - want).max() / bound)
    print(f"H {H}, nwin {nwin}, span {span}: restatement error / bound {ratio:.2g}, wrap margin {margin:.3f} samples, "
          f"smallest gap between the two best X {float((xs[1] - xs[0]).min()):.3g}, prev not advanced: error / bound {bad_ratio:.3g}")
    assert np.array_equal(choice, want_choice)
    assert ratio <= 1.0
    assert margin >= WRAP_MARGIN
    assert np.abs(C._wrap(one - true, PERIOD)).max() <= 1e-9
    assert (bad_ratio > 1.0) == (nwin > TTRACK_THREADS), bad_ratio
    assert (xs[1] - xs[0]).min() > 0.0                       # no ties here: the device's argmin rounds nothing, so choice is equal


@pytest.mark.parametrize("H,period", SPIKE_TABLES)
def test_spike_table_steps_of_half_a_period_go_up(H, period):
    """ψ = s_h exactly, so the host statement's steps at span 1 are exact multiples of period / H in (-P/2, P/2], and every raw
    step of exactly +P/2 or -P/2 comes out as +P/2: the interval is closed at the top."""
    stat, psi, tau, choice = spike_table(H, period)
    half = 0.5 * period
    assert np.array_equal(tau[0:1], psi[0:1]) and np.array_equal(T.hypothesis_instants(period, H)[choice], psi)
    raw, steps = np.diff(psi), np.diff(tau)
    assert np.array_equal(steps, C._wrap(raw, period)) and np.array_equal(np.round(steps * H / period) * (period / H), steps)
    assert steps.min() > -half and steps.max() == half
    ties = np.abs(raw) == half
    print(f"H {H}, period {period}: {int(ties.sum())} raw steps of exactly ±P/2 ({int((raw == -half).sum())} of them down), all taken as +P/2")
    assert ties.sum() >= 40 and (raw == -half).sum() >= 10 and (raw == half).sum() >= 10 and (steps[ties] == half).all()


@pytest.mark.parametrize("name", list(NEIGHBOUR_TABLES))
def test_neighbour_ties_and_a_nan_window_on_the_host_statement(name):
    """Bitwise: every operation on these tables is exact.  A window with only SOME hypotheses NaN is not tested anywhere: the
    header does not define it (numpy's argmin takes the first NaN, the kernel's ``<`` skips it)."""
    H, period, columns, psi, tau, choice = NEIGHBOUR_TABLES[name]
    stat = _table(H, columns)
    X = stat[:, :, 0]
    got_choice = np.argmin(X, axis=0)
    w = np.arange(len(columns))
    v = T.vertex_host(X[(got_choice - 1) % H, w], X[got_choice, w], X[(got_choice + 1) % H, w], 0.5)
    want_v = [0.0 if hs is None or len(hs) == 1 else (-0.5 if hs == (H - 1, 0) else 0.5) for hs in columns]
    assert v.tolist() == want_v and (T.hypothesis_instants(period, H)[got_choice] + (period / H) * v).tolist() == psi
    got, got_choice = T.timing_track_host(stat, period, 1)
    assert got.tolist() == tau and got_choice.tolist() == choice and np.isfinite(got).all()
    steps = C._wrap(np.diff(psi), period)
    assert np.array_equal(np.diff(got), steps) and steps.min() > -0.5 * period
    raw = np.diff(psi)
    assert None in columns or ((raw == 0.5 * period).any() and (raw == -0.5 * period).any() and (steps[np.abs(raw) == 0.5 * period] == 0.5 * period).all())


@pytest.mark.parametrize("ncols", RECOVER_NCOLS)
def test_short_bursts_leave_no_choice_to_a_rounding(short_bursts, ncols):
    """The two smallest X of every window of the coarse table differ by more than 1e-6 |X|: the device's roundings, a few
    2^-53 of the window's sum, cannot flip a choice.  nwin = 1, 2, 7, 8: the rescale skipped, anchored at (0, nwin - 1), at (2, nwin - 3)."""
    _bad, _taps, _first, coarse, (rows, tau, choice) = short_bursts[ncols]
    nwin = -(-ncols // RECOVER_WINDOW)
    assert nwin == {60: 1, 128: 2, 448: 7, 512: 8}[ncols] and coarse.shape == (T.DEFAULT_HYPOTHESES, nwin, 2)
    xs = np.sort(coarse[:, :, 0], axis=0)
    gap = (xs[1] - xs[0]) / np.abs(xs[0])
    print(f"ncols {ncols}: smallest relative gap between the two best X {gap.min():.3g}")
    assert (gap > 1e-6).all()
    assert np.array_equal(np.argmin(coarse[:, :, 0], axis=0), choice) and tau.shape == (nwin,) and rows.shape == (ncols, 3)
    # the rescale is what these sizes are about: it must move the trajectory where it applies
    plain = T.timing_track_host(coarse, 2.0 * SPS, C.DEFAULT_SPAN)[0]
    moved = T.rescale_host(plain, SPS * RECOVER_WINDOW)
    # (two windows under a span of 5 share one mean: the slope is 0 there and the division by 1 - 0 changes nothing)
    assert np.array_equal(moved, plain) == (nwin <= 2) and (np.ptp(plain) > 0.0) == (nwin > 2)
    if nwin >= 2:
        ends = plain[0] + (plain - plain[0]) / (1.0 - (plain[-1] - plain[0]) / ((nwin - 1.0) * SPS * RECOVER_WINDOW))
        assert np.array_equal(moved, ends) == (nwin < 8)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture
def ctx():
    from waveforms_amd import _hip

    handle = _hip.new_ctx()
    yield handle
    _hip.free_ctx(handle)


GUARD, SENTINEL = 4, -7.5


def _resample(ctx, d_r, d_taps, first, step, ncols, W, tau, tau0):
    """The device's rows as complex128[ncols, 3], written between sentinel rows that must stay as they are."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    buf = _hip.to_device(np.full((ncols + 2 * GUARD, 3, 2), SENTINEL))
    out = dev.mf_bank_resample(d_r, d_taps, first, step, ncols, W, None if tau is None else _hip.to_device(np.array(tau, dtype=np.float64)), tau0,
                               out=buf[GUARD:GUARD + ncols], ctx=ctx)
    full = _hip.to_host(buf)
    assert (full[:GUARD] == SENTINEL).all() and (full[GUARD + ncols:] == SENTINEL).all()
    return _hip.to_host(out, True)


def _ratio(err, bound):
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("fall", [False, True])
@pytest.mark.parametrize("step,ntaps", BOUNDARY)
def test_mf_bank_resample_at_the_staged_span(ctx, step, ntaps, fall):
    """need = region - 1 and region: the tile is staged, to its last slot; region + 1: it reads global memory.  The header's
    bound, (ntaps + 12) * 2^-53 * the host statement's absolute-value sum, per component."""
    from waveforms_amd import _hip

    case = boundary_case(step, ntaps, fall)
    d_r, d_taps = _hip.to_device(np.array(case["r"])), _hip.to_device(np.array(case["taps"]))
    for d, (X, tau, want, mag) in zip((-1, 0, 1), case["runs"]):
        got = _resample(ctx, d_r, d_taps, case["first"], step, case["ncols"], case["W"], tau, BOUNDARY_TAU0)
        bound = (ntaps + 12) * U * mag
        err = _rows_error(got, want)
        print(f"step {step}, ntaps {ntaps}, {'fall' if fall else 'rise'}, need = region {d:+d}: max error / bound = {_ratio(err, bound):.3f}")
        assert want.all() and (err <= bound).all(), (d, int(np.argmax((err - bound).max(axis=1))), err.max())


@pytest.mark.gpu
def test_mf_bank_resample_later_tiles_in_every_order(ctx):
    """2 097 452 rows at step 1: every workgroup walks two tiles and two a third, staging over an old window after a tile that
    went through global memory and the other way round (the CPU test counts the orders)."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    torch = _hip.torch()
    tau, first, nsamp, fits = walk_case()
    rng = np.random.default_rng(32)
    r, taps = _complex(rng, nsamp), _complex(rng, 3, WALK_NTAPS)
    want, mag = T.mf_bank_resample_host(r, taps, first, WALK_STEP, WALK_NCOLS, WALK_W, tau, WALK_TAU0)
    d_r = _hip.to_device(r)
    out = dev.mf_bank_resample(d_r, _hip.to_device(taps), first, WALK_STEP, WALK_NCOLS, WALK_W, _hip.to_device(np.array(tau)), WALK_TAU0, ctx=ctx)
    try:
        got = _hip.to_host(out, True)
    finally:
        del d_r, out
        torch.cuda.empty_cache()
    bound = (WALK_NTAPS + 12) * U * mag
    err = _rows_error(got, want)
    worst = int(np.argmax((err - bound).max(axis=1)))
    tile = worst // 256
    print(f"later tiles: max error / bound = {_ratio(err, bound):.3f}")
    assert want.all() and (err <= bound).all(), (f"row {worst}, tile {tile} (workgroup {tile % RS_GRID}, its tile {tile // RS_GRID}, "
                                                 f"{'LDS' if fits[tile] else 'global'})", err[worst], want[worst], got[worst])


@pytest.mark.gpu
@pytest.mark.parametrize("tau0", [0.0, 0.5, -0.5])
def test_mf_bank_resample_every_instant_at_the_bursts_ends(ctx, tau0):
    """Every B from 6 before the burst to 5 behind it: the four weights go out one by one.  Dead rows are zero exactly."""
    from waveforms_amd import _hip

    rng = np.random.default_rng(41)
    # (step, ntaps, first, nsamp, ncols); the second: row 0 at B = -2 and row 13 at B = nsamp for tau0 = 1/2
    for step, ntaps, first, nsamp, ncols in ((1, 1, -6, 40, 52), (1, 5, -6, 40, 52), (8, 73, -2, 102, 16)):
        r, taps = _complex(rng, nsamp), _complex(rng, 3, ntaps)
        want, mag = T.mf_bank_resample_host(r, taps, first, step, ncols, tau0=tau0)
        B, live = tile_B(first, step, ncols, 64, None, tau0, nsamp)
        got = _resample(ctx, _hip.to_device(r), _hip.to_device(taps), first, step, ncols, 64, None, tau0)
        bound = (ntaps + 12) * U * mag
        err = _rows_error(got, want)
        print(f"tau0 {tau0}, step {step}, ntaps {ntaps}: B {int(B[0])} .. {int(B[-1])}, {int((~live).sum())} dead rows, max error / bound = {_ratio(err, bound):.3f}")
        assert (err <= bound).all(), err.max()
        assert (~live).sum() >= 2 and not got[~live].any() and not want[~live].any() and np.array_equal(got.any(axis=1), want.any(axis=1))
        if tau0 == 0.5:
            assert B[0] == (-6 if step == 1 else -2) and np.array_equal(~live, (B < -2) | (B > nsamp)) and (B == -2).any() and (B == nsamp).any()


@pytest.mark.gpu
def test_mf_bank_resample_window_lookup(ctx):
    """Windows that are no multiple of a tile, the longest window more than once, a trajectory shorter than the burst (the clamp
    at its last entry serves most rows) and longer than it (what lies beyond is not read), and entries at ±2^62."""
    from waveforms_amd import _hip

    rng = np.random.default_rng(42)
    taps = _complex(rng, 3, 9)
    d_taps = _hip.to_device(taps)
    huge = 2.0 ** 62
    cases = {
        "W 192": (SPS, 1000, 192, np.cumsum(rng.uniform(-3.0, 3.0, 6)), 0.3),
        "W 8192, three windows": (1, 3 * 8192 + 17, 8192, rng.uniform(-30.0, 30.0, 3), 0.3),
        "two entries for 16 windows": (SPS, 1000, 64, np.array([1.7, -2.6]), 0.3),
        "100 entries for 2 windows": (SPS, 100, 64, np.cumsum(rng.uniform(-3.0, 3.0, 100)), 0.3),
        "+2^62": (SPS, 100, 64, np.array([huge]), 0.0),
        "-2^62": (SPS, 100, 64, np.array([-huge]), 0.0),
        "just below 2^62": (SPS, 100, 64, np.array([huge * (1.0 - U)]), 0.0),
        "just above -2^62": (SPS, 100, 64, np.array([-huge * (1.0 - U)]), 0.0),
        "0 to 2^62": (SPS, 200, 64, np.array([0.5, huge]), 0.0),
    }
    for name, (step, ncols, W, tau, tau0) in cases.items():
        first = 40
        r = _complex(rng, first + ncols * step + 60)
        d_r = _hip.to_device(r)
        want, mag = T.mf_bank_resample_host(r, taps, first, step, ncols, W, tau, tau0)
        got = _resample(ctx, d_r, d_taps, first, step, ncols, W, tau, tau0)
        bound = (9 + 12) * U * mag
        err = _rows_error(got, want)
        zero = ~want.any(axis=1)
        print(f"{name}: max error / bound = {_ratio(err, bound):.3f}, {int(zero.sum())} zero rows of {ncols}")
        assert (err <= bound).all(), (name, err.max())
        assert np.array_equal(~got.any(axis=1), zero), name
        t = T.instants_host(ncols, W, tau, tau0)
        if "2^62" in name:
            assert np.array_equal(zero, ~(np.abs(t) < 1e6)) and zero.sum() == (ncols if name != "0 to 2^62" else ncols - 32), name
        else:
            assert not zero.any() and np.abs(t).max() < 40
        if name == "two entries for 16 windows":
            assert (t[96:] == tau0 + tau[1]).all() and t[95] != t[96]
        if name == "100 entries for 2 windows":
            assert np.array_equal(got, _resample(ctx, d_r, d_taps, first, step, ncols, W, tau[:3], tau0))
            assert not np.array_equal(want, T.mf_bank_resample_host(r, taps, first, step, ncols, W, tau[:2], tau0)[0])


def _track(stat, period, span, ctx):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    tau, choice = dev.timing_track(_hip.to_device(np.array(stat, dtype=np.float64)), period, span, ctx=ctx)      # a copy: the shared inputs are read-only
    return _hip.to_host(tau), _hip.to_host(choice)


@pytest.mark.gpu
@pytest.mark.parametrize("H,nwin,span", GRID)
def test_timing_track_on_the_segment_grid(ctx, H, nwin, span):
    """tau within the header's bound of the host statement, choice equal.  The CPU test above holds the preconditions."""
    _true, stat, want, want_choice, one = grid_case(H, nwin, span)
    tau, choice = _track(stat, PERIOD, span, ctx)
    assert tau.shape == want.shape and choice.shape == want_choice.shape and choice.dtype == np.uint8
    bound = _track_bound(one, nwin, span)
    err = np.abs(tau - want)
    print(f"H {H}, nwin {nwin}, span {span}: max |device - host| / bound = {err.max() / bound:.3g}")
    assert np.array_equal(choice, want_choice), int(np.count_nonzero(choice != want_choice))
    assert err.max() <= bound, (err.max(), int(np.argmax(err)))


@pytest.mark.gpu
@pytest.mark.parametrize("nwin", [1023, 1025, 2049, 5000])
def test_timing_refine_on_the_segment_grid(ctx, nwin):
    """Random triples with flat and concave windows mixed in: within (span + 8) * 2^-53 * δ, and bitwise at span 1."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    rng = np.random.default_rng(nwin)
    stat3 = rng.standard_normal((3, nwin, 2)) * 50.0 - 2000.0
    stat3[:, ::5, 0] = -2000.0                                           # flat: den = 0
    stat3[1, 1::5, 0] = -1000.0                                          # concave: den < 0
    d_stat3 = _hip.to_device(stat3)
    delta = 2.0
    one = T.timing_refine_host(stat3, delta, 1)
    # (of the random triples about half are convex: three windows in ten move, some of them to the clamp)
    assert not one[::5].any() and not one[1::5].any() and np.abs(one).max() == delta and np.count_nonzero(one) > nwin // 5
    for span in (1, 5, 10001):
        want = T.timing_refine_host(stat3, delta, span)
        got = _hip.to_host(dev.timing_refine(d_stat3, delta, span, ctx=ctx))
        err = np.abs(got - want).max()
        print(f"nwin {nwin}, span {span}: max |device - host| / bound = {err / ((span + 8) * U * delta):.3g}")
        assert err <= (span + 8) * U * delta
        if span == 1:
            assert np.array_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("H,period", SPIKE_TABLES)
def test_timing_track_wraps_a_tie_upwards(ctx, H, period):
    """Every step of these tables is exact on the device as on the host.  A device that closed the interval at the bottom would
    step down by P/2 somewhere (the CPU test counts the places)."""
    stat, _psi, want, want_choice = spike_table(H, period)
    tau, choice = _track(stat, period, 1, ctx)
    bound = _track_bound(want, SPIKE_NWIN, 1)
    err = np.abs(tau - want).max()
    print(f"H {H}, period {period}: max |device - host| / bound = {err / bound:.3g}, smallest device step {np.diff(tau).min():.3g}")
    assert np.array_equal(choice, want_choice)
    assert err <= bound
    assert np.diff(tau).min() > -0.5 * period


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(NEIGHBOUR_TABLES))
def test_timing_track_neighbour_ties_and_a_nan_window(ctx, name):
    """At most 8 windows, span 1, every operation exact: the device's values are the host's, bitwise.  (A window with only some
    hypotheses NaN is not defined by the header and not tested.)"""
    H, period, columns, _psi, want, want_choice = NEIGHBOUR_TABLES[name]
    assert len(columns) <= 8
    tau, choice = _track(_table(H, columns), period, 1, ctx)
    print(f"{name}: device tau {tau.tolist()}, choice {choice.tolist()}")
    assert choice.tolist() == want_choice
    assert np.array_equal(tau.view(np.uint64), np.array(want).view(np.uint64))


STRIDE_N = (1 << 24) + 3              # at most 65536 blocks of 256 threads, so element 2^24 is a second trip
STRIDE_SLICES = (slice(0, 4096), slice((1 << 24) - 2048, STRIDE_N))


def _offset_bound(x, tau0, eps, first_index):
    ok, fl, mu = T._split(tau0 + eps * (np.arange(x.size) + first_index).astype(np.float64))
    return 8.0 * U * T._interpolated(np.abs(x), np.arange(x.size) + fl, ok, np.abs(T.lagrange_host(mu)))


@pytest.mark.gpu
def test_timing_offset_past_the_grid_cap():
    """t runs from 97.25 to 98.93 here, so an output reads up to 100 samples ahead: the host statement gets each compared
    slice with that much around it (and a matching first_index), and the burst's true end for the last one."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    torch = _hip.torch()
    tau0, eps, first = -2.75, 1e-7, 10 ** 9
    reach = int(math.ceil(abs(tau0) + eps * (first + STRIDE_N))) + 8
    x = torch.randn((STRIDE_N, 2), dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(6))
    out = dev.timing_offset(x, tau0, eps, first)
    try:
        for sl in STRIDE_SLICES:
            a, b = max(sl.start - reach, 0), min(sl.stop + reach, STRIDE_N)
            z, got = _hip.to_host(x[a:b], True), _hip.to_host(out[sl], True)
            keep = slice(sl.start - a, sl.stop - a)
            want = T.timing_offset_host(z, tau0, eps, first + a)[keep]
            bound = _offset_bound(z, tau0, eps, first + a)[keep]
            err = _rows_error(got, want)
            print(f"elements {sl.start} .. {sl.stop}: max error / bound = {_ratio(err, bound):.3f}, {int((~want.astype(bool)).sum())} zeros")
            assert (err <= bound).all(), (sl, err.max())
            assert want[:-128].all() and (sl.stop < STRIDE_N or not want[-90:].any())
    finally:
        del x, out
        torch.cuda.empty_cache()


@pytest.mark.gpu
def test_timing_offset_whole_shifts_and_unusable_instants():
    """Whole shifts that leave three, two, one or no samples in range: the weights are 0 and 1, bitwise the host statement's.
    An instant at or beyond 2^62 gives a zero."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    rng = np.random.default_rng(61)
    n = 257
    x = _complex(rng, n)
    d_x = _hip.to_device(x)
    left = {}
    for tau0 in (-260.0, -258.0, -3.0, -2.0, 254.0, 255.0, 256.0, 258.0):
        want = T.timing_offset_host(x, tau0, 0.0)
        got = _hip.to_host(dev.timing_offset(d_x, tau0, 0.0), True)
        left[tau0] = int(np.count_nonzero(want))
        assert np.array_equal(got, want), tau0
        k = np.arange(n) + int(tau0)
        assert np.array_equal(want, np.where((k >= 0) & (k < n), x[np.clip(k, 0, n - 1)], 0.0))
    print(f"samples left in range per shift: {left}")
    assert left == {-260.0: 0, -258.0: 0, -3.0: 254, -2.0: 255, 254.0: 3, 255.0: 2, 256.0: 1, 258.0: 0}
    for tau0, eps, first in ((2.0 ** 62, 0.0, 0), (-2.0 ** 62, 0.0, 0), (0.0, 1e10, 1 << 52)):
        assert not T.timing_offset_host(x, tau0, eps, first).any()
        assert not _hip.to_host(dev.timing_offset(d_x, tau0, eps, first)).any(), (tau0, eps)
    assert np.array_equal(_hip.to_host(d_x, True), x)


@pytest.mark.gpu
@pytest.mark.parametrize("ncols", RECOVER_NCOLS)
def test_recover_at_one_two_seven_and_eight_windows(short_bursts, ctx, ncols):
    """``recover`` restates ``rescale_host`` as tensor operations: skipped below two windows, anchored at (0, nwin - 1) below
    eight and at (2, nwin - 3) from eight on."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    bad, taps, first, _coarse, (host_rows, host_tau, host_choice) = short_bursts[ncols]
    rec = T.TimingRecovery(SPS, window=RECOVER_WINDOW)
    rows, tau, choice = rec.recover(_hip.to_device(bad), _hip.to_device(taps), first, ncols, True, ctx=ctx)
    got = _hip.to_host(tau)
    print(f"ncols {ncols}: {got.size} windows, max |device tau - host tau| = {np.abs(got - host_tau).max():.3g}")
    assert np.array_equal(_hip.to_host(choice), host_choice)
    np.testing.assert_allclose(got, host_tau, rtol=0, atol=1e-9)
    assert np.array_equal(_hip.to_host(dev.viterbi_soft_branch(rows, True, ctx=ctx)[1]), C.map_branch_host(host_rows)[1])
