"""The carrier stages in the launch forms and at the ties that tests/test_carrier.py does not reach (include/wfhip.h:
wf_carrier_track, wf_carrier_offset_c128, wf_rows_derotate).

``carrier_track_kernel`` is one workgroup of 1024 threads that unwraps ψ as a blocked scan: thread t owns the windows
[t seg, t seg + seg), seg = ceil(nwin / 1024).  Up to 1024 windows every segment holds one window, so the loop inside a segment,
the second trip of the two strided loops and the clipped segments only run beyond that.  Here the tracker is fed synthetic
statistics directly (no rows, no detector) at 1023 .. 5000 windows, with hypotheses that tie exactly, and with statistics on
the axes, where every step of ψ is a multiple of π/2 and the wrap's closed end decides.  The two elementwise kernels run at
2^24 + 3 elements, the first size at which their grid-stride loop takes a second step.

CPU: a numpy restatement of the blocked scan against ``carrier_track_host`` and the preconditions that make the comparison
on the device sound.  GPU: the device against ``carrier_track_host`` within the header's bound
8 * 2^-52 * max(1, |phase|) * nwin, ``choice`` exactly.
"""
import functools
import math

import numpy as np
import pytest

import test_carrier as TC
from waveforms_amd.sync import carrier as C

EPS = TC.EPS
SEGMENTS = 1024                       # carrier_track_kernel's TRACK_THREADS
# (H, nwin, span): around one and two windows per segment, clipped segments (2049: seg = 3, the last 341 threads own nothing),
# a span wider than the burst, H neither a power of two nor small, and the two smallest bursts
GRID = [(1, 1023, 1), (1, 1024, 5), (8, 1025, 5), (8, 2047, 1), (3, 2049, 5), (8, 5000, 101), (256, 1500, 3001), (8, 3, 5), (1, 1, 1)]
WRAP_MARGIN = 0.25                    # rad: the least distance of a wrapped step from ±π/2 the comparisons below rely on
# Statistics on the axes, (X, Y): ψ = atan2(-Y, -X) is 0, ±π/2 or ±π (the all-zero windows: atan2(-0, -0) = -π, atan2(+0, +0) = 0)
AXIS_POINTS = [(-1.0, 0.0), (-1.0, -0.0), (1.0, 0.0), (1.0, -0.0), (0.0, -1.0), (-0.0, -1.0), (0.0, 1.0), (-0.0, 1.0), (0.0, 0.0), (-0.0, -0.0)]


def header_bound(want_phase):
    return 8.0 * EPS * np.maximum(1.0, np.abs(want_phase)) * want_phase.size


def synthetic_stat(H, nwin, seed=0):
    """-> (θ f64[nwin], stat f64[H, nwin, 2]).  θ_w = 1 + 2π 0.04 w + U(-0.2, 0.2): a step of 0.25 ± 0.4 rad, at least 0.92 rad
    from ±π/2.  Hypothesis h sees the residual r = θ_w - h π / H reduced into [-π/2, π/2] and (X, Y) = -a (cos r, sin r) with
    a = 100 (1 + cos r): the smaller |r|, the lower X, so argmin X is the nearest hypothesis and ψ = h π / H + r = θ modulo π."""
    rng = np.random.default_rng(1000 * H + nwin + seed)
    theta = 1.0 + 2.0 * math.pi * 0.04 * np.arange(nwin) + rng.uniform(-0.2, 0.2, nwin)
    r = theta[None, :] - (np.arange(H, dtype=np.float64) * math.pi / H)[:, None]
    r = r - math.pi * np.round(r / math.pi)
    a = 100.0 * (1.0 + np.cos(r))
    return theta, np.ascontiguousarray(np.stack([-a * np.cos(r), -a * np.sin(r)], axis=-1))


def wrap_margin(stat):
    """π/2 - the largest |wrapped step| of the host statement (span 1: phase = u, whose steps are the wrapped steps of ψ)."""
    u, _choice = C.carrier_track_host(stat, 1)
    return math.pi / 2.0 - float(np.abs(np.diff(u)).max()) if u.size > 1 else math.pi / 2.0


@functools.lru_cache(maxsize=None)
def grid_case(H, nwin, span):
    """One grid entry, computed once: (θ, stat, host phase, host choice, wrap margin).  Nobody writes to these."""
    theta, stat = synthetic_stat(H, nwin)
    phase, choice = C.carrier_track_host(stat, span)
    out = (theta, stat, phase, choice, wrap_margin(stat))
    for a in out[:4]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def tie_case():
    """H = 8, 2049 windows, span 5: on every third window hypothesis 2's statistics stand in hypotheses 5 and 0 as well."""
    _theta, stat = synthetic_stat(8, 2049, seed=1)
    stat = stat.copy()
    stat[5, ::3] = stat[2, ::3]
    stat[0, ::3] = stat[2, ::3]
    phase, choice = C.carrier_track_host(stat, 5)
    stat.setflags(write=False)
    return stat, phase, choice, wrap_margin(stat)


@functools.lru_cache(maxsize=None)
def axis_table(points=tuple(AXIS_POINTS), nwin=2100):
    """H = 1, span 1: ``nwin`` statistics drawn from the axis points, every point next to every other one."""
    rng = np.random.default_rng(21)
    stat = np.array(points)[rng.integers(0, len(points), nwin)][None]
    phase, choice = C.carrier_track_host(stat, 1)
    stat.setflags(write=False)
    return stat, phase, choice


def blocked_scan_restatement(stat, span, advance_prev=True):
    """``carrier_track_host`` with the running sum u taken as the header's blocked scan, in the kernel's segment layout:
    seg = ceil(nwin / 1024), segment t = [min(t seg, nwin), min(t seg + seg, nwin)); each segment adds its own wrapped steps from
    +0 (the first one starts with ψ_0), the 1024 segment sums are added in order into offsets, and u_w = offset + running sum.
    ``advance_prev=False`` seeds the defect the grid must catch: the previous ψ is not advanced inside a segment."""
    stat = np.asarray(stat, dtype=np.float64)
    H, nwin = stat.shape[0], stat.shape[1]
    choice = np.argmin(stat[:, :, 0], axis=0)
    w = np.arange(nwin)
    psi = (choice.astype(np.float64) * math.pi) / float(H) + np.arctan2(-stat[choice, w, 1], -stat[choice, w, 0])
    seg = -(-nwin // SEGMENTS)
    sums, run = np.zeros(SEGMENTS), np.empty(nwin)
    for t in range(SEGMENTS):
        a = min(t * seg, nwin)
        e = min(a + seg, nwin)
        s, prev = 0.0, (psi[a - 1] if 0 < a < nwin else 0.0)
        for j in range(a, e):
            s += psi[j] if j == 0 else float(C._wrap_pi(psi[j] - prev))
            if advance_prev:
                prev = psi[j]
            run[j] = s
        sums[t] = s
    off, u = 0.0, np.empty(nwin)
    for t in range(SEGMENTS):
        a = min(t * seg, nwin)
        e = min(a + seg, nwin)
        u[a:e] = off + run[a:e]
        off += sums[t]
    r = span // 2
    phase = np.empty(nwin)
    for j in range(nwin):
        lo, hi = max(0, j - r), min(nwin - 1, j + r)
        s = 0.0
        for i in range(lo, hi + 1):
            s += u[i]
        phase[j] = s / float(hi - lo + 1)
    return phase, choice.astype(np.uint8)


# ------------------------------------------------------------------------------------------------ CPU
def test_blocked_scan_restatement_against_the_host_statement():
    """The blocked scan is the definition's running sum to rounding: within the header's bound at every grid entry.  The inputs
    keep every wrapped step at least WRAP_MARGIN from ±π/2 and ψ on θ modulo π to 1e-9, so that an ulp between the device's atan2
    and numpy's cannot flip a wrap (measured: margins 0.92 rad and more, error / bound at most 0.0062).  The seeded defect - the
    previous ψ not advanced inside a segment - stays within the bound wherever a segment holds one window and breaks it at every
    nwin > 1024: what the device comparison at these sizes adds."""
    for H, nwin, span in GRID:
        theta, stat, want, want_choice, margin = grid_case(H, nwin, span)
        got, choice = blocked_scan_restatement(stat, span)
        bound = header_bound(want)
        ratio = float((np.abs(got - want) / bound).max())
        xs = np.sort(stat[:, :, 0], axis=0)
        gap = float((xs[1] - xs[0]).min()) if H > 1 else math.inf
        bad, _c = blocked_scan_restatement(stat, span, advance_prev=False)
        bad_ratio = float((np.abs(bad - want) / bound).max())
        print(f"H {H}, nwin {nwin}, span {span}: restatement error / bound {ratio:.2g}, wrap margin {margin:.3f} rad, "
              f"smallest gap between the two best X {gap:.3g}, prev not advanced: error / bound {bad_ratio:.3g}")
        assert np.array_equal(choice, want_choice)
        assert ratio <= 1.0, (H, nwin, span, ratio)
        assert margin >= WRAP_MARGIN, (H, nwin, span, margin)
        follow, _c = C.carrier_track_host(stat, 1)
        off = follow - theta
        assert np.abs(off - math.pi * np.round(off / math.pi)).max() <= 1e-9, (H, nwin)
        assert (bad_ratio > 1.0) == (nwin > SEGMENTS), (H, nwin, span, bad_ratio)
    stat, want, want_choice, margin = tie_case()
    got, choice = blocked_scan_restatement(stat, 5)
    assert np.array_equal(choice, want_choice) and (np.abs(got - want) <= header_bound(want)).all()
    # the ties are at the minimum on a good share of the windows, the smallest of the three wins, and the steps of ψ, now off by
    # 2 π / 8 where hypothesis 0 stands in for 2, still keep clear of ±π/2: 0.25 ± 0.4 ± π/4 lies within (-0.94, 1.44)
    xs = stat[:, :, 0]
    tied = (xs == xs.min(axis=0)).sum(axis=0)
    print(f"ties: {int((tied == 3).sum())} windows with three equal minima, wrap margin {margin:.3f} rad")
    assert (tied == 3).sum() > 50 and (tied[1::3] == 1).all() and (want_choice[tied == 3] == 0).all()
    assert margin >= 0.1, margin


def test_axis_table_steps_are_zero_or_up():
    """ψ on the axes is 0, ±π/2 or ±π exactly, every difference a multiple of π/2, and wrap(x) = x - π ceil(x / π - 1/2) sends
    it to 0 or to +π/2: (-π/2, π/2] is closed at the top, so a tie between the two directions goes up, never down."""
    stat, phase, choice = axis_table()
    psi = np.arctan2(-stat[0, :, 1], -stat[0, :, 0])
    half = math.pi / 2.0
    assert set(np.unique(psi).tolist()) == {-math.pi, -half, 0.0, half, math.pi}
    for x, y in AXIS_POINTS:
        assert np.arctan2(-y, -x) in (-math.pi, -half, 0.0, half, math.pi), (x, y)
    steps = C._wrap_pi(np.diff(psi))
    assert np.isin(steps, (0.0, half)).all() and (steps == half).sum() > 500 and (steps == 0.0).sum() > 500
    # every kind of step is there: each point follows each other one
    points, key = np.unique(np.ascontiguousarray(stat[0]).view(np.uint64), axis=0, return_inverse=True)      # by bit pattern: ±0 differ
    key = key.reshape(-1).tolist()
    assert len(points) == len(AXIS_POINTS) and len(set(zip(key[:-1], key[1:]))) == len(AXIS_POINTS) ** 2
    assert not choice.any() and phase.shape == (2100,)
    np.testing.assert_allclose(np.diff(phase), steps, rtol=0, atol=1e-9)
    assert phase[0] == psi[0] + 0.0


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture
def ctx():
    from waveforms_amd import _hip

    handle = _hip.new_ctx()
    yield handle
    _hip.free_ctx(handle)


def _track(stat, span, ctx):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    phase, choice = dev.carrier_track(_hip.to_device(np.array(stat, dtype=np.float64)), span, ctx=ctx)      # a copy: the shared inputs are read-only
    return _hip.to_host(phase), _hip.to_host(choice)


@pytest.mark.gpu
@pytest.mark.parametrize("H,nwin,span", GRID)
def test_carrier_track_on_synthetic_statistics(ctx, H, nwin, span):
    """phase within the header's bound of the host statement, choice equal everywhere (the comparison behind it rounds nothing).
    The CPU test above holds the preconditions on these inputs."""
    _theta, stat, want, want_choice, margin = grid_case(H, nwin, span)
    assert margin >= WRAP_MARGIN
    phase, choice = _track(stat, span, ctx)
    assert phase.shape == want.shape and choice.shape == want_choice.shape and choice.dtype == np.uint8
    ratio = np.abs(phase - want) / header_bound(want)
    print(f"H {H}, nwin {nwin}, span {span}: max |device - host| / bound = {ratio.max():.3g}")
    assert np.array_equal(choice, want_choice), int(np.count_nonzero(choice != want_choice))
    assert (ratio <= 1.0).all(), (ratio.max(), int(np.argmax(ratio)))


@pytest.mark.gpu
def test_carrier_track_ties_go_to_the_smallest_hypothesis(ctx):
    stat, want, want_choice, margin = tie_case()
    assert margin >= 0.1
    phase, choice = _track(stat, 5, ctx)
    ratio = np.abs(phase - want) / header_bound(want)
    print(f"ties: max |device - host| / bound = {ratio.max():.3g}")
    assert np.array_equal(choice, want_choice), int(np.count_nonzero(choice != want_choice))
    assert (ratio <= 1.0).all(), ratio.max()


@pytest.mark.gpu
def test_carrier_track_wraps_a_tie_upwards(ctx):
    """First each axis point alone: one window, H = 1, span 1, so phase[0] is ψ itself, bitwise numpy's arctan2(-Y, -X) (through
    the statement's 0 + atan2: -0 comes out as +0 on both sides).  With ψ exact, every step of the table is an exact multiple of
    π/2 on the device as on the host, and a device that closed the interval at the bottom would step down by π/2."""
    got = []
    for x, y in AXIS_POINTS:
        phase, choice = _track(np.array([[[x, y]]]), 1, ctx)
        want = np.array([0.0 + np.arctan2(-y, -x)])
        print(f"(X, Y) = ({x!r}, {y!r}): device ψ = {float(phase[0])!r}, numpy {float(want[0])!r}")
        got.append(np.array_equal(phase.view(np.uint64), want.view(np.uint64)) and not choice.any())
    assert all(got), [p for p, ok in zip(AXIS_POINTS, got) if not ok]
    stat, want, want_choice = axis_table()
    phase, choice = _track(stat, 1, ctx)
    ratio = np.abs(phase - want) / header_bound(want)
    print(f"axis table: max |device - host| / bound = {ratio.max():.3g}, smallest device step {np.diff(phase).min():.3g}")
    assert np.array_equal(choice, want_choice)
    assert (ratio <= 1.0).all(), ratio.max()
    assert np.diff(phase).min() >= -1.0, np.diff(phase).min()


STRIDE_N = (1 << 24) + 3              # both kernels: at most 65536 blocks of 256 threads, so element 2^24 is a second trip
STRIDE_SLICES = (slice(0, 4096), slice((1 << 24) - 2048, STRIDE_N))


@pytest.mark.gpu
def test_carrier_offset_past_the_grid_cap():
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    torch = _hip.torch()
    theta0, nu, first = 0.7, 1.2345678e-3, 10 ** 9
    x = torch.randn((STRIDE_N, 2), dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(8))
    out = dev.carrier_offset(x, theta0, nu, first)
    try:
        for sl in STRIDE_SLICES:
            z, got = _hip.to_host(x[sl], True), _hip.to_host(out[sl], True)
            want = C.carrier_offset_host(z, theta0, nu, first + sl.start)
            bound = TC._rot_bound(z, C.carrier_phase_host(z.size, theta0, nu, first + sl.start))
            assert (np.abs(got - want) <= bound).all(), (sl, np.abs(got - want).max())
    finally:
        del x, out
        torch.cuda.empty_cache()


@pytest.mark.gpu
def test_rows_derotate_past_the_grid_cap(ctx):
    """2^24 + 3 rows in windows of 8192 under a random-walk trajectory of 2049 phases; φ of the compared rows is formed here
    from the header's operations in the header's order."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    torch = _hip.torch()
    window, nwin = 8192, 2049
    assert -(-STRIDE_N // window) == nwin
    phase = np.cumsum(np.random.default_rng(12).uniform(-0.4, 0.4, nwin)) - 7.0
    rows = torch.randn((STRIDE_N, 3, 2), dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(9))
    out = dev.rows_derotate(rows, window, _hip.to_device(phase), 0.25, ctx=ctx)
    try:
        for sl in STRIDE_SLICES:
            z, got = _hip.to_host(rows[sl], True), _hip.to_host(out[sl], True)
            t = (np.arange(sl.start, sl.stop, dtype=np.float64) - 0.5 * float(window - 1)) / float(window)
            fl = np.floor(t)
            w = np.clip(fl.astype(np.int64), 0, nwin - 2)
            f = t - fl
            p0 = phase[w]
            d = phase[w + 1] - p0
            fd = f * d
            phi = np.where(t <= 0.0, phase[0], np.where(t >= float(nwin - 1), phase[nwin - 1], p0 + fd))
            tot = -(0.25 + phi)
            want = z * (np.cos(tot) + 1j * np.sin(tot))[:, None]
            assert (np.abs(got - want) <= TC._rot_bound(z, (0.25 + phi)[:, None])).all(), (sl, np.abs(got - want).max())
            assert sl.start or np.array_equal(phi, C.interpolate_phase_host(sl.stop, window, phase))
    finally:
        del rows, out
        torch.cuda.empty_cache()
