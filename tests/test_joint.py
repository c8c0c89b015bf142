"""Joint carrier and timing acquisition (waveforms_amd/sync/joint.py; include/wfhip.h: wf_rows_derotate_hyp,
wf_viterbi4_soft_branch_segments).

CPU: the lattice of the joint statistic (one symbol later and a quarter turn is the same burst one row later), and
``recover_joint_host`` on the reference PT chain under three joint impairments, two of them at both documented limits.
GPU: the two stacked entry points bit for bit against the unstacked ones, and the device recovery against the host statement.
"""
import ctypes
import math

import numpy as np
import pytest

from test_soft_detector import pack_rows
from test_timing import SPS, _chain
from waveforms_amd.sync import carrier as C
from waveforms_amd.sync import joint as J
from waveforms_amd.sync import timing as T

W = C.DEFAULT_WINDOW
NAMES = ("wf_rows_derotate_hyp", "wf_viterbi4_soft_branch_segments")
# (θ0 in degrees, ν sps W in turns per window, τ0 in samples, ε sps W in samples per window); the last two rows sit at
# MAX_DRIFT_TURNS and MAX_DRIFT_SAMPLES together
IMPAIRMENTS = ((40.0, 0.025, 6.0, 0.8), (-70.0, -0.05, -5.3, -1.6), (130.0, 0.05, 2.7, 1.6))


def _impair(sig, imp):
    th, nuw, tau0, epsw = imp
    return T.timing_offset_host(C.carrier_offset_host(sig, math.radians(th), nuw / (SPS * W)), tau0, epsw / (SPS * W))


def _differ(bits, want, guard, shifts):
    """Decisions that differ from ``want`` outside ``guard`` rows at each end, at the best of the row shifts."""
    w = want[guard:want.size - guard]
    return min(int(np.count_nonzero(bits[guard + sh:bits.size - guard + sh] != w)) for sh in shifts)


# ------------------------------------------------------------------------------------------------ CPU
def test_joint_entry_points_exported_bound_and_declared():
    from pathlib import Path

    from waveforms_amd import _hip, device

    header = (Path(__file__).resolve().parent.parent / "include" / "wfhip.h").read_text()
    lib = _hip.lib()
    for name in NAMES:
        assert name in _hip.SIGNATURES and hasattr(lib, name) and f"int {name}(" in header, name
    for name in ("rows_derotate_hyp", "viterbi_soft_branch_segments"):
        assert callable(getattr(device, name))
    for name in ("joint_stat_host", "recover_joint_host"):
        assert callable(getattr(J, name))
    acq = J.JointAcquisition(SPS)
    assert (acq.sps, acq.window, acq.span, acq.timing_hypotheses, acq.carrier_hypotheses, acq.refine, acq.delta, acq.stack) == (8, 256, 5, 4, 8, 1, 2.0, None)
    assert J.MAX_DRIFT_TURNS == C.MAX_DRIFT_TURNS and J.MAX_DRIFT_SAMPLES == T.MAX_DRIFT_SAMPLES
    # the default stacking: everything while the stacked rows fit the stated budget, never less than one hypothesis
    assert acq.stack_for(3999) == 8 and acq.stack_for(211_252) == 8 and acq.stack_for(10 ** 7) == 8 and acq.stack_for(10 ** 10) == 1
    assert 1 <= acq.stack_for(3 * 10 ** 7) < 8 and 48 * acq.stack_for(3 * 10 ** 7) * (-(-3 * 10 ** 7 // W) * W) <= J.STACK_BYTES


def test_joint_argument_validation_without_a_gpu():
    """Bad arguments return WF_ERR_VALUE before anything is launched (a fake context: no device exists here)."""
    from waveforms_amd import _hip

    lib = _hip.lib()
    fake = ctypes.create_string_buffer(1 << 16)
    buf = ctypes.create_string_buffer(1 << 16)
    a = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    b, c, d = a + 16384, a + 32768, a + 49152
    V = _hip.WF_ERR_VALUE
    # wf_rows_derotate_hyp(ctx, rows, ncalls, H, stride, out, stream): out of place only
    good = (fake, a, 10, 2, 64, b)
    for i, v in ((0, None), (1, None), (5, None), (2, 0), (3, 0), (3, 257), (4, 0), (4, 8), (4, 96), (4, 1 << 40), (1, a + 8), (5, b + 8), (5, a), (5, a + 96),
                 (1, b + 48)):
        args = good[:i] + (v,) + good[i + 1:]
        assert lib.wf_rows_derotate_hyp(*args, None) == V, args
    # wf_viterbi4_soft_branch_segments(ctx, rows, nseg, seglen, stride, row_bytes, differential, warmup, llr, bits, branch, stream)
    good = (fake, a, 2, 9, 10, 48, 1, 0, b, c, d)
    for i, v in ((0, None), (1, None), (8, None), (9, None), (2, 0), (2, (1 << 20) + 1), (3, 0), (3, 11), (4, 11), (4, 8), (4, 1 << 40), (5, 40), (7, -1),
                 (1, a + 8), (8, b + 4), (5, 32)):
        args = good[:i] + (v,) + good[i + 1:]
        assert lib.wf_viterbi4_soft_branch_segments(*args, None) == V, args
    # ... and the Python layer's own
    for kw in ({"window": 96}, {"span": 4}, {"timing_hypotheses": 2}, {"timing_hypotheses": 65}, {"carrier_hypotheses": 0}, {"carrier_hypotheses": 257},
               {"refine": -1}, {"delta": 0.0}, {"delta": float("nan")}, {"sps": 0}, {"stack": 0}, {"stack": 9}):
        with pytest.raises(ValueError):
            J.JointAcquisition(**{"sps": SPS, **kw})
    assert J.JointAcquisition(SPS, stack=1).stack_for(10 ** 7) == 1 and J.JointAcquisition(SPS, carrier_hypotheses=4, stack=4).stack_for(100) == 4
    with pytest.raises(ValueError):
        J.joint_stat_host(np.zeros((4, 8, 2)))


def test_joint_stat_takes_the_first_of_equal_minima_and_ignores_the_order_of_the_rotations():
    rng = np.random.default_rng(5)
    S = rng.standard_normal((4, 8, 6, 2)) * 50.0 - 2000.0
    S[1, 2, 3, 0] = S[1, 5, 3, 0] = -9000.0                    # an exact tie between two rotations
    S[2, :, 4, 0] = -2000.0                                    # all equal
    M, which = J.joint_stat_host(S)
    assert M.shape == (4, 6, 2) and which.shape == (4, 6) and which.dtype == np.uint8
    assert np.array_equal(M[:, :, 0], S[:, :, :, 0].min(axis=1)) and not M[:, :, 1].any()
    assert which[1, 3] == 2 and which[2, 4] == 0 and M[1, 3, 0] == -9000.0
    for r in range(1, 8):
        rolled, wr = J.joint_stat_host(np.roll(S, r, axis=1))
        assert np.array_equal(rolled, M)
        assert wr[1, 3] == min((2 + r) % 8, (5 + r) % 8) and wr[2, 4] == 0


@pytest.fixture(scope="module")
def pt_burst(oracle):
    """3 999 noiseless PT rows' worth of samples and the genie's decisions."""
    sig, _noise, taps, first, ncols = _chain(oracle, 4000)
    genie = C.map_branch_host(T.mf_bank_resample_host(sig, taps, first, SPS, ncols)[0])[1]
    return sig, taps, first, ncols, genie


def test_one_symbol_later_and_a_quarter_turn_is_the_same_burst_one_row_later(pt_burst):
    """The alias that makes the joint lattice finer than either recovery's: sampled at ±sps and derotated by ±π/2 the
    differential decisions are the genie's, shifted by ONE row, not inverted; without the rotation they are not."""
    sig, taps, first, ncols, genie = pt_burst
    guard = 300
    for sgn in (1, -1):
        rows = T.mf_bank_resample_host(sig, taps, first, SPS, ncols, tau0=float(sgn * SPS))[0]
        want = genie[guard + sgn:ncols - guard + sgn]
        for turn in (0.5 * math.pi, -0.5 * math.pi):
            bits = C.map_branch_host(C.derotate_host(rows, phase0=turn))[1]
            assert np.count_nonzero(bits[guard:ncols - guard] != want) == 0, (sgn, turn)
        plain = C.map_branch_host(rows)[1]
        lost = min(int(np.count_nonzero(plain[guard:ncols - guard] != genie[guard + sh:ncols - guard + sh])) for sh in (-1, 0, 1))
        print(f"sampled {sgn * SPS:+d} samples off, no rotation: {lost} decisions differ at the best shift in -1 .. +1")
        assert lost > 100


@pytest.mark.parametrize("imp", IMPAIRMENTS, ids=["40deg", "limits-", "limits+"])
def test_recover_joint_host_at_defaults(pt_burst, imp):
    """Defaults (Ht 4, Hc 8, W 256, span 5, one refinement at ±2): the decisions after the acquisition are the unimpaired burst's
    outside a guard of one window at each end, at the best shift in -3 .. +3 rows (the lattice); the trajectories' mean slopes
    are the impairment's."""
    sig, taps, first, ncols, genie = pt_burst
    _th, nuw, _tau0, epsw = imp
    bad = _impair(sig, imp)
    rows, tau, phase, tchoice, cchoice = J.recover_joint_host(bad, taps, first, ncols, SPS)
    nwin = -(-ncols // W)
    assert rows.shape == (ncols, 3) and tau.shape == phase.shape == tchoice.shape == cchoice.shape == (nwin,)
    assert _differ(C.map_branch_host(rows)[1], genie, W, range(-3, 4)) == 0
    # without the recovery the burst is lost: otherwise the line above shows nothing
    lost = _differ(C.map_branch_host(T.mf_bank_resample_host(bad, taps, first, SPS, ncols)[0])[1], genie, W, range(-3, 4))
    ts, ps = float(np.diff(tau)[4:-4].mean()), float(np.diff(phase)[4:-4].mean()) / (2.0 * math.pi)
    print(f"{imp}: {lost} decisions lost without the recovery; mean slope per window: tau {ts:+.4f} samples, phase {ps:+.5f} turns")
    assert lost > 300
    assert abs(ts + epsw) < 0.03
    assert abs(ps - nuw) < 0.002


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture
def ctx():
    from waveforms_amd import _hip

    handle = _hip.new_ctx()
    yield handle
    _hip.free_ctx(handle)


def _counters(dev, handle):
    return dev.viterbi_unmerged(reset=True, ctx=handle), dev.viterbi_repaired(reset=True, ctx=handle)


@pytest.fixture(scope="module")
def pools(oracle):
    """32 100 PT rows of the reference chain, noiseless and at 3 dB: what the segments are cut from."""
    out = {}
    for ebn0 in (None, 3.0):
        sig, noise, taps, first, ncols = _chain(oracle, 32_101, "PT", ebn0)
        out[ebn0] = T.mf_bank_resample_host(sig + noise, taps, first, SPS, ncols)[0]
        assert out[ebn0].shape[0] >= 8 * 4002
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("ncalls", [1, 63, 64, 65, 4001])
@pytest.mark.parametrize("H", [1, 3, 8])
def test_rows_derotate_hyp_bitwise(pools, ctx, H, ncalls):
    """Every copy is ``rows_derotate`` at phase0 = h π / H bit for bit, the pad rows are +0, and nothing is written in front of
    or behind the H stride rows."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    rows = pools[3.0][100:100 + ncalls]
    d_rows = _hip.to_device(rows)
    want = [_hip.to_host(dev.rows_derotate(d_rows, phase0=(h * math.pi) / H, ctx=ctx)).view(np.uint64) for h in range(H)]
    up = -(-ncalls // 64) * 64
    for stride in (up, up + 192):
        guard, sentinel = 4, -7.5
        buf = _hip.to_device(np.full((H * stride + 2 * guard, 3, 2), sentinel))
        out = dev.rows_derotate_hyp(d_rows, H, stride, out=buf[guard:guard + H * stride], ctx=ctx)
        full = _hip.to_host(buf)
        assert (full[:guard] == sentinel).all() and (full[guard + H * stride:] == sentinel).all()
        got = _hip.to_host(out).view(np.uint64).reshape(H, stride, 3, 2)
        for h in range(H):
            assert np.array_equal(got[h, :ncalls], want[h]), (h, stride)
        assert not got[:, ncalls:].any()
    fresh = _hip.to_host(dev.rows_derotate_hyp(d_rows, H, ctx=ctx)).view(np.uint64).reshape(H, up, 3, 2)
    assert all(np.array_equal(fresh[h, :ncalls], want[h]) for h in range(H))
    assert np.array_equal(_hip.to_host(d_rows, True), rows)
    with pytest.raises(ValueError):
        dev.rows_derotate_hyp(d_rows, H, up + 8, ctx=ctx)


_REFS: dict = {}


def _segment_refs(pools, ebn0, seglen, packed, differential):
    """Segment s < 8 is pool rows s (seglen + 1 - seglen % 2) .. + seglen; its reference is the burst entry point on those rows
    alone (default context: the result does not depend on chunking or warm-up) -> [(llr, bits, branch or None)] * 8, on the host."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    key = (ebn0, seglen, packed, differential)
    if key not in _REFS:
        step = seglen + 1 - seglen % 2                         # odd: the segments start on either pool parity
        refs = []
        for s in range(8):
            seg = pools[ebn0][s * step:s * step + seglen]
            if packed:
                llr, bits = dev.viterbi_soft(_hip.to_device(pack_rows(seg)), differential, 0, 32)
                refs.append((seg, _hip.to_host(llr).view(np.uint64), _hip.to_host(bits), None))
            else:
                llr, bits, branch = dev.viterbi_soft_branch(_hip.to_device(seg), differential)
                refs.append((seg, _hip.to_host(llr).view(np.uint64), _hip.to_host(bits), _hip.to_host(branch)))
        _REFS[key] = refs
    return _REFS[key]


@pytest.mark.gpu
@pytest.mark.parametrize("seglen", [1, 2, 31, 33, 517, 4001])
@pytest.mark.parametrize("nseg", [1, 3, 8])
def test_soft_branch_segments_bitwise(pools, ctx, nseg, seglen):
    """Per segment λ, bits and branches are bitwise the burst entry point's on that segment's rows alone: noisy rows at 3 dB and
    noiseless ones, both row forms, both trellises, stride = seglen rounded up to even and to 256, chunks of 32 rows and the
    library's choice, the default warm-up and one of 2 rows (which leaves most chunk starts to the repairs).  33 and 517 end a
    segment one and five rows into a chunk, inside the next chunk's warm-up reach were it not held at the segment's edge.  The pad
    rows are NaN - they are never read - and their outputs are 0.  8 segments of 4 001 rows are 1 008 chunks: four workgroups."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    repaired_any = 0
    for ebn0 in (3.0, None):
        for packed in (False, True):
            for differential in (True, False):
                refs = _segment_refs(pools, ebn0, seglen, packed, differential)
                for stride in sorted({seglen + seglen % 2, -(-seglen // 256) * 256}):
                    buf = np.full((nseg * stride, 3), np.nan + 1j * np.nan)
                    for s in range(nseg):
                        buf[s * stride:s * stride + seglen] = refs[s][0]
                    d_buf = _hip.to_device(pack_rows(buf) if packed else buf)
                    for chunk in (32, 0):
                        _hip.set_option(ctx, _hip.WF_OPT_SOFT_CHUNK_CALLS, chunk)
                        for warmup in (0, 2):
                            _counters(dev, ctx)
                            llr, bits, branch = dev.viterbi_soft_branch_segments(d_buf, nseg, seglen, stride, differential, warmup, 32 if packed else 48,
                                                                                 branch=not packed, ctx=ctx)
                            unproven, repaired = _counters(dev, ctx)
                            assert unproven == 0
                            repaired_any += repaired if warmup == 2 and ebn0 is not None else 0
                            llr, bits = _hip.to_host(llr).view(np.uint64).reshape(nseg, stride), _hip.to_host(bits).reshape(nseg, stride)
                            branch = None if packed else _hip.to_host(branch).reshape(nseg, stride)
                            where = (ebn0, packed, differential, stride, chunk, warmup)
                            for s in range(nseg):
                                _seg, want_llr, want_bits, want_branch = refs[s]
                                assert np.array_equal(llr[s, :seglen], want_llr), (where, s)
                                assert np.array_equal(bits[s, :seglen], want_bits), (where, s)
                                assert packed or np.array_equal(branch[s, :seglen], want_branch), (where, s)
                            assert not llr[:, seglen:].any() and not bits[:, seglen:].any() and (packed or not branch[:, seglen:].any()), where
    if seglen >= 517:
        assert repaired_any > 0                                # a 2-row warm-up at 3 dB: the repairs ran, and the results above are theirs


@pytest.mark.gpu
def test_one_segment_without_pad_is_the_plain_entry_point(pools, ctx):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    d_rows = _hip.to_device(pools[3.0][7:7 + 4002])
    want = dev.viterbi_soft_branch(d_rows, True, ctx=ctx)
    got = dev.viterbi_soft_branch_segments(d_rows, 1, 4002, 4002, True, ctx=ctx)
    assert np.array_equal(_hip.to_host(got[0]).view(np.uint64), _hip.to_host(want[0]).view(np.uint64))
    assert np.array_equal(_hip.to_host(got[1]), _hip.to_host(want[1])) and np.array_equal(_hip.to_host(got[2]), _hip.to_host(want[2]))
    for bad in ((1, 4002, 4003), (1, 4002, 4000), (2, 4002, 4002), (0, 4002, 4002), (1, 0, 2)):
        with pytest.raises(ValueError):
            dev.viterbi_soft_branch_segments(d_rows, *bad, ctx=ctx)
    with pytest.raises(ValueError):
        dev.viterbi_soft_branch_segments(d_rows, 1, 4002, 4002, row_bytes=32, ctx=ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("ncalls", [300, 3999])
def test_carrier_stat_on_the_stacked_buffer_is_the_separate_statistics(pools, ctx, ncalls):
    """``rows_derotate_hyp`` -> ``viterbi_soft_branch_segments`` -> ONE ``carrier_stat`` over the H stride rows, stride = nwin W, is
    [H, nwin, 2] and equals ``rows_derotate`` -> ``viterbi_soft_branch`` -> ``carrier_stat`` per hypothesis bit for bit."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    H = 8
    nwin = -(-ncalls // W)
    stride = nwin * W
    d_rows = _hip.to_device(pools[3.0][:ncalls])
    want = np.empty((H, nwin, 2))
    for h in range(H):
        turned = dev.rows_derotate(d_rows, phase0=(h * math.pi) / H, ctx=ctx)
        want[h] = _hip.to_host(dev.carrier_stat(turned, dev.viterbi_soft_branch(turned, True, ctx=ctx)[2], W, ctx=ctx))
    stacked = dev.rows_derotate_hyp(d_rows, H, stride, ctx=ctx)
    branch = dev.viterbi_soft_branch_segments(stacked, H, ncalls, stride, True, ctx=ctx)[2]
    got = _hip.to_host(dev.carrier_stat(stacked, branch, W, ctx=ctx)).reshape(H, nwin, 2)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def _host_gaps(bad, taps, first, ncols):
    """The host statement's coarse tables, restated from its public stages: (gap between the two best timing candidates per
    window, gap between the two best carrier candidates per window, the largest |X| among each window's candidates)."""
    def stat(z):
        return C.carrier_stat_host(z, C.map_branch_host(z)[2], W)

    S = np.asarray([[stat(C.derotate_host(T.mf_bank_resample_host(bad, taps, first, SPS, ncols, W, None, float(s))[0], phase0=(c * math.pi) / 8))
                     for c in range(8)] for s in T.hypothesis_instants(float(SPS), 4)])
    M = J.joint_stat_host(S)[0]
    tau = T.rescale_host(T.timing_track_host(M, float(SPS), 5)[0], float(SPS) * W)
    rows = T.mf_bank_resample_host(bad, taps, first, SPS, ncols, W, tau)[0]
    Cx = np.asarray([stat(C.derotate_host(rows, phase0=(c * math.pi) / 8))[:, 0] for c in range(8)])
    tg, cg = np.sort(M[:, :, 0], axis=0), np.sort(Cx, axis=0)
    return tg[1] - tg[0], cg[1] - cg[0], np.maximum(np.abs(M[:, :, 0]).max(axis=0), np.abs(Cx).max(axis=0))


@pytest.fixture(scope="module")
def joint_bursts(oracle):
    """3 999 PT rows under the first impairment, noiseless and at 8 dB, with the host statement's result and its coarse gaps."""
    out = {}
    for ebn0 in (None, 8.0):
        sig, noise, taps, first, ncols = _chain(oracle, 4000, "PT", ebn0)
        bad = _impair(sig, IMPAIRMENTS[0]) + noise
        out[ebn0] = (bad, taps, first, ncols, J.recover_joint_host(bad, taps, first, ncols, SPS), _host_gaps(bad, taps, first, ncols))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("ebn0", [None, 8.0])
def test_joint_acquisition_against_the_host_statement(joint_bursts, ctx, ebn0):
    """The coarse choices are the host's wherever its two best candidates lie further apart than the sums' rounding: the device's
    rows agree with the host's within (ntaps + 12) 2^-53 of their absolute-value sums (tests/test_timing.py) and a window adds 256
    terms, (21 + 256) 2^-53 < 2^-44 of the terms' absolute sum; 2^-36 of the window's largest |X| leaves that eight bits of room.
    The host statement's smallest gaps on these bursts are GAP_NOTE below - seven orders of magnitude above the bound - so no
    window is excluded; at most 1 of the 16 may be.  tau within 0.05 samples and the phase within 0.01 rad of the host's outside
    two windows at each end; the detector decides the device's rows as the host's outside one window."""
    # GAP_NOTE (the host statement's 16 windows; the bound is 3.0e-8 at the largest |X| of 2.1e3):
    #   noiseless: smallest timing gap 2.38, smallest carrier gap 7.76;   8 dB: smallest timing gap 1.43, smallest carrier gap 4.39
    #   (the timing gaps are small where the minimum lies halfway between two of the four instants; the vertex handles that)
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    bad, taps, first, ncols, (host_rows, host_tau, host_phase, host_tch, host_cch), (tgap, cgap, scale) = joint_bursts[ebn0]
    print(f"Eb/N0 {ebn0}: smallest gap of the host's two best candidates: timing {tgap.min():.3g}, carrier {cgap.min():.3g}; largest |X| {scale.max():.3g}")
    acq = J.JointAcquisition(SPS)
    acq.times = True
    rows, tau, phase, tch, cch = acq.recover(_hip.to_device(bad), _hip.to_device(taps), first, ncols, True, ctx=ctx)
    bound = 2.0 ** -36 * scale
    clear = (tgap > bound) & (cgap > bound)
    assert np.count_nonzero(~clear) <= 1
    assert np.array_equal(_hip.to_host(tch)[clear], host_tch[clear]) and np.array_equal(_hip.to_host(cch)[clear], host_cch[clear])
    dt, dp = np.abs(_hip.to_host(tau) - host_tau), np.abs(_hip.to_host(phase) - host_phase)
    print(f"   |tau - host| <= {dt[2:-2].max():.3g} samples, |phase - host| <= {dp[2:-2].max():.3g} rad (windows 2 .. -3); stages {acq.stage_times()}, {acq.launches} launches")
    assert dt[2:-2].max() < 0.05 and dp[2:-2].max() < 0.01
    bits = _hip.to_host(dev.viterbi_soft_branch(rows, True, ctx=ctx)[1])
    assert np.array_equal(bits[W:-W], C.map_branch_host(host_rows)[1][W:-W])
    assert {"resample", "derotate", "soft_branch", "stat", "min", "track", "rescale", "add"} == set(acq.stage_times())


@pytest.mark.gpu
@pytest.mark.parametrize("ebn0", [None, 8.0])
def test_unstacked_and_stacked_acquisition_agree_bitwise(joint_bursts, ctx, ebn0):
    """``stack=1`` (the existing entry points per hypothesis), ``stack=3`` (groups of 3, 3 and 2 copies written copy by copy) and
    the default (all 8 in one set of launches): the same tau, phase, choices and rows bit for bit."""
    from waveforms_amd import _hip

    bad, taps, first, ncols = joint_bursts[ebn0][:4]
    d_bad, d_taps = _hip.to_device(bad), _hip.to_device(taps)
    got = []
    for stack in (1, 3, None):
        acq = J.JointAcquisition(SPS, stack=stack)
        out = acq.recover(d_bad, d_taps, first, ncols, True, ctx=ctx)
        got.append(([_hip.to_host(v) for v in out], acq.launches))
    for other, _n in got[1:]:
        for a, b in zip(got[0][0], other):
            assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert got[0][1] > got[1][1] > got[2][1]                   # launches: 6 Hc per coarse pass unstacked, 7 stacked
