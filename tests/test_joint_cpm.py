"""Joint carrier and timing acquisition for the generic CPM chains (waveforms_amd/sync/joint_cpm.py; include/wfhip.h:
wf_cpm_soft_branch_segments, wf_cpm_soft_segments_geometry).

CPU: the entry points and the class's checks, ``joint_cpm_stat_host`` at its ties and folds, the lattice of the joint statistic
(one period later is the same burst on the phase grid turned by P/2, nh calls later) and ``recover_cpm_joint_host`` under three
joint impairments, two of them at both documented limits.
GPU: the stacked detector bit for bit against the burst entry point, the statistics on its stacked outputs, and the device
acquisition against its unstacked form and against the host statement.
"""
import ctypes
import math

import numpy as np
import pytest

from test_cpm_timing import NOISY_DB, SPS, WAVEFORMS, _chain, _differ_up_to_a_period, ref, soft_c  # noqa: F401  (ref: a fixture)
from waveforms_amd.sync import carrier_cpm as CC
from waveforms_amd.sync import joint_cpm as JC
from waveforms_amd.sync import timing as T
from waveforms_amd.sync import timing_cpm as TC

NAMES = ("wf_cpm_soft_branch_segments", "wf_cpm_soft_segments_geometry")
WC = 256


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _specs():
    from waveforms_amd.viterbi import cpm

    return {"multih": cpm.ARTM_64, "pcmfm": cpm.PCMFM_20}


# ------------------------------------------------------------------------------------------------ CPU
def test_joint_cpm_entry_points_exported_bound_and_declared():
    from pathlib import Path

    from waveforms_amd import _hip, device

    header = (Path(__file__).resolve().parent.parent / "include" / "wfhip.h").read_text()
    lib = _hip.lib()
    for name in NAMES:
        assert name in _hip.SIGNATURES and hasattr(lib, name) and f"int {name}(" in header, name
    for name in ("cpm_soft_branch_segments", "cpm_soft_segments_geometry"):
        assert callable(getattr(device, name))
    for name in ("joint_cpm_stat_host", "recover_cpm_joint_host"):
        assert callable(getattr(JC, name))
    specs = _specs()
    acq = JC.CPMJointAcquisition(specs["pcmfm"], SPS)
    assert (acq.sps, acq.timing_window, acq.carrier_window, acq.span, acq.timing_hypotheses, acq.carrier_hypotheses, acq.refine, acq.delta) == \
        (8, 256, 256, 5, 8, 2, 1, 2.0)
    acq = JC.CPMJointAcquisition(specs["multih"], SPS)
    assert (acq.timing_window, acq.carrier_window, acq.timing_hypotheses, acq.carrier_hypotheses, acq.delta) == (1024, 256, 16, 2, 1.0)
    assert set(JC.MAX_DRIFT_SAMPLES) == {"pcmfm", "multih"} and all(0.0 < JC.MAX_DRIFT_SAMPLES[k] <= TC.MAX_DRIFT_SAMPLES[k] for k in JC.MAX_DRIFT_SAMPLES)
    assert 0.0 < JC.MAX_DRIFT_PERIODS <= CC.MAX_DRIFT_PERIODS


def test_joint_cpm_argument_validation_without_a_gpu():
    """Bad arguments return WF_ERR_VALUE before the context is touched (a fake context: no device exists here)."""
    from waveforms_amd import _hip
    from waveforms_amd.viterbi import cpm

    lib = _hip.lib()
    fake = ctypes.create_string_buffer(1 << 16)
    buf = ctypes.create_string_buffer(1 << 15)
    a = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    b, c, d, e, f = a + 4096, a + 8192, a + 12288, a + 16384, a + 20480
    V = _hip.WF_ERR_VALUE
    good = cpm.ARTM_64.c_config()

    # wf_cpm_soft_branch_segments(ctx, det, rot, rot_stride, rows, nseg, seglen, row_stride, out_stride, first_call, warmup, llr, bits, branch, term, stream)
    def call(cfg=good, ctx=fake, r=a, rs=1, z=b, nseg=2, seglen=10, row=0, out=64, first=0, warmup=0, llr=c, bits=d, branch=e, term=f):
        return lib.wf_cpm_soft_branch_segments(ctx, None if cfg is None else ctypes.byref(cfg), r, rs, z, nseg, seglen, row, out, first, warmup, llr, bits,
                                               branch, term, None)

    assert call(ctx=None) == V and call(cfg=None) == V and call(r=None) == V and call(z=None) == V
    assert call(llr=None) == V and call(bits=None) == V and call(branch=None) == V
    assert call(term=f + 8) == V and call(z=b + 8) == V and call(r=a + 8) == V and call(llr=c + 4) == V
    for nseg in (0, -1, (1 << 20) + 1):
        assert call(nseg=nseg) == V
    for seglen in (0, -1):
        assert call(seglen=seglen) == V
    for row in (9, 1, -1):                                     # neither 0 nor >= seglen
        assert call(row=row) == V
    for rs in (2, -1):
        assert call(rs=rs) == V
    for out in (0, 9, 63, 65, 96 + 8):                         # < seglen, or not a multiple of 64
        assert call(out=out) == V
    assert call(seglen=65, out=64) == V
    assert call(nseg=1 << 20, out=1 << 21) == V                # nseg out_stride beyond 2^40
    assert call(first=-1) == V and call(warmup=-1) == V
    for spec in (cpm.ARTM_16, cpm.PCMFM_10, cpm.ARTM_256):       # NC != p; 256 states
        assert call(cfg=spec.c_config()) == V
    geom = (ctypes.c_int64 * 5)()
    for args in ((None, ctypes.byref(good), 2, 10, 0, geom), (fake, None, 2, 10, 0, geom), (fake, ctypes.byref(good), 2, 10, 0, None),
                 (fake, ctypes.byref(good), 0, 10, 0, geom), (fake, ctypes.byref(good), 2, 0, 0, geom), (fake, ctypes.byref(good), 2, 10, -1, geom),
                 (fake, ctypes.byref(cpm.ARTM_256.c_config()), 2, 10, 0, geom)):
        assert lib.wf_cpm_soft_segments_geometry(*args) == V, args
    # ... and the Python layer's own
    nan = float("nan")
    for kw in ({"carrier_window": 96}, {"timing_window": 96}, {"timing_window": 384}, {"timing_window": 128}, {"span": 4}, {"timing_hypotheses": 2},
               {"timing_hypotheses": 65}, {"carrier_hypotheses": 0}, {"carrier_hypotheses": 257}, {"refine": -1}, {"delta": 0.0}, {"delta": nan}, {"sps": 0},
               {"stack": 0}, {"stack": 3}, {"anchor": 4}, {"anchor": 33, "max_drift": 100.0}):
        with pytest.raises(ValueError):
            JC.CPMJointAcquisition(**{"spec": cpm.PCMFM_20, "sps": SPS, **kw})
    with pytest.raises(ValueError, match="full-phase"):
        JC.CPMJointAcquisition(cpm.ARTM_16, SPS)
    with pytest.raises(ValueError, match="64"):
        JC.CPMJointAcquisition(cpm.ARTM_256, SPS)
    with pytest.raises(ValueError):
        JC.joint_cpm_stat_host(np.zeros((4, 2, 2)), 1)
    with pytest.raises(ValueError):
        JC.joint_cpm_stat_host(np.zeros((4, 2, 5, 2)), 0)


def test_joint_cpm_stat_ties_order_and_fold():
    """min over the rotations: ties to the first c, the order of the rotations irrelevant to M; the fold adds the carrier windows
    of a timing window in increasing order, the last timing window taking what is left."""
    rng = np.random.default_rng(5)
    S = rng.standard_normal((4, 3, 10, 2)) * 50.0 - 2000.0
    S[1, 0, 3, 0] = S[1, 2, 3, 0] = -9000.0                    # an exact tie between two rotations
    S[2, :, 4, 0] = -2000.0                                    # all equal
    M1, which = JC.joint_cpm_stat_host(S, 1)
    assert M1.shape == (4, 10, 2) and which.shape == (4, 10) and which.dtype == np.uint8
    assert np.array_equal(M1[:, :, 0], S[:, :, :, 0].min(axis=1)) and not M1[:, :, 1].any()
    assert which[1, 3] == 0 and which[2, 4] == 0 and M1[1, 3, 0] == -9000.0
    for r in (1, 2):
        rolled, wr = JC.joint_cpm_stat_host(np.roll(S, r, axis=1), 1)
        assert np.array_equal(rolled, M1)
        assert wr[1, 3] == min(r % 3, (2 + r) % 3) and wr[2, 4] == 0
    m = S[:, :, :, 0].min(axis=1)
    M4, which4 = JC.joint_cpm_stat_host(S, 4)                  # 10 carrier windows: timing windows of 4, 4 and 2
    assert M4.shape == (4, 3, 2) and np.array_equal(which4, which)
    assert np.array_equal(M4[:, 0, 0], ((m[:, 0] + m[:, 1]) + m[:, 2]) + m[:, 3])
    assert np.array_equal(M4[:, 1, 0], ((m[:, 4] + m[:, 5]) + m[:, 6]) + m[:, 7])
    assert np.array_equal(M4[:, 2, 0], m[:, 8] + m[:, 9]) and not M4[:, :, 1].any()
    M16, _ = JC.joint_cpm_stat_host(S, 16)
    assert M16.shape == (4, 1, 2)


# ------------------------------------------------------------------------------------------------ GPU: the stacked detector
@pytest.fixture
def ctx():
    from waveforms_amd import _hip

    handle = _hip.new_ctx()
    yield handle
    _hip.free_ctx(handle)


def _counters(dev, handle):
    return dev.viterbi_unmerged(reset=True, ctx=handle), dev.viterbi_repaired(reset=True, ctx=handle)


NTAB = 8


def _tables(spec):
    """NTAB rotation tables, table t turned by t P / NTAB: float64[NTAB, 2p, 2]."""
    return np.stack([CC.hypothesis_table(spec, (t * CC.period(spec)) / NTAB) for t in range(NTAB)])


@pytest.fixture(scope="module")
def pools(oracle):
    """Per waveform 32 100 noisy rows of the reference chain (ARTM at 8 dB, PCM/FM at 6): what the segments are cut from, on the
    device, with the NTAB tables."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    out = {}
    for wf in WAVEFORMS:
        spec, sig, noise, templates, start0, ncalls = _chain(oracle, wf, 32_110, NOISY_DB[wf])
        assert ncalls >= 8 * 4002
        rows = dev.cpm_mf_rows_resample(_hip.to_device(sig + noise), _hip.to_device(templates), start0, SPS, ncalls)
        out[wf] = (spec, rows, _hip.to_device(_tables(spec)))
    return out


_REFS: dict = {}


def _ref(pools, wf, seglen, first, s, t):
    """``cpm_soft_branch`` of segment s's rows (pool rows s (seglen + 1) .. + seglen) under table t from call ``first``, on the
    default context (the result does not depend on chunking or warm-up) -> (llr as uint64, bits, branch, term as uint64), on the host."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    key = (wf, seglen, first, s, t)
    if key not in _REFS:
        spec, rows, tabs = pools[wf]
        seg = rows[s * (seglen + 1):s * (seglen + 1) + seglen].contiguous()
        llr, bits, branch, term = dev.cpm_soft_branch(seg, spec, first, 0, d_rot=tabs[t].contiguous())
        _REFS[key] = (_hip.to_host(llr).view(np.uint64), _hip.to_host(bits), _hip.to_host(branch), _hip.to_host(term).view(np.uint64))
    return _REFS[key]


@pytest.mark.gpu
@pytest.mark.parametrize("seglen", [1, 2, 15, 16, 17, 65, 517, 4001])
@pytest.mark.parametrize("nseg", [1, 3, 8])
@pytest.mark.parametrize("wf", WAVEFORMS)
def test_cpm_soft_branch_segments_bitwise(pools, ctx, wf, nseg, seglen):
    """Per segment λ, bits, branches and terms are bitwise ``cpm_soft_branch`` on that segment's rows, table and first call alone:
    the three uses (one set of rows under nseg tables; nseg sets of rows under one table; both), first_call 0 and 3, out_stride the
    smallest multiple of 64 and a larger one, the library's geometry and chunks of 16 calls with a warm-up of 16 (which leaves most
    chunk starts to the repairs: the rows are noisy).  15, 17, 65, 517 and 4001 end a segment inside a chunk of 16, within the next
    segment's warm-up reach were it not held at the segment's edge.  The rows between two segments are NaN - they are never read
    - and the pad outputs are 0.  8 segments of 4 001 calls in chunks of 16 are 2 008 chunks: 502 workgroups."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    spec, rows, tabs = pools[wf]
    lg, nf = spec.bits_per_symbol, spec.nfilt
    row_stride = seglen + 3
    gapped = _hip.to_device(np.full(((nseg - 1) * row_stride + seglen, nf, 2), np.nan))
    for s in range(nseg):
        gapped[s * row_stride:s * row_stride + seglen] = rows[s * (seglen + 1):s * (seglen + 1) + seglen]
    first_rows = rows[:seglen].contiguous()
    up = -(-seglen // 64) * 64
    repaired_any = 0
    for chunk, warmup in ((0, 0), (16, 16)):
        _hip.set_option(ctx, _hip.WF_OPT_CPM_SOFT_CHUNK_CALLS, chunk)
        geo = dev.cpm_soft_segments_geometry(spec, nseg, seglen, warmup, ctx=ctx)
        assert geo["chunks"] == nseg * geo["chunks_per_segment"] and geo["chunks_per_segment"] == -(-seglen // geo["chunk_calls"])
        assert chunk == 0 or (geo["chunk_calls"], geo["warmup"]) == (16, 16)
        for first in (0, 3):
            for rs, ts in ((0, 1), (row_stride, 0), (row_stride, 1)):
                for out_stride in (up, up + 192):
                    _counters(dev, ctx)
                    llr, bits, branch, term = dev.cpm_soft_branch_segments(first_rows if rs == 0 else gapped, spec, nseg, seglen, rs, out_stride, tabs, ts,
                                                                           first, warmup, ctx=ctx)
                    unproven, repaired = _counters(dev, ctx)
                    assert unproven == 0
                    repaired_any += repaired if chunk else 0
                    llr = _hip.to_host(llr).view(np.uint64).reshape(nseg, out_stride, lg)
                    bits = _hip.to_host(bits).reshape(nseg, out_stride, lg)
                    branch = _hip.to_host(branch).reshape(nseg, out_stride)
                    term = _hip.to_host(term).view(np.uint64).reshape(nseg, out_stride, 2)
                    where = (chunk, first, rs, ts, out_stride)
                    for s in range(nseg):
                        want = _ref(pools, wf, seglen, first, s if rs else 0, s if ts else 0)
                        assert np.array_equal(llr[s, :seglen].reshape(-1), want[0]), (where, s)
                        assert np.array_equal(bits[s, :seglen].reshape(-1), want[1]), (where, s)
                        assert np.array_equal(branch[s, :seglen], want[2]), (where, s)
                        assert np.array_equal(term[s, :seglen], want[3]), (where, s)
                    assert not llr[:, seglen:].any() and not bits[:, seglen:].any() and not branch[:, seglen:].any() and not term[:, seglen:].any(), where
    print(f"{wf}, {nseg} x {seglen}: {repaired_any} chunk repairs with chunks of 16 calls and a warm-up of 16")
    if seglen >= 65:                                           # (up to 17 calls every chunk's warm-up reaches its segment's start: exact)
        assert repaired_any > 0                                # the repairs ran, and the results above are theirs


@pytest.mark.gpu
@pytest.mark.parametrize("wf", WAVEFORMS)
def test_one_cpm_segment_without_pad_is_the_plain_entry_point(pools, ctx, wf):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    spec, rows, tabs = pools[wf]
    n = 4032
    d_rows = rows[7:7 + n].contiguous()
    want = dev.cpm_soft_branch(d_rows, spec, 0, 0, ctx=ctx, d_rot=tabs[0].contiguous())
    got = dev.cpm_soft_branch_segments(d_rows, spec, 1, n, 0, n, tabs, 0, ctx=ctx)
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(_hip.to_host(g).view(np.uint8), _hip.to_host(w).view(np.uint8))
    got = dev.cpm_soft_branch_segments(d_rows, spec, 1, n, 0, n, tabs, 0, ctx=ctx, terms=False)
    assert got[3] is None and np.array_equal(_hip.to_host(got[2]), _hip.to_host(want[2]))
    for bad in ((1, n, 5, n), (1, n, 0, n - 64), (1, n, 0, n + 8), (2, n, n, n), (0, n, 0, n), (1, 0, 0, 64)):
        with pytest.raises(ValueError):
            dev.cpm_soft_branch_segments(d_rows, spec, *bad, tabs, 0, ctx=ctx)
    with pytest.raises(ValueError):
        dev.cpm_soft_branch_segments(d_rows, spec, 1, n, 0, n, tabs, 2, ctx=ctx)
    with pytest.raises(ValueError):
        dev.cpm_soft_branch_segments(d_rows, spec, 2, n, 0, n, tabs[0].contiguous(), 1, ctx=ctx)       # two tables asked of one


@pytest.mark.gpu
@pytest.mark.parametrize("ncalls", [300, 3999])
@pytest.mark.parametrize("wf", WAVEFORMS)
def test_statistics_on_the_stacked_outputs_are_the_separate_statistics(pools, ctx, wf, ncalls):
    """ONE ``llr_stat`` and ONE ``carrier_stat_terms`` over the nseg out_stride stacked calls, out_stride = nwin W, are [nseg, nwin, 2]
    and equal the statistics of ``cpm_soft_branch`` per table bit for bit."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    spec, rows, tabs = pools[wf]
    lg = spec.bits_per_symbol
    nwin = -(-ncalls // WC)
    d_rows = rows[11:11 + ncalls].contiguous()
    want_l, want_t = np.empty((NTAB, nwin, 2)), np.empty((NTAB, nwin, 2))
    for t in range(NTAB):
        llr, _bits, _branch, term = dev.cpm_soft_branch(d_rows, spec, 0, 0, ctx=ctx, d_rot=tabs[t].contiguous())
        want_l[t] = _hip.to_host(dev.llr_stat(llr, lg, WC, ctx=ctx))
        want_t[t] = _hip.to_host(dev.carrier_stat_terms(term, WC, ctx=ctx))
    llr, _bits, _branch, term = dev.cpm_soft_branch_segments(d_rows, spec, NTAB, ncalls, 0, nwin * WC, tabs, 1, ctx=ctx)
    got_l = _hip.to_host(dev.llr_stat(llr, lg, WC, ctx=ctx)).reshape(NTAB, nwin, 2)
    got_t = _hip.to_host(dev.carrier_stat_terms(term, WC, ctx=ctx)).reshape(NTAB, nwin, 2)
    assert np.array_equal(got_l.view(np.uint64), want_l.view(np.uint64))
    assert np.array_equal(got_t.view(np.uint64), want_t.view(np.uint64))


# ------------------------------------------------------------------------------------------------ CPU: the host statement
def detect_c(ref, spec):
    """``detect(rows, rot)`` -> (λ, x, y) from tests/cpm_carrier_ref.c: the detector of ``cpm_map_branch_host``, fast."""
    K = (ctypes.c_int * 2)(*(list(spec.K) + [0])[:2])

    def detect(rows, rot=None):
        rows = np.ascontiguousarray(rows, dtype=np.complex128).reshape(-1, spec.nfilt)
        n, lg = rows.shape[0], spec.bits_per_symbol
        llr, bits = np.empty(n * lg), np.empty(n * lg, dtype=np.uint8)
        branch, term = np.empty(n, dtype=np.uint8), np.empty((n, 2))
        rot = np.ascontiguousarray(CC.hypothesis_table(spec) if rot is None else rot)
        assert ref[1].cpm_soft_branch_rows(spec.M, spec.p, len(spec.K), K, spec.Lp, _p(rot), _p(rows), ctypes.c_int64(n), ctypes.c_int64(0),
                                           _p(llr), _p(bits), _p(branch), _p(term)) == 0
        return llr, term[:, 0].copy(), term[:, 1].copy()

    return detect


# ARTM's coarse search with every second instant (two samples apart, inside its well of +-1.5 samples): the burst stays 8 timing
# windows long and the three cases within the time the CPU suite allows.  PCM/FM carries the full grid.
HT = {"pcmfm": None, "multih": 8}
NSYM = {"pcmfm": 4000, "multih": 8244}


@pytest.fixture(scope="module")
def bursts(oracle, ref):
    """Per waveform a noiseless burst of the reference chain, the fast detector and the genie's decisions."""
    out = {}
    for wf in WAVEFORMS:
        spec, sig, _noise, Tm, start0, ncalls = _chain(oracle, wf, NSYM[wf])
        detect = detect_c(ref, spec)
        genie = detect(TC.cpm_mf_rows_resample_host(sig, Tm, start0, SPS, ncalls)[0])[0] < 0
        out[wf] = (spec, sig, Tm, start0, ncalls, detect, genie, TC.defaults(spec)["window"])
    return out


def _impair(spec, sig, Wt, deg, fraction, tau0, epsw):
    """``deg`` degrees and ``fraction`` of P per carrier window, then ``tau0`` samples and ``epsw`` samples per timing window."""
    from waveforms_amd.sync import carrier as C

    return T.timing_offset_host(C.carrier_offset_host(sig, math.radians(deg), (fraction / spec.p) / (SPS * WC)), tau0, epsw / (SPS * Wt))


def test_one_period_later_is_the_same_burst_on_the_grid_turned_by_half_a_step(bursts):
    """The symmetry the lattice rests on, as ``timing_cpm.py`` states it: read one period of nh sps samples later, the rows are
    the burst's own nh calls later on a phase grid turned by P/2.  So with the two rotations 0 and P/2 the per-window statistics
    of the late burst are the burst's own, nh calls later, with the rotations SWAPPED, and M - the minimum over them - is the
    same: M has period nh sps in τ.  About two timing windows; the statistics agree to the rounding of the turned table
    (cos and sin of an angle with P/2 added, against P/2 added to the index), 1e-9 of their magnitude."""
    for wf in WAVEFORMS:
        spec, sig, Tm, start0, _ncalls, detect, _genie, Wt = bursts[wf]
        nh, lg, P = len(spec.K), spec.bits_per_symbol, CC.period(spec)
        n = max(2 * Wt, 4 * WC) + nh                           # (four carrier windows at least: the first and the last are left out)
        tables = [CC.hypothesis_table(spec, c * P / 2.0) for c in range(2)]
        rows = TC.cpm_mf_rows_resample_host(sig, Tm, start0, SPS, n)[0]
        late = TC.cpm_mf_rows_resample_host(sig, Tm, start0 + nh * SPS, SPS, n - nh)[0]
        assert np.array_equal(late, rows[nh:])                 # the same rows, nh calls later: only the call index differs
        own = np.stack([TC.llr_stat_host(detect(rows, tables[c])[0][nh * lg:], lg, WC) for c in range(2)])
        got = np.stack([TC.llr_stat_host(detect(late, tables[c])[0], lg, WC) for c in range(2)])
        inner = slice(1, got.shape[1] - 1)                     # (the burst's free start and end differ between the two)
        scale = np.abs(own[:, inner, 0]).max()
        assert np.abs(got[::-1, inner, 0] - own[:, inner, 0]).max() < 1e-9 * scale, wf
        assert np.abs(got[:, inner, 0] - own[:, inner, 0]).max() > 1e-3 * scale, wf       # ... and not without the swap
        M_own, M_got = (JC.joint_cpm_stat_host(s[None], Wt // WC)[0][0, :, 0] for s in (own[:, inner], got[:, inner]))
        assert np.abs(M_got - M_own).max() < 1e-9 * np.abs(M_own).max(), wf


# The scatter of a window's own estimate about the impairment on the host statements, noiseless: τ - the largest standard
# deviation tests/test_cpm_timing.py prints over its six cases per waveform, in samples; the phase - half the spread of the
# matched filters' constant offset that carrier_cpm.py documents (0.9 to 2.6 degrees), in radians, for both waveforms.
TAU_SCATTER = {"pcmfm": 0.158, "multih": 0.071}
PHASE_SCATTER = math.radians(0.85)
# (θ0 in degrees, the drift in P per carrier window over MAX_DRIFT_PERIODS, τ0 in samples, the drift in samples per timing
# window over MAX_DRIFT_SAMPLES): 40 degrees with half of each drift and 6 samples late, then both documented limits at either sign
CASES = ((40.0, 0.5, 6.0, 0.5), (40.0, 1.0, -2.7, 1.0), (40.0, -1.0, 2.7, -1.0))


def _slope_bound(sigma, n):
    """Three standard deviations of the least-squares slope through n windows whose errors are independent with deviation sigma."""
    w = np.arange(n, dtype=np.float64)
    return 3.0 * sigma / float(np.sqrt(((w - w.mean()) ** 2).sum()))


@pytest.mark.parametrize("case", CASES, ids=["40deg-half", "limits+", "limits-"])
@pytest.mark.parametrize("wf", WAVEFORMS)
def test_recover_cpm_joint_host_at_defaults(bursts, wf, case):
    """Defaults per waveform (ARTM: Ht 8): every decision of the plain detector on the recovered rows is the genie's, up to a shift
    by whole periods, outside one timing window at each end; the fitted slopes of τ and of the phase are the impairment's."""
    spec, sig, Tm, start0, ncalls, detect, genie, Wt = bursts[wf]
    deg, cf, tau0, tf = case
    fraction, epsw = cf * JC.MAX_DRIFT_PERIODS, tf * JC.MAX_DRIFT_SAMPLES[wf]
    bad = _impair(spec, sig, Wt, deg, fraction, tau0, epsw)
    rows, tau, phase, tch, cch = JC.recover_cpm_joint_host(spec, bad, Tm, start0, SPS, ncalls, timing_hypotheses=HT[wf], detect=detect)
    nwt, nwc = -(-ncalls // Wt), -(-ncalls // WC)
    assert rows.shape == (ncalls, spec.nfilt) and tau.shape == tch.shape == (nwt,) and phase.shape == cch.shape == (nwc,)
    assert _differ_up_to_a_period(spec, detect(rows)[0] < 0, genie, Wt) == 0
    lost = _differ_up_to_a_period(spec, detect(TC.cpm_mf_rows_resample_host(bad, Tm, start0, SPS, ncalls)[0])[0] < 0, genie, Wt)
    # the slopes: least squares through the windows 2 .. -3 (the two at either end carry the clipped mean's lag).  τ falls by the
    # drift per timing window; the phase rises by fraction P per carrier window of rows that are themselves taken along τ, i.e.
    # per Wc sps (1 - eps) samples: fraction P (1 - eps), the product with 1 - eps being within the bound by far
    ts = float(np.polyfit(np.arange(nwt - 4), tau[2:-2], 1)[0])
    ps = float(np.polyfit(np.arange(nwc - 4), phase[2:-2], 1)[0])
    tb, pb = _slope_bound(TAU_SCATTER[wf], nwt - 4), _slope_bound(PHASE_SCATTER, nwc - 4)
    want_p = fraction * CC.period(spec)
    print(f"{wf} {case}: {lost} decisions differ without the acquisition; slope of tau {ts:+.4f} (drift {-epsw:+.4f}, bound {tb:.4f}) samples per window, "
          f"of the phase {ps:+.5f} (drift {want_p:+.5f}, bound {pb:.5f}) rad per window")
    assert tb < abs(epsw) and abs(ts + epsw) < tb
    assert pb < 0.15 * abs(want_p) and abs(ps - want_p) < pb


# ------------------------------------------------------------------------------------------------ GPU: the acquisition
def _host_gaps(spec, bad, Tm, start0, ncalls, detect, Ht):
    """The host statement's two coarse tables, restated from its public stages -> (per timing window the gap between the two best
    M over the instants and the largest |M|, per carrier window the gap between the two best X over the rotations and the largest |X|)."""
    Wt, lg, P = TC.defaults(spec)["window"], spec.bits_per_symbol, CC.period(spec)
    Ht = TC.defaults(spec)["hypotheses"] if Ht is None else Ht
    per = float(len(spec.K) * SPS)
    tables = [CC.hypothesis_table(spec, c * P / 2.0) for c in range(2)]
    S = np.asarray([[TC.llr_stat_host(detect(TC.cpm_mf_rows_resample_host(bad, Tm, start0, SPS, ncalls, Wt, None, float(s))[0], tables[c])[0], lg, WC)
                     for c in range(2)] for s in T.hypothesis_instants(per, Ht)])
    M = JC.joint_cpm_stat_host(S, Wt // WC)[0][:, :, 0]
    tau = T.rescale_host(T.timing_track_host(JC.joint_cpm_stat_host(S, Wt // WC)[0], per, 5)[0], float(SPS) * Wt)
    rows = TC.cpm_mf_rows_resample_host(bad, Tm, start0, SPS, ncalls, Wt, tau)[0]
    X = np.asarray([CC.carrier_stat_terms_host(*detect(rows, tables[c])[1:], WC)[:, 0] for c in range(2)])
    tg, cg = np.sort(M, axis=0), np.sort(X, axis=0)
    return tg[1] - tg[0], np.abs(M).max(axis=0), cg[1] - cg[0], np.abs(X).max(axis=0)


# calls of the device tests' bursts: PCM/FM 8 windows of 256 and 52 calls, ARTM 4 timing windows of 1024 and 52 calls (Ht 8: the
# host statement stays within seconds)
JOINT_NSYM = {"pcmfm": 2100, "multih": 4148}


@pytest.fixture(scope="module")
def joint_bursts(oracle, ref):
    """Per waveform a burst under 40 degrees, half of each documented drift and 6 samples late, noiseless and noisy (ARTM at 8 dB,
    PCM/FM at 6), with the host statement's result and its coarse gaps."""
    out = {}
    for wf in WAVEFORMS:
        for noisy in (False, True):
            spec, sig, noise, Tm, start0, ncalls = _chain(oracle, wf, JOINT_NSYM[wf], NOISY_DB[wf] if noisy else None, seed=8)
            detect = detect_c(ref, spec)
            Wt = TC.defaults(spec)["window"]
            bad = _impair(spec, sig, Wt, 40.0, 0.5 * JC.MAX_DRIFT_PERIODS, 6.0, 0.5 * JC.MAX_DRIFT_SAMPLES[wf]) + noise
            host = JC.recover_cpm_joint_host(spec, bad, Tm, start0, SPS, ncalls, timing_hypotheses=HT[wf], detect=detect)
            out[wf, noisy] = (spec, bad, Tm, start0, ncalls, detect, host, _host_gaps(spec, bad, Tm, start0, ncalls, detect, HT[wf]))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("wf", WAVEFORMS)
def test_cpm_joint_acquisition_against_the_host_statement(joint_bursts, ctx, wf, noisy):
    """The coarse choices are the host's wherever its best and second-best M (timing) or X (carrier) differ by more than 1e-9 of
    their magnitude; at most 5 % of the windows may be left out that way, and on these bursts the host statement leaves out none
    (GAP_NOTE).  τ within 1e-9 samples and the phase within 1e-9 rad of the host's (tests/test_cpm_timing.py's bound for a
    trajectory whose statistics agree to rounding); the detector decides the device's rows as the host's."""
    # GAP_NOTE, the host statement's smallest gap over its windows as a share of the largest magnitude, computed on the CPU:
    #   PCM/FM noiseless: timing 2.3e-3, carrier 3.1e-4;   at 6 dB: timing 1.6e-2, carrier 2.3e-3
    #   ARTM noiseless:   timing 4.6e-1, carrier 1.1e-3;   at 8 dB: timing 6.4e-2, carrier 1.6e-5
    # (the carrier gaps are small where the phase passes midway between the two rotations; the tracker's angle handles that)
    # - four orders of magnitude above the bound at the least, so no window is left out.
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    spec, bad, Tm, start0, ncalls, detect, (host_rows, host_tau, host_phase, host_tch, host_cch), (tgap, tmag, cgap, cmag) = joint_bursts[wf, noisy]
    tclear, cclear = tgap > 1e-9 * tmag, cgap > 1e-9 * cmag
    out_share = (np.count_nonzero(~tclear) + np.count_nonzero(~cclear)) / float(tclear.size + cclear.size)
    print(f"{wf} noisy {noisy}: smallest gap / magnitude: timing {(tgap / tmag).min():.3g}, carrier {(cgap / cmag).min():.3g}; {100.0 * out_share:.1f} % of the windows left out")
    assert out_share <= 0.05
    acq = JC.CPMJointAcquisition(spec, SPS, timing_hypotheses=HT[wf])
    acq.times = True
    rows, tau, phase, tch, cch = acq.recover(_hip.to_device(bad), _hip.to_device(Tm), start0, ncalls, ctx=ctx)
    assert np.array_equal(_hip.to_host(tch)[tclear], host_tch[tclear]) and np.array_equal(_hip.to_host(cch)[cclear], host_cch[cclear])
    dt, dp = np.abs(_hip.to_host(tau) - host_tau).max(), np.abs(_hip.to_host(phase) - host_phase).max()
    print(f"   |tau - host| <= {dt:.3g} samples, |phase - host| <= {dp:.3g} rad; stages {acq.stage_times()}, {acq.launches} launches")
    assert dt < 1e-9 and dp < 1e-9
    bits = _hip.to_host(dev.cpm_soft(rows, spec, ctx=ctx)[1]).astype(bool)
    assert np.array_equal(bits, detect(host_rows)[0] < 0)
    assert {"resample", "derotate", "soft_branch", "stat", "min", "track", "rescale", "add"} == set(acq.stage_times())


@pytest.mark.gpu
@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("wf", WAVEFORMS)
def test_unstacked_and_stacked_cpm_acquisition_agree_bitwise(joint_bursts, ctx, wf, noisy):
    """``stack=1`` (``cpm_soft_branch`` per table and per buffer) and the stacked form: the same rows, tau, phase and choices bit
    for bit, with and without an anchor; the stacked form makes fewer launches."""
    from waveforms_amd import _hip

    spec, bad, Tm, start0, ncalls = joint_bursts[wf, noisy][:5]
    d_bad, d_T = _hip.to_device(bad), _hip.to_device(Tm)
    for anchor in (0, 33):
        got = []
        for stack in (1, None):
            acq = JC.CPMJointAcquisition(spec, SPS, timing_hypotheses=HT[wf], stack=stack, anchor=anchor)
            out = acq.recover(d_bad, d_T, start0, ncalls, ctx=ctx)
            got.append(([_hip.to_host(v) for v in out], acq.launches))
            assert (acq.timing_found is None) == (anchor == 0) and (acq.carrier_found is None) == (anchor == 0)
        for a, b in zip(got[0][0], got[1][0]):
            assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
        assert got[0][1] > got[1][1]
