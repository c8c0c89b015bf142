"""Symbol timing recovery for the generic CPM chains (waveforms_amd/sync/timing_cpm.py; include/wfhip.h:
wf_cpm_mf_rows_resample_c128, wf_llr_stat).

The definition of wf_cpm_mf_rows_resample_c128 is restated sequentially in C (tests/cpm_timing_ref.c, explicit fma()): the device
must agree with it BITWISE.  The numpy host statement forms every fma exactly and is held to the C restatement within the
running-error bound (and, as it happens, to the bit).  The detector behind the statistic is restated in tests/cpm_carrier_ref.c
(the 64-state host passes are slow in numpy).

CPU: the host statements at their edges, the three facts the design rests on (the statistic's wells, their period of nh symbols,
the phase grid turned by P/2 one period off) and ``recover_cpm_timing_host`` at the documented drift.
GPU: every device stage against its restatement, and the whole recovery end to end.
"""
import ctypes
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_timing import _trajectories
from waveforms_amd.sync import carrier as C
from waveforms_amd.sync import carrier_cpm as CC
from waveforms_amd.sync import timing as T
from waveforms_amd.sync import timing_cpm as TC

SPS = 8
U = 2.0 ** -53
HERE = Path(__file__).resolve().parent
NAMES = ("wf_cpm_mf_rows_resample_c128", "wf_cpm_mf_rows_resample_geometry", "wf_llr_stat")
WAVEFORMS = ["pcmfm", "multih"]
NOISY_DB = {"multih": 8.0, "pcmfm": 6.0}


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    """The two C restatements: (cpm_timing_ref.c, cpm_carrier_ref.c)."""
    libs = []
    for name in ("cpm_timing_ref", "cpm_carrier_ref"):
        so = tmp_path_factory.mktemp(name) / f"lib{name}.so"
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", str(so), str(HERE / f"{name}.c"), "-lm"])
        libs.append(ctypes.CDLL(str(so)))
    libs[0].cpm_mf_rows_resample_ref.restype = ctypes.c_int
    libs[1].cpm_soft_branch_rows.restype = ctypes.c_int
    return tuple(libs)


def restate(ref, r, templates, start0, sps, ncalls, window=64, tau=None, tau0=0.0):
    """tests/cpm_timing_ref.c -> rows complex128[ncalls, nfilt]."""
    r = np.ascontiguousarray(r, dtype=np.complex128)
    Tm = np.ascontiguousarray(templates, dtype=np.complex128)
    nh, nfilt, ntm = Tm.shape
    out = np.empty((ncalls, nfilt), dtype=np.complex128)
    tau = None if tau is None else np.ascontiguousarray(tau, dtype=np.float64)
    assert ref[0].cpm_mf_rows_resample_ref(_p(r), ctypes.c_int64(r.size), _p(Tm), nh, nfilt, ntm, ctypes.c_int64(start0), int(sps),
                                           ctypes.c_int64(ncalls), int(window), None if tau is None else _p(tau),
                                           ctypes.c_int64(0 if tau is None else tau.size), ctypes.c_double(tau0), _p(out)) == 0
    return out


def soft_c(ref, spec):
    """``soft(rows, rot)`` -> λ from tests/cpm_carrier_ref.c: the detector of ``cpm_map_branch_host``, fast."""
    K = (ctypes.c_int * 2)(*(list(spec.K) + [0])[:2])

    def soft(rows, rot=None):
        rows = np.ascontiguousarray(rows, dtype=np.complex128).reshape(-1, spec.nfilt)
        n, lg = rows.shape[0], spec.bits_per_symbol
        llr, bits = np.empty(n * lg), np.empty(n * lg, dtype=np.uint8)
        branch, term = np.empty(n, dtype=np.uint8), np.empty((n, 2))
        rot = np.ascontiguousarray(CC.hypothesis_table(spec) if rot is None else rot)
        assert ref[1].cpm_soft_branch_rows(spec.M, spec.p, len(spec.K), K, spec.Lp, _p(rot), _p(rows), ctypes.c_int64(n), ctypes.c_int64(0),
                                           _p(llr), _p(bits), _p(branch), _p(term)) == 0
        return llr

    return soft


def _chain(oracle, waveform, nsym, ebn0=None, seed=5):
    """The reference chain on random symbols up to the channel: (full-phase spec, signal, noise, templates complex128[nh, nfilt, 9],
    start0, ncalls)."""
    from waveforms_amd.viterbi import cpm

    rng = np.random.default_rng(seed)
    if waveform == "multih":
        sym, pulse = oracle.multih_mapper(rng.integers(0, 2, 2 * nsym).astype(np.uint8))[0], oracle.freq_pulse_multih_irig(SPS)
        ospec, spec = oracle.ARTM_64, cpm.ARTM_64
    else:
        sym, pulse = oracle.pcmfm_mapper(rng.integers(0, 2, nsym).astype(np.uint8)), oracle.freq_pulse_pcmfm(SPS)
        ospec, spec = oracle.CPMDetectorSpec(M=2, p=10, K=(7,), Lp=2, NC=10, D=32), cpm.PCMFM_20
    h = np.asarray(ospec.K, dtype=np.float64) / ospec.p
    _t, sig = oracle.cpm_modulate(np.asarray(sym, dtype=np.int8), h if h.size > 1 else float(h[0]), pulse, SPS)
    sig = sig * np.exp(-1j * np.pi / 4)
    noise = np.zeros(sig.size, dtype=np.complex128)
    if ebn0 is not None:
        noise = oracle.numpy_awgn(oracle.cpm_sigma_for_ebn0(ebn0, SPS, spec.bits_per_symbol), sig.size, np.random.Generator(np.random.PCG64(seed)))
    geo = oracle.cpm_geometry(pulse, SPS, ospec, np.asarray(sym).size)
    return spec, sig, noise, np.ascontiguousarray(oracle.cpm_templates(pulse, SPS, ospec)), int(geo["start0"]), int(geo["ncalls"])


def _differ_up_to_a_period(spec, bits, genie, guard):
    """Symbols decided otherwise than the genie's outside ``guard`` calls at each end, at the best of the shifts 0, +nh, -nh calls."""
    lg, nh = spec.bits_per_symbol, len(spec.K)
    bits, genie = bits.reshape(-1, lg), genie.reshape(-1, lg)
    want = genie[guard:genie.shape[0] - guard]
    return min(int(np.count_nonzero((bits[guard + sh:bits.shape[0] - guard + sh] != want).any(axis=1))) for sh in (0, nh, -nh))


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# ------------------------------------------------------------------------------------------------ CPU
def test_cpm_timing_entry_points_exported_bound_and_declared():
    import inspect

    from waveforms_amd import _hip, device
    from waveforms_amd.encoding import coded
    from waveforms_amd.viterbi import cpm

    header = (HERE.parent / "include" / "wfhip.h").read_text()
    lib = _hip.lib()
    for name in NAMES:
        assert name in _hip.SIGNATURES and hasattr(lib, name) and f"int {name}(" in header, name
    for name in ("cpm_mf_rows_resample", "cpm_mf_rows_resample_geometry", "llr_stat"):
        assert callable(getattr(device, name))
    for name in ("cpm_mf_rows_resample_host", "llr_stat_host", "recover_cpm_timing_host"):
        assert callable(getattr(TC, name))
    rec = TC.CPMTimingRecovery(cpm.PCMFM_20, SPS)
    assert (rec.sps, rec.window, rec.span, rec.hypotheses, rec.refine, rec.delta) == (8, 256, 5, 8, 1, 2.0)
    rec = TC.CPMTimingRecovery(cpm.ARTM_64, SPS)
    assert (rec.sps, rec.span, rec.hypotheses, rec.refine, rec.delta) == (8, 5, 16, 1, 1.0) and rec.window in (256, 512, 1024)
    assert set(TC.MAX_DRIFT_SAMPLES) == {"pcmfm", "multih"} and 0.0 < TC.MAX_DRIFT_SAMPLES["multih"] < TC.MAX_DRIFT_SAMPLES["pcmfm"] < SPS / 2
    for cls in (coded.CodedCPMLink, coded.IterativeCPMLink):
        assert {"clock", "clock_recovery"} <= set(inspect.signature(cls.__init__).parameters)
    # (rows per tile, grid cap, LDS bytes): at most a workgroup's threads, and within what a CU has
    for shape in ((1, 4, 9, 8), (2, 16, 9, 8), (1, 2, 1, 1), (2, 8, 4, 3), (1, 64, 11, 10), (2, 4, 65, 64), (1, 2, 257, 7)):
        syms, cap, lds = device.cpm_mf_rows_resample_geometry(*shape)
        assert 1 <= syms <= 256 and cap >= 1 and lds <= 160 * 1024, shape


def test_cpm_timing_argument_validation_without_a_gpu():
    """Bad arguments return WF_ERR_VALUE before anything is launched (a fake context: no device exists here)."""
    from waveforms_amd import _hip
    from waveforms_amd.viterbi import cpm

    lib = _hip.lib()
    fake = ctypes.create_string_buffer(1 << 16)
    buf = ctypes.create_string_buffer(1 << 15)
    a = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    b, c, d = a + 4096, a + 8192, a + 12288
    V = _hip.WF_ERR_VALUE
    nan, inf = float("nan"), float("inf")
    # wf_cpm_mf_rows_resample_c128(ctx, r, nsamp, templates, nh, nfilt, ntm, start0, sps, ncalls, W, tau, nwin, tau0, rows, stream)
    good = (fake, a, 100, b, 1, 4, 9, 0, 8, 10, 64, c, 1, 0.0, d)
    for i, v in ((0, None), (1, None), (3, None), (14, None), (2, 0), (2, (1 << 40) + 1), (4, 0), (4, 3), (5, 3), (5, 32), (5, 0), (6, 0), (6, 258), (7, (1 << 40) + 1),
                 (7, -(1 << 40) - 1), (8, 0), (8, 257), (9, 0), (9, (1 << 40) + 1), (10, 96), (10, 32), (10, 8256), (12, 0), (13, nan), (13, inf), (1, a + 8), (3, b + 8),
                 (14, d + 8), (11, c + 4)):
        args = good[:i] + (v,) + good[i + 1:]
        assert lib.wf_cpm_mf_rows_resample_c128(*args, None) == V, args
    # a tile that cannot fit LDS: 64 filters of 257 taps on two columns
    assert lib.wf_cpm_mf_rows_resample_c128(*(good[:4] + (2, 64, 257, 0, 256) + good[9:]), None) == V
    geom = (ctypes.c_int64 * 3)()
    for args in ((1, 4, 9, 8, None), (3, 4, 9, 8, geom), (1, 5, 9, 8, geom), (1, 4, 0, 8, geom), (1, 4, 9, 0, geom), (2, 64, 257, 256, geom)):
        assert lib.wf_cpm_mf_rows_resample_geometry(*args) == V, args
    # wf_llr_stat(ctx, llr, ncalls, bits_per_call, W, stat, stream)
    good = (fake, a, 100, 2, 64, b)
    for i, v in ((0, None), (1, None), (5, None), (2, 0), (2, (1 << 40) + 1), (3, 0), (3, 9), (4, 0), (4, 96), (4, 8256), (1, a + 4), (5, b + 4)):
        args = good[:i] + (v,) + good[i + 1:]
        assert lib.wf_llr_stat(*args, None) == V, args
    # ... and the Python layer's own
    for kw in ({"window": 96}, {"span": 4}, {"hypotheses": 2}, {"hypotheses": 65}, {"refine": -1}, {"delta": 0.0}, {"delta": nan}, {"sps": 0}):
        with pytest.raises(ValueError):
            TC.CPMTimingRecovery(**{"spec": cpm.PCMFM_20, "sps": SPS, **kw})
    with pytest.raises(ValueError, match="full-phase"):
        TC.CPMTimingRecovery(cpm.ARTM_16, SPS)                  # NC = 4 of p = 16 phases: not the full-phase trellis
    with pytest.raises(ValueError, match="64"):
        TC.CPMTimingRecovery(cpm.ARTM_256, SPS)
    with pytest.raises(ValueError):
        TC.llr_stat_host(np.zeros(5), 2, 64)
    with pytest.raises(ValueError):
        TC.llr_stat_host(np.zeros(0), 1, 64)
    with pytest.raises(ValueError):
        TC.cpm_mf_rows_resample_host(np.zeros(10, dtype=complex), np.zeros((3, 4, 9), dtype=complex), 0, 8, 1)


def test_exact_fma_in_numpy():
    """``_fma`` against exact rational arithmetic rounded once, on operands that cancel (where two roundings differ from one)."""
    from fractions import Fraction

    rng = np.random.default_rng(4)
    a, b = rng.standard_normal(2000), rng.standard_normal(2000)
    c = -(a * b) * (1.0 + rng.integers(-3, 4, 2000) * 2.0 ** -52)
    c[::3] = rng.standard_normal(c[::3].size)
    c[1::7] = 0.0
    got = TC._fma(a, b, c)
    want = np.array([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a, b, c)])
    assert np.array_equal(got, want) and np.count_nonzero(got != a * b + c) > 100


@pytest.mark.parametrize("waveform", WAVEFORMS)
def test_resample_host_against_the_oracle_and_the_c_restatement(oracle, ref, waveform):
    spec, sig, noise, Tm, start0, ncalls = _chain(oracle, waveform, 400, NOISY_DB[waveform])
    r = sig + noise
    rows, mag = TC.cpm_mf_rows_resample_host(r, Tm, start0, SPS, ncalls)
    assert np.array_equal(rows, oracle.cpm_mf_rows(r, Tm, start0, SPS, ncalls)) and (mag >= np.abs(rows) * (1 - 1e-12)).all()
    for j in (3, -5, 16):
        assert np.array_equal(TC.cpm_mf_rows_resample_host(r, Tm, start0, SPS, ncalls, tau0=float(j))[0], oracle.cpm_mf_rows(r, Tm, start0 + j, SPS, ncalls)), j
    assert not TC.cpm_mf_rows_resample_host(r, Tm, start0, SPS, 5, 64, np.array([np.nan]))[0].any()
    assert not TC.cpm_mf_rows_resample_host(r, Tm, start0, SPS, 5, 64, np.array([1e7]))[0].any()
    assert not TC.cpm_mf_rows_resample_host(r, Tm, start0, SPS, 5, 64, None, 2.0 ** 62)[0].any()
    for name, (f0, W, tau, tau0) in _trajectories(ncalls, 64, r.size, start0).items():
        got, mag = TC.cpm_mf_rows_resample_host(r, Tm, f0, SPS, ncalls, W, tau, tau0)
        want = restate(ref, r, Tm, f0, SPS, ncalls, W, tau, tau0)
        bound = (2 * Tm.shape[2] + 12) * U * mag
        err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag))
        print(f"{waveform} {name}: max error {err.max():.3g}, bitwise {_bits_equal(got, want)}")
        assert (err <= bound).all(), name


@pytest.mark.parametrize("waveform", WAVEFORMS)
def test_the_statistic_its_period_and_the_turned_grid(oracle, ref, waveform):
    """Noiseless, 400 symbols, whole-sample offsets over two periods either way.  S(j) = -Σ |λ| of the whole burst with the plain
    table and with the table turned by P/2."""
    spec, sig, _noise, Tm, start0, ncalls = _chain(oracle, waveform, 400)
    soft, lg, per = soft_c(ref, spec), spec.bits_per_symbol, len(spec.K) * SPS
    turned_table = CC.hypothesis_table(spec, 0.5 * CC.period(spec))
    plain, turned = {}, {}
    for j in range(-per - 2, per + 3):
        rows = TC.cpm_mf_rows_resample_host(sig, Tm, start0, SPS, ncalls, tau0=float(j))[0]
        plain[j] = TC.llr_stat_host(soft(rows), lg, 8192)[0, 0]
        turned[j] = TC.llr_stat_host(soft(rows, turned_table), lg, 8192)[0, 0]
    print(waveform, {j: (round(plain[j]), round(turned[j])) for j in plain})
    best = {j: min(plain[j], turned[j]) for j in plain}
    wells = (0, per, -per)
    others = [j for j in range(-per - 1, per + 2) if min(abs(j - w) for w in wells) > 1]
    # the minimum at 0, and again at ±nh symbols: each lower than its neighbours and than every offset outside the three wells
    for w in wells:
        assert best[w] <= best[w - 1] and best[w] <= best[w + 1] and all(best[w] < best[j] for j in others), w
    # one period off the rows fit the turned grid, at 0 the plain one
    assert plain[0] < turned[0] and turned[per] < plain[per] and turned[-per] < plain[-per]
    assert min(plain, key=plain.get) == 0
    if waveform == "multih":
        # ONE symbol off there is no minimum: not half as deep as the well, on either grid
        assert best[SPS] > 0.5 * best[0] and best[-SPS] > 0.5 * best[0]


def test_llr_stat_host_at_its_edges():
    rng = np.random.default_rng(7)
    one = TC.llr_stat_host(np.array([-3.5]), 1, 64)
    assert one.shape == (1, 2) and one[0, 0] == -3.5 and one[0, 1] == 0.0 and not np.signbit(one[0, 1])
    for bpc in (1, 2):
        lam = rng.standard_normal((64 + 1) * bpc)                # a last window of one call
        st = TC.llr_stat_host(lam, bpc, 64)
        assert st.shape == (2, 2) and st[1, 0] == -np.abs(lam[64 * bpc:]).sum() and not st[:, 1].any()
        # the order of additions: 64 lane partials, then the butterfly
        a = np.abs(lam[:64 * bpc]).reshape(bpc, 64)
        p = a[0] + (a[1] if bpc == 2 else 0.0)
        d = 32
        while d:
            p[:d] = p[:d] + p[d:2 * d]
            d //= 2
        assert st[0, 0] == -p[0]
    assert TC.llr_stat_host(np.array([-0.0, 0.0]), 2, 64)[0, 0] == 0.0
    assert np.isnan(TC.llr_stat_host(np.array([1.0, np.nan, 2.0]), 1, 64)[0, 0])


@pytest.fixture(scope="module")
def bursts(oracle, ref):
    """Per waveform a noiseless burst of the reference chain and the genie's decisions."""
    from waveforms_amd.viterbi import cpm

    out = {}
    for waveform, spec in (("pcmfm", cpm.PCMFM_20), ("multih", cpm.ARTM_64)):
        W = TC.defaults(spec)["window"]
        spec, sig, _noise, Tm, start0, ncalls = _chain(oracle, waveform, max(4000, 7 * W + 52))
        soft = soft_c(ref, spec)
        genie = soft(TC.cpm_mf_rows_resample_host(sig, Tm, start0, SPS, ncalls)[0]) < 0
        out[waveform] = (spec, sig, Tm, start0, ncalls, soft, genie, W)
    return out


# Printed by the test below at the documented drift (4 000 calls of PCM/FM, 7 W + 52 of ARTM): the decisions lost without the
# recovery are 188 .. 629 (PCM/FM) and 1565 .. 3522 (ARTM); the residual's scatter (standard deviation over the windows 2 .. -3)
# is at most 0.158 samples (PCM/FM) and 0.071 (ARTM).  RESIDUAL is three times that.
LOST_FLOOR = {"pcmfm": 150, "multih": 1000}
RESIDUAL = {"pcmfm": 0.474, "multih": 0.213}
_RECOVERED: dict = {}


def _recovered(bursts, waveform, tau0, sign):
    """(impaired signal, eps, what ``recover_cpm_timing_host`` returns) of one case, computed once."""
    key = (waveform, tau0, sign)
    if key not in _RECOVERED:
        spec, sig, Tm, start0, ncalls, soft, _genie, W = bursts[waveform]
        eps = sign * TC.MAX_DRIFT_SAMPLES[waveform] / (SPS * W)
        bad = T.timing_offset_host(sig, tau0, eps)
        _RECOVERED[key] = (bad, eps) + TC.recover_cpm_timing_host(spec, bad, Tm, start0, SPS, ncalls, soft=soft)
    return _RECOVERED[key]


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("tau0", [-2.7, 2.7, 6.0])
@pytest.mark.parametrize("waveform", WAVEFORMS)
def test_recover_cpm_timing_host_at_the_documented_drift(bursts, waveform, tau0, sign):
    """Defaults per waveform: the decisions after recovery are the unimpaired burst's, up to a shift of nh calls (the instant is
    recovered modulo nh symbols), outside a guard of one window at each end."""
    spec, sig, Tm, start0, ncalls, soft, genie, W = bursts[waveform]
    drift = TC.MAX_DRIFT_SAMPLES[waveform]
    bad, eps, rows, tau, choice, grid = _recovered(bursts, waveform, tau0, sign)
    assert tau.shape == choice.shape == (-(-ncalls // W),) and grid in (0, 1)
    assert _differ_up_to_a_period(spec, soft(rows) < 0, genie, W) == 0
    lost = _differ_up_to_a_period(spec, soft(TC.cpm_mf_rows_resample_host(bad, Tm, start0, SPS, ncalls)[0]) < 0, genie, W)
    print(f"{waveform} tau0 {tau0}, drift {sign * drift:+.2f} per window: {lost} decisions lost without the recovery, grid {grid}")
    assert lost > LOST_FLOOR[waveform]
    # the trajectory is the impairment's modulo nh symbols: -(tau0 + eps n) at the window centres.  RESIDUAL is three times the
    # printed scatter; the clipped mean lags by up to one window's drift at the burst's two ends: those are held to the drift only.
    per = float(len(spec.K) * SPS)
    centre = start0 + SPS * (W * np.arange(tau.size) + 0.5 * (W - 1))
    resid = C._wrap(tau + tau0 + eps * centre, per)
    print(f"   residual against the impairment: windows 2 .. -3 mean {resid[2:-2].mean():+.3f}, scatter {resid[2:-2].std():.3f}, "
          f"largest {np.abs(resid[2:-2]).max():.3f} samples; all windows {np.abs(resid).max():.3f}")
    assert np.abs(resid[2:-2]).max() < RESIDUAL[waveform] and np.abs(resid).max() < RESIDUAL[waveform] + drift


def test_both_grids_occur(bursts):
    """PCM/FM: tau0 = 6.0 lies beyond half a period: the rows come back one period off, on the turned grid."""
    grids = {(tau0, sign): _recovered(bursts, "pcmfm", tau0, sign)[5] for tau0 in (-2.7, 2.7, 6.0) for sign in (1.0, -1.0)}
    print(grids)
    assert set(grids.values()) == {0, 1}


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture
def ctx():
    from waveforms_amd import _hip

    handle = _hip.new_ctx()
    yield handle
    _hip.free_ctx(handle)


def _check_resample(ref, d_r, r, d_T, Tm, f0, sps, ncalls, W, tau, tau0, ctx, name):
    """One device call into a sentinel-guarded buffer against the C restatement (bitwise) and the numpy statement (the bound)."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    nfilt, guard, sentinel = Tm.shape[1], 3, -7.5
    buf = _hip.to_device(np.full((ncalls + 2 * guard, nfilt, 2), sentinel))
    out = dev.cpm_mf_rows_resample(d_r, d_T, f0, sps, ncalls, W, None if tau is None else _hip.to_device(tau), tau0, out=buf[guard:guard + ncalls], ctx=ctx)
    assert out.data_ptr() == buf[guard:].data_ptr()
    full = _hip.to_host(buf)
    assert (full[:guard] == sentinel).all() and (full[guard + ncalls:] == sentinel).all(), name
    got = _hip.to_host(out, True)
    want = restate(ref, r, Tm, f0, sps, ncalls, W, tau, tau0)
    assert np.array_equal(got, want), (name, np.abs(got - want).max())
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("ncalls", [1, 63, 257, 1000])
@pytest.mark.parametrize("waveform", WAVEFORMS)
def test_cpm_mf_rows_resample_against_the_restatements(oracle, ref, ctx, waveform, ncalls):
    """Both link template sets at sps 8 on noisy samples over the trajectories the SOQPSK-TG bank serves.  BITWISE against
    tests/cpm_timing_ref.c; per component within (2 ntm + 12) * 2^-53 * the absolute-value sum of the numpy statement."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    spec, sig, noise, Tm, start0, have = _chain(oracle, waveform, 1003, NOISY_DB[waveform])
    assert have >= 1000 and Tm.shape == ((1, 4, 9) if waveform == "pcmfm" else (2, 16, 9))
    r = sig + noise
    d_r, d_T = _hip.to_device(r), _hip.to_device(Tm)
    plain = _hip.to_host(dev.cpm_mf_rows(d_r, d_T, start0, SPS, ncalls), True)
    for name, (f0, W, tau, tau0) in _trajectories(ncalls, 64, r.size, start0).items():
        got = _check_resample(ref, d_r, r, d_T, Tm, f0, SPS, ncalls, W, tau, tau0, ctx, name)
        want, mag = TC.cpm_mf_rows_resample_host(r, Tm, f0, SPS, ncalls, W, tau, tau0)
        err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag))
        assert (err <= (2 * Tm.shape[2] + 12) * U * mag).all(), (name, err.max())
        print(f"{waveform} {ncalls} {name}: max error against numpy {err.max():.3g}, {int((~want.any(axis=1)).sum())} zero rows")
        if name == "none":
            assert (got == plain).all()
        if name == "nan":
            dead = np.isnan(T.instants_host(ncalls, W, tau, tau0))
            assert dead.any() and not got[dead].any() and (ncalls < 3 * 64 or got[~dead].any())
        if name == "far away":
            assert not got.any()
        if name in ("before 0", "past the end") and ncalls >= 63:
            assert want.any() and not want[0 if name == "before 0" else -1].any()
    # a whole constant is wf_cpm_mf_rows_c128 at the moved start0
    for j in (3, -11):
        got = _hip.to_host(dev.cpm_mf_rows_resample(d_r, d_T, start0, SPS, ncalls, tau0=float(j), ctx=ctx), True)
        assert got.shape == (ncalls, Tm.shape[1]) and (got == _hip.to_host(dev.cpm_mf_rows(d_r, d_T, start0 + j, SPS, ncalls), True)).all(), j


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 1, 2, 1), (3, 4, 8, 2), (10, 11, 64, 1), (64, 65, 4, 2), (7, 257, 2, 1)])
def test_cpm_mf_rows_resample_other_shapes(ref, ctx, shape):
    """(sps, ntm, nfilt, nh) off the fast path: templates from LDS, tiles of other sizes (some beyond 48 KiB of LDS), random
    templates, 700 calls, a random-walk trajectory over windows of 64 rows."""
    from waveforms_amd import _hip

    sps, ntm, nfilt, nh = shape
    rng = np.random.default_rng(sum(shape))
    ncalls, W = 700, 64
    r = rng.standard_normal(ncalls * sps + ntm + 5) + 1j * rng.standard_normal(ncalls * sps + ntm + 5)
    Tm = rng.standard_normal((nh, nfilt, ntm)) + 1j * rng.standard_normal((nh, nfilt, ntm))
    tau = np.cumsum(rng.standard_normal(-(-ncalls // W)) * 0.7 * sps)
    got = _check_resample(ref, _hip.to_device(r), r, _hip.to_device(Tm), Tm, 2, sps, ncalls, W, tau, -0.375, ctx, str(shape))
    assert got.any()


@pytest.mark.gpu
def test_cpm_mf_rows_resample_more_tiles_than_workgroups(ref, ctx):
    """The smallest burst whose tiles outnumber the launch's workgroups (the grid-stride loop runs twice in one of them):
    two filters of three taps at sps 2, a drifting trajectory with a jump wider than a tile's window near the end."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    sps, ntm, nfilt, nh, W = 2, 3, 2, 1, 8192
    syms, cap, _lds = dev.cpm_mf_rows_resample_geometry(nh, nfilt, ntm, sps)
    ncalls = syms * cap + 1
    rng = np.random.default_rng(9)
    r = rng.standard_normal(ncalls * sps + 8) + 1j * rng.standard_normal(ncalls * sps + 8)
    Tm = rng.standard_normal((nh, nfilt, ntm)) + 1j * rng.standard_normal((nh, nfilt, ntm))
    nwin = -(-ncalls // W)
    tau = 0.37 * np.arange(nwin)
    tau[-2:] -= 5000.25
    got = _check_resample(ref, _hip.to_device(r), r, _hip.to_device(Tm), Tm, 1, sps, ncalls, W, tau, 0.5, ctx, "grid cap")
    assert got[-1].any() and got[0].any()


@pytest.mark.gpu
@pytest.mark.parametrize("bpc", [1, 2])
@pytest.mark.parametrize("W", [64, 256, 8192])
def test_llr_stat_is_bitwise_the_host_statement(ctx, W, bpc):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    rng = np.random.default_rng(W + bpc)
    for ncalls in (1, W - 1, W, 3 * W + 5):
        lam = rng.standard_normal(ncalls * bpc) * 10.0
        lam[::5] = -0.0
        want = TC.llr_stat_host(lam, bpc, W)
        buf = _hip.to_device(np.full((want.shape[0] + 2, 2), -7.5))
        got = _hip.to_host(dev.llr_stat(_hip.to_device(lam), bpc, W, out=buf[1:-1], ctx=ctx))
        assert _bits_equal(got, want), (ncalls, np.abs(got - want).max())
        full = _hip.to_host(buf)
        assert (full[0] == -7.5).all() and (full[-1] == -7.5).all()
        if ncalls > 2:
            lam[ncalls * bpc // 2] = np.nan
            want = TC.llr_stat_host(lam, bpc, W)
            got = _hip.to_host(dev.llr_stat(_hip.to_device(lam), bpc, W, ctx=ctx))
            bad = np.isnan(want[:, 0])
            assert bad.sum() == 1 and np.array_equal(np.isnan(got[:, 0]), bad) and _bits_equal(got[~bad], want[~bad]) and not got[:, 1].any()


@pytest.mark.gpu
@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("waveform", WAVEFORMS)
def test_recovery_on_the_device_against_the_host_statement(oracle, ref, ctx, waveform, noisy):
    """A burst of 4 W + 100 calls (at least 2100), 2.7 samples late and drifting at the documented limit (noiseless PCM/FM loses
    little to a constant offset: it takes the drift across a symbol boundary to lose the burst without the recovery): the device
    composition makes the host statement's choices, grid and trajectory, and its rows decide as the host statement's do."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.viterbi import cpm

    spec0 = cpm.ARTM_64 if waveform == "multih" else cpm.PCMFM_20
    W = TC.defaults(spec0)["window"]
    spec, sig, noise, Tm, start0, ncalls = _chain(oracle, waveform, max(2100, 4 * W + 100), NOISY_DB[waveform] if noisy else None, seed=8)
    soft = soft_c(ref, spec)
    eps = TC.MAX_DRIFT_SAMPLES[waveform] / (SPS * W)
    bad = T.timing_offset_host(sig, 2.7, eps) + noise
    want_rows, want_tau, want_choice, want_grid = TC.recover_cpm_timing_host(spec, bad, Tm, start0, SPS, ncalls, soft=soft)
    rec = TC.CPMTimingRecovery(spec, SPS)
    rec.times = True
    d_T = _hip.to_device(Tm)
    rows, tau, choice, grid = rec.recover(_hip.to_device(bad), d_T, start0, ncalls, ctx=ctx)
    assert np.array_equal(_hip.to_host(choice), want_choice) and int(grid.cpu()) == want_grid
    err = np.abs(_hip.to_host(tau) - want_tau).max()
    print(f"{waveform} noisy {noisy}: trajectory differs by {err:.3g} samples, grid {want_grid}")
    assert err < 1e-9
    got_bits = _hip.to_host(dev.cpm_soft(rows, spec, ctx=ctx)[1]).astype(bool)
    assert np.array_equal(got_bits, soft(want_rows) < 0)
    assert set(rec.stage_times()) == {"resample", "soft", "stat", "track", "rescale", "add", "grid"}
    if not noisy:
        genie = soft(TC.cpm_mf_rows_resample_host(sig, Tm, start0, SPS, ncalls)[0]) < 0
        assert _differ_up_to_a_period(spec, got_bits, genie, W) == 0
        lost = _differ_up_to_a_period(spec, soft(TC.cpm_mf_rows_resample_host(bad, Tm, start0, SPS, ncalls)[0]) < 0, genie, W)
        print(f"   {lost} decisions lost without the recovery")
        assert lost > 100
