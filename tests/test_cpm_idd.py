"""Iterative detection and decoding of the coded ARTM multi-h and PCM/FM chains: wf_cpm_soft_apriori (include/wfhip.h),
CodedCPMLink and IterativeCPMLink (waveforms_amd/encoding/coded.py).

The definition of wf_cpm_soft_apriori is restated sequentially in C (tests/cpm_soft_apriori_ref.c, explicit fma, compiled
here with -ffp-contract=off), pinned to brute force over all paths (the prior in the path cost, the own bit's prior taken
out) and, with no prior, to tests/cpm_soft_ref.c.  On the GPU the chunk-parallel kernels must equal the restatement BITWISE
whatever the prior, the warm-up, the chunking and the first call, and so must the whole loop pass by pass (the decoder's half
of the loop is ``decode_ext_restatement`` of tests/test_idd.py).

The algorithm's gain is checked on the CPU from the restatements alone (information Eb/N0: ARTM 7.0 dB, PCM/FM 3.0 dB; 40
demo codewords, one per burst): 8 outer x 5 inner passes at damping 0.7 must end with at most a quarter of the frame errors
of one pass of 50 iterations, in fewer iterations in total.  The factor 4 is a cap, not a measurement.
"""
import ctypes
import itertools
import subprocess
import types
from pathlib import Path

import numpy as np
import pytest

import test_cpm_soft as TC
import test_idd as TI
import test_ldpc as TL
from waveforms_amd.encoding import ldpc

SPS = 8
HERE = Path(__file__).resolve().parent
_p, _K, _specs = TC._p, TC._K, TC._specs
EXT_SAT = 6.25 * SPS                      # the links' default


def _compile(tmp, name):
    so = tmp / f"lib{name}.so"
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", str(so), str(HERE / f"{name}.c"), "-lm"])
    return ctypes.CDLL(str(so))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    """tests/cpm_soft_ref.c: the plain detector's definition."""
    lib = _compile(tmp_path_factory.mktemp("cpm_soft_ref"), "cpm_soft_ref")
    lib.cpm_soft_rec.restype = ctypes.c_int
    lib.cpm_soft_rows.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module")
def apref(tmp_path_factory):
    lib = _compile(tmp_path_factory.mktemp("cpm_soft_apriori_ref"), "cpm_soft_apriori_ref")
    lib.cpm_soft_apriori_rec.restype = ctypes.c_int
    lib.cpm_soft_apriori_rows.restype = ctypes.c_int
    return lib


def _prior_arg(prior):
    if prior is None:
        return None, None
    prior = np.ascontiguousarray(prior, dtype=np.float32).reshape(-1)
    return prior, _p(prior)


def restate_rec(apref, spec, inc, prior, scale, first_call=0):
    """The header's definition over given increments inc[n][S][M] -> (ext, bits)."""
    n, lg = inc.shape[0], spec.bits_per_symbol
    ext, bits = np.empty(n * lg), np.empty(n * lg, dtype=np.uint8)
    keep, pp = _prior_arg(prior)
    assert keep is None or keep.size == n * lg
    assert apref.cpm_soft_apriori_rec(spec.M, spec.p, len(spec.K), _K(spec), spec.Lp, _p(inc), ctypes.c_int64(n), ctypes.c_int64(first_call),
                                      pp, ctypes.c_double(scale), _p(ext), _p(bits)) == 0
    return ext, bits


def restate(apref, spec, rows, prior, scale, first_call=0):
    """The header's definition over complex128 rows [n][M^Lp] and a float32 prior [n lgM] (or None) -> (ext, bits)."""
    from waveforms_amd.viterbi.cpm import rotation_table

    rows = np.ascontiguousarray(rows, dtype=np.complex128).reshape(-1, spec.nfilt)
    n, lg = rows.shape[0], spec.bits_per_symbol
    ext, bits = np.empty(n * lg), np.empty(n * lg, dtype=np.uint8)
    rot = rotation_table(spec)
    keep, pp = _prior_arg(prior)
    assert keep is None or keep.size == n * lg
    assert apref.cpm_soft_apriori_rows(spec.M, spec.p, len(spec.K), _K(spec), spec.Lp, _p(rot), _p(rows), ctypes.c_int64(n),
                                       ctypes.c_int64(first_call), pp, ctypes.c_double(scale), _p(ext), _p(bits)) == 0
    return ext, bits


def _increments(ref, spec, rows, first_call=0):
    from waveforms_amd.viterbi.cpm import rotation_table

    rows = np.ascontiguousarray(rows, dtype=np.complex128).reshape(-1, spec.nfilt)
    n = rows.shape[0]
    inc = np.empty((n, spec.nstates, spec.M))
    rot = rotation_table(spec)
    ref.cpm_soft_incs(spec.M, spec.p, len(spec.K), _K(spec), spec.Lp, _p(rot), _p(rows), ctypes.c_int64(n), ctypes.c_int64(first_call), _p(inc))
    return inc


def apriori_brute_force(spec, inc, pi, first_call):
    """λᵉ[lgM k + i] = min over paths with bit i of u_k = 1 of (Σ inc + Σ of π over every 1-bit of the path EXCEPT bit (k, i))
    - the same with that bit 0; every start state, every input.  pi: float64 [n][lgM]."""
    n, S, M = inc.shape
    lg = spec.bits_per_symbol
    ends = [TC._ends(spec, first_call + k) for k in range(n)]
    ub = [[(u >> (lg - 1 - i)) & 1 for i in range(lg)] for u in range(M)]
    best = np.full((n, lg, 2), np.inf)
    for s0 in range(S):
        for us in itertools.product(range(M), repeat=n):
            s, cost = s0, 0.0
            for k in range(n):
                cost += inc[k, s, us[k]]
                s = ends[k][s][us[k]]
            tot = cost + sum(ub[us[k]][i] * pi[k][i] for k in range(n) for i in range(lg))
            for k in range(n):
                for i in range(lg):
                    b = ub[us[k]][i]
                    best[k, i, b] = min(best[k, i, b], tot - b * pi[k][i])
    return (best[:, :, 1] - best[:, :, 0]).reshape(-1)


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("waveform", ["multih", "pcmfm"])
def test_restatement_equals_brute_force(ref, apref, waveform):
    spec = _specs()[waveform]
    S, M, lg = spec.nstates, spec.M, spec.bits_per_symbol
    rng = np.random.default_rng(11 + M)
    for first_call in (0, 1, 2):
        for n in range(1, 5):
            # integer-valued increments and priors: every sum is exact, so the normalised recursions give the brute force exactly
            inc = rng.integers(-8, 9, (n, S, M)).astype(np.float64)
            prior = rng.integers(-12, 13, n * lg).astype(np.float32)
            ext, bits = restate_rec(apref, spec, inc, prior, 1.0, first_call)
            want = apriori_brute_force(spec, inc, prior.astype(np.float64).reshape(n, lg), first_call)
            assert np.array_equal(ext, want), (first_call, n, ext, want)
            assert np.array_equal(bits, ((want + prior) < 0).astype(np.uint8))
            # real-valued: increments from random rows (the definition's fma), equal up to the normalisations' rounding
            rows = rng.standard_normal((n, spec.nfilt)) + 1j * rng.standard_normal((n, spec.nfilt))
            prior = (3.0 * rng.standard_normal(n * lg)).astype(np.float32)
            ext, _ = restate(apref, spec, rows, prior, 0.7, first_call)
            want = apriori_brute_force(spec, _increments(ref, spec, rows, first_call), (0.7 * prior.astype(np.float64)).reshape(n, lg), first_call)
            np.testing.assert_allclose(ext, want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("waveform", ["multih", "pcmfm"])
def test_no_prior_is_the_plain_detector_and_the_output_is_extrinsic(ref, apref, waveform):
    spec = _specs()[waveform]
    lg = spec.bits_per_symbol
    rng = np.random.default_rng(17)
    n = 60
    for first_call in (0, 3):
        rows = rng.standard_normal((n, spec.nfilt)) + 1j * rng.standard_normal((n, spec.nfilt))
        llr, hard = TC.restate(ref, spec, rows, first_call)
        for prior in (None, np.zeros(n * lg, dtype=np.float32), -np.zeros(n * lg, dtype=np.float32)):
            for scale in (0.7, -1.0):
                ext, bits = restate(apref, spec, rows, prior, scale, first_call)
                assert np.array_equal(ext.view(np.uint64), llr.view(np.uint64)) and np.array_equal(bits, hard)
    # a strong prior on ONE bit, against the channel's decision: its own λᵉ does not move, its decision follows the prior,
    # the neighbouring symbols' λᵉ move and, for ARTM, so does the other bit of its own symbol
    base, _ = restate(apref, spec, rows, None, 1.0, 3)
    for i in range(lg):
        j = lg * 30 + i
        prior = np.zeros(n * lg, dtype=np.float32)
        prior[j] = -100.0 if base[j] > 0 else 100.0
        ext, bits = restate(apref, spec, rows, prior, 1.0, 3)
        assert ext[j] == base[j]
        assert bits[j] == (prior[j] < 0)
        assert np.any(ext[lg * 28:lg * 30] != base[lg * 28:lg * 30]) and np.any(ext[lg * 31:lg * 33] != base[lg * 31:lg * 33])
        if lg == 2:
            assert ext[j ^ 1] != base[j ^ 1]


def test_entry_point_exported_bound_and_refuses_bad_arguments_without_a_gpu():
    """Bad arguments return WF_ERR_VALUE before the context is touched (a fake context: no device exists here)."""
    from waveforms_amd import _hip, device
    from waveforms_amd.encoding import coded
    from waveforms_amd.viterbi import cpm

    lib = _hip.lib()
    assert "wf_cpm_soft_apriori" in _hip.SIGNATURES and hasattr(lib, "wf_cpm_soft_apriori")
    assert "int wf_cpm_soft_apriori(" in (HERE.parent / "include" / "wfhip.h").read_text()
    assert callable(device.cpm_soft_apriori)
    assert issubclass(coded.IterativeCPMLink, coded.CodedCPMLink)

    fake = ctypes.create_string_buffer(1 << 16)
    buf = ctypes.create_string_buffer(8192)
    base = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    rot, rows, ext, bits, pri = base, base + 1024, base + 4096, base + 6144, base + 7168
    V = _hip.WF_ERR_VALUE
    good = cpm.ARTM_64.c_config()
    inf, nan = float("inf"), float("nan")

    def call(cfg=good, ctx=fake, r=rot, z=rows, n=10, first=0, warmup=0, prior=pri, scale=1.0, out=ext, b=bits):
        return lib.wf_cpm_soft_apriori(ctx, None if cfg is None else ctypes.byref(cfg), r, z, n, first, warmup, prior, scale, out, b, None)

    assert call(ctx=None) == V and call(cfg=None) == V and call(r=None) == V and call(z=None) == V
    assert call(out=None) == V and call(b=None) == V
    for n in (0, -1):
        assert call(n=n) == V
    assert call(first=-1) == V and call(warmup=-1) == V
    for scale in (inf, -inf, nan):
        assert call(scale=scale) == V and call(prior=None, scale=scale) == V
    assert call(prior=pri + 2) == V and call(z=rows + 8) == V and call(r=rot + 8) == V and call(out=ext + 4) == V
    for spec in (cpm.ARTM_16, cpm.PCMFM_10, cpm.ARTM_256):       # NC != p; 256 states
        assert call(cfg=spec.c_config()) == V and call(cfg=spec.c_config(), prior=None) == V
    for field, value in (("M", 3), ("M", 8), ("nh", 3), ("nh", 0), ("Lp", 0), ("Lp", 4), ("NC", 8)):
        cfg = cpm.ARTM_64.c_config()
        setattr(cfg, field, value)
        assert call(cfg=cfg) == V, (field, value)


def test_python_wrappers_refuse_bad_arguments_without_a_gpu():
    """The Python wrappers' own checks come before any device call."""
    import torch

    from waveforms_amd import device as dev
    from waveforms_amd.encoding.coded import CodedCPMLink, IterativeCPMLink
    from waveforms_amd.viterbi import cpm

    class _T:                                                        # the few tensor attributes the wrapper looks at
        def __init__(self, n, contiguous=True, dtype=torch.float32):
            self._n, self._c, self.dtype = n, contiguous, dtype

        def numel(self):
            return self._n

        def is_contiguous(self):
            return self._c

    spec = cpm.ARTM_64
    per = 2 * spec.nfilt
    rows = _T(10 * per, dtype=torch.float64)
    with pytest.raises(ValueError):
        dev.cpm_soft_apriori(_T(10 * per, False), spec, _T(20))
    with pytest.raises(ValueError):
        dev.cpm_soft_apriori(_T(10 * per + 1), spec, _T(20))
    for bad in (_T(19), _T(10), _T(20, False), _T(20, dtype=torch.float64)):
        with pytest.raises(ValueError):
            dev.cpm_soft_apriori(rows, spec, bad)
    with pytest.raises(ValueError):
        dev.cpm_soft_apriori(_T(10 * 2 * cpm.PCMFM_20.nfilt), cpm.PCMFM_20, _T(20))      # one value per call there
    for scale in (float("inf"), float("nan")):
        with pytest.raises(ValueError):
            dev.cpm_soft_apriori(rows, spec, _T(20), scale)
        with pytest.raises(ValueError):
            dev.cpm_soft_apriori(rows, spec, None, scale)

    code = ldpc.demo_code()
    for kw in ({"outer": 0}, {"inner": 0}, {"damping": 0.0}, {"damping": float("nan")}, {"ext_sat": float("inf")}, {"ext_clip": 0.0},
               {"prior_warmup": -1}, {"waveform": "soqpsk"}):
        with pytest.raises(ValueError):
            IterativeCPMLink(code, 4, **kw)
    with pytest.raises(ValueError):
        CodedCPMLink(code, 4, waveform="XX")
    with pytest.raises(ValueError):
        CodedCPMLink(code, 0)
    odd = types.SimpleNamespace(n_tx=2047, k=1024)
    for cls in (CodedCPMLink, IterativeCPMLink):
        with pytest.raises(ValueError, match="odd"):
            cls(odd, 4, waveform="multih")


def test_apriori_kernels_resources():
    """The bar of the plain cpm_soft_* kernels: no VGPR or SGPR spills, no private segment, no scratch access and no
    v_writelane inside loops — for every a-priori kernel the entry point can launch."""
    import sys

    sys.path.insert(0, str(HERE.parent / "tools"))
    import kernel_resources as kr
    from waveforms_amd.csrc.build import build

    so = build(verbose=False)
    tab = {k: v for k, v in kr.kernel_table(so).items() if k.startswith("cpm_soft_ap_")}
    forms = [(m, lp) for m in (2, 4) for lp in (1, 2, 3)]
    want = {f"cpm_soft_ap_bounds_kernel<{m}, {lp}>" for m, lp in forms} | {f"cpm_soft_ap_llr_kernel<{m}, {lp}>" for m, lp in forms}
    want |= {f"cpm_soft_ap_repair_kernel<{m}, {lp}, {b}>" for m, lp in forms for b in ("true", "false")} | {"cpm_soft_ap_verify_kernel"}
    assert set(tab) == want, sorted(set(tab) ^ want)
    asm = kr.loop_spill_counts(so, "cpm_soft_ap_")
    for name, row in tab.items():
        assert row["vgpr_spill_count"] == 0 and row["sgpr_spill_count"] == 0 and row["private_segment_fixed_size"] == 0, (name, row)
        a = asm[name]
        assert a["scratch_load_in_loop"] == 0 and a["scratch_store_in_loop"] == 0, (name, a)
        assert a["v_writelane_in_loop"] == 0, (name, a)


# ---- the loop on the CPU -----------------------------------------------------------------------------------------------
def _wave(oracle, waveform):
    """(full-phase spec, the oracle's spec, pulse, mapper) of a waveform."""
    from waveforms_amd.viterbi import cpm

    if waveform == "multih":
        return cpm.ARTM_64, oracle.ARTM_64, oracle.freq_pulse_multih_irig(SPS), lambda b: oracle.multih_mapper(b)[0]
    return cpm.PCMFM_20, oracle.CPMDetectorSpec(M=2, p=10, K=(7,), Lp=2, NC=10, D=32), oracle.freq_pulse_pcmfm(SPS), oracle.pcmfm_mapper


def _cpu_bursts(oracle, ref, code, waveform, ncw, ebn0, seed, pad=8):
    """ncw bursts of one demo codeword each through the oracle's chain -> (information bits, increments ncw x N x S x M)."""
    spec, ospec, pulse, mapper = _wave(oracle, waveform)
    lg = spec.bits_per_symbol
    rng = np.random.default_rng(seed)
    u = rng.integers(0, 2, (ncw, code.k), dtype=np.uint8)
    tx = code.encode_host(u)
    sigma = oracle.cpm_sigma_for_ebn0(ebn0 + 10 * np.log10(code.k / code.n_tx), SPS, lg)
    n = code.n_tx // lg + 4
    incs = []
    for b in range(ncw):
        sym = mapper(np.concatenate([tx[b], np.zeros(pad * lg, np.uint8)]))
        res = oracle.cpm_detection_run(sym, pulse, SPS, ospec, sigma=sigma, rng=rng)
        rows = np.ascontiguousarray(res["rows"], dtype=np.complex128).reshape(-1, spec.nfilt)
        assert rows.shape[0] >= n
        incs.append(_increments(ref, spec, rows[:n]))
    return u, np.array(incs)


def _tables(spec, N):
    """Per call k of a burst from call 0: (end[s][u], for every end state its M entering (s, u))."""
    cache, out = {}, []
    for k in range(N):
        m_old = k - spec.Lp + 1
        key = -1 if m_old < 0 else m_old % len(spec.K)
        if key not in cache:
            ends = np.array(TC._ends(spec, k))
            S, M = ends.shape
            ps, pu = [[] for _ in range(S)], [[] for _ in range(S)]
            for s in range(S):
                for u in range(M):
                    ps[ends[s, u]].append(s)
                    pu[ends[s, u]].append(u)
            assert all(len(x) == M for x in ps)
            cache[key] = (ends, np.array(ps), np.array(pu))
        out.append(cache[key])
    return out


def _siso_batch(spec, inc, prior, scale):
    """The restatement vectorised over bursts of equal length from call 0 (the same float64 operations per burst, section by
    section; the minima in numpy's order, which the header shows not to matter).  inc: B x N x S x M, prior: float32 B x N lgM
    -> ext B x N lgM."""
    B, N, S, M = inc.shape
    lg = spec.bits_per_symbol
    pi = (np.float64(scale) * prior.astype(np.float64)).reshape(B, N, lg)
    tabs = _tables(spec, N)
    incp = inc.copy()                                                 # inc': Π(u) added on u != 0, one addition
    if M == 2:
        incp[..., 1] += pi[:, :, None, 0]
    else:
        incp[..., 1] += pi[:, :, None, 1]
        incp[..., 2] += pi[:, :, None, 0]
        incp[..., 3] += (pi[..., 0] + pi[..., 1])[:, :, None]
    A = np.zeros((N + 1, B, S))
    a = np.zeros((B, S))
    for k in range(N):
        _ends, ps, pu = tabs[k]
        new = (a[:, :, None] + incp[:, k])[:, ps, pu].min(-1)
        a = new - new.min(1, keepdims=True)
        A[k + 1] = a
    ext = np.empty((B, N, lg))
    bt = np.zeros((B, S))
    for k in range(N - 1, -1, -1):
        ends = tabs[k][0]
        be = bt[:, ends]                                              # B x S x M
        ak = A[k]
        x = inc[:, k]
        if M == 2:
            tot = (ak[:, :, None] + x) + be
            ext[:, k, 0] = tot[:, :, 1].min(1) - tot[:, :, 0].min(1)
        else:
            p0, p1 = pi[:, k, 0][:, None], pi[:, k, 1][:, None]
            t0 = (ak + x[:, :, 0]) + be[:, :, 0]
            # bit 0 (MSB): the LSB's prior on u = 1, 3
            m1 = np.minimum((ak + x[:, :, 2]) + be[:, :, 2], (ak + (x[:, :, 3] + p1)) + be[:, :, 3]).min(1)
            m0 = np.minimum(t0, (ak + (x[:, :, 1] + p1)) + be[:, :, 1]).min(1)
            ext[:, k, 0] = m1 - m0
            # bit 1 (LSB): the MSB's prior on u = 2, 3
            m1 = np.minimum((ak + x[:, :, 1]) + be[:, :, 1], (ak + (x[:, :, 3] + p0)) + be[:, :, 3]).min(1)
            m0 = np.minimum(t0, (ak + (x[:, :, 2] + p0)) + be[:, :, 2]).min(1)
            ext[:, k, 1] = m1 - m0
        new = (incp[:, k] + be).min(2)
        bt = new - new.min(1, keepdims=True)
    return ext.reshape(B, N * lg)


@pytest.mark.parametrize("waveform", ["multih", "pcmfm"])
def test_siso_batch_is_the_restatement(oracle, ref, apref, waveform):
    code = ldpc.demo_code()
    spec = _specs()[waveform]
    _u, inc = _cpu_bursts(oracle, ref, code, waveform, 2, 5.0, 5)
    inc = np.ascontiguousarray(inc[:, :150])
    prior = (8.0 * np.random.default_rng(1).standard_normal((2, 150 * spec.bits_per_symbol))).astype(np.float32)
    got = _siso_batch(spec, inc, prior, 0.7)
    for b in range(2):
        want, _ = restate_rec(apref, spec, inc[b], prior[b], 0.7)
        assert np.array_equal(got[b].view(np.uint64), want.view(np.uint64))


def _gain_on_the_cpu(oracle, ref, waveform, ebn0, seed=2):
    code = ldpc.demo_code()
    spec = _specs()[waveform]
    ncw, outer, inner, damping, sat = 40, 8, 5, 0.7, EXT_SAT
    u, inc = _cpu_bursts(oracle, ref, code, waveform, ncw, ebn0, seed)
    nt, npr = code.n_tx, inc.shape[1] * spec.bits_per_symbol
    lam = _siso_batch(spec, inc, np.zeros((ncw, npr), dtype=np.float32), damping)[:, :nt]
    one_info, _post, one_it = TL.decode_restatement(code, lam, 1.0, 0.75, 50)
    one_fe = int(np.any(one_info != u, axis=1).sum())

    prior = np.zeros((ncw, npr), dtype=np.float32)
    state = np.zeros(ncw, dtype=np.uint8)
    iters = np.zeros(ncw, dtype=np.int32)
    info = np.zeros((ncw, code.k), dtype=np.uint8)
    per_pass = []
    for _o in range(outer):
        ext = _siso_batch(spec, inc, prior, damping)
        TI.decode_ext_restatement(code, ext[:, :nt], state, prior[:, :nt], info, iters, 1.0, 0.75, inner, np.inf, sat)
        per_pass.append(int(np.any(info != u, axis=1).sum()))
    print(f"{waveform} {ebn0} dB, one pass: {one_fe} of {ncw} frame errors, mean iterations {one_it.mean():.2f}; iterative: per pass "
          f"{per_pass}, mean inner iterations {iters.mean():.2f}, open {int((state == 0).sum())}")
    assert one_fe >= 4                                       # (otherwise the condition below says nothing)
    assert 4 * per_pass[-1] <= one_fe
    assert iters.sum() < one_it.sum()


def test_iterative_gain_on_the_cpu_artm(oracle, ref):
    """ARTM, information Eb/N0 7.0 dB.  On this test's seed: one pass fails 34 of 40 codewords at 44.6 mean iterations, the
    loop 0 of 40 at 7.9 (frame errors per pass 38, 7, 3, 1, 0, ...)."""
    _gain_on_the_cpu(oracle, ref, "multih", 7.0)


def test_iterative_gain_on_the_cpu_pcmfm(oracle, ref):
    """PCM/FM, information Eb/N0 3.0 dB.  On this test's seed: one pass fails 27 of 40 codewords at 37.1 mean iterations, the
    loop 0 of 40 at 8.1 (frame errors per pass 37, 4, 1, 0, ...)."""
    _gain_on_the_cpu(oracle, ref, "pcmfm", 3.0)


# ------------------------------------------------------------------------------------------------ GPU
_counters = TC._counters


@pytest.fixture
def soft_ctx():
    from waveforms_amd import _hip

    ctx = _hip.new_ctx()
    yield ctx
    _hip.free_ctx(ctx)


def _priors(rng, n, sat=EXT_SAT, sigma=8.0):
    """name -> float32 prior per bit: zero, normal at the scale of λ clipped to ±sat, ±sat in runs of a codeword's length as a
    frozen codeword leaves them, and a mixture of runs of all three."""
    normal = np.clip(sigma * rng.standard_normal(n), -sat, sat).astype(np.float32)
    sats = np.where(rng.integers(0, 2, n) == 1, np.float32(-sat), np.float32(sat)).astype(np.float32)
    run = max(1, min(2048, n // 7))
    kind = np.repeat(rng.integers(0, 3, n // run + 1), run)[:n]      # per run: saturated, normal, zero
    mixed = np.where(kind == 0, sats, np.where(kind == 1, normal, np.float32(0.0))).astype(np.float32)
    return {"zero": np.zeros(n, dtype=np.float32), "normal": normal, "sat": sats, "mixed": mixed}


@pytest.mark.gpu
@pytest.mark.parametrize("waveform", ["multih", "pcmfm"])
@pytest.mark.parametrize("ebn0", [0.0, 6.0, 10.0])
def test_cpm_soft_apriori_bitwise_equals_the_definition(apref, soft_ctx, waveform, ebn0):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.viterbi.cpm import full_phase

    torch = _hip.torch()
    rows, _syms, spec = TC._link_rows(waveform, 100_000, ebn0)
    fspec = full_phase(spec)
    host = _hip.to_host(rows, complex_pairs=True)
    nb = rows.shape[0] * fspec.bits_per_symbol
    rng = np.random.default_rng(int(ebn0) + 3)
    _hip.set_option(soft_ctx, _hip.WF_OPT_DET_FINAL_VERIFY, 1)
    plain_llr, plain_bits = dev.cpm_soft(rows, fspec, 0, 0, ctx=soft_ctx)
    _counters(dev, soft_ctx)
    for name, prior in _priors(rng, nb).items():
        want_ext, want_bits = restate(apref, fspec, host, prior, 0.7)
        dp = _hip.to_device(prior)
        for warmup in (0, 2):
            ext, bits = dev.cpm_soft_apriori(rows, fspec, dp, 0.7, 0, warmup, ctx=soft_ctx)
            ext, bits = _hip.to_host(ext), _hip.to_host(bits)
            unproven, repaired = _counters(dev, soft_ctx)
            assert unproven == 0, (name, warmup)
            assert np.array_equal(ext.view(np.uint64), want_ext.view(np.uint64)), (name, warmup, int(np.count_nonzero(ext != want_ext)))
            assert np.array_equal(bits, want_bits), (name, warmup)
            if warmup == 2 and name == "zero":
                assert repaired > 0      # the short warm-up missed: the result above came through the repairs
        if name == "zero":
            assert np.array_equal(want_ext.view(np.uint64), _hip.to_host(plain_llr).view(np.uint64))
    ext, bits = dev.cpm_soft_apriori(rows, fspec, None, 0.7, 0, 0, ctx=soft_ctx)
    assert torch.equal(ext.view(torch.int64), plain_llr.view(torch.int64)) and torch.equal(bits, plain_bits)


@pytest.mark.gpu
@pytest.mark.parametrize("waveform", ["multih", "pcmfm"])
def test_cpm_soft_apriori_any_chunking_short_bursts_and_first_call(apref, soft_ctx, waveform):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    spec = _specs()[waveform]
    lg = spec.bits_per_symbol
    rng = np.random.default_rng(7)
    for n in (1, 2, 3, 5, 33, 1001):
        rows = 2.0 * (rng.standard_normal((n, spec.nfilt)) + 1j * rng.standard_normal((n, spec.nfilt)))
        prior = _priors(rng, n * lg, sat=12.0, sigma=4.0)["mixed" if n > 5 else "normal"]
        d_rows, dp = _hip.to_device(rows), _hip.to_device(prior)
        for first_call in (0, 1, 2, 5):
            want_ext, want_bits = restate(apref, spec, rows, prior, 1.3, first_call)
            for chunk in (0, 1, 7, 64):
                _hip.set_option(soft_ctx, _hip.WF_OPT_CPM_SOFT_CHUNK_CALLS, chunk)
                for warmup in (0, 1, 3):
                    ext, bits = dev.cpm_soft_apriori(d_rows, spec, dp, 1.3, first_call, warmup, ctx=soft_ctx)
                    assert np.array_equal(_hip.to_host(ext).view(np.uint64), want_ext.view(np.uint64)), (n, first_call, chunk, warmup)
                    assert np.array_equal(_hip.to_host(bits), want_bits), (n, first_call, chunk, warmup)
                    assert _counters(dev, soft_ctx)[0] == 0


@pytest.mark.gpu
def test_cpm_soft_apriori_proof_is_real(apref, soft_ctx):
    """Under a strong random prior a 2-call warm-up at 0 dB misses chunk starts and ends: with the repairs on the result is
    the definition through them, with the repairs off the same launch counts unproven chunks."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.viterbi.cpm import full_phase

    rows, _syms, spec = TC._link_rows("multih", 50_000, 0.0)
    fspec = full_phase(spec)
    nb = rows.shape[0] * fspec.bits_per_symbol
    prior = np.clip(30.0 * np.random.default_rng(31).standard_normal(nb), -EXT_SAT, EXT_SAT).astype(np.float32)
    want_ext, want_bits = restate(apref, fspec, _hip.to_host(rows, complex_pairs=True), prior, 1.0)
    dp = _hip.to_device(prior)
    _counters(dev, soft_ctx)
    ext, bits = dev.cpm_soft_apriori(rows, fspec, dp, 1.0, 0, 2, ctx=soft_ctx)
    assert np.array_equal(_hip.to_host(ext).view(np.uint64), want_ext.view(np.uint64)) and np.array_equal(_hip.to_host(bits), want_bits)
    unproven, repaired = _counters(dev, soft_ctx)
    assert unproven == 0 and repaired > 0
    _hip.set_option(soft_ctx, _hip.WF_OPT_DET_REPAIR, 1)
    dev.cpm_soft_apriori(rows, fspec, dp, 1.0, 0, 2, ctx=soft_ctx)
    unproven, repaired = _counters(dev, soft_ctx)
    assert unproven > 0 and repaired == 0


@pytest.mark.gpu
@pytest.mark.parametrize("waveform", ["multih", "pcmfm"])
def test_detector_keywords_take_the_apriori_path(apref, waveform):
    """CPMTrellisDetector.detect_soft(apriori=...) is the entry point; the defaults are today's plain path."""
    from waveforms_amd.viterbi.cpm import CPMTrellisDetector

    spec = _specs()[waveform]
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((300, spec.nfilt)) + 1j * rng.standard_normal((300, spec.nfilt))
    prior = (5.0 * rng.standard_normal(300 * spec.bits_per_symbol)).astype(np.float32)
    det = CPMTrellisDetector(spec)
    ext, bits = det.detect_soft(rows, 1, 0, apriori=prior, apriori_scale=0.5)
    want_ext, want_bits = restate(apref, spec, rows, prior, 0.5, 1)
    assert np.array_equal(ext.view(np.uint64), want_ext.view(np.uint64)) and np.array_equal(bits, want_bits)
    llr, _ = det.detect_soft(rows, 1)
    want_llr, _ = restate(apref, spec, rows, None, 1.0, 1)
    assert np.array_equal(llr.view(np.uint64), want_llr.view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("waveform,ebn0", [("multih", 7.0), ("pcmfm", 3.0)])
def test_gpu_loop_pass_by_pass(apref, waveform, ebn0):
    """A burst of 8 demo codewords, 4 outer passes: the prior buffer, the states, the information bits and the iterations
    after every pass equal the host chain made of the two restatements, fed the GPU's rows."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.encoding.coded import IterativeCPMLink

    code = ldpc.demo_code()
    link = IterativeCPMLink(code, 8, waveform=waveform, outer=4, inner=5, per_pass=True)
    spec, lg = link.spec, link.spec.bits_per_symbol
    info = link.info_bits(0)
    rows, _ = link.front_end(dev.ldpc_encode(code, info), ebn0, 7, 0)
    z = _hip.to_host(rows, complex_pairs=True)
    n = z.shape[0]
    assert n == link.ncalls and n * lg >= link.nbits
    snaps = []
    prior = np.zeros(n * lg, dtype=np.float32)
    state, iters, dec = np.zeros(8, dtype=np.uint8), np.zeros(8, dtype=np.int32), np.zeros((8, code.k), dtype=np.uint8)
    link.begin(n)
    for o in range(4):
        ext, hard = link.detect(rows, first=o == 0)
        link.decode(ext)
        want_ext, want_bits = restate(apref, spec, z, prior, link.damping)
        assert np.array_equal(_hip.to_host(ext).reshape(-1).view(np.uint64), want_ext[:link.nbits].view(np.uint64)), o
        assert np.array_equal(_hip.to_host(hard), want_bits[:link.nbits]), o
        TI.decode_ext_restatement(code, want_ext[:link.nbits].reshape(8, code.n_tx), state, prior[:link.nbits].reshape(8, code.n_tx),
                                  dec, iters, 1.0, link.alpha, 5, link.ext_clip, link.ext_sat)
        snaps.append(int(state.sum()))
        assert np.array_equal(_hip.to_host(link.prior).view(np.uint32), prior.view(np.uint32)), o
        assert np.array_equal(_hip.to_host(link.state), state) and np.array_equal(_hip.to_host(link.iters), iters), o
        assert np.array_equal(_hip.to_host(link.decided), dec), o
    _hip.device_check()
    assert (prior[link.nbits:] == 0).all()
    print("frozen after each pass:", snaps)
    assert snaps[-1] > snaps[0]                              # the loop does something on this burst


@pytest.mark.gpu
@pytest.mark.parametrize("waveform,ebn0", [("multih", 7.0), ("pcmfm", 3.0)])
def test_gpu_outer_1_is_the_one_pass_link_and_noiseless_freezes_at_once(waveform, ebn0):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.encoding.coded import CodedCPMLink, IterativeCPMLink

    code = ldpc.demo_code()
    it = IterativeCPMLink(code, 61, waveform=waveform, outer=1, inner=5)
    one = CodedCPMLink(code, 61, waveform=waveform, max_iter=5)
    it.run_block(ebn0, seed=5, stream_id=2)
    llr, _info = one.channel_llrs(ebn0, seed=5, stream_id=2)
    want = dev.ldpc_decode(code, llr, alpha=one.alpha, max_iter=5)
    assert _hip.torch().equal(it.decided, want["info_bits"]) and _hip.torch().equal(it.iters, want["iters"])
    one.run_block(ebn0, seed=5, stream_id=2)
    a, b = it.result(), one.result()
    assert a[:2] == b[:2] and a[3:] == b[3:] and it.uncoded_result() == one.uncoded_result()
    assert a[2] >= b[2]                                      # (open after 5 iterations includes "converged exactly at the 5th")
    assert it.uncoded_result()[0] > 0

    # Noiseless: no errors, every codeword frozen in pass 1.  The burst starts from a free state before any symbol has been
    # sent, so the λ of its FIRST symbol can have the wrong sign even without noise (tests/test_cpm_soft.py leaves the first
    # symbols out for that reason): the burst's first codeword may need one decoder iteration, no other needs any.
    quiet = IterativeCPMLink(code, 37, waveform=waveform, outer=3, inner=5, per_pass=True)
    quiet.run_block(None, seed=1, stream_id=0)
    quiet.run_block(None, seed=1, stream_id=1)
    lg = quiet.spec.bits_per_symbol
    be, fe, nc, m, its = quiet.result()
    assert (be, fe, nc, m) == (0, 0, 0, 2 * 37 * code.k) and its * 2 * 37 <= 2
    assert quiet.pass_results() == [(0, 0, 0, its)] * 3
    assert int(quiet.state.sum()) == 37 and int(quiet.iters[1:].sum()) == 0
    ue, um = quiet.uncoded_result()
    assert ue <= 2 * lg and um == 2 * 37 * code.n_tx


@pytest.mark.gpu
@pytest.mark.parametrize("waveform,ebn0", [("multih", 7.0), ("pcmfm", 3.0)])
def test_gpu_iterative_gain_on_a_full_block(waveform, ebn0):
    """One 1e7-channel-bit block (4 882 demo codewords in ONE burst) at the CPU test's operating points: the CPU test's
    condition against CodedCPMLink (50 iterations) on the same seed, and the three result tuples agree with each other.
    Measured on one MI355X: ARTM 7.0 dB, one pass 3 803 of 4 882 frame errors at 42.78 mean iterations, iterative 7 (4 810,
    961, 161, 62, 24, 13, 9, 7 after passes 1 ... 8) at 7.96; PCM/FM 3.0 dB, one pass 3 097 at 38.10, iterative 0 (4 830, 697,
    42, 5, 1, 1, 0, 0) at 8.12."""
    from waveforms_amd.encoding.coded import CodedCPMLink, IterativeCPMLink

    code = ldpc.demo_code()
    ncw = int(1e7) // code.n_tx
    assert ncw == 4882
    one = CodedCPMLink(code, ncw, waveform=waveform, max_iter=50)
    one.run_block(ebn0, seed=9, stream_id=0)
    _be1, fe1, _nc1, m1, it1 = one.result()
    idd = IterativeCPMLink(code, ncw, waveform=waveform, outer=8, inner=5, damping=0.7, per_pass=True)
    idd.run_block(ebn0, seed=9, stream_id=0)
    be, fe, nc, m, its = idd.result()
    passes = idd.pass_results()
    print(f"{waveform} {ebn0} dB, one pass: {fe1} of {ncw} frame errors, mean iterations {it1:.2f}; iterative: {fe} frame errors, {nc} open, "
          f"mean inner iterations {its:.2f}; per pass {passes}; uncoded {idd.uncoded_result()}")
    assert fe1 >= 4
    assert 4 * fe <= fe1
    assert its < it1
    # the tuples agree: the last pass is the result, the first detector pass is the one-pass link's, iterations only grow
    assert m == m1 == ncw * code.k and len(passes) == 8
    assert passes[-1] == (be, fe, nc, its)
    assert idd.uncoded_result() == one.uncoded_result() and idd.uncoded_result()[1] == ncw * code.n_tx
    assert all(b[3] >= a[3] for a, b in zip(passes, passes[1:])) and all(b[2] <= a[2] for a, b in zip(passes, passes[1:]))
    assert (fe == 0) == (be == 0) and fe <= be and nc <= ncw
