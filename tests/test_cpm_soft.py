"""Max-log-MAP soft output of the generic CPM trellis (wf_cpm_soft, include/wfhip.h): ARTM multi-h and PCM/FM.

The soft output is defined on the full-phase trellis (NC = p) of the shipped matched filters.  The definition is restated
sequentially in a few lines of C (tests/cpm_soft_ref.c, explicit fma, compiled here with -ffp-contract=off), pinned to
brute force on short bursts and to the sequential hard detector of oracle/cpm_oracle.c (CPU).  On the GPU the
chunk-parallel kernels must equal the restatement BITWISE whatever the warm-up, chunking and first call; λ < 0 must be the
full-phase hard detector's decision, and the LLRs must be ordered.
"""
import ctypes
import itertools
import subprocess
from pathlib import Path

import numpy as np
import pytest

SPS = 8
HERE = Path(__file__).resolve().parent


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    so = tmp_path_factory.mktemp("cpm_soft_ref") / "libcpmsoftref.so"
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", str(so), str(HERE / "cpm_soft_ref.c"), "-lm"])
    lib = ctypes.CDLL(str(so))
    lib.cpm_soft_rec.restype = ctypes.c_int
    lib.cpm_soft_rows.restype = ctypes.c_int
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _K(spec):
    return (ctypes.c_int * 2)(spec.K[0], spec.K[-1])


def _specs():
    from waveforms_amd.viterbi import cpm

    return {"multih": cpm.ARTM_64, "pcmfm": cpm.PCMFM_20}


def restate(ref, spec, rows, first_call=0):
    """The header's definition over complex128 rows [n][M^Lp] -> (llr, bits), lgM per call."""
    from waveforms_amd.viterbi.cpm import rotation_table

    rows = np.ascontiguousarray(rows, dtype=np.complex128).reshape(-1, spec.nfilt)
    n, lg = rows.shape[0], spec.bits_per_symbol
    llr, bits = np.empty(n * lg), np.empty(n * lg, dtype=np.uint8)
    rot = rotation_table(spec)
    assert ref.cpm_soft_rows(spec.M, spec.p, len(spec.K), _K(spec), spec.Lp, _p(rot), _p(rows), ctypes.c_int64(n),
                             ctypes.c_int64(first_call), _p(llr), _p(bits)) == 0
    return llr, bits


def _ends(spec, n):
    """end[s][u] of the full-phase trellis at global call n (cpm_oracle.c with NC = p), written independently of the C."""
    M, p, Lp, K = spec.M, spec.p, spec.Lp, spec.K
    m_old = n - Lp + 1
    K_old = K[m_old % len(K)] if m_old >= 0 else 0
    msub = M ** max(Lp - 2, 0)
    out = []
    for s in range(spec.nstates):
        v, corr = s % p, s // p
        row = []
        for u in range(M):
            u_old = u if Lp == 1 else corr // msub
            corr2 = 0 if Lp == 1 else u + M * (corr % msub)
            row.append((v + K_old * u_old) % p + p * corr2)
        out.append(row)
    return out


def brute_force(spec, inc, first_call):
    """λ[lgM k + i] = min over paths with bit i of u_k = 1 - min over paths with it 0; every start state, every input."""
    n, S, M = inc.shape
    lg = spec.bits_per_symbol
    ends = [_ends(spec, first_call + k) for k in range(n)]
    best = np.full((n, lg, 2), np.inf)
    for s0 in range(S):
        for us in itertools.product(range(M), repeat=n):
            s, cost = s0, 0.0
            for k in range(n):
                cost += inc[k, s, us[k]]
                s = ends[k][s][us[k]]
            for k in range(n):
                for i in range(lg):
                    b = (us[k] >> (lg - 1 - i)) & 1
                    best[k, i, b] = min(best[k, i, b], cost)
    return (best[:, :, 1] - best[:, :, 0]).reshape(-1)


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("waveform", ["multih", "pcmfm"])
def test_recursion_equals_brute_force(ref, waveform):
    from waveforms_amd.viterbi.cpm import rotation_table

    spec = _specs()[waveform]
    S, M, lg = spec.nstates, spec.M, spec.bits_per_symbol
    rng = np.random.default_rng(5 + M)
    for first_call in (0, 1, 2):
        for n in range(1, 5):
            # integer-valued increments: every sum is exact, so the normalised recursions give the brute force's λ exactly
            inc = rng.integers(-8, 9, (n, S, M)).astype(np.float64)
            llr, bits = np.empty(n * lg), np.empty(n * lg, dtype=np.uint8)
            assert ref.cpm_soft_rec(M, spec.p, len(spec.K), _K(spec), spec.Lp, _p(inc), ctypes.c_int64(n), ctypes.c_int64(first_call),
                                    _p(llr), _p(bits)) == 0
            want = brute_force(spec, inc, first_call)
            assert np.array_equal(llr, want), (first_call, n, llr, want)
            assert np.array_equal(bits, (want < 0).astype(np.uint8))
            # real-valued: increments from random rows (the definition's fma), equal up to the normalisations' rounding
            rows = rng.standard_normal((n, spec.nfilt)) + 1j * rng.standard_normal((n, spec.nfilt))
            inc = np.empty((n, S, M))
            rot = rotation_table(spec)
            ref.cpm_soft_incs(M, spec.p, len(spec.K), _K(spec), spec.Lp, _p(rot), _p(rows), ctypes.c_int64(n), ctypes.c_int64(first_call), _p(inc))
            llr, _ = restate(ref, spec, rows, first_call)
            np.testing.assert_allclose(llr, brute_force(spec, inc, first_call), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("waveform", ["multih", "pcmfm"])
def test_restatement_pinned_to_the_sequential_detector(oracle, ref, waveform):
    """On the oracle's rows of the full-phase design: noiseless, λ < 0 is the transmitted bits; at 10 dB it is the
    sequential hard detector's decision (cpm_oracle.c, decided D - 1 calls later), away from the ends."""
    spec = _specs()[waveform]
    M, lg = spec.M, spec.bits_per_symbol
    if waveform == "multih":
        bits = oracle.glfsr_bits(oracle.lfsr_mask(23), (1 << 23) - 1, 2 * 3000)[0]
        sym, pulse = oracle.multih_mapper(bits)[0], oracle.freq_pulse_multih_irig(SPS)
        ospec = oracle.ARTM_64
    else:
        sym, pulse = oracle.pcmfm_mapper(oracle.pn_sequence(15)[:3000]), oracle.freq_pulse_pcmfm(SPS)
        ospec = oracle.CPMDetectorSpec(M=2, p=10, K=(7,), Lp=2, NC=10, D=32)
    tx = oracle.u_to_bits(oracle.symbols_to_u(sym, M), M)
    res = oracle.cpm_detection_run(sym, pulse, SPS, ospec)
    n = res["rows"].shape[0]
    assert n > 2900
    _, sbits = restate(ref, spec, res["rows"])
    lo, hi = 8 * lg, (n - 8) * lg
    assert np.array_equal(sbits[lo:hi], tx[lo:hi])

    noise = oracle.numpy_awgn(oracle.cpm_sigma_for_ebn0(10.0, SPS, lg), (sym.size + 1) * SPS, np.random.Generator(np.random.PCG64(5)))
    res = oracle.cpm_detection_run(sym, pulse, SPS, ospec, noise=noise)
    _, sbits = restate(ref, spec, res["rows"])
    dec = oracle.u_to_bits(res["decisions"], M)            # symbol j, decided at call j + D - 1
    m = res["decisions"].size * lg
    assert np.array_equal(sbits[lo:m], dec[lo:m])


def test_argument_checks_and_geometry_without_a_gpu():
    """Bad arguments return WF_ERR_VALUE before the context is touched (a fake context: no device exists here)."""
    from waveforms_amd import _hip
    from waveforms_amd.viterbi import cpm

    lib = _hip.lib()
    fake = ctypes.create_string_buffer(1 << 16)
    buf = ctypes.create_string_buffer(8192)
    base = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    rot, rows, llr, bits = base, base + 1024, base + 4096, base + 6144
    V = _hip.WF_ERR_VALUE
    good = cpm.ARTM_64.c_config()

    def call(cfg=good, ctx=fake, r=rot, z=rows, n=10, first=0, warmup=0, out=llr, b=bits):
        return lib.wf_cpm_soft(ctx, None if cfg is None else ctypes.byref(cfg), r, z, n, first, warmup, out, b, None)

    assert call(ctx=None) == V and call(cfg=None) == V and call(r=None) == V and call(z=None) == V
    assert call(out=None) == V and call(b=None) == V
    for n in (0, -1):
        assert call(n=n) == V
    assert call(first=-1) == V and call(warmup=-1) == V
    for spec in (cpm.ARTM_16, cpm.PCMFM_10, cpm.ARTM_256):       # NC != p; 256 states
        assert call(cfg=spec.c_config()) == V
    for field, value in (("M", 3), ("M", 8), ("nh", 3), ("nh", 0), ("Lp", 0), ("Lp", 4), ("NC", 8)):
        cfg = cpm.ARTM_64.c_config()
        setattr(cfg, field, value)
        assert call(cfg=cfg) == V, (field, value)
    g = (ctypes.c_int64 * 4)()
    geo = lib.wf_cpm_soft_geometry
    assert geo(None, ctypes.byref(good), 100, 0, g) == V and geo(fake, None, 100, 0, g) == V
    assert geo(fake, ctypes.byref(good), 0, 0, g) == V and geo(fake, ctypes.byref(good), 100, -1, g) == V
    assert geo(fake, ctypes.byref(good), 100, 0, None) == V
    assert geo(fake, ctypes.byref(cpm.ARTM_256.c_config()), 100, 0, g) == V
    # the geometry is a host computation: the library's defaults on a context with default options
    assert geo(fake, ctypes.byref(good), 10_000_000, 0, g) == 0
    assert (g[0], g[1], g[2]) == (1232, 8117, 64) and g[3] >= 10_000_000 * 64 * 8 // 16
    assert geo(fake, ctypes.byref(good), 1000, 2, g) == 0 and (g[0], g[1], g[2]) == (64, 16, 2)
    assert geo(fake, ctypes.byref(cpm.PCMFM_20.c_config()), 200_000, 0, g) == 0 and (g[0], g[1], g[2]) == (64, 3125, 64)
    assert lib.wf_ctx_set_option(fake, _hip.WF_OPT_CPM_SOFT_CHUNK_CALLS, 8193) == V
    assert lib.wf_ctx_set_option(fake, _hip.WF_OPT_CPM_SOFT_CHUNK_CALLS, -1) == V
    assert lib.wf_ctx_set_option(fake, _hip.WF_OPT_CPM_SOFT_CHUNK_CALLS, 7) == 0
    assert geo(fake, ctypes.byref(good), 1000, 0, g) == 0 and (g[0], g[1]) == (7, 143)


def test_exports_bound_and_kernels_do_not_spill():
    import sys

    from waveforms_amd import _hip, device
    from waveforms_amd.viterbi import cpm

    lib = _hip.lib()
    for name in ("wf_cpm_soft", "wf_cpm_soft_geometry"):
        assert name in _hip.SIGNATURES and hasattr(lib, name)
    assert callable(device.cpm_soft) and callable(device.cpm_soft_geometry)
    assert callable(cpm.CPMTrellisDetector.detect_soft) and callable(cpm.CPMTrellisDetector.detect_soft_device)
    assert cpm.full_phase(cpm.ARTM_16) == cpm.ARTM_64 and cpm.full_phase(cpm.PCMFM_10) == cpm.PCMFM_20
    assert {"PCMFM_20", "full_phase"} <= set(cpm.__all__)

    sys.path.insert(0, str(HERE.parent / "tools"))
    import kernel_resources as kr
    from waveforms_amd.csrc.build import build

    so = build(verbose=False)
    tab = {k: v for k, v in kr.kernel_table(so).items() if k.startswith("cpm_soft_")}
    asm = kr.loop_spill_counts(so, "cpm_soft_")
    assert len(tab) >= 25, sorted(tab)
    for name, row in tab.items():
        assert row["vgpr_spill_count"] == 0 and row["sgpr_spill_count"] == 0 and row["private_segment_fixed_size"] == 0, (name, row)
        a = asm[name]
        assert a["scratch_load_in_loop"] == 0 and a["scratch_store_in_loop"] == 0, (name, a)
        # (v_readlane in the loops are the wave-wide minima's; with no SGPR spills none of them reloads a spill)
        assert a["v_writelane_in_loop"] == 0, (name, a)


# ------------------------------------------------------------------------------------------------ GPU
def _torch():
    import torch

    return torch


def _link_rows(waveform, n, ebn0, seed=1):
    """Rows (float64[calls, nfilt, 2]), transmitted symbols (alpha, int8) and the reduced design of one CPMLink block."""
    from waveforms_amd.link import CPMLink

    torch = _torch()
    link = CPMLink(n, SPS, waveform=waveform, private_ctx=True)
    link.run_block(ebn0, seed=seed)
    lay = link.layout()
    calls, nf = lay["calls"], link.spec.nfilt
    rows = link.workspace[lay["off_rows"]:lay["off_rows"] + calls * nf * 16].clone().view(torch.float64).view(calls, nf, 2)
    syms = link.workspace[lay["off_syms"]:lay["off_syms"] + n].clone().view(torch.int8)
    spec = link.spec
    torch.cuda.synchronize()
    del link
    return rows, syms, spec


def _tx_bits(syms, M):
    u = ((syms.to(_torch().int16) + (M - 1)) // 2).to(_torch().uint8)
    return _hip_host(_u_bits(u, M))


def _u_bits(u, M):
    torch = _torch()
    return u.view(-1, 1) if M == 2 else torch.stack([(u >> 1) & 1, u & 1], dim=1).reshape(-1)


def _hip_host(x):
    from waveforms_amd import _hip

    return _hip.to_host(x).reshape(-1)


def _counters(dev, ctx):
    return dev.viterbi_unmerged(reset=True, ctx=ctx), dev.viterbi_repaired(reset=True, ctx=ctx)


@pytest.fixture
def soft_ctx():
    from waveforms_amd import _hip

    ctx = _hip.new_ctx()
    yield ctx
    _hip.free_ctx(ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("waveform", ["multih", "pcmfm"])
@pytest.mark.parametrize("ebn0", [0.0, 6.0, 10.0])
def test_cpm_soft_bitwise_equals_the_definition(ref, soft_ctx, waveform, ebn0):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.viterbi.cpm import full_phase

    rows, _syms, spec = _link_rows(waveform, 200_000, ebn0)
    fspec = full_phase(spec)
    want_llr, want_bits = restate(ref, fspec, _hip.to_host(rows, complex_pairs=True))
    _hip.set_option(soft_ctx, _hip.WF_OPT_DET_FINAL_VERIFY, 1)
    _counters(dev, soft_ctx)
    for warmup in (0, 2):
        llr, bits = dev.cpm_soft(rows, fspec, 0, warmup, ctx=soft_ctx)
        llr, bits = _hip.to_host(llr), _hip.to_host(bits)
        unproven, repaired = _counters(dev, soft_ctx)
        assert unproven == 0, warmup
        assert np.array_equal(llr.view(np.uint64), want_llr.view(np.uint64)), (warmup, int(np.count_nonzero(llr != want_llr)))
        assert np.array_equal(bits, want_bits), warmup
        if warmup == 2:
            assert repaired > 0          # the short warm-up missed: the result above came through the repairs


@pytest.mark.gpu
@pytest.mark.parametrize("waveform", ["multih", "pcmfm"])
def test_cpm_soft_any_chunking_short_bursts_and_first_call(ref, soft_ctx, waveform):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    spec = _specs()[waveform]
    rng = np.random.default_rng(7)
    for n in (1, 2, 3, 5, 33, 1001):
        rows = 2.0 * (rng.standard_normal((n, spec.nfilt)) + 1j * rng.standard_normal((n, spec.nfilt)))
        d_rows = _hip.to_device(rows)
        for first_call in (0, 1, 2, 5):
            want_llr, want_bits = restate(ref, spec, rows, first_call)
            for chunk in (0, 1, 7, 64):
                _hip.set_option(soft_ctx, _hip.WF_OPT_CPM_SOFT_CHUNK_CALLS, chunk)
                for warmup in (0, 1, 3):
                    llr, bits = dev.cpm_soft(d_rows, spec, first_call, warmup, ctx=soft_ctx)
                    assert np.array_equal(_hip.to_host(llr).view(np.uint64), want_llr.view(np.uint64)), (n, first_call, chunk, warmup)
                    assert np.array_equal(_hip.to_host(bits), want_bits), (n, first_call, chunk, warmup)
                    assert _counters(dev, soft_ctx)[0] == 0


@pytest.mark.gpu
def test_cpm_soft_proof_is_real(soft_ctx):
    """With the repairs off, a 2-call warm-up at 0 dB leaves chunks unproven: the proof detects what it repairs."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.viterbi.cpm import full_phase

    rows, _syms, spec = _link_rows("multih", 50_000, 0.0)
    _hip.set_option(soft_ctx, _hip.WF_OPT_DET_REPAIR, 1)
    _counters(dev, soft_ctx)
    dev.cpm_soft(rows, full_phase(spec), 0, 2, ctx=soft_ctx)
    unproven, repaired = _counters(dev, soft_ctx)
    assert unproven > 0 and repaired == 0


@pytest.mark.gpu
@pytest.mark.parametrize("waveform", ["multih", "pcmfm"])
def test_cpm_soft_alignment_and_api(waveform):
    """Noiseless link rows: bits = the transmitted bits (bit j with λ[j]); the reduced design's detect_soft is the
    full-phase one's; the hard carry is untouched."""
    from waveforms_amd import _hip
    from waveforms_amd.viterbi.cpm import CPMTrellisDetector, full_phase

    torch = _torch()
    rows, syms, spec = _link_rows(waveform, 4000, None)
    lg = spec.bits_per_symbol
    tx = _tx_bits(syms, spec.M)
    host = _hip.to_host(rows, complex_pairs=True)
    det = CPMTrellisDetector(spec)
    det.detect(host[:1000])
    i0, carry = det.i, det._d_state.clone()
    llr, bits = det.detect_soft(host)
    assert det.i == i0 and torch.equal(det._d_state, carry)
    n = rows.shape[0]
    assert n > 3900 and bits.size == n * lg
    lo, hi = 8 * lg, (n - 8) * lg
    assert np.array_equal(bits[lo:hi], tx[lo:hi])
    full_llr, full_bits = CPMTrellisDetector(full_phase(spec)).detect_soft(host)
    assert np.array_equal(llr.view(np.uint64), full_llr.view(np.uint64)) and np.array_equal(bits, full_bits)
    d_llr, _ = det.detect_soft_device(rows)
    assert np.array_equal(_hip.to_host(d_llr), llr)
    assert np.array_equal(det.detect(host[1000:2000]), CPMTrellisDetector(spec).detect(host[:2000])[1000 - spec.D + 1:])


@pytest.mark.gpu
@pytest.mark.parametrize("waveform", ["multih", "pcmfm"])
def test_cpm_soft_decisions_are_the_ml_sequence(soft_ctx, waveform):
    """At 10 dB, λ < 0 is the full-phase hard detector's decision (its call k + D - 1 decides symbol k), away from the last D."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.viterbi.cpm import CPMTrellisDetector, full_phase

    rows, _syms, spec = _link_rows(waveform, 1_000_000, 10.0)
    fspec = full_phase(spec)
    lg, D = fspec.bits_per_symbol, fspec.D
    _llr, bits = dev.cpm_soft(rows, fspec, 0, 0, ctx=soft_ctx)
    assert _counters(dev, soft_ctx)[0] == 0
    dec = CPMTrellisDetector(fspec).detect_device(rows)
    n = rows.shape[0]
    hard = _hip_host(_u_bits(dec[D - 1:], fspec.M))
    soft = _hip.to_host(bits)[:(n - D + 1) * lg]
    diff = np.flatnonzero(soft[8 * lg:] != hard[8 * lg:])
    assert diff.size == 0, f"{diff.size} differences, first at {diff[:8]}"


@pytest.mark.gpu
def test_cpm_soft_full_size_any_warmup(soft_ctx):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.viterbi.cpm import full_phase

    torch = _torch()
    rows, _syms, spec = _link_rows("multih", 10_000_000, 6.0)
    fspec = full_phase(spec)
    _hip.set_option(soft_ctx, _hip.WF_OPT_DET_FINAL_VERIFY, 1)
    _counters(dev, soft_ctx)
    a_llr, a_bits = dev.cpm_soft(rows, fspec, 0, 0, ctx=soft_ctx)
    assert _counters(dev, soft_ctx)[0] == 0
    b_llr, b_bits = dev.cpm_soft(rows, fspec, 0, 6, ctx=soft_ctx)
    unproven, repaired = _counters(dev, soft_ctx)
    assert unproven == 0 and repaired > 0
    assert torch.equal(a_llr.view(torch.int64), b_llr.view(torch.int64))
    assert torch.equal(a_bits, b_bits)


@pytest.mark.gpu
def test_cpm_soft_llr_is_ordered(soft_ctx):
    """At 6 dB the error rate of λ < 0 falls across unit-wide bins of |λ|/σ² (bins with >= 200 errors)."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.viterbi.cpm import full_phase, sigma_for_ebn0

    ebn0 = 6.0
    rows, syms, spec = _link_rows("multih", 1_000_000, ebn0)
    fspec = full_phase(spec)
    llr, bits = dev.cpm_soft(rows, fspec, 0, 0, ctx=soft_ctx)
    llr, bits, tx = _hip.to_host(llr), _hip.to_host(bits), _tx_bits(syms, spec.M)
    lg = spec.bits_per_symbol
    m = min(tx.size, bits.size) - 8 * lg
    err = bits[:m] != tx[:m]
    x = np.abs(llr[:m]) / sigma_for_ebn0(ebn0, SPS, lg) ** 2
    b = np.floor(x).astype(np.int64)
    nb = int(b.max()) + 1
    errs, tot = np.bincount(b, weights=err, minlength=nb), np.bincount(b, minlength=nb)
    keep = np.flatnonzero(errs >= 200)
    rates = errs[keep] / tot[keep]
    assert keep.size >= 4, (errs, tot)
    assert np.all(np.diff(rates) < 0), list(zip(keep.tolist(), rates.tolist()))
