"""Iterative detection and decoding of the coded SOQPSK-TG chain: wf_viterbi4_soft_apriori, wf_ldpc_decode_ext, wf_ldpc_count
(include/wfhip.h) and IterativeSOQPSKLink (waveforms_amd/encoding/coded.py).

The two definitions are restated here on top of the restatements of tests/test_soft_detector.py and tests/test_ldpc.py:
``apriori_restatement`` (a loop over sections in float64, pinned to brute force over all paths) and ``decode_ext_restatement``
(the decoder restatement run on the open codewords only).  On the GPU both kernels must equal them BITWISE, and so must the
whole loop pass by pass.

The algorithm's gain is checked on the CPU from the restatements alone (PT, information Eb/N0 4.5 dB, 40 demo codewords, one
per burst): 8 outer x 5 inner passes at damping 0.7 must end with at most a quarter of the frame errors of one pass of 50
iterations, in fewer iterations in total.  The factor 4 is a cap, not a measurement: on this test's seed the one-pass chain
fails 39 of 40 codewords at 50.0 mean iterations, the loop 0 of 40 at 12.35 (frame errors per pass 40, 31, 7, 0, ...).
"""
import ctypes
import itertools

import numpy as np
import pytest

import test_ldpc as TL
import test_soft_detector as TS
from waveforms_amd.encoding import ldpc

SPS = 8
PAD = 16


# ------------------------------------------------------------------------------------------------ restatements
def apriori_restatement(oracle, rows, prior, scale, differential):
    """The header's definition of wf_viterbi4_soft_apriori, one section at a time -> (ext, bits).  ``prior``: float32 per
    row or None."""
    brs = TS._branches(oracle, differential)
    inc = TS._increments(oracle, rows, differential).tolist()
    n = len(inc)
    if prior is None:
        pi = [0.0] * n
    else:
        pi = (np.float64(scale) * np.asarray(prior, dtype=np.float32).astype(np.float64)).tolist()
    inf = float("inf")
    alpha = [None] * (n + 1)
    a = [0.0, 0.0, 0.0, 0.0]
    alpha[0] = a
    for k in range(n):
        ik, new = inc[k], [inf, inf, inf, inf]
        for (b, s, e, i, _x) in brs[k & 1]:
            v = a[s] + ((ik[b] + pi[k]) if i else ik[b])
            if v < new[e]:
                new[e] = v
        mn = min(new)
        a = [v - mn for v in new]
        alpha[k + 1] = a
    ext = np.empty(n)
    bt = [0.0, 0.0, 0.0, 0.0]
    for k in range(n - 1, -1, -1):
        ik, a, new = inc[k], alpha[k], [inf, inf, inf, inf]
        m = [inf, inf]
        for (b, s, e, i, _x) in brs[k & 1]:
            t = (a[s] + ik[b]) + bt[e]
            if t < m[i]:
                m[i] = t
            v = ((ik[b] + pi[k]) if i else ik[b]) + bt[e]
            if v < new[s]:
                new[s] = v
        ext[k] = m[1] - m[0]
        mn = min(new)
        bt = [v - mn for v in new]
    return ext, ((ext + np.array(pi)) < 0).astype(np.uint8)


def apriori_brute_force(oracle, rows, pi, differential):
    """λᵉ_k = min over paths with u_k = 1 of (Σ_j inc_j + Σ_{j != k} u_j π_j) - the same with u_k = 0, every start state."""
    t = oracle.trellis_tables(TS.TRELLIS[differential])
    inc = TS._increments(oracle, rows, differential)
    n = inc.shape[0]
    bidx = {}
    for c, brs in enumerate(TS._branches(oracle, differential)):
        for (b, s, _e, i, _x) in brs:
            bidx[(c, s, i)] = b
    best = np.full((n, 2), np.inf)
    for s0 in range(4):
        for u in itertools.product((0, 1), repeat=n):
            s, cost = s0, 0.0
            for k in range(n):
                cost += inc[k, bidx[(k & 1, s, u[k])]]
                s = int(t["next"][k & 1, s, u[k]])
            tot = cost + sum(u[j] * pi[j] for j in range(n))
            for k in range(n):
                best[k, u[k]] = min(best[k, u[k]], tot - u[k] * pi[k])
    return best[:, 1] - best[:, 0]


def decode_ext_restatement(code, llr, state, ext, info, iters, scale=1.0, alpha=0.75, max_iter=5, ext_clip=np.inf, ext_sat=50.0,
                           post=None):
    """The header's definition of wf_ldpc_decode_ext on top of the decoder restatement: ``state`` (u8 ncw), ``ext`` (float32
    ncw x n_tx), ``info`` (u8 ncw x k), ``iters`` (int32 ncw) and ``post`` (float32 ncw x n or None) are updated IN PLACE for the
    open codewords; frozen ones are not looked at."""
    llr = np.atleast_2d(np.asarray(llr, dtype=np.float64))
    act = np.flatnonzero(state == 0)
    if act.size == 0:
        return
    t = code.c_tables()
    got_info, got_post, its = TL.decode_restatement(code, llr[act], scale, alpha, max_iter)
    conv = TL._syndrome_ok(t, got_post)                       # stopped with H x̂ = 0 (a stopped codeword is never updated again)
    assert (conv | (its == max_iter)).all()
    lch = (scale * llr[act]).astype(np.float32)
    lt = got_post[:, code.tx_order]
    e = np.clip(lt - lch, -np.float32(ext_clip), np.float32(ext_clip)).astype(np.float32)
    sat = np.where(lt < 0, -np.float32(ext_sat), np.float32(ext_sat)).astype(np.float32)
    ext[act] = np.where(conv[:, None], sat, e)
    info[act] = got_info
    iters[act] += its
    state[act] = conv.astype(np.uint8)
    if post is not None:
        post[act] = got_post


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("differential", [True, False])
def test_apriori_restatement_equals_brute_force(oracle, differential):
    rng = np.random.default_rng(5 + differential)
    for n in range(1, 11):
        # integer rows and integer priors: every sum is exact
        rows = rng.integers(-8, 9, (n, 3)) + 1j * rng.integers(-8, 9, (n, 3))
        prior = rng.integers(-12, 13, n).astype(np.float32)
        ext, bits = apriori_restatement(oracle, rows, prior, 1.0, differential)
        want = apriori_brute_force(oracle, rows, prior.astype(np.float64), differential)
        assert np.array_equal(ext, want), (n, ext, want)
        assert np.array_equal(bits, ((want + prior) < 0).astype(np.uint8))
        # real-valued: equal up to the rounding of the normalisations
        rows = rng.standard_normal((n, 3)) + 1j * rng.standard_normal((n, 3))
        prior = (3.0 * rng.standard_normal(n)).astype(np.float32)
        ext, _ = apriori_restatement(oracle, rows, prior, 0.7, differential)
        want = apriori_brute_force(oracle, rows, 0.7 * prior.astype(np.float64), differential)
        np.testing.assert_allclose(ext, want, rtol=1e-12, atol=1e-12)
        # zero prior (and none): the plain detector's restatement, bitwise
        llr, hard = TS.soft_restatement(oracle, rows, differential)
        for p in (None, np.zeros(n, dtype=np.float32), -np.zeros(n, dtype=np.float32)):
            ext, bits = apriori_restatement(oracle, rows, p, 0.7, differential)
            assert np.array_equal(ext.view(np.uint64), llr.view(np.uint64)) and np.array_equal(bits, hard)


def test_apriori_prior_moves_the_neighbours_not_its_own_bit(oracle):
    """Extrinsic: λᵉ_k does not depend on π_k; a strong prior on bit k decides bit k (through bits) and shifts λᵉ elsewhere."""
    rng = np.random.default_rng(17)
    rows = rng.standard_normal((40, 3)) + 1j * rng.standard_normal((40, 3))
    base, _ = apriori_restatement(oracle, rows, None, 1.0, True)
    prior = np.zeros(40, dtype=np.float32)
    prior[20] = -100.0 if base[20] > 0 else 100.0             # against the channel's decision
    ext, bits = apriori_restatement(oracle, rows, prior, 1.0, True)
    assert ext[20] == base[20]
    assert bits[20] == (prior[20] < 0)
    assert np.any(ext[18:23] != base[18:23])


def _noisy(code, rng, ncw, sigma):
    u = rng.integers(0, 2, (ncw, code.k), dtype=np.uint8)
    tx = code.encode_host(u)
    return u, 2.0 * ((1.0 - 2.0 * tx) + rng.normal(0, sigma, tx.shape)) / sigma**2


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_decode_ext_restatement(seed):
    """Frozen codewords untouched, saturation on convergence (at iteration 0 too), clip, punctured codes."""
    code = TL.random_code(seed, punct=bool(seed % 2))
    rng = np.random.default_rng(100 + seed)
    ncw = 12
    u, llr = _noisy(code, rng, ncw, 0.8)
    llr[0] = 4.0 * (1.0 - 2.0 * code.encode_host(u[:1])[0])          # clean: converged at iteration 0
    llr[-2:] = rng.normal(0, 8.0, (2, code.n_tx))                    # garbage: not converged
    state = np.zeros(ncw, dtype=np.uint8)
    state[[3, 7]] = 1
    ext = np.full((ncw, code.n_tx), 123.0, dtype=np.float32)
    info = np.full((ncw, code.k), 9, dtype=np.uint8)
    iters = np.full(ncw, 1000, dtype=np.int32)
    post = np.full((ncw, code.n), -7.0, dtype=np.float32)
    decode_ext_restatement(code, llr, state, ext, info, iters, 0.5, 0.75, 4, 1.5, 20.0, post)
    w_info, w_post, w_it = TL.decode_restatement(code, llr, 0.5, 0.75, 4)
    ok = TL._syndrome_ok(code.c_tables(), w_post)
    for b in range(ncw):
        if b in (3, 7):
            assert state[b] == 1 and (ext[b] == 123.0).all() and (info[b] == 9).all() and iters[b] == 1000 and (post[b] == -7.0).all()
            continue
        assert np.array_equal(info[b], w_info[b]) and iters[b] == 1000 + w_it[b] and state[b] == ok[b]
        assert np.array_equal(post[b].view(np.uint32), w_post[b].view(np.uint32))
        lt = w_post[b, code.tx_order]
        if ok[b]:
            assert np.array_equal(ext[b], np.where(lt < 0, np.float32(-20.0), np.float32(20.0)))
        else:
            want = lt - (0.5 * llr[b]).astype(np.float32)
            assert want.dtype == np.float32 and np.abs(ext[b]).max() <= 1.5
            assert np.array_equal(ext[b], np.minimum(np.maximum(want, np.float32(-1.5)), np.float32(1.5)))
    assert state[0] == 1 and (iters[0] == 1000 or seed % 2) and state[-1] == 0 and state[-2] == 0      # (punctured: L = 0 there)
    assert (np.abs(ext[-1]) == 1.5).any()                            # the clip acts
    assert ext.shape[1] == code.n_tx < code.n or not seed % 2         # punctured variables have no entry
    # a second pass decodes only what is still open, and adds its iterations
    before = (ext.copy(), info.copy(), iters.copy(), state.copy())
    decode_ext_restatement(code, llr, state, ext, info, iters, 0.5, 0.75, 4, 1.5, 20.0)
    frozen = before[3] == 1
    assert np.array_equal(ext[frozen], before[0][frozen]) and np.array_equal(iters[frozen], before[2][frozen])
    assert np.array_equal(iters[~frozen], before[2][~frozen] + w_it[~frozen])


def test_idd_entry_points_exported_and_bound():
    from waveforms_amd import _hip
    from waveforms_amd import device
    from waveforms_amd.encoding import coded

    lib = _hip.lib()
    for name in ("wf_viterbi4_soft_apriori", "wf_ldpc_decode_ext", "wf_ldpc_count"):
        assert name in _hip.SIGNATURES and hasattr(lib, name)
    assert callable(device.viterbi_soft_apriori) and callable(device.ldpc_decode_ext) and callable(device.ldpc_count)
    assert issubclass(coded.IterativeSOQPSKLink, coded.CodedSOQPSKLink)


def test_idd_argument_validation_without_a_gpu():
    """Bad arguments return WF_ERR_VALUE before the context (a fake one: no device exists here) or the code is touched."""
    from waveforms_amd import _hip

    lib = _hip.lib()
    V = _hip.WF_ERR_VALUE if hasattr(_hip, "WF_ERR_VALUE") else 1
    buf = (ctypes.c_double * 64)()
    fake = ctypes.cast(buf, ctypes.c_void_p)
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 2)
    inf, nan = float("inf"), float("nan")
    f = lib.wf_viterbi4_soft_apriori
    assert f(None, p, 10, 48, 1, 0, p, 1.0, p, p, None) == V
    assert f(fake, None, 10, 48, 1, 0, p, 1.0, p, p, None) == V
    assert f(fake, p, 10, 48, 1, 0, p, 1.0, None, p, None) == V
    assert f(fake, p, 10, 48, 1, 0, p, 1.0, p, None, None) == V
    assert f(fake, p, 0, 48, 1, 0, p, 1.0, p, p, None) == V
    assert f(fake, p, 10, 40, 1, 0, p, 1.0, p, p, None) == V
    assert f(fake, p, 10, 48, 1, -1, p, 1.0, p, p, None) == V
    assert f(fake, p, 10, 48, 1, 0, p, inf, p, p, None) == V
    assert f(fake, p, 10, 48, 1, 0, p, nan, p, p, None) == V
    assert f(fake, p, 10, 48, 1, 0, None, nan, p, p, None) == V
    assert f(fake, p, 10, 48, 1, 0, odd, 1.0, p, p, None) == V
    assert f(fake, odd, 10, 48, 1, 0, p, 1.0, p, p, None) == V
    g = lib.wf_ldpc_decode_ext
    assert g(fake, None, p, 10, 1.0, 0.75, 5, p, p, None, p, p, 2048, inf, 50.0, None) == V
    assert g(None, fake, p, 10, 1.0, 0.75, 5, p, p, None, p, p, 2048, inf, 50.0, None) == V
    c = lib.wf_ldpc_count
    assert c(fake, None, p, p, p, p, 10, p, None) == V
    assert c(None, fake, p, p, p, p, 10, p, None) == V


def test_idd_python_argument_validation_without_a_gpu():
    """The Python wrappers' own checks come before any device call."""
    from waveforms_amd import device as dev

    class _T:                                                        # the few tensor attributes the wrappers look at
        def __init__(self, n, contiguous=True):
            self._n, self._c = n, contiguous

        def numel(self):
            return self._n

        def is_contiguous(self):
            return self._c

    code = ldpc.demo_code()
    with pytest.raises(ValueError):
        dev.ldpc_decode_ext(code, _T(code.n_tx + 1), None, None)
    with pytest.raises(ValueError):
        dev.ldpc_decode_ext(code, _T(0), None, None)
    with pytest.raises(ValueError):
        dev.ldpc_decode_ext(code, _T(code.n_tx, False), None, None)
    from waveforms_amd.encoding.coded import IterativeSOQPSKLink

    for kw in ({"outer": 0}, {"inner": 0}, {"damping": 0.0}, {"damping": float("nan")}, {"ext_sat": float("inf")}, {"ext_clip": 0.0},
               {"detector": "XX"}):
        with pytest.raises(ValueError):
            IterativeSOQPSKLink(code, 4, **kw)


def test_idd_kernels_resources():
    """No spills, no scratch, nothing spilled in a loop; the occupancy the design needs: 4 waves per SIMD (at most 128
    VGPRs) for both.  The detector's geometry cuts a burst for 2^18 lanes = 4 waves on each of the 1024 SIMDs
    (wf_viterbi_soft.h: kSoftLanes); the decoder's workgroups of 4 waves are LDS-bound at 3 per CU for the demo code
    (48 KiB each) and 4 per CU is what tests/test_ldpc.py asks of the existing decoder."""
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
    import kernel_resources as kr
    from waveforms_amd.csrc.build import build

    so = build(verbose=False)
    table = kr.kernel_table(so)
    tab = {k: v for k, v in table.items() if k.startswith(("soft_ap_", "idd_"))}
    want = {f"soft_ap_bounds_kernel<{p}, {d}>" for p in ("true", "false") for d in (0, 1)}
    want |= {f"soft_ap_llr_kernel<{p}, {d}>" for p in ("true", "false") for d in (0, 1)}
    want |= {f"soft_ap_fixup_kernel<{p}, {b}, {d}>" for p in ("true", "false") for b in ("true", "false") for d in (0, 1)}
    want |= {"idd_decode_kernel<true>", "idd_decode_kernel<false>", "idd_count_kernel"}
    assert set(tab) == want, sorted(set(tab) ^ want)
    asm = {**kr.loop_spill_counts(so, "soft_ap_"), **kr.loop_spill_counts(so, "idd_")}
    for name, row in tab.items():
        assert row["vgpr_spill_count"] == 0 and row["sgpr_spill_count"] == 0 and row["private_segment_fixed_size"] == 0, (name, row)
        a = asm[name]
        assert a["scratch_load_in_loop"] == 0 and a["scratch_store_in_loop"] == 0, (name, a)
        assert a["v_readlane_in_loop"] == 0 and a["v_writelane_in_loop"] == 0, (name, a)
        waves = kr.waves_per_simd(row["vgpr_count"], row.get("agpr_count", 0))
        assert waves >= 4, (name, row["vgpr_count"], waves)
    # the decoder's own static LDS on top of the dynamic L + check state stays small (the geometry leaves 1 KiB for it)
    for name in ("idd_decode_kernel<true>", "idd_decode_kernel<false>"):
        assert tab[name]["group_segment_fixed_size"] <= 1024, tab[name]


def _cpu_bursts(oracle, code, ncw, ebn0, detector, seed):
    """ncw bursts of one demo codeword each through the oracle's chain -> (information bits, rows ncw x N x 3)."""
    rng = np.random.default_rng(seed)
    u = rng.integers(0, 2, (ncw, code.k), dtype=np.uint8)
    tx = code.encode_host(u)
    sigma = oracle.sigma_for_ebn0(ebn0 + 10 * np.log10(code.k / code.n_tx), SPS)
    g = oracle.freq_pulse_soqpsk_tg(SPS)
    rows = []
    for b in range(ncw):
        bits = np.concatenate([tx[b], np.zeros(PAD, np.uint8)])
        res = oracle.detection_run(bits, g, 0.25, SPS, sigma, rng=rng, detector=detector, timing_offset=-1 if detector == "PT" else 0)
        rows.append(np.asarray(res["mf_rows"])[:code.n_tx + 8])
    return u, np.array(rows)


def _siso_batch(oracle, rows, prior, scale):
    """apriori_restatement vectorised over bursts of equal length (same float64 operations per burst, section by section)."""
    brs = TS._branches(oracle, True)
    B, N, _ = rows.shape
    inc = np.stack([TS._increments(oracle, r, True) for r in rows])
    pi = np.float64(scale) * prior.astype(np.float64)
    A = np.zeros((N + 1, B, 4))
    a = np.zeros((B, 4))
    for k in range(N):
        new = np.full((B, 4), np.inf)
        for (b, s, e, i, _x) in brs[k & 1]:
            new[:, e] = np.minimum(new[:, e], a[:, s] + ((inc[:, k, b] + pi[:, k]) if i else inc[:, k, b]))
        a = new - new.min(1, keepdims=True)
        A[k + 1] = a
    ext = np.empty((B, N))
    bt = np.zeros((B, 4))
    for k in range(N - 1, -1, -1):
        a, new = A[k], np.full((B, 4), np.inf)
        m = [np.full(B, np.inf), np.full(B, np.inf)]
        for (b, s, e, i, _x) in brs[k & 1]:
            m[i] = np.minimum(m[i], (a[:, s] + inc[:, k, b]) + bt[:, e])
            new[:, s] = np.minimum(new[:, s], ((inc[:, k, b] + pi[:, k]) if i else inc[:, k, b]) + bt[:, e])
        ext[:, k] = m[1] - m[0]
        bt = new - new.min(1, keepdims=True)
    return ext


def test_siso_batch_is_the_restatement(oracle):
    code = ldpc.demo_code()
    _u, rows = _cpu_bursts(oracle, code, 2, 4.5, "PT", 5)
    rows = rows[:, :300]
    prior = (8.0 * np.random.default_rng(1).standard_normal((2, 300))).astype(np.float32)
    got = _siso_batch(oracle, rows, prior, 0.7)
    for b in range(2):
        want, _ = apriori_restatement(oracle, rows[b], prior[b], 0.7, True)
        assert np.array_equal(got[b].view(np.uint64), want.view(np.uint64))


def test_iterative_gain_on_the_cpu(oracle):
    """The algorithm's gain from the restatements alone: PT, information Eb/N0 4.5 dB, 40 demo codewords, one per burst."""
    code = ldpc.demo_code()
    ncw, outer, inner, damping, sat = 40, 8, 5, 0.7, 6.25 * SPS
    u, rows = _cpu_bursts(oracle, code, ncw, 4.5, "PT", 2)
    N = rows.shape[1]
    lam = _siso_batch(oracle, rows, np.zeros((ncw, N), dtype=np.float32), damping)[:, 1:1 + code.n_tx]
    one_info, _post, one_it = TL.decode_restatement(code, lam, 1.0, 0.75, 50)
    one_fe = int(np.any(one_info != u, axis=1).sum())

    prior = np.zeros((ncw, N), dtype=np.float32)
    state = np.zeros(ncw, dtype=np.uint8)
    iters = np.zeros(ncw, dtype=np.int32)
    info = np.zeros((ncw, code.k), dtype=np.uint8)
    per_pass = []
    for _o in range(outer):
        ext = _siso_batch(oracle, rows, prior, damping)
        decode_ext_restatement(code, ext[:, 1:1 + code.n_tx], state, prior[:, 1:1 + code.n_tx], info, iters, 1.0, 0.75, inner, np.inf, sat)
        per_pass.append(int(np.any(info != u, axis=1).sum()))
    idd_fe = per_pass[-1]
    print(f"one pass: {one_fe} of {ncw} frame errors, mean iterations {one_it.mean():.2f}; iterative: per pass {per_pass}, "
          f"mean inner iterations {iters.mean():.2f}, open {int((state == 0).sum())}")
    assert one_fe >= 4                                       # (otherwise the condition below says nothing)
    assert 4 * idd_fe <= one_fe
    assert iters.sum() < one_it.sum()


# ------------------------------------------------------------------------------------------------ GPU
def _counters(dev, ctx):
    return dev.viterbi_unmerged(reset=True, ctx=ctx), dev.viterbi_repaired(reset=True, ctx=ctx)


@pytest.fixture
def soft_ctx():
    from waveforms_amd import _hip

    ctx = _hip.new_ctx()
    yield ctx
    _hip.free_ctx(ctx)


def _priors(rng, n, sat=50.0):
    """name -> float32 prior per row: zero, normal at the scale of λ, ±sat patterns, a mixture."""
    normal = (11.0 * rng.standard_normal(n)).astype(np.float32)
    sats = np.where(rng.integers(0, 2, n) == 1, np.float32(-sat), np.float32(sat)).astype(np.float32)
    mixed = np.where(rng.integers(0, 3, n) == 0, sats, normal).astype(np.float32)
    mixed[rng.integers(0, 4, n) == 0] = 0.0
    return {"zero": np.zeros(n, dtype=np.float32), "normal": normal, "sat": sats, "mixed": mixed}


@pytest.mark.gpu
@pytest.mark.parametrize("detector", ["PT", "PAM"])
@pytest.mark.parametrize("ebn0", [0.0, 4.0, 10.0])
def test_apriori_bitwise_equals_the_definition(oracle, soft_ctx, detector, ebn0):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    d_rows, rb, _tx, _counts = TS._link_rows(6000, detector, ebn0)                    # the links' packed rows
    assert rb == 32
    rows = _hip.to_host(d_rows).reshape(-1, 4)
    rows48 = _hip.to_host(TS._unpack_rows(_hip.to_device(rows))).reshape(-1, 3, 2)
    z = rows48[..., 0] + 1j * rows48[..., 1]
    n = z.shape[0]
    rng = np.random.default_rng(int(ebn0) + 3)
    _hip.set_option(soft_ctx, _hip.WF_OPT_DET_FINAL_VERIFY, 1)
    d32, d48 = _hip.to_device(rows), _hip.to_device(z)
    plain_llr, plain_bits = dev.viterbi_soft(d32, True, 0, 32, ctx=soft_ctx)
    for name, prior in _priors(rng, n).items():
        want_ext, want_bits = apriori_restatement(oracle, z, prior, 0.7, True)
        dp = _hip.to_device(prior)
        _counters(dev, soft_ctx)
        for rb, d_rows in ((32, d32), (48, d48)):
            for warmup in (0, 3):
                ext, bits = dev.viterbi_soft_apriori(d_rows, dp, 0.7, True, warmup, rb, ctx=soft_ctx)
                assert np.array_equal(_hip.to_host(ext).view(np.uint64), want_ext.view(np.uint64)), (name, rb, warmup)
                assert np.array_equal(_hip.to_host(bits), want_bits), (name, rb, warmup)
                assert _counters(dev, soft_ctx)[0] == 0
        if name == "zero":
            assert np.array_equal(want_ext.view(np.uint64), _hip.to_host(plain_llr).view(np.uint64))
    ext, bits = dev.viterbi_soft_apriori(d32, None, 0.7, True, 0, 32, ctx=soft_ctx)
    assert _hip.torch().equal(ext.view(_hip.torch().int64), plain_llr.view(_hip.torch().int64)) and _hip.torch().equal(bits, plain_bits)


@pytest.mark.gpu
@pytest.mark.parametrize("differential", [True, False])
def test_apriori_any_chunking_and_short_bursts(oracle, soft_ctx, differential):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    rng = np.random.default_rng(23 + differential)
    for n in (1, 2, 5, 31, 700, 9000):
        rows = rng.standard_normal((n, 3)) + 1j * rng.standard_normal((n, 3))
        prior = _priors(rng, n, sat=12.0)["mixed"]
        want_ext, want_bits = apriori_restatement(oracle, rows, prior, 1.3, differential)
        dp = _hip.to_device(prior)
        for chunk in (0, 1, 2, 3, 7, 64, 1000, 8192):
            _hip.set_option(soft_ctx, _hip.WF_OPT_SOFT_CHUNK_CALLS, chunk)
            for warmup in (0, 1, 5):
                ext, bits = dev.viterbi_soft_apriori(_hip.to_device(rows), dp, 1.3, differential, warmup, 48, ctx=soft_ctx)
                assert np.array_equal(_hip.to_host(ext).view(np.uint64), want_ext.view(np.uint64)), (n, chunk, warmup)
                assert np.array_equal(_hip.to_host(bits), want_bits)
                ext, _ = dev.viterbi_soft_apriori(_hip.to_device(TS.pack_rows(rows)), dp, 1.3, differential, warmup, 32, ctx=soft_ctx)
                assert np.array_equal(_hip.to_host(ext).view(np.uint64), want_ext.view(np.uint64)), (n, chunk, warmup, "packed")
                _counters(dev, soft_ctx)


@pytest.mark.gpu
def test_apriori_proof_is_real(oracle, soft_ctx):
    """With a 2-row warm-up chunks miss their start / end: the repairs run (and give the definition); with the repairs
    off the same launch counts unproven chunks."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    rng = np.random.default_rng(29)
    n = 20000
    rows = 0.3 * (rng.standard_normal((n, 3)) + 1j * rng.standard_normal((n, 3)))
    prior = (0.5 * rng.standard_normal(n)).astype(np.float32)
    want_ext, _ = apriori_restatement(oracle, rows, prior, 1.0, True)
    _hip.set_option(soft_ctx, _hip.WF_OPT_SOFT_CHUNK_CALLS, 16)
    _counters(dev, soft_ctx)
    ext, _ = dev.viterbi_soft_apriori(_hip.to_device(rows), _hip.to_device(prior), 1.0, True, 2, 48, ctx=soft_ctx)
    assert np.array_equal(_hip.to_host(ext).view(np.uint64), want_ext.view(np.uint64))
    unproven, repaired = _counters(dev, soft_ctx)
    assert unproven == 0 and repaired > 0
    _hip.set_option(soft_ctx, _hip.WF_OPT_DET_REPAIR, 1)
    dev.viterbi_soft_apriori(_hip.to_device(rows), _hip.to_device(prior), 1.0, True, 2, 48, ctx=soft_ctx)
    unproven, repaired = _counters(dev, soft_ctx)
    assert unproven > 0 and repaired == 0


def _check_decode_ext(code, llr, rng, scale=1.0, max_iter=5, clip=np.inf, sat=50.0, stride=None):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    ncw = llr.shape[0]
    stride = code.n_tx if stride is None else stride
    state = (rng.integers(0, 3, ncw) == 0).astype(np.uint8)         # a third frozen on entry
    ext = rng.standard_normal((ncw, stride)).astype(np.float32)
    info = rng.integers(0, 2, (ncw, code.k), dtype=np.uint8)
    iters = rng.integers(0, 100, ncw).astype(np.int32)
    post = rng.standard_normal((ncw, code.n)).astype(np.float32)
    d = {k: _hip.to_device(v) for k, v in (("state", state), ("ext", ext), ("info", info), ("iters", iters), ("post", post))}
    for _pass in range(2):                                           # the second pass meets the states the first one left
        dev.ldpc_decode_ext(code, _hip.to_device(np.ascontiguousarray(llr)), d["state"], d["ext"], stride, scale=scale, max_iter=max_iter,
                            ext_clip=clip, ext_sat=sat, info_bits=d["info"], iters=d["iters"], post=d["post"])
        view = ext[:, :code.n_tx]
        decode_ext_restatement(code, llr, state, view, info, iters, scale, 0.75, max_iter, clip, sat, post)
        _hip.device_check()
        assert np.array_equal(_hip.to_host(d["state"]), state), code.n
        assert np.array_equal(_hip.to_host(d["iters"]), iters)
        assert np.array_equal(_hip.to_host(d["info"]), info)
        assert np.array_equal(_hip.to_host(d["ext"]).view(np.uint32), ext.view(np.uint32))         # (the stride's gaps included)
        assert np.array_equal(_hip.to_host(d["post"]).view(np.uint32), post.view(np.uint32))
    return state


@pytest.mark.gpu
@pytest.mark.parametrize("max_iter", [1, 5])
def test_gpu_decode_ext_small_and_demo_codes(max_iter):
    rng = np.random.default_rng(51 + max_iter)
    demo = ldpc.demo_code()
    for code in [demo] + TL.random_codes():
        for ncw in (1, 7, 203):
            u, llr = _noisy(code, rng, ncw, 0.9)
            llr[0] = 4.0 * (1.0 - 2.0 * code.encode_host(u[:1])[0])
            state = _check_decode_ext(code, llr, rng, scale=0.5, max_iter=max_iter, clip=2.0, sat=30.0, stride=code.n_tx + (ncw % 3))
        assert 0 < state.sum()
        garbage = rng.normal(0, 3.0, (9, code.n_tx))
        _check_decode_ext(code, garbage, rng, max_iter=max_iter)


@pytest.mark.gpu
def test_gpu_decode_ext_large_code_scratch_form():
    from waveforms_amd import device as dev

    code = ldpc.demo_code(1024)
    assert dev.ldpc_decode_geometry(code, 300)["state_in_scratch"] == 1
    rng = np.random.default_rng(61)
    _u, llr = _noisy(code, rng, 300, 0.95)
    _check_decode_ext(code, llr, rng, max_iter=6)


@pytest.mark.gpu
def test_gpu_ldpc_count():
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    code = ldpc.demo_code()
    rng = np.random.default_rng(71)
    ncw = 333
    ref = rng.integers(0, 2, (ncw, code.k), dtype=np.uint8)
    info = ref.copy()
    flip = rng.random((ncw, code.k)) < 0.01
    flip[rng.integers(0, 2, ncw) == 0] = False
    info ^= flip.astype(np.uint8)
    state = rng.integers(0, 2, ncw).astype(np.uint8)
    iters = rng.integers(0, 41, ncw).astype(np.int32)
    counts = dev.ldpc_count(code, _hip.to_device(info), _hip.to_device(ref), _hip.to_device(state), _hip.to_device(iters))
    counts = dev.ldpc_count(code, _hip.to_device(info), _hip.to_device(ref), _hip.to_device(state), _hip.to_device(iters), counts)
    e = flip.sum(axis=1)
    assert _hip.to_host(counts).tolist() == [2 * int(e.sum()), 2 * int((e > 0).sum()), 2 * int((state == 0).sum()), 2 * int(iters.sum())]


@pytest.mark.gpu
def test_gpu_loop_pass_by_pass(oracle):
    """A burst of 8 demo codewords at 4.5 dB, 4 outer passes: the prior buffer, the states, the information bits and the
    iterations after every pass equal the host chain made of the two restatements, fed the GPU's rows."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.encoding.coded import IterativeSOQPSKLink

    code = ldpc.demo_code()
    link = IterativeSOQPSKLink(code, 8, detector="PT", outer=4, inner=5)
    info = link.info_bits(0)
    rows, _ = link.front_end(dev.ldpc_encode(code, info), 4.5, 7, 0)
    h = _hip.to_host(rows).reshape(-1, 3, 2)
    z = h[..., 0] + 1j * h[..., 1]
    n = z.shape[0]
    # the host chain sees every row of the burst; only the first 1 + nbits carry a prior
    snaps = []
    prior = np.zeros(n, dtype=np.float32)
    state, iters, dec = np.zeros(8, dtype=np.uint8), np.zeros(8, dtype=np.int32), np.zeros((8, code.k), dtype=np.uint8)
    link.begin(n)
    for o in range(4):
        ext, _ = link.detect(rows, first=o == 0)
        link.decode(ext)
        want_ext, _ = apriori_restatement(oracle, z, prior, link.damping, True)
        assert np.array_equal(_hip.to_host(ext).reshape(-1).view(np.uint64), want_ext[1:1 + link.nbits].view(np.uint64)), o
        decode_ext_restatement(code, want_ext[1:1 + link.nbits].reshape(8, code.n_tx), state, prior[1:1 + link.nbits].reshape(8, code.n_tx),
                               dec, iters, 1.0, link.alpha, 5, link.ext_clip, link.ext_sat)
        snaps.append(int(state.sum()))
        assert np.array_equal(_hip.to_host(link.prior).view(np.uint32), prior.view(np.uint32)), o
        assert np.array_equal(_hip.to_host(link.state), state) and np.array_equal(_hip.to_host(link.iters), iters), o
        assert np.array_equal(_hip.to_host(link.decided), dec), o
    _hip.device_check()
    assert prior[0] == 0 and (prior[1 + link.nbits:] == 0).all()
    print("frozen after each pass:", snaps)
    assert snaps[-1] > snaps[0]                              # the loop does something on this burst


@pytest.mark.gpu
@pytest.mark.parametrize("detector", ["PT", "PAM"])
def test_gpu_outer_1_is_the_one_pass_link_and_noiseless_freezes_at_once(detector):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.encoding.coded import CodedSOQPSKLink, IterativeSOQPSKLink

    code = ldpc.demo_code()
    it = IterativeSOQPSKLink(code, 61, detector=detector, outer=1, inner=5)
    one = CodedSOQPSKLink(code, 61, detector=detector, max_iter=5)
    it.run_block(4.5, seed=5, stream_id=2)
    llr, _info = one.channel_llrs(4.5, seed=5, stream_id=2)
    want = dev.ldpc_decode(code, llr, alpha=one.alpha, max_iter=5)
    assert _hip.torch().equal(it.decided, want["info_bits"]) and _hip.torch().equal(it.iters, want["iters"])
    one.run_block(4.5, seed=5, stream_id=2)
    a, b = it.result(), one.result()
    assert a[:2] == b[:2] and a[3:] == b[3:] and it.uncoded_result() == one.uncoded_result()
    assert a[2] >= b[2]                                      # (open after 5 iterations includes "converged exactly at the 5th": none)

    quiet = IterativeSOQPSKLink(code, 37, detector=detector, outer=3, inner=5, per_pass=True)
    quiet.run_block(None, seed=1, stream_id=0)
    quiet.run_block(None, seed=1, stream_id=1)
    assert quiet.result() == (0, 0, 0, 2 * 37 * code.k, 0.0)
    assert quiet.pass_results() == [(0, 0, 0, 0.0)] * 3
    assert int(quiet.state.sum()) == 37 and quiet.uncoded_result() == (0, 2 * 37 * code.n_tx)


@pytest.mark.gpu
def test_gpu_iterative_gain_on_a_full_block():
    """One 1e7-channel-bit block (4 882 demo codewords in ONE burst) at 4.5 dB: the CPU test's condition against
    CodedSOQPSKLink (50 iterations) on the same seed.  Measured on one MI355X: one pass 4 596 of 4 882 frame errors at 48.60
    mean iterations; iterative 6 frame errors (3 295, 565, 94, 30, 14, 10, 6 after passes 2 ... 8) at 11.84."""
    from waveforms_amd.encoding.coded import CodedSOQPSKLink, IterativeSOQPSKLink

    code = ldpc.demo_code()
    ncw = int(1e7) // code.n_tx
    assert ncw == 4882
    one = CodedSOQPSKLink(code, ncw, detector="PT", max_iter=50)
    one.run_block(4.5, seed=9, stream_id=0)
    _be1, fe1, _nc1, _m1, it1 = one.result()
    idd = IterativeSOQPSKLink(code, ncw, detector="PT", outer=8, inner=5, damping=0.7, per_pass=True)
    idd.run_block(4.5, seed=9, stream_id=0)
    _be, fe, nc, _m, its = idd.result()
    print(f"one pass: {fe1} of {ncw} frame errors, mean iterations {it1:.2f}; iterative: {fe} frame errors, {nc} open, "
          f"mean inner iterations {its:.2f}; per pass {idd.pass_results()}")
    assert fe1 >= 4
    assert 4 * fe <= fe1
    assert its < it1
