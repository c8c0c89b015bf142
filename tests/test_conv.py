"""Convolutional codes: wf_conv_code_create / wf_conv_encode / wf_conv_siso (include/wfhip.h) and ConvCode
(waveforms_amd/encoding/conv.py).

The decoder's definition is restated here in numpy float32, one step at a time and in the header's order
(``siso_restatement``), and pinned to brute force over all 2^k codewords with integer-valued inputs, where every sum is exact.
On the GPU the kernels must equal the restatement BITWISE.

The loop's gain is checked on the CPU from the restatements alone (tests/test_idd.py's SOQPSK detector restatement and this
file's decoder): (7, 5), k = 1022, QPP interleaver, PT, information Eb/N0 4.0 dB, 24 bursts of one codeword, 8 passes at
damping 0.7 and clip 50.  Frame errors per pass on this seed: 24, 21, 7, 0, 0, 0, 0, 0.
"""
import ctypes
import itertools

import numpy as np
import pytest

import test_idd as TI
from waveforms_amd.encoding import conv

# constraint length -> generators for n_out = 2, 3, 4 (every one with both end taps)
GENS = {3: (0o7, 0o5, 0o7, 0o5), 4: (0o17, 0o15, 0o13, 0o17), 5: (0o23, 0o35, 0o25, 0o37), 6: (0o53, 0o75, 0o47, 0o77),
        7: (0o171, 0o133, 0o165, 0o117)}
PUNCTURE = {2: [[1, 1, 0], [1, 0, 1]], 3: [[1, 1], [1, 0], [0, 1]], 4: [[1, 0], [1, 1], [0, 1], [1, 1]]}


def make_code(K, n_out, k, punct=False, seed=0):
    """A code of the grid; ``punct``: punctured AND transmitted in a random order."""
    if not punct:
        return conv.ConvCode(GENS[K][:n_out], k, K)
    plain = conv.ConvCode(GENS[K][:n_out], k, K, puncture=PUNCTURE[n_out])
    order = np.random.default_rng(seed).permutation(plain.n_tx)
    return conv.ConvCode(GENS[K][:n_out], k, K, puncture=PUNCTURE[n_out], tx_order=order)


# ------------------------------------------------------------------------------------------------ restatement
def _trellis(code):
    """next[u][s], and bits[u][s, j] = c_j of branch (s, u): reg = (u << nu) | s, c_j = parity(reg & g_j), s' = reg >> 1."""
    nu = code.K - 1
    s = np.arange(1 << nu)
    nxt, bits = [], []
    for u in (0, 1):
        reg = (u << nu) | s
        nxt.append(reg >> 1)
        bits.append(np.array([[bin(int(r) & g).count("1") & 1 for g in code.generators] for r in reg], dtype=bool))
    return nxt, bits


def siso_restatement(code, llr, prior=None, scale=1.0, ext_clip=np.inf):
    """The header's definition of wf_conv_siso, one step at a time in float32, vectorised over the codewords ->
    (info bits u8 B x k, Λ float32 B x k, ext float32 B x n_tx, P float32 B x n)."""
    llr = np.atleast_2d(np.asarray(llr, dtype=np.float64))
    B, k, T, n_out, nu = llr.shape[0], code.k, code.T, code.n_out, code.K - 1
    S = 1 << nu
    nxt, bits = _trellis(code)
    L = np.zeros((B, code.n), dtype=np.float32)
    L[:, code.tx_var] = (np.float64(scale) * llr).astype(np.float32)
    A = np.zeros((B, k), dtype=np.float32) if prior is None else np.asarray(prior, dtype=np.float32).reshape(B, k)
    ninf = np.float32(-np.inf)

    def gamma(i, u):
        g = np.repeat((-A[:, i])[:, None], S, axis=1) if u else np.zeros((B, S), dtype=np.float32)      # (u ? -A_i : +0)
        for j in range(n_out):
            g = np.where(bits[u][:, j][None, :], g - L[:, n_out * i + j][:, None], g)
        assert g.dtype == np.float32
        return g

    alpha = [None] * (T + 1)
    a = np.full((B, S), ninf, dtype=np.float32)
    a[:, 0] = 0.0
    alpha[0] = a
    for i in range(T):
        new = np.full((B, S), ninf, dtype=np.float32)
        for u in ((0, 1) if i < k else (0,)):
            cand = a + gamma(i, u)                                    # by source state; s and s ^ 1 enter the same s'
            new[:, u * (S // 2):(u + 1) * (S // 2)] = cand.reshape(B, S // 2, 2).max(axis=2)
        a = new
        alpha[i + 1] = a
    lam = np.zeros((B, k), dtype=np.float32)
    P = np.zeros((B, code.n), dtype=np.float32)
    b = np.full((B, S), ninf, dtype=np.float32)
    b[:, 0] = 0.0
    cb = [np.concatenate([bits[0][:, j], bits[1][:, j]]) for j in range(n_out)]
    for i in range(T - 1, -1, -1):
        V, W = [], []
        for u in (0, 1):
            if u and i >= k:
                V.append(np.full((B, S), ninf, dtype=np.float32))
                W.append(np.full((B, S), ninf, dtype=np.float32))
                continue
            g = gamma(i, u)
            V.append((alpha[i] + g) + b[:, nxt[u]])
            W.append(g + b[:, nxt[u]])
        if i < k:
            lam[:, i] = V[0].max(axis=1) - V[1].max(axis=1)
        VV = np.concatenate(V, axis=1)
        for j in range(n_out):
            P[:, n_out * i + j] = np.where(~cb[j][None, :], VV, ninf).max(axis=1) - np.where(cb[j][None, :], VV, ninf).max(axis=1)
        b = np.maximum(W[0], W[1])
    clip = np.float32(ext_clip)
    ext = np.minimum(np.maximum(P[:, code.tx_var] - L[:, code.tx_var], -clip), clip).astype(np.float32)
    assert lam.dtype == P.dtype == ext.dtype == np.float32
    return (lam < 0).astype(np.uint8), lam, ext, P


def siso_brute_force(code, L, A):
    """Over all 2^k codewords with the metric -Σ c L - Σ u A (float64): max with bit = 0 minus max with bit = 1 -> (Λ k, P n).
    ``L`` by variable (0 where punctured)."""
    msgs = np.array(list(itertools.product((0, 1), repeat=code.k)), dtype=np.uint8)
    cws = code.codeword_host(msgs).astype(np.float64)
    metric = -(cws @ np.asarray(L, dtype=np.float64)) - (msgs.astype(np.float64) @ np.asarray(A, dtype=np.float64))

    def split(bit):
        return np.array([metric[bit[:, i] == 0].max() - metric[bit[:, i] == 1].max() for i in range(bit.shape[1])])

    return split(msgs), split(cws.astype(np.uint8))


def _integer_case(code, rng):
    """Integer-valued λ in [-9, 9] with a quarter of them 0, integer prior: every sum is exact."""
    llr = rng.integers(-9, 10, code.n_tx).astype(np.float64)
    llr[rng.integers(0, 4, code.n_tx) == 0] = 0.0
    return llr, rng.integers(-6, 7, code.k).astype(np.float32)


def _check_against_brute_force(code, rng, siso):
    llr, A = _integer_case(code, rng)
    L = np.zeros(code.n)
    L[code.tx_var] = llr
    want_lam, want_P = siso_brute_force(code, L, A)
    bits, lam, ext, P = siso(code, llr[None, :], A[None, :])
    assert np.isfinite(lam).all() and np.isfinite(ext).all()
    assert np.array_equal(lam[0].astype(np.float64), want_lam), (code.generators, lam[0], want_lam)
    assert np.array_equal(bits[0], (want_lam < 0).astype(np.uint8))
    assert np.array_equal(ext[0].astype(np.float64), (want_P - L)[code.tx_var])
    if P is not None:
        assert np.isfinite(P).all() and np.array_equal(P[0].astype(np.float64), want_P)


# ------------------------------------------------------------------------------------------------ CPU
def test_encoder_facts():
    c = conv.nasa_k3(4)
    assert (c.k, c.K, c.T, c.n, c.n_tx, c.rate) == (4, 3, 6, 12, 12, 4 / 12)
    assert c.encode_host([[1, 0, 1, 1]])[0].tolist() == [1, 1, 1, 0, 0, 0, 0, 1, 0, 1, 1, 1]
    # the impulse response is the generators' bits, MSB first
    c = conv.ccsds_k7(5)
    out = c.codeword_host([[1, 0, 0, 0, 0]])[0].reshape(c.T, 2)
    for j, g in enumerate((0o171, 0o133)):
        assert out[:7, j].tolist() == [(g >> (6 - d)) & 1 for d in range(7)] and not out[7:, j].any()
    assert conv.ConvCode((0o171, 0o133), 5).K == 7                    # K from the widest generator


@pytest.mark.parametrize("preset, k, dfree", [(conv.nasa_k3, 12, 5), (conv.ccsds_k7, 11, 10)])
def test_free_distance(preset, k, dfree):
    code = preset(k)
    msgs = np.array(list(itertools.product((0, 1), repeat=k)), dtype=np.uint8)[1:]
    assert int(code.codeword_host(msgs).sum(axis=1).min()) == dfree


@pytest.mark.parametrize("gens", [(0o7, 0o5), (0o23, 0o35), (0o171, 0o133), (0o133, 0o171, 0o165)])
def test_restatement_equals_brute_force(gens):
    rng = np.random.default_rng(sum(gens))
    for _ in range(4):
        _check_against_brute_force(conv.ConvCode(gens, 7), rng, siso_restatement)


def test_restatement_equals_brute_force_punctured_and_permuted():
    rng = np.random.default_rng(3)
    for K, n_out in ((3, 2), (5, 3), (7, 2), (4, 4)):
        code = make_code(K, n_out, 7, punct=True, seed=K)
        assert code.n_tx < code.n and not np.array_equal(code.tx_var, np.sort(code.tx_var))
        _check_against_brute_force(code, rng, siso_restatement)


def test_restatement_properties():
    code = make_code(5, 2, 40, punct=True)
    rng = np.random.default_rng(9)
    llr = rng.normal(0, 4.0, (3, code.n_tx))
    A = rng.normal(0, 2.0, (3, code.k)).astype(np.float32)
    bits, lam, ext, _P = siso_restatement(code, llr, A, 0.5, 1.5)
    assert np.abs(ext).max() == 1.5 and np.isfinite(lam).all()
    # no prior is a zero prior (of either sign), bit for bit
    ref = siso_restatement(code, llr)
    for zero in (np.zeros_like(A), -np.zeros_like(A)):
        got = siso_restatement(code, llr, zero)
        assert all(np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes() for x, y in zip(got, ref))
    # all-zero input: every Λ and every ext is 0, every bit 0
    bits, lam, ext, _P = siso_restatement(code, np.zeros((2, code.n_tx)))
    assert not bits.any() and not lam.any() and not ext.any()
    # a clean codeword decodes to its message
    u = rng.integers(0, 2, (4, code.k), dtype=np.uint8)
    bits, _lam, ext, _P = siso_restatement(code, 4.0 * (1.0 - 2.0 * code.encode_host(u)))
    assert np.array_equal(bits, u)


def test_c_create_refuses_invalid_codes_without_a_gpu():
    """Every kind of invalid code: WF_ERR_VALUE before the context or device memory is touched (a fake context)."""
    from waveforms_amd import _hip

    lib = _hip.lib()
    fake = ctypes.create_string_buffer(1 << 16)
    V = _hip.WF_ERR_VALUE
    t = make_code(5, 3, 20, punct=True).c_tables()

    def create(**over):
        a = dict(t, **over)
        out = ctypes.c_void_p()
        gen = np.ascontiguousarray(a["gen"], dtype=np.uint32)
        tx = np.ascontiguousarray(a["tx_var"], dtype=np.int32)
        return lib.wf_conv_code_create(fake, a["K"], a["n_out"], gen.ctypes.data, a["k"], a["n_tx"], tx.ctypes.data, ctypes.byref(out)), out.value

    g = [int(v) for v in t["gen"]]
    bad = [dict(K=2, gen=[3, 3, 3]), dict(K=8, gen=[0o371, 0o233, 0o365]), dict(n_out=1), dict(n_out=5, gen=g + g),
           dict(gen=[g[0] & ~1, g[1], g[2]]), dict(gen=[g[0], g[1] & 0o17, g[2]]), dict(gen=[g[0], g[1], g[2] | 0o40]),
           dict(k=0), dict(k=32768 // 3), dict(n_tx=0), dict(n_tx=3 * 24 + 1)]
    tx = t["tx_var"].copy()
    tx[1] = tx[0]
    bad.append(dict(tx_var=tx))
    tx = t["tx_var"].copy()
    tx[2] = 3 * 24
    bad.append(dict(tx_var=tx))
    tx = t["tx_var"].copy()
    tx[0] = -1
    bad.append(dict(tx_var=tx))
    for over in bad:
        rc, h = create(**over)
        assert rc == V and h is None, over
    assert lib.wf_conv_code_create(None, 3, 2, None, 4, 12, None, None) == V
    assert lib.wf_conv_code_free(None) == 0
    geom = (ctypes.c_int64 * 5)()
    assert lib.wf_conv_siso_geometry(fake, None, 10, geom) == V
    assert lib.wf_conv_encode(fake, None, None, 10, None, None) == V
    assert lib.wf_conv_siso(fake, None, None, 10, 1.0, None, None, None, None, 0, 1.0, None, None, None) == V


def test_python_validation():
    with pytest.raises(ValueError):
        conv.ConvCode((0o7, 0o5), 10, puncture=[[1, 0], [1, 1], [1, 1]])          # three rows for two outputs
    with pytest.raises(ValueError):
        conv.ConvCode((0o7, 0o5), 10, puncture=[1, 0, 1])
    with pytest.raises(ValueError):
        conv.ConvCode((0o7, 0o5), 10, puncture=[[1, 2], [1, 1]])
    with pytest.raises(ValueError):
        conv.ConvCode((0o7, 0o5), 10, puncture=[[0, 0], [0, 0]])
    with pytest.raises(ValueError):
        conv.ConvCode((0o7, 0o5), 10, tx_order=np.arange(23))
    with pytest.raises(ValueError):
        conv.ConvCode((0o7, 0o5), 10, tx_order=np.zeros(24, dtype=int))
    for gens, K in (((0o7, 0o4), 3), ((0o7, 0o3), 3), ((0o7,), 3), ((0o7, 0o5), 2), ((0o7, 0o5), 8), ((0o7, 0o5, 0o7, 0o5, 0o7), 3)):
        with pytest.raises(ValueError):
            conv.ConvCode(gens, 10, K)
    with pytest.raises(ValueError):
        conv.ConvCode((0o7, 0o5), 0)
    with pytest.raises(ValueError):
        conv.ConvCode((0o7, 0o5), 16383)
    assert conv.ConvCode((0o7, 0o5), 16382).n == 32768
    with pytest.raises(ValueError):
        conv.qpp_order(2048, 32, 64)                                              # an even f1 collides at once
    with pytest.raises(ValueError):
        conv.qpp_order(15, 1, 3)
    q = conv.qpp_order(2048, 31, 64)
    assert np.array_equal(np.sort(q), np.arange(2048)) and q[:3].tolist() == [0, 95, 318]
    code = conv.ConvCode((0o7, 0o5), 5, puncture=[[1, 1, 0], [1, 0, 1]])
    assert code.tx_var.tolist() == [0, 1, 2, 5, 6, 7, 8, 11, 12, 13] and code.rate == 0.5


def test_conv_entry_points_exported_and_bound():
    from waveforms_amd import _hip
    from waveforms_amd import device

    lib = _hip.lib()
    for name in ("wf_conv_code_create", "wf_conv_code_free", "wf_conv_encode", "wf_conv_siso", "wf_conv_siso_geometry"):
        assert name in _hip.SIGNATURES and hasattr(lib, name)
    assert callable(device.conv_encode) and callable(device.conv_siso) and callable(device.conv_siso_geometry)


def test_conv_kernels_resources():
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
    import kernel_resources as kr
    from waveforms_amd.csrc.build import build

    so = build(verbose=False)
    tab = {k: v for k, v in kr.kernel_table(so).items() if k.startswith("conv_")}
    want = {"conv_encode_kernel"} | {f"conv_siso_kernel<{nu}, {n_out}>" for nu in range(2, 7) for n_out in (2, 3, 4)}
    assert set(tab) == want, sorted(set(tab) ^ want)
    asm = kr.loop_spill_counts(so, "conv_")
    for name, row in tab.items():
        assert row["vgpr_spill_count"] == 0 and row["sgpr_spill_count"] == 0 and row["private_segment_fixed_size"] == 0, (name, row)
        a = asm[name]
        assert a["scratch_load_in_loop"] == 0 and a["scratch_store_in_loop"] == 0 and a["v_writelane_in_loop"] == 0, (name, a)
        assert row.get("wavefront_size", 64) == 64
    # one wave per workgroup: 4 waves per SIMD need at most 128 VGPRs; the LDS of the widest form (K = 3, n_out = 4) lets 7 on a CU
    for name in tab:
        if name.startswith("conv_siso"):
            assert kr.waves_per_simd(tab[name]["vgpr_count"], tab[name].get("agpr_count", 0)) >= 4, tab[name]
            assert tab[name]["group_segment_fixed_size"] <= 22 * 1024, tab[name]


def run_loop_restatement(oracle, code, u, rows, passes, damping, clip):
    """The SCCC loop from the two restatements, one codeword per burst -> frame errors after every pass."""
    B, N = rows.shape[0], rows.shape[1]
    prior = np.zeros((B, N), dtype=np.float32)
    per_pass = []
    for _o in range(passes):
        ext = TI._siso_batch(oracle, rows, prior, damping)
        bits, _lam, e, _P = siso_restatement(code, ext[:, 1:1 + code.n_tx], None, 1.0, clip)
        prior[:, 1:1 + code.n_tx] = e
        per_pass.append(int(np.any(bits != u, axis=1).sum()))
    return per_pass


def test_loop_gain_on_the_cpu(oracle):
    """(7, 5), k = 1022, qpp_order(2048, 31, 64), PT, 4.0 dB, 24 bursts, seed 3, 8 passes, clip 50: 24 -> 0."""
    code = conv.nasa_k3(1022, tx_order=conv.qpp_order(2048, 31, 64))
    u, rows = TI._cpu_bursts(oracle, code, 24, 4.0, "PT", 3)
    per_pass = run_loop_restatement(oracle, code, u, rows, 8, 0.7, 50.0)
    print("frame errors per pass:", per_pass)
    assert per_pass[0] >= 4
    assert 4 * per_pass[-1] <= per_pass[0]


# ------------------------------------------------------------------------------------------------ GPU
def _geometry(code, ncw=1):
    from waveforms_amd import device as dev

    return dev.conv_siso_geometry(code, ncw)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [3, 4, 5, 6, 7])
def test_gpu_encoder_is_the_host_encoder(K):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    rng = np.random.default_rng(K)
    for n_out, k, punct in itertools.product((2, 3), (1, 7, 64, 65, 1000), (False, True)):
        code = make_code(K, n_out, k, punct, seed=k)
        G = _geometry(code)["codewords_per_wave"]
        assert G == 64 >> (K - 1)
        for ncw in sorted({1, max(G - 1, 1), G, G + 1, 130}):
            u = rng.integers(0, 2, (ncw, k), dtype=np.uint8)
            got = _hip.to_host(dev.conv_encode(code, _hip.to_device(u)))
            assert np.array_equal(got, code.encode_host(u)), (K, n_out, k, punct, ncw)
    assert np.array_equal(code.encode(u), code.encode_host(u))
    _hip.device_check()


def _check_siso(code, ncw, rng, scale=1.0, clip=np.inf, with_prior=True, stride=None, sigma=4.0):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    llr = rng.normal(0, sigma, (ncw, code.n_tx))
    A = rng.normal(0, 3.0, (ncw, code.k)).astype(np.float32) if with_prior else None
    stride = code.n_tx if stride is None else stride
    ext0 = rng.standard_normal((ncw, stride)).astype(np.float32)
    d_ext = _hip.to_device(ext0)
    out = dev.conv_siso(code, _hip.to_device(llr), scale=scale, prior=None if A is None else _hip.to_device(A), ext=d_ext, ext_stride=stride,
                        ext_clip=clip)
    bits, lam, ext, _P = siso_restatement(code, llr, A, scale, clip)
    _hip.device_check()
    tag = (code.K, code.n_out, code.k, code.n_tx, ncw)
    assert np.array_equal(_hip.to_host(out["info_post"]).view(np.uint32), lam.view(np.uint32)), tag
    assert np.array_equal(_hip.to_host(out["info_bits"]), bits), tag
    want = ext0.copy()
    want[:, :code.n_tx] = ext
    assert np.array_equal(_hip.to_host(d_ext).view(np.uint32), want.view(np.uint32)), tag          # (the stride's gaps included)
    return llr, A, (bits, lam, ext)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [3, 4, 5, 6, 7])
def test_gpu_siso_bitwise_equals_the_restatement(K):
    """Gaussian λ and prior over the encoder's grid: both n_out, every k, every ncw, plain AND punctured + permuted for every
    (k, ncw) with k <= 65; T around the checkpoint spacing, a strided ext, a clip, a scale.  At k = 1000 every ncw runs too, but
    plain and punctured alternate with ncw instead of both running: the restatement of 130 long codewords costs up to half a
    second, and puncturing changes only the var -> src table's contents, which no launch path, segment count or lane
    assignment depends on (those depend on K, n_out, T and ncw, all of which the long code meets in full)."""
    rng = np.random.default_rng(10 + K)
    probe = make_code(K, 2, 8)
    geo = _geometry(probe)
    G, C = geo["codewords_per_wave"], geo["checkpoint_steps"]
    nu = K - 1
    ncws = sorted({1, max(G - 1, 1), G, G + 1, 130})
    for n_out in (2, 3):
        for k, ncw, punct in itertools.product((1, 7, 64, 65), ncws, (False, True)):
            code = make_code(K, n_out, k, punct, seed=ncw)
            _check_siso(code, ncw, rng, scale=0.5 if punct else 1.0, clip=3.0 if ncw % 2 else np.inf, stride=code.n_tx + ncw % 3)
        for idx, ncw in enumerate(ncws):
            _check_siso(make_code(K, n_out, 1000, bool((idx + n_out) % 2), seed=ncw), ncw, rng, scale=1.7, clip=20.0)
        for T in (C - 1, C, C + 1, 2 * C + 3):
            code = make_code(K, n_out, T - nu, T % 2 == 0, seed=T)
            assert code.T == T
            _check_siso(code, G + 1, rng, with_prior=T != C)
    _check_siso(make_code(K, 4, 65, True, seed=4), 2 * G + 1, rng, scale=0.8, clip=6.0)
    _check_siso(make_code(K, 4, 2 * C + 3 - nu), 3, rng)


@pytest.mark.gpu
def test_gpu_siso_null_outputs_null_prior_and_counts():
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    rng = np.random.default_rng(77)
    for code in (make_code(3, 2, 70, True), make_code(7, 3, 41)):
        ncw = 37
        u = rng.integers(0, 2, (ncw, code.k), dtype=np.uint8)
        llr = 2.0 * (1.0 - 2.0 * code.encode_host(u)) + rng.normal(0, 2.0, (ncw, code.n_tx))
        A = rng.normal(0, 1.0, (ncw, code.k)).astype(np.float32)
        bits, lam, ext, _P = siso_restatement(code, llr, A, 1.0, 5.0)
        d_llr, d_A, d_u = _hip.to_device(llr), _hip.to_device(A), _hip.to_device(u)
        counts = None
        for wb, wp, we in itertools.product((False, True), repeat=3):
            out = dev.conv_siso(code, d_llr, prior=d_A, ext_clip=5.0, ref_info=d_u, counts=counts, want_bits=wb, want_post=wp, want_ext=we)
            counts = out["counts"]
            assert (out["info_bits"] is not None) == wb and (out["info_post"] is not None) == wp and (out["ext"] is not None) == we
            if wb:
                assert np.array_equal(_hip.to_host(out["info_bits"]), bits)
            if wp:
                assert np.array_equal(_hip.to_host(out["info_post"]).view(np.uint32), lam.view(np.uint32))
            if we:
                assert np.array_equal(_hip.to_host(out["ext"]).view(np.uint32), ext.view(np.uint32))
        # the counts are ADDED: eight calls, eight times the errors (also with no other output at all)
        e = (bits != u).sum(axis=1)
        assert int(e.sum()) > 0
        assert _hip.to_host(counts).tolist() == [8 * int(e.sum()), 8 * int((e > 0).sum())]
        # a NULL prior is a zero prior
        none = dev.conv_siso(code, d_llr, ext_clip=5.0)
        zero = dev.conv_siso(code, d_llr, prior=_hip.to_device(np.zeros_like(A)), ext_clip=5.0)
        for key in ("info_bits", "info_post", "ext"):
            assert _hip.torch().equal(none[key], zero[key]), key
        got = code.siso(llr, A, ext_clip=5.0)
        assert np.array_equal(got["info_bits"], bits) and np.array_equal(got["ext"].view(np.uint32), ext.view(np.uint32))
    _hip.device_check()


@pytest.mark.gpu
def test_gpu_siso_in_several_launches():
    """More waves than one launch takes (64 per compute unit): the call slices the batch, every slice with its own pointers."""
    from waveforms_amd import _hip

    code = make_code(7, 2, 1)                                         # one codeword per wave, T = 7
    cus = _hip.torch().cuda.get_device_properties(0).multi_processor_count
    ncw = 64 * cus + 5
    rng = np.random.default_rng(8)
    u = rng.integers(0, 2, (ncw, 1), dtype=np.uint8)
    llr, _A, (bits, _lam, _ext) = _check_siso(code, ncw, rng, clip=4.0, stride=code.n_tx + 1)
    from waveforms_amd import device as dev

    out = dev.conv_siso(code, _hip.to_device(llr), ref_info=_hip.to_device(u), want_post=False, want_ext=False)
    plain = siso_restatement(code, llr)[0]
    e = (plain != u).sum(axis=1)
    assert np.array_equal(_hip.to_host(out["info_bits"]), plain)
    assert _hip.to_host(out["counts"]).tolist() == [int(e.sum()), int((e > 0).sum())] and e.sum() > 0
    _hip.device_check()


def _gpu_siso(code, llr, A):
    out = code.siso(llr, A)
    return out["info_bits"], out["info_post"], out["ext"], None


@pytest.mark.gpu
def test_gpu_siso_equals_brute_force():
    rng = np.random.default_rng(5)
    for K, n_out, punct in ((3, 2, False), (5, 2, False), (7, 2, False), (7, 3, False), (4, 3, True), (6, 4, True), (7, 2, True)):
        for _ in range(3):
            _check_against_brute_force(make_code(K, n_out, 6, punct, seed=K), rng, _gpu_siso)


@pytest.mark.gpu
def test_gpu_siso_all_zero_llrs():
    for code in (make_code(3, 2, 100), make_code(7, 2, 100, True), make_code(5, 4, 33)):
        out = code.siso(np.zeros((19, code.n_tx)))
        assert not out["info_bits"].any() and not out["info_post"].any() and not out["ext"].any()
