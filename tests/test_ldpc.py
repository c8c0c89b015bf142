"""LDPC codes (waveforms_amd/encoding/ldpc.py) and the HIP encoder / layered min-sum decoder (wf_ldpc_*, include/wfhip.h).

The decoder's definition is restated here twice: a vectorised numpy form (over codewords and the checks of a layer) and
a scalar loop form, pinned to each other bitwise on the CPU.  On the GPU the decoder must equal the restatement BITWISE
(decisions, posteriors as uint32, iterations, counts) and the encoder must equal the host encoder.
"""
import ctypes

import numpy as np
import pytest

from waveforms_amd.encoding import ldpc


# ------------------------------------------------------------------------------------------------ restatement
def _layer_tables(code):
    """Per layer: (variables sz x D, edge ids sz x D, valid sz x D) in the C ABI's numbering (checks in layer order)."""
    t = code.c_tables()
    cp, ev, lp = t["check_ptr"], t["edge_var"], t["layer_ptr"]
    out = []
    for li in range(t["nlayers"]):
        cs = range(lp[li], lp[li + 1])
        D = max(cp[c + 1] - cp[c] for c in cs)
        V = np.zeros((len(cs), D), dtype=np.int64)
        E = np.zeros((len(cs), D), dtype=np.int64)
        ok = np.zeros((len(cs), D), dtype=bool)
        for j, c in enumerate(cs):
            d = cp[c + 1] - cp[c]
            V[j, :d], E[j, :d], ok[j, :d] = ev[cp[c]:cp[c + 1]], np.arange(cp[c], cp[c + 1]), True
        out.append((V, E, ok))
    return t, out


def _syndrome_ok(t, L):
    x = (L < 0).astype(np.int64)[:, t["edge_var"]]
    return ~np.any(np.add.reduceat(x, t["check_ptr"][:-1], axis=1) & 1, axis=1)


def decode_restatement(code, llr, scale=1.0, alpha=0.75, max_iter=50):
    """The header's definition, vectorised over codewords and the checks of a layer -> (info_bits, post, iters)."""
    t, layers = _layer_tables(code)
    llr = np.atleast_2d(np.asarray(llr, dtype=np.float64))
    ncw = llr.shape[0]
    L = np.zeros((ncw, code.n), dtype=np.float32)
    L[:, code.tx_order] = (scale * llr).astype(np.float32)
    R = np.zeros((ncw, t["edge_var"].size), dtype=np.float32)
    a32 = np.float32(alpha)
    iters = np.full(ncw, max_iter, dtype=np.int32)
    done = _syndrome_ok(t, L)
    iters[done] = 0
    for it in range(1, max_iter + 1):
        act = np.flatnonzero(~done)
        if act.size == 0:
            break
        La, Ra = L[act], R[act]
        for V, E, ok in layers:
            T = La[:, V] - Ra[:, E]
            mag = np.where(ok, np.abs(T), np.float32(np.inf))
            e1 = np.argmin(mag, axis=2)
            m1 = np.take_along_axis(mag, e1[..., None], axis=2)[..., 0]
            mag2 = mag.copy()
            np.put_along_axis(mag2, e1[..., None], np.float32(np.inf), axis=2)
            m2 = mag2.min(axis=2)
            neg = (T < 0) & ok
            S = (neg.sum(axis=2) & 1).astype(bool)
            r1, r2 = a32 * m1, a32 * m2
            first = np.arange(V.shape[1])[None, None, :] == e1[..., None]
            rm = np.where(first, r2[..., None], r1[..., None])
            Rn = np.where(S[..., None] ^ neg, -rm, rm)
            Ln = T + Rn
            La[:, V[ok]] = Ln[:, ok]
            Ra[:, E[ok]] = Rn[:, ok]
        L[act], R[act] = La, Ra
        fin = act[_syndrome_ok(t, La)]
        done[fin] = True
        iters[fin] = it
    return (L[:, code.info_var] < 0).astype(np.uint8), L, iters


def decode_scalar(code, llr, scale=1.0, alpha=0.75, max_iter=50):
    """The same definition one codeword, one check and one edge at a time (float32 scalars)."""
    t = code.c_tables()
    cp, ev, lp = t["check_ptr"], t["edge_var"].tolist(), t["layer_ptr"]
    f32 = np.float32
    llr = np.atleast_2d(np.asarray(llr, dtype=np.float64))
    src = {int(v): i for i, v in enumerate(code.tx_order)}
    posts, its = [], []
    for row in llr:
        L = [f32(scale * row[src[v]]) if v in src else f32(0.0) for v in range(code.n)]
        R = [f32(0.0)] * len(ev)

        def ok():
            return all(sum(1 for e in range(cp[c], cp[c + 1]) if L[ev[e]] < 0) % 2 == 0 for c in range(code.m))

        its_b = 0 if ok() else max_iter
        if its_b:
            for it in range(1, max_iter + 1):
                for li in range(t["nlayers"]):
                    for c in range(lp[li], lp[li + 1]):
                        es = range(cp[c], cp[c + 1])
                        T = {e: f32(L[ev[e]] - R[e]) for e in es}
                        m1, m2, e1, S = f32(np.inf), f32(np.inf), None, 0
                        for e in es:
                            a = abs(T[e])
                            if a < m1:
                                m1, m2, e1 = a, m1, e
                            elif a < m2:
                                m2 = a
                            S ^= int(T[e] < 0)
                        for e in es:
                            r = f32(f32(alpha) * (m2 if e == e1 else m1))
                            if S ^ int(T[e] < 0):
                                r = -r
                            R[e] = r
                            L[ev[e]] = f32(T[e] + r)
                if ok():
                    its_b = it
                    break
        posts.append(np.array(L, dtype=np.float32))
        its.append(its_b)
    post = np.array(posts)
    return (post[:, code.info_var] < 0).astype(np.uint8), post, np.array(its, dtype=np.int32)


# ------------------------------------------------------------------------------------------------ codes
def random_code(seed, punct=False):
    """A small irregular code built with a seed: n 24 .. 600, check degrees 2 .. 12, every variable in at least one
    check; with ``punct`` a few variables are left out of tx_order (the encoder must be able to pivot on them)."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(24, 601))
    m = int(rng.integers(n // 4, n // 2 + 1))
    H = np.zeros((m, n), dtype=np.uint8)
    for c in range(m):
        d = int(rng.integers(2, 13))
        H[c, rng.choice(n, size=min(d, n), replace=False)] = 1
    for v in np.flatnonzero(H.sum(axis=0) == 0):
        H[rng.integers(0, m), v] = 1
    tx = rng.permutation(n)
    if punct:
        for _ in range(50):
            drop = rng.choice(n, size=max(1, n // 20), replace=False)
            try:
                return ldpc.LDPCCode.from_parity_check(H, tx_order=np.setdiff1d(tx, drop, assume_unique=False)[rng.permutation(n - drop.size)])
            except ValueError:
                continue
        raise AssertionError("no puncturable set found")
    return ldpc.LDPCCode.from_parity_check(H, tx_order=tx)


def random_codes():
    return [random_code(s, punct=bool(s % 2)) for s in range(6)]


def _girth_at_least_6(code):
    H = code.parity_check_matrix().astype(np.int64)
    overlap = H @ H.T
    np.fill_diagonal(overlap, 0)
    return overlap.max() <= 1


# ------------------------------------------------------------------------------------------------ CPU
def test_demo_code_parameters_and_girth():
    c = ldpc.demo_code()
    assert (c.n, c.m, c.n_tx, c.k) == (2048, 1024, 2048, 1024) and c.punctured.size == 0
    H = c.parity_check_matrix()
    assert (H.sum(axis=0) == 3).all() and (H.sum(axis=1) == 6).all()
    assert _girth_at_least_6(c)
    assert len(c.layers) == 8 and all(len(layer) == 128 for layer in c.layers)
    assert np.array_equal(ldpc._demo_search(128), np.array(ldpc.DEMO_SHIFTS_128))
    assert np.array_equal(np.sort(c.tx_order), np.arange(2048)) and not np.array_equal(c.tx_order, np.arange(2048))
    # consecutive channel bits land in different block columns
    assert np.all(c.tx_order[1:] // 128 != c.tx_order[:-1] // 128)


def test_demo_code_large():
    c = ldpc.demo_code(1024)
    assert (c.n, c.m, c.k) == (16384, 8192, 8192)
    E = ldpc._demo_search(1024)
    assert ((E >= 0).sum(axis=0) == 3).all() and ((E >= 0).sum(axis=1) == 6).all()


def test_host_encoder_demo():
    c = ldpc.demo_code()
    rng = np.random.default_rng(5)
    u = rng.integers(0, 2, (10_000, c.k), dtype=np.uint8)
    cw = c.codeword_host(u)
    H = c.parity_check_matrix().astype(np.float32)
    assert not np.any(np.rint(H @ cw.T.astype(np.float32)).astype(np.int64) & 1)
    assert np.array_equal(cw[:, c.info_var], u)
    tx = c.encode_host(u[:50])
    assert np.array_equal(tx, cw[:50, c.tx_order])


@pytest.mark.parametrize("seed", range(6))
def test_host_encoder_random_codes(seed):
    c = random_code(seed, punct=bool(seed % 2))
    assert c.punctured.size > 0 if seed % 2 else c.punctured.size == 0
    rng = np.random.default_rng(100 + seed)
    u = rng.integers(0, 2, (10_000, c.k), dtype=np.uint8)
    cw = c.codeword_host(u)
    H = c.parity_check_matrix().astype(np.int64)
    assert not np.any((H @ cw.T.astype(np.int64)) & 1)
    assert np.array_equal(cw[:, c.info_var], u)
    assert np.array_equal(c.encode_host(u[:20]), cw[:20, c.tx_order])
    assert np.isin(c.punctured, c.parity_var).all()
    # layers: every check once, no shared variable inside a layer (greedy default)
    flat = sorted(x for layer in c.layers for x in layer)
    assert flat == list(range(c.m))


def test_greedy_layering_rule():
    H = np.array([[1, 1, 0, 0, 0, 0], [0, 0, 1, 1, 0, 0], [1, 0, 1, 0, 0, 0], [0, 0, 0, 0, 1, 1], [0, 1, 0, 0, 1, 0]])
    c = ldpc.LDPCCode.from_parity_check(H)
    assert c.layers == [[0, 1, 3], [2, 4]]


def test_invalid_codes_raise():
    ok = np.array([[1, 1, 0, 1], [0, 1, 1, 1]])
    with pytest.raises(ValueError, match="degree"):
        ldpc.LDPCCode.from_parity_check(np.array([[1, 0, 0, 0], [0, 1, 1, 1]]))
    wide = np.zeros((2, 40), dtype=np.uint8)
    wide[0, :33] = 1
    wide[1, 30:] = 1
    with pytest.raises(ValueError, match="degree"):
        ldpc.LDPCCode.from_parity_check(wide)
    with pytest.raises(ValueError, match="share"):
        ldpc.LDPCCode.from_parity_check(ok, layers=[[0, 1]])
    with pytest.raises(ValueError, match="exactly once"):
        ldpc.LDPCCode.from_parity_check(ok, layers=[[0]])
    with pytest.raises(ValueError, match="distinct"):
        ldpc.LDPCCode.from_parity_check(ok, tx_order=[0, 1, 1, 2])
    with pytest.raises(ValueError, match="distinct"):
        ldpc.LDPCCode.from_parity_check(ok, tx_order=[0, 1, 7])
    with pytest.raises(ValueError, match="n = "):
        ldpc.LDPCCode.from_exponent_matrix(np.zeros((1, 3), dtype=int), 16384)
    with pytest.raises(ValueError, match="punctured"):
        # columns 0 and 3 are equal in H: both cannot be parity variables
        ldpc.LDPCCode.from_parity_check(np.array([[1, 1, 0, 1], [1, 0, 1, 1]]), tx_order=[1, 2])


def _c_create(lib, ctx, t, **over):
    t = dict(t, **over)
    out = ctypes.c_void_p()
    p = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data  # noqa: E731
    keep = [t[k] for k in ("check_ptr", "edge_var", "layer_ptr", "tx_var", "info_var", "parity_gen")]
    rc = lib.wf_ldpc_code_create(ctx, t["n"], t["m"], p(keep[0]), p(keep[1]), t["nlayers"], p(keep[2]), t["n_tx"], p(keep[3]), t["k"],
                                 p(keep[4]), p(keep[5]), ctypes.byref(out))
    return rc, out.value


def test_c_create_refuses_invalid_codes_without_a_gpu():
    """Every kind of invalid code: WF_ERR_VALUE before the context or device memory is touched (a fake context)."""
    from waveforms_amd import _hip

    lib = _hip.lib()
    fake = ctypes.create_string_buffer(1 << 16)
    V = _hip.WF_ERR_VALUE
    t = random_code(1, punct=True).c_tables()
    i32 = lambda a: np.asarray(a, dtype=np.int32)  # noqa: E731
    bad = []
    cp = t["check_ptr"].copy()
    cp[1] = cp[0] + 1                                              # a degree-1 check
    bad.append(dict(check_ptr=cp))
    ev = t["edge_var"].copy()
    ev[0] = t["n"]                                                  # a variable outside the code
    bad.append(dict(edge_var=ev))
    ev = t["edge_var"].copy()
    ev[1] = ev[0]                                                   # a variable twice in one check
    bad.append(dict(edge_var=ev))
    bad.append(dict(nlayers=1, layer_ptr=i32([0, t["m"]])))         # one layer whose checks share variables
    tx = t["tx_var"].copy()
    tx[1] = tx[0]                                                   # tx_order not a bijection
    bad.append(dict(tx_var=tx))
    bad.append(dict(n=40000))                                       # n > 32768
    bad.append(dict(n=1))
    bad.append(dict(k=0))
    info = t["info_var"].copy()
    info[1] = info[0]
    bad.append(dict(info_var=info))
    for over in bad:
        rc, h = _c_create(lib, fake, t, **over)
        assert rc == V and h is None, over
    assert lib.wf_ldpc_code_create(None, 4, 2, None, None, 1, None, 4, None, 2, None, None, None) == V
    assert lib.wf_ldpc_code_free(None) == 0
    g = (ctypes.c_int64 * 5)()
    assert lib.wf_ldpc_decode_geometry(fake, None, 10, g) == V
    assert lib.wf_ldpc_decode(fake, None, None, 10, 1.0, 0.75, 50, None, None, None, None, None, None) == V
    assert lib.wf_ldpc_encode(fake, None, None, 10, None, None) == V


def test_restatement_forms_agree_bitwise():
    rng = np.random.default_rng(7)
    for code in random_codes()[:4]:
        cw = code.encode_host(rng.integers(0, 2, (12, code.k), dtype=np.uint8))
        llr = (1.0 - 2.0 * cw) * 2.0 + rng.normal(0, 1.3, cw.shape)
        llr[-3:] = rng.normal(0, 1.0, (3, code.n_tx))               # garbage: runs to max_iter
        for max_iter in (1, 12):
            a = decode_restatement(code, llr, 0.7, 0.75, max_iter)
            b = decode_scalar(code, llr, 0.7, 0.75, max_iter)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]), (code.n, max_iter)
            assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), (code.n, max_iter)


def test_restatement_properties():
    code = ldpc.demo_code()
    rng = np.random.default_rng(9)
    u = rng.integers(0, 2, (16, code.k), dtype=np.uint8)
    tx = code.encode_host(u)
    clean = 4.0 * (1.0 - 2.0 * tx)
    info, _post, iters = decode_restatement(code, clean)
    assert (iters == 0).all() and np.array_equal(info, u)
    # one weak wrong sign among strong correct ones: corrected within 2 iterations (girth >= 6)
    weak = clean.copy()
    for b in range(16):
        weak[b, rng.integers(0, code.n_tx)] *= -0.05
    info, _post, iters = decode_restatement(code, weak)
    assert np.array_equal(info, u) and (iters >= 1).all() and (iters <= 2).all()
    # scale invariance of normalized min-sum: 2 λ gives the same decisions and iterations
    noisy = clean / 4.0 + rng.normal(0, 0.8, clean.shape)
    a, b = decode_restatement(code, noisy), decode_restatement(code, 2.0 * noisy)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])


def test_ldpc_kernels_resources():
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
    import kernel_resources as kr
    from waveforms_amd.csrc.build import build

    so = build(verbose=False)
    tab = {k: v for k, v in kr.kernel_table(so).items() if k.startswith("ldpc_")}
    assert set(tab) == {"ldpc_encode_kernel", "ldpc_decode_kernel<true>", "ldpc_decode_kernel<false>"}, sorted(tab)
    asm = kr.loop_spill_counts(so, "ldpc_")
    for name, row in tab.items():
        assert row["vgpr_spill_count"] == 0 and row["sgpr_spill_count"] == 0 and row["private_segment_fixed_size"] == 0, (name, row)
        a = asm[name]
        assert a["scratch_load_in_loop"] == 0 and a["scratch_store_in_loop"] == 0 and a["v_writelane_in_loop"] == 0, (name, a)
    # the decoder's occupancy claim: 4 workgroups of 4 waves per CU need at most 128 VGPRs (4 waves per SIMD)
    for name in ("ldpc_decode_kernel<true>", "ldpc_decode_kernel<false>"):
        assert kr.waves_per_simd(tab[name]["vgpr_count"], tab[name].get("agpr_count", 0)) >= 4, tab[name]


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def small_codes():
    return random_codes()


@pytest.mark.gpu
def test_gpu_encoder_is_the_host_encoder(small_codes):
    from waveforms_amd import _hip

    rng = np.random.default_rng(21)
    demo = ldpc.demo_code()
    plain = ldpc.LDPCCode.from_exponent_matrix(np.array(ldpc.DEMO_SHIFTS_128), 128)
    for code, ncw in [(demo, 5000), (plain, 5000), (ldpc.demo_code(1024), 64)] + [(c, 333) for c in small_codes]:
        u = rng.integers(0, 2, (ncw, code.k), dtype=np.uint8)
        got = _hip.to_host(code.encode_device(_hip.to_device(u)))
        assert np.array_equal(got, code.encode_host(u)), code.n
    u = rng.integers(0, 2, (3, demo.k), dtype=np.uint8)
    assert np.array_equal(demo.encode(u), demo.encode_host(u))
    info = demo.decode(4.0 * (1.0 - 2.0 * demo.encode_host(u)))
    assert np.array_equal(info["info_bits"], u) and (info["iters"] == 0).all()


def _check_decoder(code, llr, u=None, scale=1.0, alpha=0.75, max_iter=50):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    want_info, want_post, want_it = decode_restatement(code, llr, scale, alpha, max_iter)
    ref = _hip.to_device(u if u is not None else np.zeros_like(want_info))
    out = dev.ldpc_decode(code, _hip.to_device(np.ascontiguousarray(llr)), scale=scale, alpha=alpha, max_iter=max_iter,
                          ref_info=ref, want_post=True)
    info, post, it = _hip.to_host(out["info_bits"]), _hip.to_host(out["post"]), _hip.to_host(out["iters"])
    counts = _hip.to_host(out["counts"])
    _hip.device_check()
    assert np.array_equal(it, want_it), (code.n, int(np.count_nonzero(it != want_it)))
    assert np.array_equal(info, want_info)
    assert np.array_equal(post.view(np.uint32), want_post.view(np.uint32)), int(np.count_nonzero(post != want_post))
    r = u if u is not None else np.zeros_like(want_info)
    e = (want_info != r).sum(axis=1)
    want_counts = [int(e.sum()), int((e > 0).sum()), int((want_it == max_iter).sum() - np.count_nonzero(
        (want_it == max_iter) & _restated_converged_at_last(code, want_post, max_iter, want_it))), int(want_it.sum())]
    assert counts.tolist() == want_counts, (counts.tolist(), want_counts)
    return want_it


def _restated_converged_at_last(code, post, max_iter, iters):
    """Codewords whose iters == max_iter but whose syndrome is zero (they converged exactly at max_iter)."""
    t = code.c_tables()
    return _syndrome_ok(t, post) & (iters == max_iter)


@pytest.mark.gpu
@pytest.mark.parametrize("max_iter", [1, 50])
def test_gpu_decoder_synthetic_llrs(small_codes, max_iter):
    rng = np.random.default_rng(31 + max_iter)
    demo = ldpc.demo_code()
    for code in [demo] + small_codes:
        for ncw in (1, 7, 203):
            u = rng.integers(0, 2, (ncw, code.k), dtype=np.uint8)
            tx = code.encode_host(u)
            sigma = 0.9
            llr = 2.0 * ((1.0 - 2.0 * tx) + rng.normal(0, sigma, tx.shape)) / sigma**2
            _check_decoder(code, llr, u, scale=0.5, max_iter=max_iter)
        garbage = rng.normal(0, 3.0, (9, code.n_tx)) * rng.choice([-1.0, 1.0], (9, code.n_tx))
        _check_decoder(code, garbage, None, max_iter=max_iter)


@pytest.mark.gpu
def test_gpu_decoder_large_code_scratch_form():
    from waveforms_amd import device as dev

    code = ldpc.demo_code(1024)
    geom = dev.ldpc_decode_geometry(code, 300)
    assert geom["state_in_scratch"] == 1 and geom["codewords_per_workgroup"] == 1
    assert dev.ldpc_decode_geometry(ldpc.demo_code(), 300)["state_in_scratch"] == 0
    rng = np.random.default_rng(41)
    u = rng.integers(0, 2, (300, code.k), dtype=np.uint8)
    tx = code.encode_host(u)
    sigma = 0.95
    llr = 2.0 * ((1.0 - 2.0 * tx) + rng.normal(0, sigma, tx.shape)) / sigma**2
    it = _check_decoder(code, llr, u, max_iter=30)
    assert it.max() > 2


@pytest.mark.gpu
@pytest.mark.parametrize("ebn0", [3.0, 5.0, 7.0])
def test_gpu_decoder_on_soft_detector_llrs(ebn0):
    """λ from the real chain (CodedSOQPSKLink: viterbi_soft on the PT rows) at information Eb/N0 3, 5 and 7 dB."""
    from waveforms_amd import _hip
    from waveforms_amd.encoding.coded import CodedSOQPSKLink

    code = ldpc.demo_code()
    link = CodedSOQPSKLink(code, 301, detector="PT")
    llr, info = link.channel_llrs(ebn0, seed=3)
    llr, info = _hip.to_host(llr), _hip.to_host(info)
    it = _check_decoder(code, llr, info, scale=link.llr_scale)
    if ebn0 == 3.0:
        assert (it == 50).sum() > 30
