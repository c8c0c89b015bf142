"""Turbo codes: wf_turbo_code_create / wf_turbo_encode / wf_turbo_decode (include/wfhip.h) and TurboCode
(waveforms_amd/encoding/turbo.py).

The decoder's definition is restated here in numpy float32, one step at a time and in the header's order (``siso_restatement``
for one constituent, ``decode_restatement`` for the half-iterations), and the constituent's SISO is pinned to brute force over
all 2^k messages with integer-valued inputs, where every sum is exact.  On the GPU the kernels must equal the restatement
BITWISE.

The constituents of the brute-force cases are written (feedback, parity generators) in octal: (13, 15) with K = 4, (7, 5) with
K = 3, (23, 33 25 37) with K = 5 and (5, 7) with K = 3.  (The issue lists each as the feedback mask and the set of ALL output
masks, the systematic output's being the feedback mask itself.  Read that way its fourth entry, (7, {5, 7}), is the second one
again; it is run as feedback 5 with parity 7, the other K = 3 constituent there is, so that four DIFFERENT codes are checked.)

The loop's gain is checked on the CPU from the restatements alone; the figures seen are in the tests' docstrings.
"""
import ctypes
import itertools

import numpy as np
import pytest

import test_idd as TI
from waveforms_amd.encoding import turbo

# constraint length -> (feedback, parity generators for n_par = 1, 2, 3)
MASKS = {3: (0o7, (0o5, 0o5, 0o5)), 4: (0o13, (0o15, 0o17, 0o11)), 5: (0o23, (0o33, 0o25, 0o37))}      # (K = 3 has one mask besides 7)
PUNCTURE = {2: [[1, 1], [1, 0], [1, 1], [0, 1]], 3: [[1, 1, 1], [1, 0, 1], [0, 1, 1], [1, 1, 0], [1, 1, 0], [1, 0, 1]],
            4: [[1, 1], [1, 0], [0, 1], [1, 1], [1, 1], [0, 1], [1, 0], [1, 1]]}
N_PARS = (1, 2)                                                       # the grids; n_par = 3 has cases of its own


def make_code(K, n_par, k, punct=False, seed=0):
    """A code of the grid with a random interleaver; ``punct``: punctured AND transmitted in a random order."""
    fb, gens = MASKS[K]
    rng = np.random.default_rng(1000 * K + 10 * k + seed)
    perm = rng.permutation(k)
    if not punct:
        return turbo.TurboCode(k, perm, fb, gens[:n_par], K)
    plain = turbo.TurboCode(k, perm, fb, gens[:n_par], K, puncture=PUNCTURE[1 + n_par])
    return turbo.TurboCode(k, perm, fb, gens[:n_par], K, puncture=PUNCTURE[1 + n_par], tx_order=rng.permutation(plain.n_tx))


def send_everything(code):
    """The same code with EVERY variable transmitted, constituent 2's systematic output included (the C ABI allows it; the
    Python constructor never builds it)."""
    code.tx_var = np.arange(code.n, dtype=np.int64)
    code.n_tx = code.n
    code.rate = code.k / code.n_tx
    return code


# ------------------------------------------------------------------------------------------------ restatement
def _trellis(code):
    """next[a][s], and bits[a][s, j] = c_j of branch (s, a): reg = (a << nu) | s, c_0 = parity(reg & fb) (= u),
    c_j = parity(reg & g_j), s' = reg >> 1."""
    nu = code.K - 1
    s = np.arange(1 << nu)
    masks = (code.feedback,) + code.parity
    nxt, bits = [], []
    for a in (0, 1):
        reg = (a << nu) | s
        nxt.append(reg >> 1)
        bits.append(np.array([[bin(int(r) & g).count("1") & 1 for g in masks] for r in reg], dtype=bool))
    return nxt, bits


def siso_restatement(code, Lc, A):
    """SISO(c, A) of the header: ``Lc`` B x T x m float32 (the constituent's channel values), ``A`` B x k float32 -> P (B x T x m
    float32); Λ_i is P[:, i, 0] for i < k."""
    B, T, m = Lc.shape
    k, nu = code.k, code.K - 1
    S = 1 << nu
    nxt, bits = _trellis(code)
    assert Lc.dtype == np.float32 and A.dtype == np.float32 and A.shape == (B, k)
    ninf = np.float32(-np.inf)
    zero = np.zeros((B, S), dtype=np.float32)

    def gamma(i, a):
        g = np.where(bits[a][:, 0][None, :], (-A[:, i])[:, None], zero) if i < k else zero          # (u ? -A_i : +0)
        for j in range(m):
            g = np.where(bits[a][:, j][None, :], g - Lc[:, i, j][:, None], g)
        assert g.dtype == np.float32
        return g

    alpha = [None] * (T + 1)
    al = np.full((B, S), ninf, dtype=np.float32)
    al[:, 0] = 0.0
    alpha[0] = al
    for i in range(T):
        new = np.full((B, S), ninf, dtype=np.float32)
        for a in ((0, 1) if i < k else (0,)):
            cand = al + gamma(i, a)                                   # by source state; s and s ^ 1 enter the same s'
            new[:, a * (S // 2):(a + 1) * (S // 2)] = cand.reshape(B, S // 2, 2).max(axis=2)
        al = new
        alpha[i + 1] = al
    P = np.zeros((B, T, m), dtype=np.float32)
    b = np.full((B, S), ninf, dtype=np.float32)
    b[:, 0] = 0.0
    cb = [np.concatenate([bits[0][:, j], bits[1][:, j]]) for j in range(m)]
    for i in range(T - 1, -1, -1):
        V, W = [], []
        for a in (0, 1):
            if a and i >= k:
                V.append(np.full((B, S), ninf, dtype=np.float32))
                W.append(np.full((B, S), ninf, dtype=np.float32))
                continue
            g = gamma(i, a)
            V.append((alpha[i] + g) + b[:, nxt[a]])
            W.append(g + b[:, nxt[a]])
        VV = np.concatenate(V, axis=1)
        for j in range(m):
            P[:, i, j] = np.where(~cb[j][None, :], VV, ninf).max(axis=1) - np.where(cb[j][None, :], VV, ninf).max(axis=1)
        b = np.maximum(W[0], W[1])
    return P


def channel_values(code, llr, scale=1.0):
    """L by variable (B x T x 2m float32, 0 where punctured) and the two constituents' values (B x T x m each): constituent 2's
    systematic value at i < k is constituent 1's at π(i), whatever its own variable holds."""
    llr = np.atleast_2d(np.asarray(llr, dtype=np.float64))
    m = 1 + code.n_par
    L = np.zeros((llr.shape[0], code.n), dtype=np.float32)
    L[:, code.tx_var] = (np.float64(scale) * llr).astype(np.float32)
    Lv = L.reshape(-1, code.T, 2 * m)
    L1 = np.ascontiguousarray(Lv[:, :, :m])
    L2 = np.ascontiguousarray(Lv[:, :, m:])
    L2[:, :code.k, 0] = L1[:, code.interleaver, 0]
    return Lv, L1, L2


def decode_restatement(code, llr, half_iters, scale=1.0, ext_scale=0.75, early_stop=True, a1=None, ext_clip=np.inf):
    """The header's definition of wf_turbo_decode -> dict(bits u8 B x k, post float32 B x k, iters int32 B, halves int B (the
    half-iterations run), a1 float32 B x k, ext float32 B x n_tx or None when half_iters is odd)."""
    Lv, L1, L2 = channel_values(code, llr, scale)
    B, k, H, perm = Lv.shape[0], code.k, int(half_iters), code.interleaver
    es = np.float32(ext_scale)
    A1 = np.zeros((B, k), dtype=np.float32) if a1 is None else np.array(a1, dtype=np.float32).reshape(B, k)
    A2 = np.zeros((B, k), dtype=np.float32)
    bits, post = np.zeros((B, k), dtype=np.uint8), np.zeros((B, k), dtype=np.float32)
    lam1, lam2 = np.zeros((B, k), dtype=np.float32), np.zeros((B, k), dtype=np.float32)
    P1, P2 = np.zeros_like(L1), np.zeros_like(L2)
    iters, halves = np.full(B, (H + 1) // 2, dtype=np.int32), np.full(B, H, dtype=np.int64)
    active = np.ones(B, dtype=bool)
    for h in range(1, H + 1):
        act = active.copy()
        if not act.any():
            break
        if h & 1:
            P = siso_restatement(code, L1, A1)
            lam = P[:, :k, 0]
            E = es * ((lam - A1) - L1[:, :k, 0])
            assert E.dtype == np.float32
            A2[act] = E[act][:, perm]                                 # A2_i = E1_π(i)
            lam1[act], P1[act] = lam[act], P[act]
            if h == H:
                bits[act], post[act] = (lam[act] < 0), lam[act]
        else:
            P = siso_restatement(code, L2, A2)
            lam = P[:, :k, 0]
            E = es * ((lam - A2) - L2[:, :k, 0])
            de = np.zeros((B, k), dtype=np.float32)
            de[:, perm] = E                                           # A1_π(i) = E2_i
            A1[act] = de[act]
            de[:, perm] = lam
            post[act], bits[act] = de[act], (de[act] < 0)
            lam2[act], P2[act] = lam[act], P[act]
            if early_stop:
                stop = act & ((lam < 0) == (lam1[:, perm] < 0)).all(axis=1)
                iters[stop], halves[stop] = h // 2, h
                active &= ~stop
    ext = None
    if H % 2 == 0:
        X = np.concatenate([P1, P2], axis=2) - Lv
        de = np.zeros((B, k), dtype=np.float32)
        de[:, perm] = lam2
        X[:, :k, 0] = de - L1[:, :k, 0]
        clip = np.float32(ext_clip)
        ext = np.minimum(np.maximum(X.reshape(B, code.n)[:, code.tx_var], -clip), clip).astype(np.float32)
    return dict(bits=bits, post=post, iters=iters, halves=halves, a1=A1, ext=ext)


def constituent_brute_force(code, Lc, A):
    """Over all 2^k messages of ONE constituent with the metric -Σ c L - Σ u A (float64): max with bit = 0 minus max with
    bit = 1 -> P (T x m); +inf for a bit that is 0 in every codeword."""
    msgs = np.array(list(itertools.product((0, 1), repeat=code.k)), dtype=np.uint8)
    cws = code._constituent_host(msgs).reshape(msgs.shape[0], -1)
    metric = -(cws.astype(np.float64) @ np.asarray(Lc, dtype=np.float64).reshape(-1)) - (msgs.astype(np.float64) @ np.asarray(A, dtype=np.float64))
    def best(sel):
        return metric[sel].max() if sel.any() else -np.inf           # (k < K - 1: a tail bit that is 0 in every codeword)

    return np.array([best(cws[:, v] == 0) - best(cws[:, v] == 1) for v in range(cws.shape[1])]).reshape(code.T, -1)


def _integer_case(code, rng):
    """Integer-valued λ in [-9, 9] with a quarter of them 0, integer prior: every sum is exact."""
    llr = rng.integers(-9, 10, code.n_tx).astype(np.float64)
    llr[rng.integers(0, 4, code.n_tx) == 0] = 0.0
    return llr, rng.integers(-6, 7, code.k).astype(np.float32)


def mixed_batch(code, ncw, rng):
    """λ of a batch that mixes three kinds of codeword: clean ones (b % 3 == 0: they stop at iteration 1), noisy ones
    (b % 3 == 1) and garbage that never stops (b % 3 == 2) -> (messages, λ ncw x n_tx)."""
    u = rng.integers(0, 2, (ncw, code.k), dtype=np.uint8)
    tx = code.encode_host(u).astype(np.float64)
    kind = np.arange(ncw) % 3
    amp = np.where(kind == 2, 0.0, 4.0)[:, None]
    sig = np.where(kind == 0, 0.0, np.where(kind == 1, 3.0, 4.0))[:, None]
    return u, amp * (1.0 - 2.0 * tx) + sig * rng.standard_normal(tx.shape)


# ------------------------------------------------------------------------------------------------ CPU
def test_encoder_facts():
    rng = np.random.default_rng(1)
    for K, n_par, k in ((4, 1, 40), (3, 1, 9), (5, 3, 23), (4, 2, 1), (4, 1, 2), (5, 2, 1), (3, 1, 2)):
        code = make_code(K, n_par, k)
        m, nu = 1 + n_par, K - 1
        assert (code.k, code.K, code.n_par, code.T, code.n) == (k, K, n_par, k + nu, 2 * m * (k + nu))
        assert code.n_tx == (2 * m - 1) * k + 2 * m * nu and code.rate == k / code.n_tx
        v = np.arange(code.n)
        assert np.array_equal(code.tx_var, v[~((v % (2 * m) == m) & (v // (2 * m) < k))])
        u = rng.integers(0, 2, (6, k), dtype=np.uint8)
        c = code.codeword_host(u).reshape(6, code.T, 2 * m)          # (both final states are 0: asserted by the host encoder itself)
        assert np.array_equal(c[:, :k, 0], u) and np.array_equal(c[:, :k, m], u[:, code.interleaver])
        assert np.array_equal(code.codeword_host(u[0] ^ u[1]), code.codeword_host(u[0]) ^ code.codeword_host(u[1]))
        assert not code.codeword_host(np.zeros((1, k), dtype=np.uint8)).any()
        assert np.array_equal(code.encode_host(u), code.codeword_host(u)[:, code.tx_var])
    # the final state is 0 for every message: the tail bits are the feedback parity, so the register's input is 0
    code = make_code(4, 1, 6)
    msgs = np.array(list(itertools.product((0, 1), repeat=6)), dtype=np.uint8)
    tail = code.codeword_host(msgs).reshape(64, code.T, 4)[:, 6:, 0]
    assert tail.any() and len({tuple(t) for t in tail}) == 8         # all 8 final states of the message part occur
    assert turbo.TurboCode.qpp(512, 31, 64).n_tx == 1548
    q = turbo.TurboCode.qpp(512, 31, 64)
    assert (q.K, q.feedback, q.parity) == (4, 0o13, (0o15,)) and q.interleaver[:3].tolist() == [0, 95, 318]
    # the impulse response of the (13, 15) constituent: the parity stream of 1 / (1 + D^2 + D^3) times (1 + D + D^3)
    imp = turbo.TurboCode(8, np.arange(8), 0o13, (0o15,))._constituent_host(np.array([[1, 0, 0, 0, 0, 0, 0, 0]], dtype=np.uint8))[0]
    assert imp[:8, 0].tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and imp[:8, 1].tolist() == [1, 1, 1, 1, 0, 0, 1, 0]


@pytest.mark.parametrize("fb, gens, K", [(0o13, (0o15,), 4), (0o7, (0o5,), 3), (0o23, (0o33, 0o25, 0o37), 5), (0o5, (0o7,), 3)])
def test_siso_restatement_equals_brute_force(fb, gens, K):
    rng = np.random.default_rng(fb + sum(gens))
    for k in (7, 7, 7, 1, 2):
        code = turbo.TurboCode(k, rng.permutation(k), fb, gens, K)
        llr, A = _integer_case(code, rng)
        _Lv, L1, L2 = channel_values(code, llr)
        for Lc in (L1, L2):
            P = siso_restatement(code, Lc, A[None, :])
            assert np.isfinite(P[:, :k, 0]).all() and (np.isfinite(P).all() or k < K - 1) and not np.isnan(P).any()
            assert np.array_equal(P[0].astype(np.float64), constituent_brute_force(code, Lc[0], A)), (fb, gens, k)


def test_one_half_iteration_is_the_map_decoder_of_constituent_1():
    rng = np.random.default_rng(12)
    for K, n_par in ((4, 1), (5, 2), (3, 1)):
        code = make_code(K, n_par, 7, punct=True)
        llr, _A = _integer_case(code, rng)
        out = decode_restatement(code, llr[None, :], 1)
        _Lv, L1, _L2 = channel_values(code, llr)
        want = constituent_brute_force(code, L1[0], np.zeros(7))[:7, 0]
        assert np.array_equal(out["post"][0].astype(np.float64), want) and np.array_equal(out["bits"][0], (want < 0).astype(np.uint8))
        assert out["iters"].tolist() == [1] and out["ext"] is None


def test_stop_rule_a1_carry_and_ext_on_a_mixed_batch():
    code = make_code(4, 1, 40, punct=True)
    rng = np.random.default_rng(4)
    u, llr = mixed_batch(code, 9, rng)
    out = decode_restatement(code, llr, 8, ext_clip=5.0)
    kind = np.arange(9) % 3
    assert (out["iters"][kind == 0] == 1).all() and (out["halves"][kind == 0] == 2).all()
    assert (out["iters"][kind == 2] == 4).all() and (out["halves"][kind == 2] == 8).all()
    assert np.array_equal(out["bits"][kind == 0], u[kind == 0])
    assert np.isfinite(out["post"]).all() and np.isfinite(out["ext"]).all() and np.abs(out["ext"]).max() == 5.0
    # a stopped codeword keeps the outputs of its stopping half-iteration: the same as a call that ends there
    two = decode_restatement(code, llr, 2, ext_clip=5.0)
    for key in ("bits", "post", "a1", "ext"):
        assert np.array_equal(out[key][kind == 0], two[key][kind == 0]), key
    # without the stop rule: two calls of H = 2 with A1 carried are one call of H = 4, bit for bit
    four = decode_restatement(code, llr, 4, early_stop=False, ext_clip=5.0)
    first = decode_restatement(code, llr, 2, early_stop=False)
    second = decode_restatement(code, llr, 2, early_stop=False, a1=first["a1"], ext_clip=5.0)
    for key in ("bits", "post", "a1", "ext"):
        assert second[key].tobytes() == four[key].tobytes(), key
    assert (four["iters"] == 2).all()
    # the ext of constituent 1's systematic variable is the deinterleaved Λ2 minus its channel value
    full = decode_restatement(code, llr, 2, early_stop=False)
    Lv, _L1, _L2 = channel_values(code, llr)
    src = {int(v): t for t, v in enumerate(code.tx_var)}
    for i in range(code.k):
        if 4 * i in src:
            assert np.array_equal(full["ext"][:, src[4 * i]], full["post"][:, i] - Lv[:, i, 0])
    # every variable sent, constituent 2's systematic output too: its own channel value plays no part in the decoding
    every = send_everything(make_code(4, 1, 12))
    llr = rng.normal(0, 3.0, (2, every.n_tx))
    other = llr.copy()
    other[:, [4 * i + 2 for i in range(12)]] += 5.0
    a, b = decode_restatement(every, llr, 4), decode_restatement(every, other, 4)
    assert a["post"].tobytes() == b["post"].tobytes() and a["ext"].tobytes() != b["ext"].tobytes()


def test_loop_gain_on_awgn_llrs():
    """TurboCode.qpp(512, 31, 64), ±1 + AWGN with λ = 2 y / σ², 1.5 dB per information bit, 24 codewords, 8 iterations,
    ext_scale 0.75.  Frame errors after each iteration on this seed: 23, 4, 1, 0, 0, 0, 0, 0."""
    code = turbo.TurboCode.qpp(512, 31, 64)
    rng = np.random.default_rng(6)
    u = rng.integers(0, 2, (24, code.k), dtype=np.uint8)
    sigma = np.sqrt(1.0 / (2.0 * code.rate * 10 ** (1.5 / 10)))
    y = (1.0 - 2.0 * code.encode_host(u)) + sigma * rng.standard_normal((24, code.n_tx))
    llr = 2.0 * y / sigma ** 2
    fe, a1 = [], None
    for _it in range(8):
        out = decode_restatement(code, llr, 2, ext_scale=0.75, early_stop=False, a1=a1)
        a1 = out["a1"]
        fe.append(int(np.any(out["bits"] != u, axis=1).sum()))
    print("frame errors per iteration:", fe)
    assert fe[0] >= 4
    assert 4 * fe[-1] <= fe[0]


def test_loop_gain_behind_the_oracle_chain(oracle):
    """The same code behind the oracle's SOQPSK-TG chain, PT detector, seed 3, 16 bursts of one codeword.  One detector pass at
    6 dB, 6 turbo iterations: frame errors 13, 0, 0, 0, 0, 0.  The detector in the loop at 4 dB (outer 6, 1 iteration each,
    damping 0.7, clip 50): frame errors 16, 16, 16, 10, 8, 4, information bit errors 1405, 1132, 794, 599, 384, 284."""
    code = turbo.TurboCode.qpp(512, 31, 64)
    u, rows = TI._cpu_bursts(oracle, code, 16, 6.0, "PT", 3)
    B, N = rows.shape[0], rows.shape[1]
    lam = TI._siso_batch(oracle, rows, np.zeros((B, N), dtype=np.float32), 0.7)[:, 1:1 + code.n_tx]
    fe, a1 = [], None
    for _it in range(6):
        out = decode_restatement(code, lam, 2, early_stop=False, a1=a1)
        a1 = out["a1"]
        fe.append(int(np.any(out["bits"] != u, axis=1).sum()))
    print("6 dB, one detector pass: frame errors per iteration:", fe)
    assert 4 * fe[-1] <= fe[0] and fe[0] >= 4

    u, rows = TI._cpu_bursts(oracle, code, 16, 4.0, "PT", 3)
    prior = np.zeros((B, N), dtype=np.float32)
    fe, be, a1 = [], [], None
    for _o in range(6):
        lam = TI._siso_batch(oracle, rows, prior, 0.7)[:, 1:1 + code.n_tx]
        out = decode_restatement(code, lam, 2, early_stop=False, a1=a1, ext_clip=50.0)
        a1 = out["a1"]
        prior[:, 1:1 + code.n_tx] = out["ext"]
        fe.append(int(np.any(out["bits"] != u, axis=1).sum()))
        be.append(int((out["bits"] != u).sum()))
    print("4 dB, detector in the loop: frame errors per pass:", fe, "bit errors per pass:", be)
    assert 2 * be[-1] <= be[0]


def _fake_create(lib, t, **over):
    a = dict(t, **over)
    out = ctypes.c_void_p()
    gen = np.ascontiguousarray(a["gen"], dtype=np.uint32)
    perm = np.ascontiguousarray(a["perm"], dtype=np.int32)
    tx = np.ascontiguousarray(a["tx_var"], dtype=np.int32)
    fake = ctypes.create_string_buffer(1 << 16)
    return lib.wf_turbo_code_create(fake, a["K"], a["n_par"], a["fb"], gen.ctypes.data, a["k"], perm.ctypes.data, a["n_tx"], tx.ctypes.data,
                                    ctypes.byref(out)), out.value


def test_c_entry_points_refuse_invalid_arguments_without_a_gpu():
    """Every kind of invalid code or call: WF_ERR_VALUE before the context or device memory is touched (a fake context)."""
    from waveforms_amd import _hip

    lib = _hip.lib()
    V = _hip.WF_ERR_VALUE
    t = make_code(5, 2, 20, punct=True).c_tables()
    g = [int(v) for v in t["gen"]]
    N = 2 * 3 * 24
    bad = [dict(K=2, fb=3, gen=[3, 1]), dict(K=6, fb=0o53, gen=[0o75, 0o47]), dict(n_par=0), dict(n_par=4, gen=g + g),
           dict(fb=t["fb"] & ~1), dict(fb=t["fb"] & 0o17), dict(fb=t["fb"] | 0o40), dict(gen=[g[0] & ~1, g[1]]), dict(gen=[g[0], g[1] & 0o17]),
           dict(gen=[g[0], t["fb"]]), dict(k=0), dict(k=32768 // 6), dict(n_tx=0), dict(n_tx=N + 1)]
    for idx, val in ((1, t["tx_var"][0]), (2, N), (0, -1)):
        tx = t["tx_var"].copy()
        tx[idx] = val
        bad.append(dict(tx_var=tx))
    for idx, val in ((1, t["perm"][0]), (2, 20), (0, -1)):
        p = t["perm"].copy()
        p[idx] = val
        bad.append(dict(perm=p))
    for over in bad:
        rc, h = _fake_create(lib, t, **over)
        assert rc == V and h is None, over
    assert lib.wf_turbo_code_create(None, 4, 1, 0o13, None, 4, None, 12, None, None) == V
    assert lib.wf_turbo_code_free(None) == 0
    fake = ctypes.create_string_buffer(1 << 16)
    geom = (ctypes.c_int64 * 5)()
    assert lib.wf_turbo_decode_geometry(fake, None, 10, geom) == V
    assert lib.wf_turbo_encode(fake, None, None, 10, None, None) == V
    assert lib.wf_turbo_decode(fake, None, None, 10, 1.0, 0.75, 2, 1, None, None, None, None, None, 0, 1.0, None, None, None) == V


def test_c_decode_refuses_every_invalid_argument_without_a_gpu():
    """Every argument check of wf_turbo_decode, one invalid argument at a time: WF_ERR_VALUE each, before the geometry or the
    device is touched.  The context and the code are zeroed buffers (device 0) with the code's n_tx set: every check reads only
    those.  The last case is the valid call except for a code that lives on another device."""
    from waveforms_amd import _hip

    lib = _hip.lib()
    V = _hip.WF_ERR_VALUE
    fake = ctypes.create_string_buffer(1 << 16)
    code = (ctypes.c_int32 * 64)()                                    # wf_turbo_code: device, K, nu, n_par, m, k, T, N, n_tx, ...
    code[8] = 100
    buf = ctypes.create_string_buffer(4096)
    base = (ctypes.addressof(buf) + 63) & ~63                         # 64-byte aligned; + 1 / + 4 below: misaligned for 4 / 8 bytes
    inf, nan = float("inf"), float("nan")
    ok = dict(ctx=fake, code=code, llr=base, ncw=3, scale=1.0, es=0.75, H=4, early=1, a1=None, bits=None, post=None, iters=None, ext=None,
              stride=0, clip=1.0, ref=None, counts=None)

    def call(**over):
        a = dict(ok, **over)
        return lib.wf_turbo_decode(a["ctx"], a["code"], a["llr"], a["ncw"], a["scale"], a["es"], a["H"], a["early"], a["a1"], a["bits"], a["post"],
                                   a["iters"], a["ext"], a["stride"], a["clip"], a["ref"], a["counts"], None)

    ext = dict(ext=base + 512, stride=100, clip=2.0)                  # a valid extrinsic output (H = 4 is even)
    bad = [dict(ctx=None), dict(code=None), dict(llr=None), dict(ncw=0), dict(ncw=-5),
           dict(scale=0.0), dict(scale=-1.0), dict(scale=inf), dict(scale=nan),
           dict(es=0.0), dict(es=-0.5), dict(es=inf), dict(es=nan),
           dict(H=0), dict(H=-2), dict(H=65),
           dict(ext, H=3), dict(ext, H=1), dict(ext, stride=99), dict(ext, stride=0), dict(ext, clip=0.0), dict(ext, clip=-1.0), dict(ext, clip=nan),
           dict(ref=base + 1024), dict(llr=base + 4), dict(ref=base + 1024, counts=base + 2048 + 4), dict(a1=base + 1), dict(a1=base + 2),
           dict(post=base + 1), dict(post=base + 3), dict(ext, ext=base + 512 + 2), dict(iters=base + 1), dict(iters=base + 2)]
    for over in bad:
        assert call(**over) == V, over
    other = (ctypes.c_int32 * 64)()
    other[0], other[8] = 1, 100
    assert call(code=other) == V
    assert call(**dict(ext, code=other, ref=base + 1024, counts=base + 2048, a1=base + 256, post=base + 768, iters=base + 3072)) == V
    assert "device" in lib.wf_last_error_string().decode()


def test_python_validation():
    T = turbo.TurboCode
    ok = np.arange(10)
    for kw in (dict(feedback=0o12), dict(feedback=0o3, K=4), dict(parity=(0o14,)), dict(parity=(0o13,)), dict(parity=()),
               dict(parity=(0o15, 0o17, 0o11, 0o15)), dict(K=2), dict(K=6), dict(feedback=0o53, parity=(0o75,)),
               dict(puncture=[[1, 0], [1, 1], [1, 1]]), dict(puncture=[1, 0, 1, 1]), dict(puncture=[[1, 2], [1, 1], [1, 1], [1, 1]]),
               dict(puncture=[[0], [0], [0], [0]]), dict(tx_order=np.arange(5)), dict(tx_order=np.zeros(42, dtype=int))):
        with pytest.raises(ValueError):
            T(10, ok, **kw)
    for perm in (np.arange(9), np.zeros(10, dtype=int), np.arange(1, 11)):
        with pytest.raises(ValueError):
            T(10, perm)
    with pytest.raises(ValueError):
        T(0, [])
    with pytest.raises(ValueError):
        T(8190, np.arange(8190))                                      # n = 4 x 8193 > 32768
    assert T(8189, np.arange(8189)).n == 32768
    with pytest.raises(ValueError):
        T.qpp(512, 32, 64)
    assert T(10, ok).n_tx == 42 and T(10, ok, K=4).K == 4
    code = T(4, [2, 0, 3, 1], puncture=[[1, 1], [1, 0], [1, 1], [0, 1]])
    assert code.tx_var.tolist() == [0, 1, 4, 7, 8, 9, 12, 15, 16, 17, 18, 20, 22, 23, 24, 25, 26]
    with pytest.raises(ValueError):
        code.codeword_host(np.zeros((1, 5), dtype=np.uint8))


def test_turbo_entry_points_exported_and_bound():
    from waveforms_amd import _hip
    from waveforms_amd import device

    lib = _hip.lib()
    for name in ("wf_turbo_code_create", "wf_turbo_code_free", "wf_turbo_encode", "wf_turbo_decode", "wf_turbo_decode_geometry"):
        assert name in _hip.SIGNATURES and hasattr(lib, name)
    assert callable(device.turbo_encode) and callable(device.turbo_decode) and callable(device.turbo_decode_geometry)


def test_turbo_kernels_resources():
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
    import kernel_resources as kr
    from waveforms_amd.csrc.build import build

    so = build(verbose=False)
    tab = {k: v for k, v in kr.kernel_table(so).items() if k.startswith("turbo_")}
    want = {"turbo_encode_kernel"} | {f"turbo_decode_kernel<{nu}, {n_par}>" for nu in (2, 3, 4) for n_par in (1, 2, 3)}
    assert set(tab) == want, sorted(set(tab) ^ want)
    asm = kr.loop_spill_counts(so, "turbo_")
    for name, row in tab.items():
        assert row["vgpr_spill_count"] == 0 and row["sgpr_spill_count"] == 0 and row["private_segment_fixed_size"] == 0, (name, row)
        a = asm[name]
        assert a["scratch_load_in_loop"] == 0 and a["scratch_store_in_loop"] == 0 and a["v_writelane_in_loop"] == 0, (name, a)
        assert row.get("wavefront_size", 64) == 64
    for name in tab:
        if name.startswith("turbo_decode"):
            assert kr.waves_per_simd(tab[name]["vgpr_count"], tab[name].get("agpr_count", 0)) >= 4, tab[name]
            assert tab[name]["group_segment_fixed_size"] <= 22 * 1024, tab[name]


# ------------------------------------------------------------------------------------------------ GPU
def _geometry(code, ncw=1):
    from waveforms_amd import device as dev

    return dev.turbo_decode_geometry(code, ncw)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [3, 4, 5])
def test_gpu_encoder_is_the_host_encoder(K):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    rng = np.random.default_rng(K)
    for n_par, k, punct in itertools.product(N_PARS, (1, 7, 64, 65, 1000), (False, True)):
        code = make_code(K, n_par, k, punct, seed=k)
        G = _geometry(code)["codewords_per_wave"]
        assert G == 64 >> (K - 1)
        for ncw in sorted({1, max(G - 1, 1), G, G + 1, 130}):
            u = rng.integers(0, 2, (ncw, k), dtype=np.uint8)
            got = _hip.to_host(dev.turbo_encode(code, _hip.to_device(u)))
            assert np.array_equal(got, code.encode_host(u)), (K, n_par, k, punct, ncw)
    assert np.array_equal(code.encode(u), code.encode_host(u))
    _hip.device_check()


@pytest.mark.gpu
def test_gpu_encoder_long_codeword_and_every_variable():
    """k = 6144: 256 runs of 24 steps per constituent, the scan over all of them; and a code that sends every variable."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    rng = np.random.default_rng(2)
    for code in (turbo.TurboCode.qpp(6144, 263, 480), send_everything(make_code(5, 2, 300)), make_code(4, 1, 2049)):
        u = rng.integers(0, 2, (3, code.k), dtype=np.uint8)
        assert np.array_equal(_hip.to_host(dev.turbo_encode(code, _hip.to_device(u))), code.encode_host(u)), code.k
    _hip.device_check()


def _check_decode(code, llr, H, rng, scale=1.0, ext_scale=0.75, early_stop=True, with_a1=False, clip=np.inf, stride=None, nulls=False,
                  ref=None):
    """One call against the restatement, bit for bit: bits, post, iters, a1, and ext (H even) including the stride's gaps."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    ncw = llr.shape[0]
    a1 = rng.normal(0, 2.0, (ncw, code.k)).astype(np.float32) if with_a1 else None
    want = decode_restatement(code, llr, H, scale, ext_scale, early_stop, a1, clip)
    tag = (code.K, code.n_par, code.k, code.n_tx, ncw, H, early_stop, with_a1)
    even = H % 2 == 0
    stride = code.n_tx if stride is None else stride
    ext0 = rng.standard_normal((ncw, stride)).astype(np.float32)
    d_ext = _hip.to_device(ext0) if even else None
    d_a1 = None if a1 is None else _hip.to_device(a1)
    out = dev.turbo_decode(code, _hip.to_device(llr), half_iters=H, scale=scale, ext_scale=ext_scale, early_stop=early_stop, a1=d_a1,
                           want_a1=not nulls, ext=d_ext, ext_stride=stride, ext_clip=clip, want_bits=not nulls, want_post=True,
                           want_iters=not nulls, ref_info=None if ref is None else _hip.to_device(ref))
    _hip.device_check()
    assert np.array_equal(_hip.to_host(out["info_post"]).view(np.uint32), want["post"].view(np.uint32)), tag
    if nulls:
        assert out["info_bits"] is None and out["iters"] is None and (out["a1"] is None) == (a1 is None)
    else:
        assert np.array_equal(_hip.to_host(out["info_bits"]), want["bits"]), tag
        assert np.array_equal(_hip.to_host(out["iters"]), want["iters"]), tag
    if out["a1"] is not None:
        assert np.array_equal(_hip.to_host(out["a1"]).view(np.uint32), want["a1"].view(np.uint32)), tag
    if even:
        full = ext0.copy()
        full[:, :code.n_tx] = want["ext"]
        assert np.array_equal(_hip.to_host(d_ext).view(np.uint32), full.view(np.uint32)), tag            # (the stride's gaps included)
    if ref is not None:
        e = (want["bits"] != ref).sum(axis=1)
        assert _hip.to_host(out["counts"]).tolist() == [int(e.sum()), int((e > 0).sum()), int(want["halves"].sum())], tag
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("K", [3, 4, 5])
def test_gpu_decoder_bitwise_equals_the_restatement(K):
    """Mixed batches (clean, noisy and garbage codewords side by side in a wave) over the grid: both n_par, k in 1, 7, 64, 65,
    every ncw, plain AND punctured + permuted; H in 1, 2, 3, 8 (each of them with plain and with punctured codes, for every K,
    n_par and k), the stop rule on and off, with and without d_a1, a scale, a clip, a strided ext and NULL outputs rotate
    through the grid; T around the checkpoint spacing; one k = 1000 code with H = 4; two n_par = 3 codes per K."""
    rng = np.random.default_rng(20 + K)
    geo = _geometry(make_code(K, 1, 8))
    G, C = geo["codewords_per_wave"], geo["checkpoint_steps"]
    nu = K - 1
    ncws = sorted({1, max(G - 1, 1), G, G + 1, 130})
    n = 0
    stopped = open_ = 0
    for n_par in N_PARS:
        for k, ncw, punct in itertools.product((1, 7, 64, 65), ncws, (False, True)):
            code = make_code(K, n_par, k, punct, seed=ncw)
            u, llr = mixed_batch(code, ncw, rng)
            H, early = (1, 2, 3, 8)[(n // 2) % 4], (n // 8) % 2 == 0  # (punct is n % 2: both kinds of code meet every H)
            want = _check_decode(code, llr, H, rng, scale=0.5 if punct else 1.0, ext_scale=(0.75, 1.0, 0.5)[n % 3], early_stop=early,
                                 with_a1=(n // 16) % 2 == 1, clip=3.0 if ncw % 2 else np.inf, stride=code.n_tx + ncw % 3, nulls=n % 5 == 4,
                                 ref=u if n % 3 == 0 else None)
            if H == 8 and early and ncw > 3 and k >= 64:
                stopped += int((want["halves"] < 8).sum())
                open_ += int((want["halves"] == 8).sum())
            n += 1
        for T in (C - 1, C, C + 1, 2 * C + 3):
            code = make_code(K, n_par, T - nu, T % 2 == 0, seed=T)
            assert code.T == T
            u, llr = mixed_batch(code, G + 1, rng)
            _check_decode(code, llr, 4 if T != C else 3, rng, with_a1=T == C + 1, clip=20.0, ref=u)
    assert stopped > 0 and open_ > 0                                  # codewords that stop early beside ones that do not
    code = make_code(K, N_PARS[-1], 1000, K == 4, seed=1)
    u, llr = mixed_batch(code, G + 1, rng)
    want = _check_decode(code, llr, 4, rng, scale=1.7, clip=20.0, ref=u)
    assert want["halves"].min() == 2 and want["halves"].max() == 4
    # n_par = 3 (four outputs per step, the widest LDS rows): plain with an odd H, punctured + permuted with the ext output
    code = make_code(K, 3, 65)
    _check_decode(code, mixed_batch(code, 2 * G + 1, rng)[1], 3, rng, scale=0.8, with_a1=True)
    code = make_code(K, 3, 2 * C + 3 - nu, True, seed=3)
    u, llr = mixed_batch(code, G + 1, rng)
    _check_decode(code, llr, 8, rng, clip=6.0, stride=code.n_tx + 2, ref=u)
    code = send_everything(make_code(K, 1, 33))
    _check_decode(code, mixed_batch(code, G + 2, rng)[1], 4, rng, clip=9.0, stride=code.n_tx + 5)


@pytest.mark.gpu
def test_gpu_one_half_iteration_equals_brute_force():
    from waveforms_amd import _hip

    rng = np.random.default_rng(5)
    for K, n_par, punct in ((3, 1, False), (4, 1, False), (4, 2, True), (5, 2, False), (5, 1, True)):
        code = make_code(K, n_par, 7, punct, seed=K)
        for _ in range(3):
            llr, _A = _integer_case(code, rng)
            out = code.decode(llr[None, :], half_iters=1)
            _Lv, L1, _L2 = channel_values(code, llr)
            want = constituent_brute_force(code, L1[0], np.zeros(7))[:7, 0]
            assert np.array_equal(out["info_post"][0].astype(np.float64), want) and np.array_equal(out["info_bits"][0], (want < 0).astype(np.uint8))
            assert out["iters"].tolist() == [1]
    _hip.device_check()


@pytest.mark.gpu
def test_gpu_all_zero_llrs_and_counts_are_added():
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    rng = np.random.default_rng(31)
    for code in (make_code(3, 1, 100), make_code(4, 2, 50, True), make_code(5, 1, 33)):
        zeros = np.zeros((19, code.n_tx))
        want = decode_restatement(code, zeros, 4, ext_clip=7.0)
        out = code.decode(zeros, half_iters=4, want_ext=True, ext_clip=7.0)
        assert np.isfinite(out["info_post"]).all() and np.isfinite(out["ext"]).all()
        assert np.array_equal(out["info_post"].view(np.uint32), want["post"].view(np.uint32)) and np.array_equal(out["info_bits"], want["bits"])
        assert np.array_equal(out["ext"].view(np.uint32), want["ext"].view(np.uint32)) and np.array_equal(out["iters"], want["iters"])
        # the three counts are ADDED, also with no other output at all
        u, llr = mixed_batch(code, 37, rng)
        want = decode_restatement(code, llr, 6)
        e = (want["bits"] != u).sum(axis=1)
        assert e.sum() > 0
        d_llr, d_u, counts = _hip.to_device(llr), _hip.to_device(u), None
        for _rep in range(3):
            counts = dev.turbo_decode(code, d_llr, half_iters=6, ref_info=d_u, counts=counts, want_bits=False, want_post=False,
                                      want_iters=False)["counts"]
        assert _hip.to_host(counts).tolist() == [3 * int(e.sum()), 3 * int((e > 0).sum()), 3 * int(want["halves"].sum())]
    _hip.device_check()


@pytest.mark.gpu
def test_gpu_decode_in_several_launches():
    """More waves than one launch takes (64 per compute unit): the call slices the batch, every slice with its own pointers."""
    from waveforms_amd import _hip

    code = make_code(5, 1, 1)                                         # four codewords per wave, T = 5
    cus = _hip.torch().cuda.get_device_properties(0).multi_processor_count
    ncw = 4 * 64 * cus + 5
    assert _geometry(code, ncw)["waves"] > 64 * cus
    rng = np.random.default_rng(8)
    u, llr = mixed_batch(code, ncw, rng)
    _check_decode(code, llr, 4, rng, with_a1=True, clip=4.0, stride=code.n_tx + 1, ref=u)
    _hip.device_check()
