"""The SOQPSK 4-state detectors under exact ties and under rows whose survivors never merge.

Every 4-state detector here is chunk-parallel: it re-derives its metrics over a warm-up, proves every chunk boundary bitwise
and repairs what fails, round after round (wf_viterbi4.h: vit_fixup_verify / vit_fixup_rounds; the soft directions and the
live windows keep records of their own).  The rest of the suite feeds them Gaussian-noise rows, which never tie and merge
within a few rows.  The row families of this module are the two cases noise does not reach:

  grid        integer-grid rows (components in -2 .. 2): every sum is exact and an eighth of the ACS compares tie
  gaps        noise with two runs of all-zero rows (a squelched front end): inside a gap EVERY compare ties
  zeros       all +0.0, all -0.0 and a random mixture of the two
  perm        test_cascade's survivor-permutation rows: no chunk derived from zeros ever meets the true metrics, in either
              direction, so every repair hands on and a cascade runs through the whole burst
  perm_exact  the same with rows [9:] rounded to multiples of 8: forward nothing merges, backward everything is equal from
              the first row on, so exactly one direction cascades

The tie rule is the reference's list order (strict '<', the first arg-min: waveforms/viterbi/algorithm.py:79-83, :92); the
hard decisions are checked against the sequential oracle (pinned here to the reference's own iteration() on tie rows through
tests/golden/detect_ties.npz), the soft outputs bitwise against the sequential restatements of tests/test_soft_detector.py
and tests/test_idd.py.  What a repair counter must at least show is derived on the host: ``soft_chunk_sim`` and
``window_chunk_sim`` run every chunk the way the first launch does (from zeros over the warm-up) and the way the sequential
detector does, and count the boundaries that differ.  No bound comes from what a GPU printed.
"""
import numpy as np
import pytest

import test_cascade as TC
import test_idd as TI
import test_soft_detector as TS

INF = float("inf")


# ------------------------------------------------------------------------------------------------ row families
def grid_rows(n):
    rng = np.random.default_rng(1)
    re = rng.integers(-2, 3, (n, 3))
    im = rng.integers(-2, 3, (n, 3))
    return re + 1j * im


def gaps_rows(n):
    rng = np.random.default_rng(2)
    rows = 2.0 * (rng.standard_normal((n, 3)) + 1j * rng.standard_normal((n, 3)))
    rows[300:900] = 0
    rows[1200:1210] = 0
    return rows


def zeros_rows(n):
    """name -> burst: all +0.0, all -0.0, a random mixture of the two in every component."""
    pos = np.zeros((n, 3), dtype=np.complex128)
    neg = (-np.zeros((n, 3, 2))).view(np.complex128).reshape(n, 3)
    mix = np.where(np.random.default_rng(3).integers(0, 2, (n, 3, 2)) == 1, -0.0, 0.0).view(np.complex128).reshape(n, 3)
    assert np.signbit(neg.view(np.float64)).all() and 0 < np.signbit(mix.view(np.float64)).sum() < 6 * n
    return {"+0": pos, "-0": neg, "mixed": mix}


def perm_rows(n):
    return TC._survivor_permutation_rows(n, True)


def perm_exact_rows(n):
    rows = perm_rows(n).copy()
    v = rows[9:].view(np.float64)
    v[...] = np.round(v / 8.0) * 8.0
    return rows


def family(name, n):
    return {"grid": grid_rows, "gaps": gaps_rows, "perm": perm_rows, "perm_exact": perm_exact_rows}[name](n)


def tie_priors(n, seed=7):
    """Integer-valued float32 priors in ±12 (λ + π ties and lands on exactly 0), a tenth of the rows saturated at ±50."""
    rng = np.random.default_rng(seed)
    p = rng.integers(-12, 13, n).astype(np.float32)
    sat = rng.integers(0, 10, n) == 0
    p[sat] = np.where(rng.integers(0, 2, int(sat.sum())) == 1, np.float32(-50.0), np.float32(50.0))
    return p


def small_priors(n, seed=9):
    """float32 priors in ±3: with the scale 0.7 the tests use, |scale·π| <= 2.1 (what the never-merging rows tolerate)."""
    return np.random.default_rng(seed).uniform(-3.0, 3.0, n).astype(np.float32)


# ------------------------------------------------------------------------------------------------ host chunk simulation
class SoftSteps:
    """The soft recursions' single steps, sequential float64 in the header's order of operations (wf_viterbi_soft.h: soft_fwd,
    soft_bwd, soft_llr).  ``prior`` None is the plain detector: no addition of π anywhere."""

    def __init__(self, oracle, rows, differential, prior=None, scale=1.0):
        self.brs = TS._branches(oracle, differential)
        self.inc = TS._increments(oracle, rows, differential).tolist()
        self.n = len(self.inc)
        self.pi = None if prior is None else (np.float64(scale) * np.asarray(prior, dtype=np.float32).astype(np.float64)).tolist()

    def _inc(self, k, b, i):
        return self.inc[k][b] + self.pi[k] if (i and self.pi is not None) else self.inc[k][b]

    def fwd(self, a, k):
        new = [INF, INF, INF, INF]
        for (b, s, e, i, _x) in self.brs[k & 1]:
            v = a[s] + self._inc(k, b, i)
            if v < new[e]:
                new[e] = v
        mn = min(new)
        return [v - mn for v in new]

    def bwd(self, bt, k):
        new = [INF, INF, INF, INF]
        for (b, s, e, i, _x) in self.brs[k & 1]:
            v = self._inc(k, b, i) + bt[e]
            if v < new[s]:
                new[s] = v
        mn = min(new)
        return [v - mn for v in new]

    def lam(self, a, bt, k):
        m = [INF, INF]
        for (b, s, e, i, _x) in self.brs[k & 1]:
            t = (a[s] + self.inc[k][b]) + bt[e]
            if t < m[i]:
                m[i] = t
        return m[1] - m[0]

    def forward_ties(self):
        """(ACS compares of the forward recursion whose two candidates are equal, compares in all)."""
        a, ties = [0.0] * 4, 0
        for k in range(self.n):
            cand = [[], [], [], []]
            for (b, s, e, i, _x) in self.brs[k & 1]:
                cand[e].append(a[s] + self._inc(k, b, i))
            ties += sum(1 for c in cand if c[0] == c[1])
            a = self.fwd(a, k)
        return ties, 4 * self.n


def _u64(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def soft_chunk_sim(steps, ch, warmup, backward, lo=0, hi=None):
    """Every chunk of rows [lo, hi) cut into pieces of ``ch`` from lo, one direction, as wf_viterbi_soft.h walks it
    (soft_bounds_body): the start derived from zeros ``warmup`` rows away (exact where that reaches the edge), the end the
    chunk's own rows then give, and the sequential metrics at both places.  Records in the order a repair cascades: chunk 0
    first forward, the LAST chunk first backward (the kernel's mirrored records).  -> dict of uint64[nch, 4] arrays
    start0, end0 (derived from zeros) and start, end (sequential)."""
    hi = steps.n if hi is None else hi
    nch = (hi - lo + ch - 1) // ch
    seq = {}
    if backward:
        m = [0.0] * 4
        seq[hi] = m
        for k in range(hi - 1, lo - 1, -1):
            m = steps.bwd(m, k)
            seq[k] = m
    else:
        m = [0.0] * 4
        seq[lo] = m
        for k in range(lo, hi):
            m = steps.fwd(m, k)
            seq[k + 1] = m
    start0, end0, start, end = [], [], [], []
    for r in range(nch):
        c = nch - 1 - r if backward else r
        a, e = lo + c * ch, min(lo + (c + 1) * ch, hi)
        m = [0.0] * 4
        if backward:
            for k in range(min(e + warmup, hi) - 1, e - 1, -1):
                m = steps.bwd(m, k)
            start0.append(m)
            for k in range(e - 1, a - 1, -1):
                m = steps.bwd(m, k)
            start.append(seq[e]), end.append(seq[a])
        else:
            for k in range(max(a - warmup, lo), a):
                m = steps.fwd(m, k)
            start0.append(m)
            for k in range(a, e):
                m = steps.fwd(m, k)
            start.append(seq[a]), end.append(seq[e])
        end0.append(m)
    return {k: _u64(v).reshape(nch, 4) for k, v in (("start0", start0), ("end0", end0), ("start", start), ("end", end))}


def _rows_differ(x, y):
    return (x != y).any(axis=1)


def sim_counts(sim):
    """From a chunk simulation -> dict:
    unmerged   records r >= 1 whose start derived from zeros is not the sequential value (a boundary that did not merge)
    unproven   records r >= 1 whose start is not the predecessor's RECORDED end: what the proof lists first, and what it
               counts when the repairs are off
    must_hand_on  records r >= 1 whose end differs once run from the true start: each is repaired at least once with a
               changed end, so the cascade counter is at least this
    interior   records r >= 1"""
    return {"unmerged": int(_rows_differ(sim["start0"][1:], sim["start"][1:]).sum()),
            "unproven": int(_rows_differ(sim["start0"][1:], sim["end0"][:-1]).sum()),
            "must_hand_on": int(_rows_differ(sim["end0"][1:], sim["end"][1:]).sum()),
            "interior": int(sim["start0"].shape[0] - 1)}


def sim_lambda(steps):
    """λ of the whole burst from the step functions alone: one chunk that covers the burst."""
    n = steps.n
    alpha = [[0.0] * 4]
    for k in range(n):
        alpha.append(steps.fwd(alpha[-1], k))
    lam, bt = np.empty(n), [0.0] * 4
    for k in range(n - 1, -1, -1):
        lam[k] = steps.lam(alpha[k], bt, k)
        bt = steps.bwd(bt, k)
    return lam


def window_geometry(n, warmup):
    """(chunk length, warm-up rows) of wf_viterbi4_detect_window for a burst of n rows — the rule stated at its launch site
    (wf_viterbi.hip): W = the warm-up (default 32) rounded up to even; calls per lane = ceil(n / 131072) rounded up to even,
    but at least 4·W."""
    W = warmup if warmup else 32
    W = min((W + 1) // 2 * 2, 4096)
    ch = (n + 131071) // 131072
    ch = (ch + 1) // 2 * 2
    return max(ch, 4 * W), W


def window_chunk_sim(oracle, rows, L, differential, warmup):
    """The window detector's carried metrics C at every chunk boundary, as ``soft_chunk_sim`` (forward only).  One call k of
    the reference (algorithm.py:65-87, stage j = 0): C' = ACS over the branches of section (k - 1) % 2 of (C - min C) with
    the increments of row k - L + 1, which that row got BY LIST POSITION from section (k - L + 1) % 2; rows before the burst
    are zeros; L = 1 updates the metrics in place, state by state."""
    brs = TS._branches(oracle, differential)
    inc = TS._increments(oracle, rows, differential).tolist()
    n = len(inc)
    ch, W = window_geometry(n, warmup)
    zero8 = [0.0] * 8

    def step(C, k):
        mn = min(C)
        m = [c - mn for c in C]
        ik = inc[k - L + 1] if k - L + 1 >= 0 else zero8
        new = m if L == 1 else [INF] * 4
        for st in range(4):
            best = INF
            for (b, s, e, _i, _x) in brs[(k - 1) & 1]:
                if e != st:
                    continue
                v = m[s] + ik[b]
                if v < best:
                    best = v
            new[st] = best
        return new

    seq = [[0.0] * 4]
    for k in range(n):
        seq.append(step(seq[-1], k))
    nch = (n + ch - 1) // ch
    start0, end0, start, end = [], [], [], []
    for c in range(nch):
        a, e = c * ch, min((c + 1) * ch, n)
        C = [0.0] * 4
        for k in range(0 if a <= W else a - W, a):
            C = step(C, k)
        start0.append(C)
        for k in range(a, e):
            C = step(C, k)
        end0.append(C), start.append(seq[a]), end.append(seq[e])
    return {k: _u64(v).reshape(nch, 4) for k, v in (("start0", start0), ("end0", end0), ("start", start), ("end", end))}


# ------------------------------------------------------------------------------------------------ CPU
N_SOFT = 2001
SOFT_CASCADE = [(16, 2), (16, 32)]                            # (chunk, warm-up) of the soft cascade tests below
WINDOW_LENGTHS = (1, 2, 3, 17, 64)
N_WINDOW = 4001


@pytest.mark.parametrize("differential", [True, False])
def test_simulation_steps_are_the_restatements(oracle, differential):
    """The simulation's step functions over one chunk that covers the burst give bitwise the restatements' λ, plain and
    with a prior, on tie rows and on never-merging rows; and one chunk covering the burst is exact in the chunk
    simulation."""
    n = 300
    for rows in (grid_rows(n), gaps_rows(1300)[850:1250], perm_rows(n)):
        want, _ = TS.soft_restatement(oracle, rows, differential)
        steps = SoftSteps(oracle, rows, differential)
        assert np.array_equal(sim_lambda(steps).view(np.uint64), want.view(np.uint64))
        prior = tie_priors(len(rows))
        want, _ = TI.apriori_restatement(oracle, rows, prior, 0.7, differential)
        steps = SoftSteps(oracle, rows, differential, prior, 0.7)
        assert np.array_equal(sim_lambda(steps).view(np.uint64), want.view(np.uint64))
        for backward in (False, True):
            whole = soft_chunk_sim(steps, len(rows), 5, backward)
            assert sim_counts(whole) == {"unmerged": 0, "unproven": 0, "must_hand_on": 0, "interior": 0}
            cut = soft_chunk_sim(steps, 16, 4096, backward)     # a warm-up that always reaches the edge: every start exact
            c = sim_counts(cut)
            assert (c["unmerged"], c["unproven"], c["must_hand_on"]) == (0, 0, 0) and c["interior"] == (len(rows) + 15) // 16 - 1
            assert np.array_equal(cut["end0"][-1], whole["end0"][0])


@pytest.mark.parametrize("differential", [True, False])
@pytest.mark.parametrize("name", ["grid", "gaps"])
def test_tie_families_tie(oracle, name, differential):
    """Conditions the GPU tests rely on, n = 2001: at least 10 % of the forward ACS compares tie and at least 100 rows
    have λ = 0 exactly (all of them +0).  Measured: grid 1011 of 8004 compares (12.6 %), λ = 0 on 441 rows (differential)
    and 303 (plain); gaps 2424 of 8004 (30.3 %), λ = 0 on 610 and 606 rows.  With the integer priors of ``tie_priors``
    λᵉ + π = 0 on some rows as well, where ``bits`` must be 0 (grid: 88 differential, 75 plain; gaps: 14 and 14)."""
    rows = family(name, N_SOFT)
    steps = SoftSteps(oracle, rows, differential)
    ties, compares = steps.forward_ties()
    lam, _ = TS.soft_restatement(oracle, rows, differential)
    zero = int((lam == 0).sum())
    prior = tie_priors(N_SOFT)
    ext, _ = TI.apriori_restatement(oracle, rows, prior, 1.0, differential)
    on_zero = int(((ext + prior.astype(np.float64)) == 0).sum())
    print(f"{name} differential={differential}: {ties} of {compares} forward compares tie, λ = 0 on {zero} rows, λ + π = 0 on {on_zero}")
    assert 10 * ties >= compares
    assert zero >= 100
    assert not np.signbit(lam[lam == 0]).any()
    assert on_zero >= 10


@pytest.mark.parametrize("differential", [True, False])
@pytest.mark.parametrize("with_prior", [False, True])
def test_perm_families_never_merge(oracle, differential, with_prior):
    """n = 2001, chunks of 16 (126 chunks, 125 interior boundaries), warm-ups 2 and 32, with and without the small prior:
    on ``perm`` every interior boundary is unmerged in both directions but for at most 2 next to the burst's ends (measured:
    123 to 125 of 125), and every such chunk's end but at most one differs once run from the true start (122 to 125); on
    ``perm_exact`` the same forward and NONE backward (measured: 0).  On ``perm_exact`` the chunks derived from zeros agree
    with EACH OTHER though not with the sequential metrics: with the repairs off the proof fails at the first boundary only
    (unproven 1), and the repairs then walk the whole burst, one chunk per round.  A prior makes ``perm_exact`` behave as
    ``perm``."""
    prior = small_priors(N_SOFT) if with_prior else None
    for name in ("perm", "perm_exact"):
        steps = SoftSteps(oracle, family(name, N_SOFT), differential, prior, 0.7)
        for ch, warmup in SOFT_CASCADE:
            f = sim_counts(soft_chunk_sim(steps, ch, warmup, False))
            b = sim_counts(soft_chunk_sim(steps, ch, warmup, True))
            print(name, differential, with_prior, ch, warmup, "forward", f, "backward", b)
            assert f["interior"] == b["interior"] == 125
            assert f["unmerged"] >= 123 and f["must_hand_on"] >= f["unmerged"] - 1 and f["unproven"] >= 1
            if name == "perm" or with_prior:
                assert f["unproven"] >= 123
                assert b["unmerged"] >= 123 and b["must_hand_on"] >= b["unmerged"] - 1 and b["unproven"] >= 123
            else:
                assert (b["unmerged"], b["unproven"], b["must_hand_on"]) == (0, 0, 0)


@pytest.mark.parametrize("differential", [True, False])
def test_perm_never_merges_in_the_window_detector(oracle, differential):
    """n = 4001, a warm-up of 2 (chunks of 8: 500 interior boundaries) and the default (chunks of 128: 31).  At L = 2, 3, 17
    and 64 the window detector's carried metrics derived from zeros differ from the sequential ones at every interior
    boundary but those whose chunk lies in the first L + 8 calls (the first L - 1 calls consume the zero history, the next 9
    the random rows) and at most 2 more, and every such chunk's end but at most one differs once run from the true start.
    Measured, either trellis: warm-up 2: 500, 500, 498, 492 of 500 unmerged and 500, 499, 498, 492 ends; default: 31 of 31.
    L = 1 is NOT such a case: its stage updates the metrics in place, state by state, and the permutation is lost — all 500
    starts derived over 2 rows differ, but only 1 end does, and the default warm-up merges everywhere."""
    rows = perm_rows(N_WINDOW)
    for L in WINDOW_LENGTHS:
        for warmup in (2, 0):
            c = sim_counts(window_chunk_sim(oracle, rows, L, differential, warmup))
            print(L, differential, warmup, c)
            assert c["interior"] == (500 if warmup else 31)
            if L > 1:
                ch, _w = window_geometry(N_WINDOW, warmup)
                assert c["unmerged"] >= c["interior"] - (L + 8) // ch - 2 and c["must_hand_on"] >= c["unmerged"] - 1


def ties_golden_rows(g):
    return g["rows_ri"][..., 0].astype(np.float64) + 1j * g["rows_ri"][..., 1].astype(np.float64)


def test_oracle_equals_reference_on_tie_rows(oracle, golden):
    """tests/golden/detect_ties.npz: 1500 grid rows with a 300-row zero gap and element [0] of what the reference's own
    SOQPSKTrellisDetector.iteration returned for them (make_detect_ties_golden.py).  The sequential oracle — the yardstick
    of the GPU tests below — breaks every tie the way the reference does."""
    g = golden("detect_ties")
    rows = ties_golden_rows(g)
    assert rows.shape == (1500, 3) and np.array_equal(rows[:600], grid_rows(1500)[:600]) and not rows[600:900].any()
    for L in g["lengths"].tolist():
        for diff in (True, False):
            b, s = oracle.viterbi_detect(rows, L, diff)
            assert np.array_equal(b, g[f"L{L}_diff{int(diff)}_bits0"]), (L, diff)
            assert np.array_equal(s, g[f"L{L}_diff{int(diff)}_syms0"]), (L, diff)


# ------------------------------------------------------------------------------------------------ GPU
HARD_LENGTHS = (1, 2, 3, 8, 17, 64)
N_HARD = 20_001


@pytest.fixture
def soft_ctx():
    from waveforms_amd import _hip

    ctx = _hip.new_ctx()
    _hip.set_option(ctx, _hip.WF_OPT_DET_FINAL_VERIFY, 1)
    yield ctx
    _hip.free_ctx(ctx)


def _reset(dev, ctx=None):
    return (dev.viterbi_unmerged(reset=True, ctx=ctx), dev.viterbi_repaired(reset=True, ctx=ctx), dev.viterbi_cascaded(reset=True, ctx=ctx))


def _first_diff(got, want):
    d = np.flatnonzero(np.asarray(got) != np.asarray(want))
    return f"{d.size} differences, first at {d[:4].tolist()}"


def _hard_entry_points(dev, _hip, d_rows, L, diff, warmup):
    """(name, bits, syms) of every batch entry point that serves window length L, each run when it is asked for."""
    if L == 2:
        b, s = dev.viterbi_detect(d_rows, differential=diff, warmup=warmup)
        yield "batch", _hip.to_host(b), _hip.to_host(s)
    b, s = dev.viterbi_detect_window(d_rows, L, diff, warmup=warmup)
    yield "window", _hip.to_host(b), _hip.to_host(s)


def _check_hard(oracle, dev, _hip, rows, what, expect_repairs, want=None):
    from waveforms.viterbi.algorithm import SOQPSKTrellisDetector

    n = rows.shape[0]
    d_rows = _hip.to_device(rows)
    cuts = [0, 1, 78, n // 4 | 1, n // 2 & ~1, n - 3, n]       # pieces that start at odd and at even offsets
    for L in HARD_LENGTHS:
        for diff in (True, False):
            want_b, want_s = want(L, diff) if want else oracle.viterbi_detect(rows, L, diff)
            for warmup in (0, 2):
                _reset(dev)
                for name, b, s in _hard_entry_points(dev, _hip, d_rows, L, diff, warmup):
                    unproven, repaired, handed_on = _reset(dev)
                    tag = (what, name, L, diff, warmup, f"repaired {repaired}, handed on {handed_on}")
                    assert unproven == 0, tag
                    assert np.array_equal(b, want_b), (tag, _first_diff(b, want_b))
                    assert np.array_equal(s, want_s), (tag, _first_diff(s, want_s))
                    if warmup == 2 and expect_repairs:
                        assert repaired > 0, tag
            det = SOQPSKTrellisDetector(L, differantial_encoding=diff)
            parts = [det.detect(rows[a:b], warmup=2) for a, b in zip(cuts[:-1], cuts[1:])]     # (raises if anything is unproven)
            got_b, got_s = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
            assert np.array_equal(got_b, want_b), (what, "pieces", L, diff, _first_diff(got_b, want_b))
            assert np.array_equal(got_s, want_s), (what, "pieces", L, diff, _first_diff(got_s, want_s))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["grid", "gaps", "zeros", "golden"])
def test_gpu_hard_decisions_under_ties(oracle, golden, ctx_options, name):
    """The length-2 batch detector and the window detector at L = 1, 2, 3, 8, 17, 64, both trellises, the default warm-up
    and a warm-up of 2 (which must run repairs on tie rows), in one burst and through the object API in pieces cut at odd
    and even offsets: the sequential oracle's decisions, nothing unproven."""
    from waveforms_amd import _hip, device as dev

    with ctx_options(WF_OPT_DET_FINAL_VERIFY=1):
        if name == "zeros":
            for sign, rows in zeros_rows(N_HARD).items():
                _check_hard(oracle, dev, _hip, rows, f"zeros {sign}", False)
        elif name == "golden":
            g = golden("detect_ties")
            _check_hard(oracle, dev, _hip, ties_golden_rows(g), name, False,
                        want=lambda L, diff: (g[f"L{L}_diff{int(diff)}_bits0"], g[f"L{L}_diff{int(diff)}_syms0"]))
        else:
            _check_hard(oracle, dev, _hip, family(name, N_HARD), name, True)


@pytest.mark.gpu
@pytest.mark.parametrize("diff", [True, False])
def test_gpu_window_detector_cascades_through_every_chunk(oracle, ctx_options, diff):
    """vwin_fixup_kernel under a sustained cascade: ``perm`` rows, n = 4001, a warm-up of 2 (chunks of 8) and the default
    (chunks of 128): every repair re-runs its chunk through the LDS ring and hands on.  Decisions == the oracle; the
    cascade counter is at least what the host simulation requires; in two bursts cut inside the permutation rows the last
    chunk's repaired end reaches the carry (the second burst's decisions depend on it)."""
    from waveforms.viterbi.algorithm import SOQPSKTrellisDetector
    from waveforms_amd import _hip, device as dev

    rows = perm_rows(N_WINDOW)
    d_rows = _hip.to_device(rows)
    with ctx_options(WF_OPT_DET_FINAL_VERIFY=1):
        for L in WINDOW_LENGTHS:
            want_b, want_s = oracle.viterbi_detect(rows, L, diff)
            for warmup in (2, 0):
                c = sim_counts(window_chunk_sim(oracle, rows, L, diff, warmup))
                _reset(dev)
                b, s = dev.viterbi_detect_window(d_rows, L, diff, warmup=warmup)
                b, s = _hip.to_host(b), _hip.to_host(s)
                unproven, repaired, handed_on = _reset(dev)
                tag = (f"L {L} diff {diff} warm-up {warmup}: repaired {repaired}, handed on {handed_on}; host simulation: {c}")
                print(tag)
                assert unproven == 0, tag
                assert np.array_equal(b, want_b), (tag, _first_diff(b, want_b))
                assert np.array_equal(s, want_s), (tag, _first_diff(s, want_s))
                assert repaired >= c["unproven"], tag
                assert handed_on >= c["must_hand_on"], tag
                if L > 1:                                      # (never merging at these lengths: the CPU test above)
                    assert handed_on >= c["unmerged"] - 1, tag
                for cut in (2017, 2018):
                    det = SOQPSKTrellisDetector(L, differantial_encoding=diff)
                    p0, p1 = det.detect(rows[:cut], warmup=warmup), det.detect(rows[cut:], warmup=warmup)
                    got_b, got_s = np.concatenate([p0[0], p1[0]]), np.concatenate([p0[1], p1[1]])
                    assert np.array_equal(got_b, want_b), (tag, cut, _first_diff(got_b, want_b))
                    assert np.array_equal(got_s, want_s), (tag, cut, _first_diff(got_s, want_s))


def _soft_call(dev, _hip, ctx, d_rows, rb, prior, d_prior, scale, differential, warmup):
    if prior is None:
        out, bits = dev.viterbi_soft(d_rows, differential, warmup, rb, ctx=ctx)
    else:
        out, bits = dev.viterbi_soft_apriori(d_rows, d_prior, scale, differential, warmup, rb, ctx=ctx)
    return _hip.to_host(out), _hip.to_host(bits)


def _want_soft(oracle, rows, prior, scale, differential):
    if prior is None:
        return TS.soft_restatement(oracle, rows, differential)
    return TI.apriori_restatement(oracle, rows, prior, scale, differential)


def _check_soft_ties(oracle, soft_ctx, rows, prior, scale, differential, what):
    from waveforms_amd import _hip, device as dev

    want, want_bits = _want_soft(oracle, rows, prior, scale, differential)
    assert not np.signbit(want[want == 0]).any()
    forms = ((48, _hip.to_device(rows)), (32, _hip.to_device(TS.pack_rows(rows))))
    d_prior = None if prior is None else _hip.to_device(prior)
    _reset(dev, soft_ctx)
    seen_repairs = 0
    for chunk in (0, 1, 7, 16, 64):
        _hip.set_option(soft_ctx, _hip.WF_OPT_SOFT_CHUNK_CALLS, chunk)
        for warmup in (0, 2, 16):
            for rb, d_rows in forms:
                got, bits = _soft_call(dev, _hip, soft_ctx, d_rows, rb, prior, d_prior, scale, differential, warmup)
                unproven, repaired, _h = _reset(dev, soft_ctx)
                tag = (what, differential, chunk, warmup, rb, f"repaired {repaired}")
                assert unproven == 0, tag
                assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (tag, _first_diff(got.view(np.uint64), want.view(np.uint64)))
                assert np.array_equal(bits, want_bits), (tag, _first_diff(bits, want_bits))
                seen_repairs += repaired
    return seen_repairs


@pytest.mark.gpu
@pytest.mark.parametrize("differential", [True, False])
@pytest.mark.parametrize("apriori", [False, True])
@pytest.mark.parametrize("name", ["grid", "gaps", "zeros"])
def test_gpu_soft_outputs_under_ties(oracle, soft_ctx, name, apriori, differential):
    """wf_viterbi4_soft and wf_viterbi4_soft_apriori on tie rows, n = 2001: bitwise the restatement (λ = 0 as +0) at chunks
    of the library's choice, 1, 7, 16 and 64 rows, warm-ups 0 (default), 2 and 16, both row forms."""
    prior = tie_priors(N_SOFT) if apriori else None
    if name == "zeros":
        for sign, rows in zeros_rows(N_SOFT).items():
            _check_soft_ties(oracle, soft_ctx, rows, prior, 1.0, differential, f"zeros {sign}")
    else:
        _check_soft_ties(oracle, soft_ctx, family(name, N_SOFT), prior, 1.0, differential, name)


@pytest.mark.gpu
@pytest.mark.parametrize("differential", [True, False])
@pytest.mark.parametrize("apriori", [False, True])
@pytest.mark.parametrize("name", ["perm", "perm_exact"])
def test_gpu_soft_cascades_in_both_directions(oracle, soft_ctx, name, apriori, differential):
    """The soft detectors' repairs under rows that never merge, chunks of 16, warm-ups 2 and 32.  With the repairs off the
    unproven count is EXACTLY the simulated number of boundaries whose start is not the predecessor's recorded end, both
    directions summed; with the repairs on the result is the restatement and the cascade counter is at least the simulated
    number of chunks whose end differs once run from the true start.  ``perm_exact`` (plain form) cascades forward only."""
    from waveforms_amd import _hip, device as dev

    n = N_SOFT
    rows = family(name, n)
    prior, scale = (small_priors(n), 0.7) if apriori else (None, 1.0)
    want, want_bits = _want_soft(oracle, rows, prior, scale, differential)
    steps = SoftSteps(oracle, rows, differential, prior, scale)
    d_prior = None if prior is None else _hip.to_device(prior)
    forms = ((48, _hip.to_device(rows)), (32, _hip.to_device(TS.pack_rows(rows))))
    for chunk, warmup in SOFT_CASCADE:
        _hip.set_option(soft_ctx, _hip.WF_OPT_SOFT_CHUNK_CALLS, chunk)
        g = dev.viterbi_soft_geometry(n, warmup, ctx=soft_ctx)
        assert g["chunk_calls"] == chunk and g["lanes"] == (n + chunk - 1) // chunk and g["warmup"] == warmup
        f = sim_counts(soft_chunk_sim(steps, g["chunk_calls"], g["warmup"], False))
        b = sim_counts(soft_chunk_sim(steps, g["chunk_calls"], g["warmup"], True))
        assert f["interior"] == g["lanes"] - 1
        if name == "perm_exact" and not apriori:
            assert f["must_hand_on"] >= 122 and b == {"unmerged": 0, "unproven": 0, "must_hand_on": 0, "interior": f["interior"]}
        for rb, d_rows in forms:
            _hip.set_option(soft_ctx, _hip.WF_OPT_DET_REPAIR, 1)
            _reset(dev, soft_ctx)
            _soft_call(dev, _hip, soft_ctx, d_rows, rb, prior, d_prior, scale, differential, warmup)
            unproven, repaired, handed_on = _reset(dev, soft_ctx)
            _hip.set_option(soft_ctx, _hip.WF_OPT_DET_REPAIR, 0)
            tag = f"{name} apriori {apriori} differential {differential} chunk {chunk} warm-up {warmup} rows of {rb} B: "
            off = f"repairs off: unproven {unproven}; host simulation: forward {f}, backward {b}"
            assert unproven == f["unproven"] + b["unproven"] and repaired == 0 and handed_on == 0, tag + off
            got, bits = _soft_call(dev, _hip, soft_ctx, d_rows, rb, prior, d_prior, scale, differential, warmup)
            unproven, repaired, handed_on = _reset(dev, soft_ctx)
            on = f"repairs on: unproven {unproven}, repaired {repaired}, handed on {handed_on}; " + off
            print(tag + on)
            assert unproven == 0, tag + on
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (tag + on, _first_diff(got.view(np.uint64), want.view(np.uint64)))
            assert np.array_equal(bits, want_bits), (tag + on, _first_diff(bits, want_bits))
            assert repaired >= f["unproven"] + b["unproven"], tag + on
            assert handed_on >= f["must_hand_on"] + b["must_hand_on"], tag + on


LIVE_WINDOWS = [(0, 16), (20, 21), (24, 34), (40, 90), (92, 140), (200, 1200), (1500, N_SOFT)]
SENTINEL_EXT, SENTINEL_BIT = -4321.5, 93


@pytest.mark.gpu
@pytest.mark.parametrize("differential", [True, False])
@pytest.mark.parametrize("name", ["perm", "grid"])
def test_gpu_live_windows_equal_the_definition(oracle, soft_ctx, name, differential):
    """wf_viterbi4_soft_apriori_windows against the HOST restatement of every slice (not against the burst kernel), chunks
    of 16, warm-ups 2 and 32: a window of one chunk, windows shorter than the warm-up (1 and 10 rows), two windows two rows
    apart, one of 1000 rows (63 chunks) and one that ends at n.  Rows outside every window keep their sentinel.  On ``perm``
    the repair counters are at least the sum over the windows of the simulated per-window counts: a cascade that crossed a
    window's edge or skipped a window's first or last chunk shows as a wrong λ or as an unproven boundary."""
    from waveforms_amd import _hip, device as dev

    torch = _hip.torch()
    n = N_SOFT
    rows = family(name, n)
    prior, scale = (small_priors(n), 0.7) if name == "perm" else (tie_priors(n), 1.0)
    steps = SoftSteps(oracle, rows, differential, prior, scale)
    want = [TI.apriori_restatement(oracle, rows[s:e], prior[s:e], scale, differential) for s, e in LIVE_WINDOWS]
    table = np.zeros(4 + 2 * (len(LIVE_WINDOWS) + 2), dtype=np.int64)
    table[0], table[1] = len(LIVE_WINDOWS), sum(e - s for s, e in LIVE_WINDOWS)
    table[4:4 + 2 * len(LIVE_WINDOWS)] = np.array(LIVE_WINDOWS).reshape(-1)
    d_table, d_prior = _hip.to_device(table), _hip.to_device(prior)
    forms = ((48, _hip.to_device(rows)), (32, _hip.to_device(TS.pack_rows(rows))))
    outside = np.ones(n, dtype=bool)
    for s, e in LIVE_WINDOWS:
        assert s % 2 == 0
        outside[s:e] = False
    assert (LIVE_WINDOWS[5][1] - LIVE_WINDOWS[5][0] + 15) // 16 >= 60 and LIVE_WINDOWS[4][0] - LIVE_WINDOWS[3][1] == 2
    _hip.set_option(soft_ctx, _hip.WF_OPT_SOFT_CHUNK_CALLS, 16)
    for warmup in (2, 32):
        need = {"unproven": 0, "must_hand_on": 0}
        for s, e in LIVE_WINDOWS:
            for backward in (False, True):
                c = sim_counts(soft_chunk_sim(steps, 16, warmup, backward, s, e))
                need["unproven"] += c["unproven"]
                need["must_hand_on"] += c["must_hand_on"]
        if name == "perm":
            assert need["must_hand_on"] >= 100                 # (the long window alone has 62 interior boundaries per direction)
        for rb, d_rows in forms:
            ext = torch.full((n,), SENTINEL_EXT, dtype=torch.float64, device="cuda")
            bits = torch.full((n + 16,), SENTINEL_BIT, dtype=torch.uint8, device="cuda")
            _reset(dev, soft_ctx)
            dev.viterbi_soft_apriori_windows(d_rows, d_prior, d_table, scale, differential, warmup, rb, ctx=soft_ctx, out=(ext, bits))
            unproven, repaired, handed_on = _reset(dev, soft_ctx)
            _hip.check(_hip.lib().wf_ctx_check(soft_ctx, _hip.stream()))
            tag = (f"{name} differential {differential} warm-up {warmup} rows of {rb} B: unproven {unproven}, repaired {repaired}, "
                   f"handed on {handed_on}; host simulation, summed over the windows: {need}")
            print(tag)
            ext, bits = _hip.to_host(ext), _hip.to_host(bits)
            assert unproven == 0, tag
            for (s, e), (w_ext, w_bits) in zip(LIVE_WINDOWS, want):
                assert np.array_equal(ext[s:e].view(np.uint64), w_ext.view(np.uint64)), (tag, s, e, _first_diff(ext[s:e].view(np.uint64), w_ext.view(np.uint64)))
                assert np.array_equal(bits[s:e], w_bits), (tag, s, e, _first_diff(bits[s:e], w_bits))
            assert (ext[outside] == SENTINEL_EXT).all() and (bits[:n][outside] == SENTINEL_BIT).all() and (bits[n:] == SENTINEL_BIT).all(), tag
            assert repaired >= need["unproven"] and handed_on >= need["must_hand_on"], tag
