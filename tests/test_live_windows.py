"""The iterative SOQPSK loop's detector on the open codewords only: wf_idd_windows, wf_viterbi4_soft_apriori_windows
(include/wfhip.h) and IterativeSOQPSKLink(live_only=True) (waveforms_amd/encoding/coded.py).

Two definitions, two oracles that exist without this feature:
  * the window table is ``waveforms_amd.encoding.live.windows_host`` (numpy, written from the definition; pinned below on
    hand-made states), and the device table must equal it bit for bit;
  * inside a window the windowed detector is, bitwise, the EXISTING wf_viterbi4_soft_apriori on the slice, and outside every
    window it writes nothing.
The link is then checked three ways: with a guard of the whole burst it is the full loop bit for bit; at the default guard it
is, after every pass, a loop driven by hand from the existing entry points on the table's slices; and on full blocks its
frame errors stay with the full loop's.

Why the default guard is allowed to be as small as 128 rows is a premise about the data (a window's edge starts from free
metrics; the frozen neighbours' saturated priors make the metrics merge within a few rows): the CPU test below keeps it as a
regression on a seeded burst, from the restatements of tests/test_idd.py alone.
"""
import ctypes
import math
import sys
from pathlib import Path

import numpy as np
import pytest

import test_idd as TI
import test_soft_detector as TS
from waveforms_amd.encoding import ldpc
from waveforms_amd.encoding import live

SPS = 8


# ------------------------------------------------------------------------------------------------ CPU: the host statement
def _win(state, nrows, n_tx, **kw):
    w, rows, nopen = live.windows_host(np.array(state, dtype=np.uint8), nrows, n_tx, **kw)
    assert rows == int((w[:, 1] - w[:, 0]).sum()) and nopen == int((np.array(state) == 0).sum())
    assert (w[:, 0] % 2 == 0).all() and (w[:, 0] >= 0).all() and (w[:, 1] <= nrows).all() and (w[:, 1] > w[:, 0]).all()
    assert (w[1:, 0] >= w[:-1, 1]).all()                       # increasing and disjoint
    return w.tolist()


def test_windows_host_on_hand_made_states():
    n_tx, ncw = 100, 10
    nrows = 1 + ncw * n_tx + 8                                # coded bit j is row j + 1, eight tail rows
    # none open
    assert _win([1] * ncw, nrows, n_tx, guard=16) == []
    # all open, G > 0: neighbours touch (s - previous e = -2 G < G), one window; the tail (8 rows) is within G
    assert _win([0] * ncw, nrows, n_tx, guard=16) == [[0, nrows]]
    # ... and when it is not, the window ends G behind the last codeword
    assert _win([0] * ncw, nrows, n_tx, guard=3) == [[0, 1 + ncw * n_tx + 3]]
    # all open, G = 0, codewords on even rows: s - previous e = 0 < 0 is false for neighbours, one window per codeword
    assert _win([0] * ncw, nrows, n_tx, first=0, guard=0) == [[b * n_tx, (b + 1) * n_tx] for b in range(ncw)]
    # ... but behind the detector's row 0 a codeword starts on an ODD row (1 + b n_tx): its window starts one row early, on
    # the previous codeword's last row, -1 < 0 merges, and the windows of a table never overlap
    assert _win([0] * ncw, nrows, n_tx, guard=0) == [[0, 1 + ncw * n_tx]]
    assert _win([0, 1, 0, 0, 1, 0], nrows, n_tx, guard=0) == [[0, 101], [200, 401], [500, 601]]
    # an isolated codeword: a_4 = 401, rows [401 - 16, 501 + 16), the start already even after the guard (385 -> 384)
    st = [1] * ncw
    st[4] = 0
    assert _win(st, nrows, n_tx, guard=16) == [[384, 517]]
    assert _win(st, nrows, n_tx, guard=15) == [[386, 516]]
    # two open codewords 1, 2, 3 apart: the gap between their spans is 0, 100, 200 rows less two guards; the rule is
    # s - previous e < G.  G = 40: gaps -80 (merge), 20 (merge: 20 < 40), 120 (apart).
    for apart, want in ((1, [[160, 441]]), (2, [[160, 541]]), (3, [[160, 341], [460, 641]])):
        st = [1] * ncw
        st[2] = st[2 + apart] = 0
        assert _win(st, nrows, n_tx, guard=40) == want, apart
    # the boundary of the rule itself: period 150 leaves 50 rows between codewords 2 (rows 301 .. 400) and 3 (from 451):
    # s = (451 - G) & ~1, previous e = 401 + G.  G = 16: 434 - 417 = 17 >= 16 apart; G = 17: 434 - 418 = 16 < 17 merged
    st = [1] * ncw
    st[2] = st[3] = 0
    assert _win(st, 2000, n_tx, period=150, guard=16) == [[284, 417], [434, 567]]
    assert _win(st, 2000, n_tx, period=150, guard=17) == [[284, 568]]
    # clipping at both ends: codeword 0 (s = max(0, 1 - G)) and the last one (e = min(nrows, ...))
    st = [1] * ncw
    st[0] = st[-1] = 0
    assert _win(st, nrows, n_tx, guard=64) == [[0, 165], [836, nrows]]
    # framed geometry: first = 1 + p̂ + L, period L + n_tx
    L, p = 64, 37
    st = [1] * ncw
    st[0] = st[5] = 0
    a0, a5 = 1 + p + L, 1 + p + L + 5 * (L + n_tx)
    assert _win(st, 3000, n_tx, period=L + n_tx, first=1 + p + L, guard=10) == [[(a0 - 10) & ~1, a0 + n_tx + 10], [(a5 - 10) & ~1, a5 + n_tx + 10]]
    # a wrong lock: spans wholly beyond nrows give no window (and one that straddles the end is clipped); the open
    # codewords are still counted
    w, rows, nopen = live.windows_host(np.zeros(ncw, dtype=np.uint8), 500, n_tx, period=164, first=300, guard=10)
    assert w.tolist() == [[290, 410], [454, 500]] and rows == 166 and nopen == ncw
    tab = live.table_host(np.zeros(ncw, dtype=np.uint8), 500, n_tx, period=164, first=300, guard=10)
    assert tab.dtype == np.int64 and tab.tolist() == [2, 166, ncw, 0, 290, 410, 454, 500]
    for bad in ({"guard": -1}, {"period": n_tx - 1}):
        with pytest.raises(ValueError):
            live.windows_host(np.zeros(3, dtype=np.uint8), 500, n_tx, **bad)


def test_windows_host_merge_is_the_sequential_rule():
    """Random states against a literal transcription of the definition's loop (the host statement uses the same loop; this
    pins its arguments' meaning: first, period, the even start, both clips)."""
    rng = np.random.default_rng(3)
    for _ in range(200):
        ncw, n_tx = int(rng.integers(1, 40)), int(rng.integers(1, 60))
        P, first, G = n_tx + int(rng.integers(0, 30)), int(rng.integers(0, 90)), int(rng.integers(0, 80))
        nrows = int(rng.integers(1, first + ncw * P + 40))
        state = (rng.random(ncw) < rng.random()).astype(np.uint8)
        want = []
        for b in range(ncw):
            if state[b]:
                continue
            a = first + b * P
            s, e = max(0, a - G) & ~1, min(nrows, a + n_tx + G)
            if e <= s:
                continue
            if want and s - want[-1][1] < G:
                want[-1][1] = max(want[-1][1], e)
            else:
                want.append([s, e])
        assert _win(state, nrows, n_tx, period=P, first=first, guard=G) == want


# ------------------------------------------------------------------------------------------------ CPU: the guard premise
def test_guard_premise_on_a_seeded_burst(oracle):
    """12 demo codewords back to back in ONE burst at 4.7 dB (PT, seed 7), the loop of the restatements (damping 0.7, 5 inner
    iterations, ext_sat 50): on entry to pass 3 some codewords are open and some frozen, and the windowed pass
    (apriori_restatement on the slices of the host statement's windows, default guard) gives BITWISE the full pass's λᵉ on
    every row of an open codeword."""
    import test_ldpc as TL  # noqa: F401  (decode_ext_restatement's decoder)

    code = ldpc.demo_code()
    ncw, n_tx = 12, code.n_tx
    rng = np.random.default_rng(7)
    u = rng.integers(0, 2, (ncw, code.k), dtype=np.uint8)
    tx = code.encode_host(u)
    sigma = oracle.sigma_for_ebn0(4.7 + 10 * np.log10(code.k / n_tx), SPS)
    bits = np.concatenate([tx.reshape(-1), np.zeros(TI.PAD, np.uint8)])
    res = oracle.detection_run(bits, oracle.freq_pulse_soqpsk_tg(SPS), 0.25, SPS, sigma, rng=rng, detector="PT", timing_offset=-1)
    rows = np.asarray(res["mf_rows"])[:ncw * n_tx + 8]
    n = rows.shape[0]
    prior = np.zeros(n, dtype=np.float32)
    state, iters, info = np.zeros(ncw, dtype=np.uint8), np.zeros(ncw, dtype=np.int32), np.zeros((ncw, code.k), dtype=np.uint8)
    checked = 0
    for o in range(3):
        ext, _ = TI.apriori_restatement(oracle, rows, prior, 0.7, True)
        nopen = int((state == 0).sum())
        if o == 2:
            assert 0 < nopen < ncw, nopen                      # (otherwise the comparison says nothing)
            win, live_rows, _n = live.windows_host(state, n, n_tx, guard=live.DEFAULT_GUARD)
            assert 0 < live_rows < n
            for s, e in win.tolist():
                got, _ = TI.apriori_restatement(oracle, rows[s:e], prior[s:e], 0.7, True)
                for b in np.flatnonzero(state == 0):
                    a = 1 + b * n_tx
                    if s <= a and a + n_tx <= e:
                        assert np.array_equal(got[a - s:a - s + n_tx].view(np.uint64), ext[a:a + n_tx].view(np.uint64)), (b, s, e)
                        checked += 1
            assert checked == nopen
        pv = prior[1:1 + ncw * n_tx].reshape(ncw, n_tx)
        TI.decode_ext_restatement(code, ext[1:1 + ncw * n_tx].reshape(ncw, n_tx), state, pv, info, iters, 1.0, 0.75, 5, np.inf, 50.0)
    print(f"open on entry to pass 3: {nopen} of {ncw}, windows {win.tolist()}, live rows {live_rows} of {n}")


# ------------------------------------------------------------------------------------------------ CPU: interface
def test_live_entry_points_exported_and_bound():
    from waveforms_amd import _hip
    from waveforms_amd import device
    from waveforms_amd.encoding import coded

    lib = _hip.lib()
    for name in ("wf_idd_windows", "wf_viterbi4_soft_apriori_windows"):
        assert name in _hip.SIGNATURES and hasattr(lib, name)
    assert callable(device.idd_windows) and callable(device.viterbi_soft_apriori_windows)
    assert callable(coded.IterativeSOQPSKLink.live_results)
    assert live.DEFAULT_GUARD == 128


def test_live_argument_validation_without_a_gpu():
    """Bad arguments return WF_ERR_VALUE before the context (a fake one: no device exists here) is touched."""
    from waveforms_amd import _hip

    lib = _hip.lib()
    V = _hip.WF_ERR_VALUE
    buf = (ctypes.c_double * 64)()
    fake = p = ctypes.cast(buf, ctypes.c_void_p)
    odd2 = ctypes.c_void_p(ctypes.addressof(buf) + 2)
    odd4 = ctypes.c_void_p(ctypes.addressof(buf) + 4)
    inf, nan = float("inf"), float("nan")
    w = lib.wf_idd_windows
    #            ctx  state ncw nrows n_tx P   off lock L  G   table stream
    good = [fake, p, 10, 1000, 64, 64, 1, None, 0, 128, p, None]
    for i, bad in ((0, None), (1, None), (10, None), (2, 0), (2, (1 << 31) + 1), (3, 0), (4, 0), (5, 63), (6, -1), (8, -1), (9, -1), (10, odd4),
                   (7, odd4)):
        args = list(good)
        args[i] = bad
        assert w(*args) == V, (i, bad)
    f = lib.wf_viterbi4_soft_apriori_windows
    #            ctx  rows ncalls rb  diff warm prior scale table maxw ext bits stream
    good = [fake, p, 10, 48, 1, 0, p, 1.0, p, 4, p, p, None]
    for i, bad in ((0, None), (1, None), (6, None), (8, None), (10, None), (11, None), (2, 0), (3, 40), (5, -1), (7, inf), (7, nan), (9, 0), (9, -3),
                   (1, odd2), (6, odd2), (8, odd4), (10, odd4)):
        args = list(good)
        args[i] = bad
        assert f(*args) == V, (i, bad)


def test_live_python_argument_validation_without_a_gpu():
    """The Python wrappers' and the link's own checks come before any device call."""
    import torch

    from waveforms_amd import device as dev
    from waveforms_amd.encoding.coded import IterativeSOQPSKLink

    code = ldpc.demo_code()
    for kw in ({"guard": -1}, {"live_only": True, "guard": -5}):
        with pytest.raises(ValueError, match="guard"):
            IterativeSOQPSKLink(code, 4, **kw)
    state = torch.zeros(4, dtype=torch.uint8)
    for kw in ({"guard": -1}, {"nrows": 0}, {"n_tx": 0}, {"period": 7}, {"row_offset": -1}, {"marker_bits": -1}):
        args = {"nrows": 100, "n_tx": 8, **kw}
        with pytest.raises(ValueError):
            dev.idd_windows(state, **args)
    with pytest.raises(ValueError):
        dev.idd_windows(torch.zeros(4, dtype=torch.int32), 100, 8)
    with pytest.raises(ValueError):
        dev.idd_windows(state, 100, 8, out=torch.zeros(11, dtype=torch.int64))
    rows, prior, table = torch.zeros((10, 3, 2), dtype=torch.float64), torch.zeros(10, dtype=torch.float32), torch.zeros(12, dtype=torch.int64)
    for bad in ((rows, None, table, {}), (rows, prior[:9], table, {}), (rows, prior, table[:5], {}), (rows, prior, table.to(torch.int32), {}),
                (rows, prior, table, {"row_bytes": 40}), (rows, prior, table, {"max_windows": 5}), (rows, prior, table, {"max_windows": 0}),
                (rows, prior, table, {"out": (torch.zeros(9, dtype=torch.float64), torch.zeros(10, dtype=torch.uint8))}),
                (rows, prior, table, {"out": (torch.zeros(10, dtype=torch.float64), torch.zeros(9, dtype=torch.uint8))})):
        with pytest.raises(ValueError):
            dev.viterbi_soft_apriori_windows(bad[0], bad[1], bad[2], **bad[3])


def test_live_kernels_resources():
    """The exact set of live_* kernels; no spills and no scratch in any of them; for the detector's kernels nothing spilled in
    a loop and at least 4 waves per SIMD (at most 128 VGPRs), what tests/test_idd.py asks of soft_ap_*: the launches are cut
    for the same 2^18 lanes."""
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
    import kernel_resources as kr
    from waveforms_amd.csrc.build import build

    so = build(verbose=False)
    tab = {k: v for k, v in kr.kernel_table(so).items() if k.startswith("live_")}
    det = {f"live_bounds_kernel<{p}, {d}>" for p in ("true", "false") for d in (0, 1)}
    det |= {f"live_llr_kernel<{p}, {d}>" for p in ("true", "false") for d in (0, 1)}
    det |= {f"live_fixup_kernel<{p}, {b}, {d}>" for p in ("true", "false") for b in ("true", "false") for d in (0, 1)}
    want = det | {"live_windows_kernel", "live_plan_kernel"}
    assert set(tab) == want, sorted(set(tab) ^ want)
    asm = kr.loop_spill_counts(so, "live_")
    for name, row in tab.items():
        assert row["vgpr_spill_count"] == 0 and row["sgpr_spill_count"] == 0 and row["private_segment_fixed_size"] == 0, (name, row)
        a = asm[name]
        assert a["scratch_load"] == 0 and a["scratch_store"] == 0, (name, a)
        if name in det:
            assert a["v_readlane_in_loop"] == 0 and a["v_writelane_in_loop"] == 0, (name, a)
            waves = kr.waves_per_simd(row["vgpr_count"], row.get("agpr_count", 0))
            assert waves >= 4, (name, row["vgpr_count"], waves)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture
def soft_ctx():
    from waveforms_amd import _hip

    ctx = _hip.new_ctx()
    yield ctx
    _hip.free_ctx(ctx)


def _device_table(dev, _hip, state, nrows, n_tx, period=None, first=1, guard=128, lock=None, L=0):
    """wf_idd_windows on the device -> the table's specified words (row_offset = first - p̂ - L)."""
    p = 0 if lock is None else int(lock[0])
    d_lock = None if lock is None else _hip.to_device(np.asarray(lock, dtype=np.int64))
    out = _hip.to_device(np.full(4 + 2 * len(state), -7, dtype=np.int64))
    got = dev.idd_windows(_hip.to_device(np.asarray(state, dtype=np.uint8)), nrows, n_tx, period, first - p - L, d_lock, L, guard, out=out)
    got = _hip.to_host(got)
    return got[:4 + 2 * int(got[0])], got


@pytest.mark.gpu
def test_gpu_window_table_equals_the_host_statement():
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    code = ldpc.demo_code()
    n_tx, ncw = code.n_tx, 4882
    nrows = 1 + ncw * n_tx + 24
    rng = np.random.default_rng(41)
    for frac in (0.0, 0.001, 0.07, 0.5, 1.0):
        state = (rng.random(ncw) >= frac).astype(np.uint8)
        if frac == 0.001:
            state[[0, ncw - 1]] = 0                            # both clips
        for guard in (0, 16, 128, 512, 3000):
            want = live.table_host(state, nrows, n_tx, guard=guard)
            got, full = _device_table(dev, _hip, state, nrows, n_tx, guard=guard)
            assert np.array_equal(got, want), (frac, guard, got[:12], want[:12])
            assert full.size == 4 + 2 * ncw
        # framed, the lock record in device memory: p̂ = 1234, a marker of 64
        L, p = 64, 1234
        lock = [p, 1, 0, 0]
        nr = 1 + p + ncw * (L + n_tx) + 24
        want = live.table_host(state, nr, n_tx, L + n_tx, 1 + p + L, 128)
        got, _ = _device_table(dev, _hip, state, nr, n_tx, L + n_tx, 1 + p + L, 128, lock, L)
        assert np.array_equal(got, want), ("framed", frac)
        # a wrong lock near the end of the period: the last codewords' spans leave the burst
        lock = [L + n_tx - 1, -1, 0, 0]
        want = live.table_host(state, nr - 3000, n_tx, L + n_tx, 1 + lock[0] + L, 128)
        got, _ = _device_table(dev, _hip, state, nr - 3000, n_tx, L + n_tx, 1 + lock[0] + L, 128, lock, L)
        assert np.array_equal(got, want), ("wrong lock", frac)
    # the hand-made cases of the CPU test, and small shapes (fewer codewords than threads, one codeword)
    n_tx, ncw = 100, 10
    nrows = 1 + ncw * n_tx + 8
    cases = [([1] * ncw, {"guard": 16}), ([0] * ncw, {"guard": 16}), ([0] * ncw, {"guard": 3}), ([0] * ncw, {"guard": 0}), ([0], {"guard": 5}), ([1], {"guard": 5})]
    for apart in (1, 2, 3):
        st = [1] * ncw
        st[2] = st[2 + apart] = 0
        cases.append((st, {"guard": 40}))
    st = [1] * ncw
    st[2] = st[3] = 0
    cases += [(st, {"period": 150, "guard": 16}), (st, {"period": 150, "guard": 17}), ([0] * ncw, {"first": 0, "guard": 0})]
    st = [1] * ncw
    st[0] = st[-1] = 0
    cases.append((st, {"guard": 64}))
    cases.append(([0] * ncw, {"period": 164, "first": 300, "guard": 10, "nrows": 500}))
    for st, kw in cases:
        kw = dict(kw)
        nr = kw.pop("nrows", nrows if kw.get("period") is None else 2000)
        want = live.table_host(np.array(st, dtype=np.uint8), nr, n_tx, **kw)
        got, _ = _device_table(dev, _hip, st, nr, n_tx, **kw)
        assert np.array_equal(got, want), (st, kw, got, want)
    rng = np.random.default_rng(43)
    for _ in range(60):
        ncw, n_tx = int(rng.integers(1, 700)), int(rng.integers(1, 60))
        P, first, G = n_tx + int(rng.integers(0, 30)), int(rng.integers(0, 90)), int(rng.integers(0, 80))
        nr = int(rng.integers(1, first + ncw * P + 40))
        state = (rng.random(ncw) < rng.random()).astype(np.uint8)
        want = live.table_host(state, nr, n_tx, P, first, G)
        got, _ = _device_table(dev, _hip, state, nr, n_tx, P, first, G)
        assert np.array_equal(got, want), (ncw, n_tx, P, first, G, nr)
    _hip.device_check()


def _table(windows, room):
    t = np.zeros(4 + 2 * room, dtype=np.int64)
    t[0], t[1] = len(windows), sum(e - s for s, e in windows)
    t[4:4 + 2 * len(windows)] = np.array(windows, dtype=np.int64).reshape(-1)
    return t


PATTERN_EXT, PATTERN_BIT = -1234.5, 77


def _check_windowed(_hip, dev, ctx, d_rows, rb, d_prior, n, windows, scale, differential, warmup, what):
    """The windowed call on pre-filled outputs against the existing entry point on every slice; rows outside stay filled."""
    torch = _hip.torch()
    ext = torch.full((n,), PATTERN_EXT, dtype=torch.float64, device="cuda")
    bits = torch.full((n + 16,), PATTERN_BIT, dtype=torch.uint8, device="cuda")
    table = _hip.to_device(_table(windows, max(len(windows), 1) + 3))
    got_ext, got_bits = dev.viterbi_soft_apriori_windows(d_rows, d_prior, table, scale, differential, warmup, rb, ctx=ctx, out=(ext, bits))
    assert got_ext.data_ptr() == ext.data_ptr() and got_bits.data_ptr() == bits.data_ptr()
    after = (dev.viterbi_unmerged(reset=True, ctx=ctx), dev.viterbi_repaired(reset=True, ctx=ctx))
    words = rb // 8
    flat = d_rows.reshape(-1)
    outside = torch.ones(n, dtype=torch.bool, device="cuda")
    for s, e in windows:
        want_ext, want_bits = dev.viterbi_soft_apriori(flat[s * words:e * words], d_prior[s:e], scale, differential, warmup, rb, ctx=ctx)
        assert torch.equal(ext[s:e].view(torch.int64), want_ext.view(torch.int64)), (what, s, e)
        assert torch.equal(bits[s:e], want_bits), (what, s, e)
        outside[s:e] = False
    assert bool((ext[outside] == PATTERN_EXT).all()) and bool((bits[:n][outside] == PATTERN_BIT).all()), what
    assert bool((bits[n:] == PATTERN_BIT).all()), what
    dev.viterbi_unmerged(reset=True, ctx=ctx), dev.viterbi_repaired(reset=True, ctx=ctx)     # (the slices' own counts)
    return after


@pytest.mark.gpu
@pytest.mark.parametrize("detector", ["PT", "PAM"])
def test_gpu_windowed_detector_equals_the_existing_one_on_every_slice(soft_ctx, detector):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    d32, rb, _tx, _counts = TS._link_rows(20000, detector, 4.0)
    assert rb == 32
    d48 = TS._unpack_rows(d32).contiguous()
    n = d32.numel() // 4
    rng = np.random.default_rng(11 + (detector == "PAM"))
    priors = TI._priors(rng, n)
    # a window of 2 rows at the burst's start and one inside, windows shorter and longer than a chunk of 32, neighbours that
    # touch (s = previous e), a window ending at nrows
    windows = [(0, 2), (10, 700), (700, 730), (2000, 5000), (5100, 5102), (9000, 17192), ((n - 501) & ~1, n)]
    TI._counters(dev, soft_ctx)
    for chunk in (32, 0, 8192):
        _hip.set_option(soft_ctx, _hip.WF_OPT_SOFT_CHUNK_CALLS, chunk)
        for (words, d_rows) in ((32, d32), (48, d48)):
            for differential in (True, False):
                for pname in ("mixed", "sat"):
                    d_prior = _hip.to_device(priors[pname])
                    for warmup in (0, 1):
                        what = (detector, chunk, words, differential, pname, warmup)
                        unproven, repaired = _check_windowed(_hip, dev, soft_ctx, d_rows, words, d_prior, n, windows, 0.7, differential, warmup, what)
                        assert unproven == 0, what
                        if warmup == 1 and chunk != 8192:      # chunks of 32 rows inside the long windows: the repairs really run
                            assert repaired > 0, what
                        if chunk == 8192:                      # every window is one chunk: exact, nothing to prove
                            assert repaired == 0, what
    # W = 0: nothing written, counters unchanged; and a table longer than its windows (room for more) is fine
    _hip.set_option(soft_ctx, _hip.WF_OPT_SOFT_CHUNK_CALLS, 0)
    d_prior = _hip.to_device(priors["mixed"])
    assert _check_windowed(_hip, dev, soft_ctx, d32, 32, d_prior, n, [], 0.7, True, 1, "W = 0") == (0, 0)
    # repairs off: the same launch counts what it does not repair
    _hip.set_option(soft_ctx, _hip.WF_OPT_DET_REPAIR, 1)
    table = _hip.to_device(_table(windows, 8))
    dev.viterbi_soft_apriori_windows(d32, d_prior, table, 0.7, True, 1, 32, ctx=soft_ctx)
    unproven, repaired = TI._counters(dev, soft_ctx)
    assert unproven > 0 and repaired == 0
    _hip.set_option(soft_ctx, _hip.WF_OPT_DET_REPAIR, 0)
    _hip.check(_hip.lib().wf_ctx_check(soft_ctx, _hip.stream()))


@pytest.mark.gpu
def test_gpu_malformed_table_touches_nothing(soft_ctx):
    """Overlapping, odd, reversed or out-of-range windows and W > max_windows: the fault word is raised, no row is written."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    torch = _hip.torch()
    n = 4000
    rng = np.random.default_rng(5)
    d_rows = _hip.to_device(rng.standard_normal((n, 3)) + 1j * rng.standard_normal((n, 3)))
    d_prior = _hip.to_device(rng.standard_normal(n).astype(np.float32))
    for windows in ([(0, 100), (98, 200)], [(3, 100)], [(100, 100)], [(200, 100)], [(0, n + 2)], [(-2, 10)]):
        ext = torch.full((n,), PATTERN_EXT, dtype=torch.float64, device="cuda")
        bits = torch.full((n,), PATTERN_BIT, dtype=torch.uint8, device="cuda")
        dev.viterbi_soft_apriori_windows(d_rows, d_prior, _hip.to_device(_table(windows, 4)), ctx=soft_ctx, out=(ext, bits))
        assert _hip.lib().wf_ctx_check(soft_ctx, _hip.stream()) == _hip.WF_ERR_DEVICE, windows
        assert bool((ext == PATTERN_EXT).all()) and bool((bits == PATTERN_BIT).all()), windows
    t = _table([(0, 10), (20, 30), (40, 50)], 4)
    ext = torch.full((n,), PATTERN_EXT, dtype=torch.float64, device="cuda")
    bits = torch.full((n,), PATTERN_BIT, dtype=torch.uint8, device="cuda")
    dev.viterbi_soft_apriori_windows(d_rows, d_prior, _hip.to_device(t), ctx=soft_ctx, out=(ext, bits), max_windows=2)
    assert _hip.lib().wf_ctx_check(soft_ctx, _hip.stream()) == _hip.WF_ERR_DEVICE
    assert bool((ext == PATTERN_EXT).all())
    assert _hip.lib().wf_ctx_check(soft_ctx, _hip.stream()) == 0          # (the check cleared the word)


def _links(code, ncw, framed, **kw):
    from waveforms_amd.encoding.coded import IterativeSOQPSKLink
    from waveforms_amd.encoding.framing import Framing

    fr = {"framing": Framing(code), "lead_bits": 1234} if framed else {}
    return IterativeSOQPSKLink(code, ncw, detector="PT", per_pass=True, **fr, **kw)


def _snapshot(_hip, dev, link, info):
    torch = _hip.torch()
    counts = dev.ldpc_count(link.code, link.decided, info, link.state, link.iters)
    return (link.prior.view(torch.int32).clone(), link.state.clone(), link.decided.clone(), link.iters.clone(), counts)


def _same(_hip, a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert _hip.torch().equal(x, y), (what, ("prior", "state", "decided", "iters", "counts")[i])


@pytest.mark.gpu
@pytest.mark.parametrize("framed", [False, True])
def test_gpu_guard_of_the_whole_burst_is_the_full_loop(framed):
    """guard >= nrows: any open codeword makes the window the whole burst, so live_only must reproduce the full loop bit for
    bit, after every pass and in its counts."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    code = ldpc.demo_code()
    ncw, outer = 40, 5
    full = _links(code, ncw, framed, outer=outer)
    info = full.info_bits(3)
    rows, _ = full.front_end(dev.ldpc_encode(code, info), 4.5, 11, 3)
    n = int(rows.shape[0])
    lv = _links(code, ncw, framed, outer=outer, live_only=True, guard=n)
    full.begin(n), lv.begin(n)
    opens = []
    for o in range(outer):
        for link in (full, lv):
            ext, _ = link.detect(rows, first=o == 0, o=o)
            link.decode(ext)
        _same(_hip, _snapshot(_hip, dev, full, info), _snapshot(_hip, dev, lv, info), (framed, o))
        opens.append(int((full.state == 0).sum()))
    print("open after each pass:", opens, "live:", lv.live_results())
    assert 0 < opens[0] and opens[-1] < opens[0]               # the loop does something on this block
    for o, (w, live_rows, nopen) in enumerate(lv.live_results()):
        if o:
            assert nopen == opens[o - 1] and (w, live_rows) == ((1, n) if nopen else (0, 0)), (o, w, live_rows, nopen)
    # and through run_block: the same counts after every pass
    full.reset_counts(), lv.reset_counts()
    full.run_block(4.5, seed=11, stream_id=3), lv.run_block(4.5, seed=11, stream_id=3)
    assert full.pass_results() == lv.pass_results() and full.result() == lv.result() and full.uncoded_result() == lv.uncoded_result()
    if framed:
        assert full.sync_result() == lv.sync_result()


@pytest.mark.gpu
@pytest.mark.parametrize("framed", [False, True])
def test_gpu_default_guard_is_the_loop_of_the_existing_entry_points_on_the_slices(framed):
    """The link at the default guard, pass by pass, against a loop driven by hand: the table is read back every pass (and is
    the host statement's), the EXISTING wf_viterbi4_soft_apriori runs on every slice into the block's ext buffer, gather and
    decoder as the link does them.  Same prior, state, decisions and iterations after every pass."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    code = ldpc.demo_code()
    ncw, outer = 48, 5
    hand = _links(code, ncw, framed, outer=outer)              # (a full link: the container of the hand-driven loop's state)
    info = hand.info_bits(1)
    rows, _ = hand.front_end(dev.ldpc_encode(code, info), 4.6, 5, 1)
    n = int(rows.shape[0])
    lv = _links(code, ncw, framed, outer=outer, live_only=True)
    assert lv.guard == live.DEFAULT_GUARD
    hand.begin(n), lv.begin(n)
    flat = rows.reshape(-1)
    ext_buf = None
    seen = []
    for o in range(outer):
        ext, _ = lv.detect(rows, first=o == 0, o=o)
        lv.decode(ext)
        if o == 0:
            ext_buf, _b = dev.viterbi_soft_apriori(rows, None, hand.damping)
        else:
            if framed:
                p = int(hand.lock.cpu()[0])
                want = live.table_host(_hip.to_host(hand.state), n, code.n_tx, hand.framing.period, 1 + p + hand.framing.L, live.DEFAULT_GUARD)
                table = _hip.to_host(dev.idd_windows(hand.state, n, code.n_tx, hand.framing.period, 1, hand.lock, hand.framing.L, live.DEFAULT_GUARD))
            else:
                want = live.table_host(_hip.to_host(hand.state), n, code.n_tx, guard=live.DEFAULT_GUARD)
                table = _hip.to_host(dev.idd_windows(hand.state, n, code.n_tx, guard=live.DEFAULT_GUARD))
            assert np.array_equal(table[:want.size], want), o
            assert np.array_equal(_hip.to_host(lv.windows)[:want.size], want), o
            seen.append((int(want[0]), int(want[1]), int(want[2])))
            for s, e in want[4:].reshape(-1, 2).tolist():
                got, _b = dev.viterbi_soft_apriori(flat[6 * s:6 * e], hand.prior[s:e], hand.damping)
                ext_buf[s:e] = got
        view = hand.deframe(ext_buf[1:], search=o == 0) if framed else ext_buf[1:1 + hand.nbits].view(ncw, code.n_tx)
        hand.decode(view)
        _same(_hip, _snapshot(_hip, dev, hand, info), _snapshot(_hip, dev, lv, info), (framed, o))
    print("windows, live rows, open per pass 2 ..:", seen, "of", n, "rows")
    assert lv.live_results()[1:] == seen
    assert any(0 < w[1] < n for w in seen)                     # some pass really worked on a part of the burst
    _hip.device_check()


@pytest.mark.gpu
@pytest.mark.parametrize("framed", [False, True])
def test_gpu_noiseless_block_has_no_live_row_after_pass_1(framed):
    from waveforms_amd import _hip  # noqa: F401

    code = ldpc.demo_code()
    full = _links(code, 37, framed, outer=3)
    lv = _links(code, 37, framed, outer=3, live_only=True)
    for link in (full, lv):
        link.run_block(None, seed=1, stream_id=0)
        link.run_block(None, seed=1, stream_id=1)
    n = int(lv.prior.numel())
    assert lv.live_results() == [(2, 2 * n, 2 * 37), (0, 0, 0), (0, 0, 0)]
    assert lv.result() == full.result() == (0, 0, 0, 2 * 37 * code.k, 0.0)
    assert lv.pass_results() == full.pass_results() == [(0, 0, 0, 0.0)] * 3
    assert int(lv.state.sum()) == 37 and lv.uncoded_result() == full.uncoded_result()
    lv.reset_counts()
    assert lv.live_results() == [(0, 0, 0)] * 3


@pytest.mark.gpu
@pytest.mark.parametrize("ebn0", [4.5, 5.0])
def test_gpu_full_block_frame_errors_stay_with_the_full_loop(ebn0):
    """One 1e7-channel-bit block (4 882 demo codewords in ONE burst), windowed and full loop on the same noise: the frame
    errors after every pass differ by at most 4 sqrt(sum of the two counts + 1).  The runs share their noise, so equal counts
    are what is expected; the bound cannot fail by chance and catches a loop that feeds the decoder stale or misplaced rows.
    The number of codewords whose final decisions differ is printed: a measurement, not a bound."""
    from waveforms_amd import _hip

    code = ldpc.demo_code()
    ncw = int(1e7) // code.n_tx
    assert ncw == 4882
    res = {}
    for name, kw in (("full", {}), ("live", {"live_only": True})):
        link = _links(code, ncw, False, outer=8, inner=5, **kw)
        link.run_block(ebn0, seed=9, stream_id=0)
        res[name] = (link.pass_results(), link.result(), link.decided.clone(), link)
    fe_full = [r[1] for r in res["full"][0]]
    fe_live = [r[1] for r in res["live"][0]]
    differ = int((res["full"][2] != res["live"][2]).any(dim=1).sum())
    lr = res["live"][3].live_results()
    print(f"{ebn0} dB: frame errors per pass full {fe_full}, live {fe_live}; codewords whose final decisions differ: {differ} of {ncw}; "
          f"(windows, live rows, open) per pass {lr}")
    if ebn0 == 4.5:
        assert fe_full[1] >= 100                               # (otherwise the comparison says nothing)
    for o, (a, b) in enumerate(zip(fe_full, fe_live)):
        assert abs(a - b) <= 4.0 * math.sqrt(a + b + 1), (o, a, b)
    assert lr[0] == (1, int(res["live"][3].prior.numel()), ncw)
    assert [x[2] for x in lr[1:]] == [r[2] for r in res["live"][0][:-1]]      # open on entry = open after the pass before
    del res
    _hip.device_check()
