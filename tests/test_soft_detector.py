"""Max-log-MAP soft output over the SOQPSK 4-state trellis (wf_viterbi4_soft, include/wfhip.h).

The definition is restated here sequentially (a loop over sections, float64, in the header's order of operations) and
pinned to brute force on short bursts (CPU).  On the GPU the chunk-parallel kernel must equal the restatement BITWISE,
whatever the warm-up and the chunking, in both row forms; its hard decisions must be the ML sequence (the long-window
detector's), and its LLRs must be ordered (error rate falling with |λ|).  No test assumes that the soft decisions have
fewer bit errors than the length-2 detector: they need not.
"""
import ctypes
import itertools

import numpy as np
import pytest

SPS = 8
STATE_EXP = (+1j, -1, +1, -1j)          # algorithm.py:30
TRELLIS = {True: "SOQPSKTrellis4x2DiffEncoded", False: "SOQPSKTrellis4x2"}


def _branches(oracle, differential):
    """Per column: [(b, start, end, inp, out_idx)] in list order, from the oracle's tables of the reference trellis."""
    t = oracle.trellis_tables(TRELLIS[differential])
    bpc = t["bpc"]
    return [[(b, int(t["br_start"][c * bpc + b]), int(t["br_end"][c * bpc + b]), int(t["br_inp"][c * bpc + b]),
              int(t["br_out_idx"][c * bpc + b])) for b in range(bpc)] for c in range(t["columns"])]


def _increments(oracle, rows, differential):
    """inc[k, b] = Re(state_exp_term[start b] * z_k[idx(out b)]) with branch list of column k % 2."""
    z = np.asarray(rows, dtype=np.complex128).reshape(-1, 3)
    inc = np.empty((z.shape[0], 8))
    for c, brs in enumerate(_branches(oracle, differential)):
        for (b, s, _e, _i, idx) in brs:
            inc[c::2, b] = (STATE_EXP[s] * z[c::2, idx]).real
    return inc


def soft_restatement(oracle, rows, differential):
    """The header's definition, one section at a time -> (llr, bits)."""
    brs = _branches(oracle, differential)
    inc = _increments(oracle, rows, differential).tolist()
    n = len(inc)
    inf = float("inf")
    alpha = [None] * (n + 1)
    a = [0.0, 0.0, 0.0, 0.0]
    alpha[0] = a
    for k in range(n):
        ik, new = inc[k], [inf, inf, inf, inf]
        for (b, s, e, _i, _x) in brs[k & 1]:
            v = a[s] + ik[b]
            if v < new[e]:
                new[e] = v
        mn = min(new)
        a = [v - mn for v in new]
        alpha[k + 1] = a
    llr = np.empty(n)
    bt = [0.0, 0.0, 0.0, 0.0]
    for k in range(n - 1, -1, -1):
        ik, a, new = inc[k], alpha[k], [inf, inf, inf, inf]
        m = [inf, inf]
        for (b, s, e, i, _x) in brs[k & 1]:
            t = (a[s] + ik[b]) + bt[e]
            if t < m[i]:
                m[i] = t
            v = ik[b] + bt[e]
            if v < new[s]:
                new[s] = v
        llr[k] = m[1] - m[0]
        mn = min(new)
        bt = [v - mn for v in new]
    return llr, (llr < 0).astype(np.uint8)


def soft_brute_force(oracle, rows, differential):
    """λ_k = min over paths with u_k = 1 - min over paths with u_k = 0, every start state and every input sequence."""
    t = oracle.trellis_tables(TRELLIS[differential])
    inc = _increments(oracle, rows, differential)
    n = inc.shape[0]
    bidx = {}                                    # (column, start, input) -> branch index within the column
    for c, brs in enumerate(_branches(oracle, differential)):
        for (b, s, _e, i, _x) in brs:
            bidx[(c, s, i)] = b
    best = np.full((n, 2), np.inf)
    for s0 in range(4):
        for u in itertools.product((0, 1), repeat=n):
            s, cost = s0, 0.0
            for k in range(n):
                cost += inc[k, bidx[(k & 1, s, u[k])]]
                s = int(t["next"][k & 1, s, u[k]])
            for k in range(n):
                best[k, u[k]] = min(best[k, u[k]], cost)
    return best[:, 1] - best[:, 0]


def pack_rows(rows):
    """48-byte rows -> the links' 32-byte detector-packed rows {Re z1, Im z1, a, b} (wf_viterbi.hip: vit_components):
    (a, b) = (Re z0, Im z2) for even calls, (Im z0, Re z2) for odd ones."""
    z = np.asarray(rows, dtype=np.complex128).reshape(-1, 3)
    p = np.empty((z.shape[0], 4))
    p[:, 0], p[:, 1] = z[:, 1].real, z[:, 1].imag
    p[0::2, 2], p[0::2, 3] = z[0::2, 0].real, z[0::2, 2].imag
    p[1::2, 2], p[1::2, 3] = z[1::2, 0].imag, z[1::2, 2].real
    return p


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("differential", [True, False])
def test_restatement_equals_brute_force(oracle, differential):
    rng = np.random.default_rng(11 + differential)
    for n in range(1, 11):
        # integer-valued rows: every sum is exact, so the normalised recursions must give the brute force's λ exactly
        rows = rng.integers(-8, 9, (n, 3)) + 1j * rng.integers(-8, 9, (n, 3))
        llr, bits = soft_restatement(oracle, rows, differential)
        want = soft_brute_force(oracle, rows, differential)
        assert np.array_equal(llr, want), (n, llr, want)
        assert np.array_equal(bits, (want < 0).astype(np.uint8))
        # real-valued rows: equal up to the rounding of the normalisations
        rows = rng.standard_normal((n, 3)) + 1j * rng.standard_normal((n, 3))
        llr, _ = soft_restatement(oracle, rows, differential)
        np.testing.assert_allclose(llr, soft_brute_force(oracle, rows, differential), rtol=1e-12, atol=1e-12)


def test_soft_entry_points_exported_and_bound():
    from waveforms_amd import _hip

    lib = _hip.lib()
    for name in ("wf_viterbi4_soft", "wf_viterbi4_soft_geometry"):
        assert name in _hip.SIGNATURES and hasattr(lib, name)
    from waveforms_amd import device
    from waveforms_amd.viterbi.algorithm import SOQPSKTrellisDetector

    assert callable(device.viterbi_soft) and callable(device.viterbi_soft_geometry)
    assert callable(SOQPSKTrellisDetector.detect_soft) and callable(SOQPSKTrellisDetector.detect_soft_device)


def test_soft_argument_validation_without_a_gpu():
    """Bad arguments return WF_ERR_VALUE before the context is touched (a fake context: no device exists here)."""
    from waveforms_amd import _hip

    lib = _hip.lib()
    fake = ctypes.create_string_buffer(1 << 16)
    buf = ctypes.create_string_buffer(4096)
    rows = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    llr, bits = rows + 1024, rows + 2048
    V = _hip.WF_ERR_VALUE
    for rb in (0, 16, 24, 40, 64):
        assert lib.wf_viterbi4_soft(fake, rows, 10, rb, 1, 0, llr, bits, None) == V
    for n in (0, -1):
        assert lib.wf_viterbi4_soft(fake, rows, n, 48, 1, 0, llr, bits, None) == V
    assert lib.wf_viterbi4_soft(fake, rows, 10, 48, 1, -1, llr, bits, None) == V
    assert lib.wf_viterbi4_soft(None, rows, 10, 48, 1, 0, llr, bits, None) == V
    assert lib.wf_viterbi4_soft(fake, None, 10, 32, 1, 0, llr, bits, None) == V
    assert lib.wf_viterbi4_soft(fake, rows, 10, 48, 1, 0, None, bits, None) == V
    assert lib.wf_viterbi4_soft(fake, rows, 10, 48, 1, 0, llr, None, None) == V
    g = (ctypes.c_int64 * 4)()
    assert lib.wf_viterbi4_soft_geometry(None, 100, 0, g) == V
    assert lib.wf_viterbi4_soft_geometry(fake, 0, 0, g) == V
    assert lib.wf_viterbi4_soft_geometry(fake, 100, -1, g) == V
    assert lib.wf_viterbi4_soft_geometry(fake, 100, 0, None) == V
    # the geometry is a host computation: the library's defaults on a context with default options
    assert lib.wf_viterbi4_soft_geometry(fake, 10_000_000, 0, g) == 0
    assert (g[0], g[1], g[2]) == (40, 250_000, 32) and g[3] >= 10_000_000 * 32
    assert lib.wf_viterbi4_soft_geometry(fake, 1000, 2, g) == 0 and (g[0], g[1], g[2]) == (32, 32, 2)
    assert lib.wf_ctx_set_option(fake, _hip.WF_OPT_SOFT_CHUNK_CALLS, 8193) == V
    assert lib.wf_ctx_set_option(fake, _hip.WF_OPT_SOFT_CHUNK_CALLS, -1) == V
    assert lib.wf_ctx_set_option(fake, _hip.WF_OPT_SOFT_CHUNK_CALLS, 7) == 0
    assert lib.wf_viterbi4_soft_geometry(fake, 1000, 0, g) == 0 and (g[0], g[1]) == (7, 143)


def test_soft_kernels_do_not_spill_in_loops():
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
    import kernel_resources as kr
    from waveforms_amd.csrc.build import build

    so = build(verbose=False)
    tab = {k: v for k, v in kr.kernel_table(so).items() if k.startswith("soft_")}
    asm = kr.loop_spill_counts(so, "soft_")
    assert len(tab) >= 10, sorted(tab)
    for name, row in tab.items():
        assert row["vgpr_spill_count"] == 0 and row["sgpr_spill_count"] == 0 and row["private_segment_fixed_size"] == 0, (name, row)
        a = asm[name]
        assert a["scratch_load_in_loop"] == 0 and a["scratch_store_in_loop"] == 0, (name, a)
        assert a["v_readlane_in_loop"] == 0 and a["v_writelane_in_loop"] == 0, (name, a)


# ------------------------------------------------------------------------------------------------ GPU
def _detection_rows(oracle, n, ebn0, detector, seed=3):
    bits, _ = oracle.glfsr_bits(0x420000, 0x7FFFFF, n)
    if ebn0 is None:
        noise = np.zeros((n + 1) * SPS, dtype=np.complex128)
    else:
        noise = oracle.philox_awgn(oracle.sigma_for_ebn0(ebn0, SPS), 5, seed, 0, (n + 1) * SPS)
    res = oracle.detection_run(bits, oracle.freq_pulse_soqpsk_tg(SPS), 0.25, SPS, None, noise=noise, detector=detector)
    return bits, res["mf_rows"]


def _counters(dev, ctx):
    return dev.viterbi_unmerged(reset=True, ctx=ctx), dev.viterbi_repaired(reset=True, ctx=ctx)


@pytest.fixture
def soft_ctx():
    from waveforms_amd import _hip

    ctx = _hip.new_ctx()
    yield ctx
    _hip.free_ctx(ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("detector", ["PT", "PAM"])
@pytest.mark.parametrize("ebn0", [0.0, 4.0, 10.0])
def test_soft_bitwise_equals_the_definition(oracle, soft_ctx, detector, ebn0):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    _bits, rows = _detection_rows(oracle, 200_000, ebn0, detector)
    want_llr, want_bits = soft_restatement(oracle, rows, True)
    _hip.set_option(soft_ctx, _hip.WF_OPT_DET_FINAL_VERIFY, 1)
    full, packed = _hip.to_device(rows), _hip.to_device(pack_rows(rows))
    _counters(dev, soft_ctx)
    for warmup in (0, 2):
        for d_rows, rb in ((full, 48), (packed, 32)):
            llr, bits = dev.viterbi_soft(d_rows, True, warmup, rb, ctx=soft_ctx)
            llr, bits = _hip.to_host(llr), _hip.to_host(bits)
            unproven, repaired = _counters(dev, soft_ctx)
            assert unproven == 0, (warmup, rb)
            assert np.array_equal(llr.view(np.uint64), want_llr.view(np.uint64)), (warmup, rb, int(np.count_nonzero(llr != want_llr)))
            assert np.array_equal(bits, want_bits), (warmup, rb)
            if warmup == 2:
                assert repaired > 0          # the short warm-up missed: the result above came through the repairs


@pytest.mark.gpu
@pytest.mark.parametrize("differential", [True, False])
def test_soft_any_chunking_and_short_bursts(oracle, soft_ctx, differential):
    """Ragged and tiny bursts, chunks of 1 and of odd lengths, both trellises."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    rng = np.random.default_rng(7)
    for n in (1, 2, 3, 5, 33, 1001):
        rows = 2.0 * (rng.standard_normal((n, 3)) + 1j * rng.standard_normal((n, 3)))
        want_llr, want_bits = soft_restatement(oracle, rows, differential)
        for chunk in (0, 1, 7, 64):
            _hip.set_option(soft_ctx, _hip.WF_OPT_SOFT_CHUNK_CALLS, chunk)
            for warmup in (0, 1, 3):
                llr, bits = dev.viterbi_soft(_hip.to_device(rows), differential, warmup, 48, ctx=soft_ctx)
                assert np.array_equal(_hip.to_host(llr), want_llr), (n, chunk, warmup)
                assert np.array_equal(_hip.to_host(bits), want_bits), (n, chunk, warmup)
                llr, _ = dev.viterbi_soft(_hip.to_device(pack_rows(rows)), differential, warmup, 32, ctx=soft_ctx)
                assert np.array_equal(_hip.to_host(llr), want_llr), (n, chunk, warmup, "packed")
                assert _counters(dev, soft_ctx)[0] == 0


@pytest.mark.gpu
def test_soft_proof_is_real(oracle, soft_ctx):
    """With the repairs off, a 2-row warm-up at 0 dB leaves chunks unproven: the proof detects what it repairs."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    _bits, rows = _detection_rows(oracle, 50_000, 0.0, "PT")
    _hip.set_option(soft_ctx, _hip.WF_OPT_DET_REPAIR, 1)
    _counters(dev, soft_ctx)
    dev.viterbi_soft(_hip.to_device(rows), True, 2, 48, ctx=soft_ctx)
    unproven, repaired = _counters(dev, soft_ctx)
    assert unproven > 0 and repaired == 0


@pytest.mark.gpu
@pytest.mark.parametrize("detector", ["PT", "PAM"])
def test_soft_alignment_on_noiseless_rows(oracle, detector):
    from waveforms_amd import _hip
    from waveforms_amd.viterbi.algorithm import SOQPSKTrellisDetector

    tx, rows = _detection_rows(oracle, 4000, None, detector)
    det = SOQPSKTrellisDetector()
    llr, bits = det.detect_soft(rows)
    m = min(tx.size, bits.size - 1)
    assert m > 3900
    assert np.array_equal(bits[1:1 + m], tx[:m])
    assert det.i == 0                                  # a fresh burst: the detector's own state is untouched
    d_llr, _ = det.detect_soft_device(_hip.to_device(rows))
    assert np.array_equal(_hip.to_host(d_llr), llr)


def _link_rows(n, detector, ebn0, seed=1):
    """Rows, transmitted bits and the length-2 counts of one SOQPSKLink block (fuse 15: detector-packed rows).  The block
    sends PN23 from the all-ones state (seed and skip 0: the bits smoke() checks against the oracle)."""
    from waveforms.glfsr import PNSequence
    from waveforms_amd.link import SOQPSKLink

    link = SOQPSKLink(n, SPS, detector=detector, fuse=15, private_ctx=True)
    link.run_block(ebn0, seed=seed)
    counts = link.result()
    lay = link.layout()
    rb, calls = lay["row_bytes"], lay["calls"]
    rows = link.workspace[lay["off_mf"]:lay["off_mf"] + calls * rb].clone().view(dtype=_torch().float64)
    tx = PNSequence(23).generate(n, device=True)
    del link
    return rows, rb, tx, counts


def _torch():
    import torch

    return torch


def _unpack_rows(rows):
    """Packed rows -> 48-byte rows holding the same four components per call (zeros elsewhere: the 4-state detectors
    read only these four of a row's six, wf_viterbi.hip: vit_components)."""
    torch = _torch()
    p = rows.view(-1, 4)
    full = torch.zeros((p.shape[0], 3, 2), dtype=torch.float64, device=p.device)
    full[:, 1, 0], full[:, 1, 1] = p[:, 0], p[:, 1]
    full[0::2, 0, 0], full[0::2, 2, 1] = p[0::2, 2], p[0::2, 3]
    full[1::2, 0, 1], full[1::2, 2, 0] = p[1::2, 2], p[1::2, 3]
    return full


@pytest.mark.gpu
@pytest.mark.parametrize("detector", ["PT", "PAM"])
@pytest.mark.parametrize("ebn0", [4.0, 10.0])
def test_soft_decisions_are_the_ml_sequence(soft_ctx, detector, ebn0):
    """λ < 0 is the length-64 window detector's decision (its output k + 63 pairs with λ_k), away from the last 64."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    rows, rb, _tx, _ = _link_rows(1_000_000, detector, ebn0)
    assert rb == 32
    _llr, bits = dev.viterbi_soft(rows, True, 0, 32, ctx=soft_ctx)
    wbits, _ = dev.viterbi_detect_window(_unpack_rows(rows), 64, True, ctx=soft_ctx)
    n = bits.numel()
    soft, win = _hip.to_host(bits)[:n - 64], _hip.to_host(wbits)[63:n - 1]
    assert _counters(dev, soft_ctx)[0] == 0
    diff = np.flatnonzero(soft != win)
    assert diff.size == 0, f"{diff.size} differences, first at {diff[:8]}"


@pytest.mark.gpu
def test_soft_full_size_link_rows_any_warmup(soft_ctx):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    rows, rb, _tx, _ = _link_rows(10_000_000, "PT", 4.0)
    _hip.set_option(soft_ctx, _hip.WF_OPT_DET_FINAL_VERIFY, 1)
    _counters(dev, soft_ctx)
    a_llr, a_bits = dev.viterbi_soft(rows, True, 0, rb, ctx=soft_ctx)
    assert _counters(dev, soft_ctx)[0] == 0
    b_llr, b_bits = dev.viterbi_soft(rows, True, 6, rb, ctx=soft_ctx)
    assert _counters(dev, soft_ctx)[0] == 0
    torch = _torch()
    assert torch.equal(a_llr.view(torch.int64), b_llr.view(torch.int64))
    assert torch.equal(a_bits, b_bits)


@pytest.mark.gpu
def test_soft_llr_is_ordered(soft_ctx):
    """At 4 dB the error rate of λ < 0 falls across unit-wide bins of |λ/σ²| (bins with >= 200 errors).  The absolute
    scale is not tested: the PT metric is an approximation and λ/σ² is over-confident."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.link import sigma_for_ebn0

    ebn0 = 4.0
    rows, rb, tx, _ = _link_rows(2_000_000, "PT", ebn0)
    llr, bits = dev.viterbi_soft(rows, True, 0, rb, ctx=soft_ctx)
    llr, bits, tx = _hip.to_host(llr), _hip.to_host(bits), _hip.to_host(tx)
    m = min(tx.size, bits.size - 1)
    err = bits[1:1 + m] != tx[:m]
    x = np.abs(llr[1:1 + m]) / sigma_for_ebn0(ebn0, SPS) ** 2
    b = np.floor(x).astype(np.int64)
    nb = int(b.max()) + 1
    errs, tot = np.bincount(b, weights=err, minlength=nb), np.bincount(b, minlength=nb)
    keep = np.flatnonzero(errs >= 200)
    rates = errs[keep] / tot[keep]
    assert keep.size >= 4, (errs, tot)
    assert np.all(np.diff(rates) < 0), list(zip(keep.tolist(), rates.tolist()))
