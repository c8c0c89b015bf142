"""Framed coded links, the four operations on their own: the randomiser, the host statements of build / search / gather /
scatter (waveforms_amd/encoding/framing.py, written from the definitions in include/wfhip.h) on hand-made and noisy λ, and
on the GPU every entry point against its host statement BITWISE."""
from __future__ import annotations

import ctypes
import types

import numpy as np
import pytest

from waveforms_amd.encoding import framing as FR
from waveforms_amd.encoding import ldpc


def _code(n_tx, k=None):
    return types.SimpleNamespace(n_tx=n_tx, k=k or n_tx // 2)


def _burst(fr, rng, nframes, lead, mu=4.0, noise=0.0, tail=0, invert=False):
    """(λ, coded bits): ``lead`` random bits, ``nframes`` frames of random codeword bits, ``tail`` random bits; λ = ±mu by the
    bit (+ for 0) plus Gaussian noise, negated when ``invert``."""
    tx = rng.integers(0, 2, (nframes, fr.n_tx), dtype=np.uint8)
    bits = np.concatenate((rng.integers(0, 2, lead, dtype=np.uint8), fr.frame_host(tx), rng.integers(0, 2, tail, dtype=np.uint8)))
    lam = mu * (1.0 - 2.0 * bits)
    if noise:
        lam = lam + noise * rng.standard_normal(lam.size)
    return (-lam if invert else lam), tx


# ------------------------------------------------------------------------------------------------ CPU
def test_randomizer_first_bytes_and_period():
    pn = FR.randomizer_bits(40)
    assert np.packbits(pn).tobytes() == bytes.fromhex("FF480EC09A")
    long = FR.randomizer_bits(3 * 255 + 17)
    assert np.array_equal(long[255:], long[:-255])
    assert not any(np.array_equal(long[d:d + 255], long[:255]) for d in range(1, 255))
    assert FR.randomizer_bits(3).tolist() == [1, 1, 1] and FR.randomizer_bits(0).size == 0


def test_frame_layout():
    fr = FR.Framing(_code(10), marker=0b1011, marker_bits=4)
    tx = np.zeros((2, 10), np.uint8)
    out = fr.frame_host(tx).reshape(2, 14)
    assert out[:, :4].tolist() == [[1, 0, 1, 1]] * 2
    assert np.array_equal(out[0, 4:], FR.randomizer_bits(10)) and np.array_equal(out[1, 4:], out[0, 4:])
    assert FR.Framing(ldpc.demo_code()).period == 2112 and FR.DEFAULT_MARKER == 0x034776C7272895B0
    with pytest.raises(ValueError):
        FR.Framing(_code(10), marker_bits=65)
    with pytest.raises(ValueError):
        FR.Framing(_code(10), marker_bits=0)


@pytest.mark.parametrize("randomize", [True, False])
@pytest.mark.parametrize("sigma", [1, -1])
def test_frame_then_gather_returns_the_codeword_signs(randomize, sigma):
    fr = FR.Framing(ldpc.demo_code(), randomize=randomize)
    P = fr.period
    for lead in (0, 1, 37, P - 1):
        rng = np.random.default_rng(lead)
        lam, tx = _burst(fr, rng, 3, lead, tail=5, invert=sigma < 0)
        out = fr.gather_host(lam, lead, sigma, 3)
        assert out.shape == (3, fr.n_tx) and np.array_equal(out < 0, tx == 1) and np.all(np.abs(out) == 4.0)
        # a fourth frame is mostly beyond the burst: +0 there
        more = fr.gather_host(lam, lead, sigma, 4)
        assert np.array_equal(more[:3], out) and np.all(more[3, 5:] == 0) and not np.signbit(more[3, 5:]).any()


def test_search_on_hand_made_llrs():
    fr = FR.Framing(_code(50), marker=0xA5F1, marker_bits=16)
    P = fr.period
    rng = np.random.default_rng(7)
    lam, _ = _burst(fr, rng, 5, 23, tail=16)
    (p, s, best, other), G = fr.search_host(lam)
    assert (p, s) == (23, 1) and best == 0.0 and G[0, 23] == 0.0 and other < 0
    assert np.all(np.delete(G.reshape(-1), 23) < 0)
    (p, s, best, other), Gn = fr.search_host(-lam)
    assert (p, s) == (23, -1) and best == 0.0 and np.array_equal(Gn[1], G[0]) and np.array_equal(Gn[0], G[1])
    (p, s, best, other), Gz = fr.search_host(np.zeros(lam.size))
    assert (p, s, best, other) == (0, 1, 0.0, 0.0) and np.all(Gz == 0)
    with pytest.raises(ValueError):
        fr.search_host(np.zeros(P + fr.L - 1))


def test_search_value_is_minus_twice_the_disagreeing_magnitude():
    fr = FR.Framing(_code(20), marker=0x2D, marker_bits=6)
    rng = np.random.default_rng(3)
    lam = rng.standard_normal(fr.period + fr.L + 9)
    _, G = fr.search_host(lam)                                   # F = 1: G is M itself
    s = 1.0 - 2.0 * fr.marker_host
    for p in (0, 5, fr.period - 1):
        w = lam[p:p + fr.L]
        assert G[0, p] == pytest.approx(-2 * np.abs(w[np.sign(w) != s]).sum(), abs=1e-12)
        assert G[1, p] == pytest.approx(-2 * np.abs(w[np.sign(w) == s]).sum(), abs=1e-12)


def test_lock_under_noise_from_the_host_forms():
    """Demo code (P = 2112), 16 frames, λ = ±0.7 + unit Gaussian (24 % raw bit errors), 50 seeded trials with random
    lead_bits and polarity: every trial locks correctly."""
    fr = FR.Framing(ldpc.demo_code())
    rng = np.random.default_rng(20261016)
    for trial in range(50):
        lead = int(rng.integers(0, fr.period))
        inv = bool(rng.integers(0, 2)) if trial >= 25 else False
        lam, _ = _burst(fr, rng, 16, lead, mu=0.7, noise=1.0, tail=16, invert=inv)
        (p, s, best, other), _ = fr.search_host(lam)
        assert (p, s) == (lead, -1 if inv else 1), (trial, lead, p, s, best - other)


def test_scatter_host_leaves_the_rest_alone():
    fr = FR.Framing(_code(12), marker=0b110, marker_bits=3)
    rng = np.random.default_rng(1)
    ext = rng.standard_normal(2 * 12).astype(np.float32)
    prior = rng.standard_normal(40).astype(np.float32)
    out = fr.scatter_host(ext, 4, -1, prior, marker_prior=0.0)
    r = 1.0 - 2.0 * fr.pn_host
    assert np.array_equal(out[:7], prior[:7]) and np.array_equal(out[19:22], prior[19:22]) and np.array_equal(out[34:], prior[34:])
    assert np.array_equal(out[7:19], (-r * ext[:12]).astype(np.float32)) and np.array_equal(out[22:34], (-r * ext[12:]).astype(np.float32))
    out = fr.scatter_host(ext, 4, 1, prior, marker_prior=9.0)
    assert out[4:7].tolist() == [-9.0, -9.0, 9.0] and out[19:22].tolist() == [-9.0, -9.0, 9.0]
    short = fr.scatter_host(ext, 4, 1, prior[:25], marker_prior=9.0)
    assert short.size == 25 and np.array_equal(short[22:25], (r[:3] * ext[12:15]).astype(np.float32))


def test_frame_entry_points_exported_and_bound():
    from waveforms_amd import _hip, device

    lib = _hip.lib()
    for name in ("wf_frame_build", "wf_frame_search", "wf_frame_gather", "wf_frame_scatter"):
        assert name in _hip.SIGNATURES and hasattr(lib, name)
        assert callable(getattr(device, name[3:]))


def test_frame_argument_validation_without_a_gpu():
    """Each refused argument returns WF_ERR_VALUE before the context (a fake one: no device exists here) is touched."""
    from waveforms_amd import _hip

    lib = _hip.lib()
    V = _hip.WF_ERR_VALUE
    buf = (ctypes.c_double * 64)()
    fake = p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 2)
    M = FR.DEFAULT_MARKER
    b = lib.wf_frame_build
    for args in ((None, p, 1, 8, M, 8, p, p), (fake, None, 1, 8, M, 8, p, p), (fake, p, 1, 8, M, 8, p, None), (fake, p, 1, 8, M, 0, p, p),
                 (fake, p, 1, 8, M, 65, p, p), (fake, p, 0, 8, M, 8, p, p), (fake, p, 1, 0, M, 8, p, p)):
        assert b(*args, None) == V, args
    s = lib.wf_frame_search
    for args in ((None, p, 100, M, 8, 20, p, p), (fake, None, 100, M, 8, 20, p, p), (fake, p, 100, M, 8, 20, None, p), (fake, p, 100, M, 0, 20, p, p),
                 (fake, p, 100, M, 65, 200, p, p), (fake, p, 100, M, 8, 8, p, p), (fake, p, 100, M, 8, 7, p, p), (fake, p, 27, M, 8, 20, p, p),
                 (fake, p, 100, M, 8, (1 << 23) + 1, p, p), (fake, odd, 100, M, 8, 20, p, p), (fake, p, 100, M, 8, 20, odd, p),
                 (fake, p, 100, M, 8, 20, p, odd)):
        assert s(*args, None) == V, args
    g = lib.wf_frame_gather
    for args in ((None, p, 100, p, 8, 12, p, 2, p), (fake, None, 100, p, 8, 12, p, 2, p), (fake, p, 100, None, 8, 12, p, 2, p),
                 (fake, p, 100, p, 8, 12, p, 2, None), (fake, p, 100, p, 0, 12, p, 2, p), (fake, p, 100, p, 65, 12, p, 2, p),
                 (fake, p, 100, p, 8, 12, p, 0, p), (fake, p, 100, p, 8, 0, p, 2, p), (fake, p, 0, p, 8, 12, p, 2, p), (fake, odd, 100, p, 8, 12, p, 2, p)):
        assert g(*args, None) == V, args
    c = lib.wf_frame_scatter
    for args in ((None, p, 12, p, M, 8, 12, p, 2, 0.0, p, 100), (fake, None, 12, p, M, 8, 12, p, 2, 0.0, p, 100),
                 (fake, p, 12, None, M, 8, 12, p, 2, 0.0, p, 100), (fake, p, 12, p, M, 8, 12, p, 2, 0.0, None, 100),
                 (fake, p, 11, p, M, 8, 12, p, 2, 0.0, p, 100), (fake, p, 12, p, M, 0, 12, p, 2, 0.0, p, 100),
                 (fake, p, 12, p, M, 65, 12, p, 2, 0.0, p, 100), (fake, p, 12, p, M, 8, 12, p, 2, float("inf"), p, 100),
                 (fake, p, 12, p, M, 8, 12, p, 2, float("nan"), p, 100), (fake, p, 12, p, M, 8, 12, p, 0, 0.0, p, 100),
                 (fake, p, 12, p, M, 8, 12, p, 2, 0.0, p, 0), (fake, odd, 12, p, M, 8, 12, p, 2, 0.0, p, 100)):
        assert c(*args, None) == V, args


def test_frame_kernels_resources():
    """Wave64 kernels without spills or scratch; the search keeps 8 waves per SIMD (at most 64 VGPRs) and 2.5 KiB of LDS per
    workgroup, so LDS never limits its occupancy."""
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
    import kernel_resources as kr
    from waveforms_amd.csrc.build import build

    so = build(verbose=False)
    tab = {k: v for k, v in kr.kernel_table(so).items() if k.startswith("frame_")}
    assert set(tab) == {f"frame_{n}_kernel" for n in ("build", "search", "fold", "pick", "gather", "scatter")}, sorted(tab)
    asm = kr.loop_spill_counts(so, "frame_")
    for name, row in tab.items():
        assert row["vgpr_spill_count"] == 0 and row["sgpr_spill_count"] == 0 and row["private_segment_fixed_size"] == 0, (name, row)
        assert asm[name]["scratch_load_in_loop"] == 0 and asm[name]["scratch_store_in_loop"] == 0, (name, asm[name])
        assert kr.waves_per_simd(row["vgpr_count"], row.get("agpr_count", 0)) >= 8, (name, row["vgpr_count"])
    assert tab["frame_search_kernel"]["group_segment_fixed_size"] == (256 + 64) * 8


# ------------------------------------------------------------------------------------------------ GPU
def _u64(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _lock_host(lock):
    a = lock.cpu().numpy()
    return int(a[0]), int(a[1]), a[2:].view(np.float64)


def _check_search(fr, lam):
    from waveforms_amd import _hip

    d = _hip.to_device(lam)
    lock, folded = fr.search(d, want_folded=True)
    lock2, none = fr.search(d)                                   # folded values kept in the context's scratch
    _hip.device_check()
    (p, s, best, other), G = fr.search_host(lam)
    assert none is None and np.array_equal(lock.cpu().numpy(), lock2.cpu().numpy())
    assert np.array_equal(_u64(folded.cpu().numpy()), _u64(G))
    gp, gs, gv = _lock_host(lock)
    assert (gp, gs) == (p, s) and np.array_equal(_u64(gv), _u64([best, other]))
    return lock, (p, s)


def _check_gather_scatter(fr, lam, lock, p, s, ncw, rng, marker_prior):
    from waveforms_amd import _hip

    d = _hip.to_device(lam)
    out = fr.gather(d, lock, ncw)
    assert np.array_equal(_u64(out.cpu().numpy()), _u64(fr.gather_host(lam, p, s, ncw)))
    for stride, nprior in ((fr.n_tx, lam.size), (fr.n_tx + 3, lam.size), (fr.n_tx, max(1, lam.size - fr.n_tx // 2)), (fr.n_tx, p + fr.L + 1)):
        ext = rng.standard_normal((ncw - 1) * stride + fr.n_tx).astype(np.float32)
        ext[::7] = 0.0
        ext[3::11] = -0.0
        prior = rng.standard_normal(nprior).astype(np.float32)
        got = fr.scatter(_hip.to_device(ext), lock, _hip.to_device(prior), marker_prior, stride)
        assert np.array_equal(_u32(got.cpu().numpy()), _u32(fr.scatter_host(ext, p, s, prior, marker_prior, stride)))
    _hip.device_check()


SHAPES = [  # (marker bits, n_tx, frames, lead bits, tail, inverted)
    (64, 2048, 1, 0, 64, False),                # F = 1
    (64, 2048, 1, 2111, 64, True),
    (32, 100, 45, 131, 40, False),              # P = 132: not a multiple of 64; F = 45: not a multiple of the slice
    (32, 100, 70, 0, 5, True),
    (1, 7, 67, 7, 3, False),                    # L = 1 (an ambiguous marker: only the equality with the host form matters)
    (64, 2048, 33, 37, 16, False),
    (17, 300, 64, 1, 0, True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("L,n_tx,nframes,lead,tail,invert", SHAPES)
def test_gpu_entry_points_bitwise(L, n_tx, nframes, lead, tail, invert):
    from waveforms_amd import _hip

    fr = FR.Framing(_code(n_tx), marker=FR.DEFAULT_MARKER >> (64 - L), marker_bits=L)
    rng = np.random.default_rng(L * 1000 + nframes)
    lam, tx = _burst(fr, rng, nframes, lead, mu=1.5, noise=1.0, tail=tail, invert=invert)
    built = fr.build(_hip.to_device(tx))
    assert built.shape == (nframes, fr.period) and np.array_equal(built.cpu().numpy().reshape(-1), fr.frame_host(tx))
    plain = FR.Framing(_code(n_tx), marker=fr.marker, marker_bits=L, randomize=False)
    assert np.array_equal(plain.build(_hip.to_device(tx)).cpu().numpy().reshape(-1), plain.frame_host(tx))
    lock, (p, s) = _check_search(fr, lam)
    if L >= 17:
        assert (p, s) == (lead, -1 if invert else 1)
    for mp in (0.0, 50.0):
        _check_gather_scatter(fr, lam, lock, p, s, nframes + 1, rng, mp)      # one frame more than the burst holds
        _check_gather_scatter(plain, lam, lock, p, s, nframes, rng, mp)


@pytest.mark.gpu
def test_gpu_search_all_zero_and_signed_zero_input():
    fr = FR.Framing(_code(100), marker=0xDEADBEEF, marker_bits=32)
    lock, (p, s) = _check_search(fr, np.zeros(5000))
    assert (p, s) == (0, 1)
    _check_search(fr, -np.zeros(5000))
    _check_gather_scatter(fr, -np.zeros(5000), lock, p, s, 3, np.random.default_rng(0), 50.0)


@pytest.mark.gpu
@pytest.mark.parametrize("invert", [False, True])
def test_gpu_search_of_a_ten_million_value_burst(invert):
    fr = FR.Framing(ldpc.demo_code())
    rng = np.random.default_rng(5)
    nframes = 10_000_000 // fr.period
    lam, _ = _burst(fr, rng, nframes, 1234, mu=0.7, noise=1.0, tail=10_000_000 - 1234 - nframes * fr.period, invert=invert)
    assert lam.size == 10_000_000
    lock, (p, s) = _check_search(fr, lam)
    assert (p, s) == (1234, -1 if invert else 1)
    _check_gather_scatter(fr, lam, lock, p, s, nframes, rng, 50.0)
