"""Coarse carrier frequency acquisition (waveforms_amd/sync/coarse.py; include/wfhip.h: wf_coarse_lines_c128, wf_coarse_estimate,
wf_carrier_offset_dev_c128).

CPU: the entry points and their refusals, the host statements on the reference PT chain's signal - accuracy with and without a
clock drift and noise, the bias the per-line step removes, the handover to the fine carrier recovery - and the estimate's edges on
crafted spectra.
GPU: every device stage against its host statement within bounds that follow from the arithmetic (stated at each test).
"""
import ctypes
import math

import numpy as np
import pytest

from test_carrier import _rot_bound, _up_to_polarity
from test_timing import SPS, _chain
from waveforms_amd.sync import carrier as C
from waveforms_amd.sync import coarse as K
from waveforms_amd.sync import timing as T

W = C.DEFAULT_WINDOW
NAMES = ("wf_coarse_lines_c128", "wf_coarse_estimate", "wf_carrier_offset_dev_c128")
FINE_LIMIT = C.MAX_DRIFT_TURNS / (SPS * W)                 # 2.4e-5 cycles per sample: what the fine carrier recovery follows
DRIFT_LIMIT = T.MAX_DRIFT_SAMPLES / (SPS * W)              # 7.8e-4: what the timing trackers follow
OFFSETS = (-0.025, 0.0, 1e-5, 0.0123, 0.025)
DRIFTS = (0.0, DRIFT_LIMIT, -DRIFT_LIMIT)


# ------------------------------------------------------------------------------------------------ CPU
def test_coarse_entry_points_exported_bound_and_declared():
    from pathlib import Path

    from waveforms_amd import _hip, device

    header = (Path(__file__).resolve().parent.parent / "include" / "wfhip.h").read_text()
    lib = _hip.lib()
    for name in NAMES:
        assert name in _hip.SIGNATURES and hasattr(lib, name) and f"int {name}(" in header, name
    assert "wf_coarse_scratch_doubles" in _hip.SIGNATURES and "int64_t wf_coarse_scratch_doubles(" in header
    for name in ("coarse_lines", "coarse_estimate", "carrier_offset_dev"):
        assert callable(getattr(device, name))
    for name in ("line_samples_host", "line_spectra_host", "coarse_estimate_host", "correct_host"):
        assert callable(getattr(K, name))
    rec = K.CoarseFrequency(SPS)
    assert (rec.sps, rec.nfft, rec.smooth, rec.search) == (8, 4096, 4, 4)
    assert K.CoarseFrequency(10, smooth=1).smooth == 1 and K.CoarseFrequency(10).smooth == 5
    assert K.MAX_OFFSET_BITS == 0.2 and K.MIN_BITS >= K.DEFAULT_NFFT
    # the scratch: two lines of nfft bins per workgroup, at most 256 workgroups; -1 where the burst fills no segment
    assert lib.wf_coarse_scratch_doubles(64 * 8 + 3, 8, 64, 4) == 2 * 64 and lib.wf_coarse_scratch_doubles(64 * 8 + 2, 8, 64, 4) == -1
    assert lib.wf_coarse_scratch_doubles(10 ** 7 * 8, 8, 4096, 4) == 256 * 2 * 4096 and lib.wf_coarse_scratch_doubles(700 * 64 * 8 + 3, 8, 64, 4) == 256 * 128
    for bad in ((0, 8, 64, 4), (10 ** 6, 1, 64, 4), (10 ** 6, 65, 64, 4), (10 ** 6, 8, 96, 4), (10 ** 6, 8, 32, 4), (10 ** 6, 8, 8192, 4), (10 ** 6, 8, 64, 0),
                (10 ** 6, 8, 64, 1025)):
        assert lib.wf_coarse_scratch_doubles(*bad) == -1, bad


def test_coarse_argument_validation_without_a_gpu():
    """Bad arguments return WF_ERR_VALUE before anything is launched (a fake context: no device exists here)."""
    from waveforms_amd import _hip

    lib = _hip.lib()
    fake = ctypes.create_string_buffer(1 << 16)
    buf = ctypes.create_string_buffer(1 << 17)
    a = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    b, c, d = a + 32768, a + 65536, a + 98304
    V = _hip.WF_ERR_VALUE
    nan, inf = float("nan"), float("inf")
    # wf_coarse_lines_c128(ctx, r, n, sps, smooth, nfft, window, scratch, spectra, stream): 64 bits of 8 samples and the halo
    n = 64 * 8 + 3
    good = (fake, a, n, 8, 4, 64, b, c, d)
    for i, v in ((0, None), (1, None), (6, None), (7, None), (8, None), (2, 0), (2, n - 1), (2, (1 << 40) + 1), (3, 1), (3, 65), (4, 0), (4, 1025), (5, 32),
                 (5, 96), (5, 8192), (1, a + 8), (6, b + 4), (7, c + 4), (8, d + 4), (8, a), (8, a + 16 * n - 8), (8, b), (8, c), (8, c + 1016), (7, a),
                 (7, b + 8)):
        args = good[:i] + (v,) + good[i + 1:]
        assert lib.wf_coarse_lines_c128(*args, None) == V, args
    # wf_coarse_estimate(ctx, spectra, nfft, sps, search, found, stream)
    good = (fake, a, 64, 8, 4, b)
    for i, v in ((0, None), (1, None), (5, None), (2, 32), (2, 100), (2, 8192), (3, 1), (3, 65), (4, 0), (4, 31), (1, a + 4), (5, b + 4), (5, a), (5, a + 1016)):
        args = good[:i] + (v,) + good[i + 1:]
        assert lib.wf_coarse_estimate(*args, None) == V, args
    # wf_carrier_offset_dev_c128(ctx, in, n, nu, gain, first_index, out, stream): in place or disjoint
    good = (fake, a, 10, b, -1.0, 0, c)
    for i, v in ((0, None), (1, None), (3, None), (6, None), (2, 0), (4, nan), (4, inf), (5, -1), (5, 1 << 53), (1, a + 8), (6, c + 8), (3, b + 4), (6, a + 16),
                 (6, a + 144), (3, c + 8), (3, c + 152)):
        args = good[:i] + (v,) + good[i + 1:]
        assert lib.wf_carrier_offset_dev_c128(*args, None) == V, args
    # ... and the Python layer's own
    for kw in ({"nfft": 96}, {"nfft": 32}, {"nfft": 8192}, {"smooth": 0}, {"search": 0}, {"search": 2047}, {"nfft": 64, "search": 31}, {"sps": 1}):
        with pytest.raises(ValueError):
            K.CoarseFrequency(**{"sps": SPS, **kw})
    assert K.CoarseFrequency(SPS, nfft=64, search=30).search == 30
    with pytest.raises(ValueError):
        K.line_spectra_host(np.zeros((2, 63), dtype=np.complex128), 64)
    with pytest.raises(ValueError):
        K.coarse_estimate_host(np.ones((2, 64)), SPS, 31)


@pytest.fixture(scope="module")
def burst(oracle):
    """8 192 noiseless bits of the reference PT chain's signal, and a fixed numpy noise at channel Eb/N0 1 dB."""
    sig = _chain(oracle, 8192)[0]
    rng = np.random.default_rng(11)
    noise = oracle.sigma_for_ebn0(1.0, SPS) * (rng.standard_normal(sig.size) + 1j * rng.standard_normal(sig.size))
    return sig, noise


def _impaired(sig, nu, eps):
    """The received samples: the clock drift first, the carrier behind it, so that nu IS the carrier frequency in cycles per
    received sample (the links apply the carrier first: the drift then scales it to nu (1 + eps), 2e-5 off at these limits)."""
    return C.carrier_offset_host(T.timing_offset_host(sig, 0.0, eps) if eps else sig, 0.7, nu)


@pytest.fixture(scope="module")
def host_spectra(burst):
    """The line periodograms of every (nu, eps, noisy) case, once."""
    sig, noise = burst
    out = {}
    for nu in OFFSETS:
        for eps in DRIFTS:
            x = _impaired(sig, nu, eps)
            for noisy in (False, True):
                out[nu, eps, noisy] = K.line_spectra_host(K.line_samples_host(x + noise[:x.size] if noisy else x, SPS, 4), 4096)
    return out


def test_host_accuracy_with_and_without_drift_and_noise(host_spectra):
    """nfft 4096, smooth 4, 8 192 bits (two segments): noiseless |nu^ - nu| <= a quarter of the fine recovery's limit (6.1e-6),
    at channel Eb/N0 1 dB half of it (1.2e-5); under a drift at the timing trackers' limit eps^ has the sign of eps and lies within
    1.5e-4 of it.  Measured here: 4.5e-7 noiseless, 1.5e-6 noisy, eps within 5.8e-6 and 5.4e-5."""
    worst = {False: [0.0, 0.0], True: [0.0, 0.0]}
    for (nu, eps, noisy), P in host_spectra.items():
        found = K.coarse_estimate_host(P, SPS)
        assert np.isfinite(found).all() and found[2] > found[3] > 0.0
        err = abs(found[0] - nu)
        worst[noisy][0] = max(worst[noisy][0], err)
        assert err <= FINE_LIMIT / (2.0 if noisy else 4.0), (nu, eps, noisy, err)
        if eps:
            worst[noisy][1] = max(worst[noisy][1], abs(found[1] - eps))
            assert found[1] * eps > 0.0 and abs(found[1] - eps) <= 1.5e-4, (nu, eps, noisy, found[1])
    for noisy, (e_nu, e_eps) in worst.items():
        print(f"{'Eb/N0 1 dB' if noisy else 'noiseless'}: max |nu^ - nu| = {e_nu:.2e} cycles per sample, max |eps^ - eps| = {e_eps:.2e}")


def test_the_split_estimate_removes_the_bias_of_the_summed_periodogram(host_spectra):
    """Under a clock drift at the limit the two lines sit 3.2 bins apart: the vertex of the SUMMED periodogram alone is off by more
    than 2e-5 (the whole fine budget), the mean of the two lines' own vertices is not - the per-line step is exercised."""
    for (nu, eps, noisy), P in host_spectra.items():
        if eps and not noisy:
            summed, split = K.summed_vertex_host(P, SPS) - nu, K.coarse_estimate_host(P, SPS)[0] - nu
            print(f"nu {nu:+.5f}, eps {eps:+.2e}: summed periodogram {summed:+.2e}, split {split:+.2e}")
            assert abs(summed) > 2e-5 and abs(split) <= FINE_LIMIT / 4.0
            star, im, ip = K.coarse_peaks_host(P)
            assert im != ip and star in (im, ip)


def test_handover_to_the_fine_carrier_recovery(oracle):
    """4 000 noiseless bits 0.02 cycles per sample (0.16 of the bit rate, 800 times the fine limit) and 40 degrees off, nfft 1024:
    ``correct_host``, the PT bank and ``carrier.recover_host`` decide every bit as the genie outside a guard of one window at each
    end, modulo the polarity; without ``correct_host`` the same chain does not."""
    sig, _noise, taps, first, ncols = _chain(oracle, 4000)
    genie = C.map_branch_host(T.mf_bank_resample_host(sig, taps, first, SPS, ncols)[0])[1]
    bad = C.carrier_offset_host(sig, math.radians(40.0), 0.02)
    fixed, found = K.correct_host(bad, SPS, nfft=1024)
    print(f"nu^ - nu = {found[0] - 0.02:+.2e}, eps^ = {found[1]:+.2e}, peak / mean = {found[2] / found[3]:.0f}")
    assert abs(found[0] - 0.02) <= FINE_LIMIT
    for samples, lost in ((fixed, False), (bad, True)):
        rows = C.recover_host(T.mf_bank_resample_host(samples, taps, first, SPS, ncols)[0])[0]
        errs = _up_to_polarity(C.map_branch_host(rows)[1], genie, W)
        assert (errs > 100) if lost else (errs == 0), (lost, errs)


def _crafted(L=64, R=4):
    """Spectra that put the estimate at its edges -> [(name, P float64[2, L], (i*, i₋, i₊))]."""
    rng = np.random.default_rng(9)
    base = rng.uniform(1.0, 2.0, (2, L))
    out = []
    P = base.copy()
    P[:, 20] = P[:, 40] = 50.0                                  # an exact tie of the summed maximum: the first
    P[0, 18] = P[0, 22] = 60.0                                  # (outside no bin of the sum is larger: 60 + 2 < 100) per-line ties: the first
    P[1, 17] = P[1, 24] = 55.0
    out.append(("ties", P, (20, 18, 17)))
    P = base.copy()
    P[:, R + 1] = 30.0
    P[0, R] = 29.0                                              # an inadmissible bin of the sum, admissible to the line's own search
    out.append(("first admissible bin", P, (R + 1, R + 1, R + 1)))
    P = base.copy()
    P[:, L - R - 2] = 30.0
    P[:, L - 1] = 99.0                                          # never looked at
    out.append(("last admissible bin", P, (L - R - 2, L - R - 2, L - R - 2)))
    out.append(("all zero", np.zeros((2, L)), (R + 1, 1, 1)))
    out.append(("all equal", np.full((2, L), 3.0), (R + 1, 1, 1)))
    P = base.copy()
    P[:, 30] = 40.0
    P[0, 31] = float("nan")
    P[1, 29] = float("inf")                                     # the largest of the sum and of its line; the NaN never wins; both vertices are guarded
    out.append(("not finite", P, (29, 30, 29)))
    return out


def test_estimate_edges_on_crafted_spectra():
    L, R = 64, 4
    for name, P, want in _crafted(L, R):
        assert K.coarse_peaks_host(P, R) == want, name
        found = K.coarse_estimate_host(P, SPS, R)
        assert np.isfinite(found[:2]).all(), (name, found)
        if name in ("all zero", "all equal", "not finite"):      # d = 0 on both lines: the bins themselves
            assert found[0] == (0.5 * (want[1] + want[2]) - 0.5 * L) / (2.0 * L * SPS) and found[1] == (want[1] - want[2]) / L, (name, found)
    # the vertex of three points of a parabola in the log is where the parabola has it, and the guards give 0
    p = np.exp(-1.4 * (np.arange(5) - 2.3) ** 2)
    assert abs(K.vertex_host(p, 2) - 0.3) < 1e-12
    for bad in ([1.0, 0.0, 1.0], [1.0, 2.0, float("inf")], [2.0, 1.0, 2.0], [1.0, 1.0, 1.0], [1.0, -1.0, 1.0], [float("nan"), 2.0, 1.0]):
        assert K.vertex_host(np.array(bad), 1) == 0.0, bad


# ------------------------------------------------------------------------------------------------ GPU
def _msk(rng, nbits, sps, nu, sigma):
    """A random h = 1/2 CPM (rectangular pulse) at nu cycles per sample in noise: the squared signal has the two lines."""
    steps = np.repeat(rng.integers(0, 2, nbits) * 2.0 - 1.0, sps) * (0.5 * math.pi / sps)
    phase = np.cumsum(steps) + 2.0 * math.pi * nu * np.arange(nbits * sps)
    return np.exp(1j * phase) + sigma * (rng.standard_normal(phase.size) + 1j * rng.standard_normal(phase.size))


# (nfft, whole segments, smooth, sps, noise only)
LINE_CASES = ((64, 1, 1, 8, False), (64, 3, 4, 8, False), (256, 3, 5, 10, False), (256, 1, 4, 8, True), (4096, 1, 4, 8, False), (4096, 3, 5, 10, False),
              (64, 700, 4, 8, False),
              # ... and one whose tile of samples does not fit into LDS beside the FFT: the lanes read their samples from memory themselves
              (4096, 1, 4, 16, False))


@pytest.fixture(scope="module")
def line_cases():
    """Per case of LINE_CASES: (samples, the host spectra, the device spectra of two launches), computed once."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    out = []
    for j, (L, nseg, S, sps, noise_only) in enumerate(LINE_CASES):
        rng = np.random.default_rng(100 + j)
        nbits = nseg * L + 3                                    # a ragged tail: three more bits, one more sample and the halo
        x = _msk(rng, nbits + 1, sps, 0.011 if not noise_only else 0.0, 0.3)[:nbits * sps + S]
        if noise_only:
            x = rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size)
        want = K.line_spectra_host(K.line_samples_host(x, sps, S), L)
        d_x, d_w = _hip.to_device(x), _hip.to_device(np.hanning(L))
        got = [_hip.to_host(dev.coarse_lines(d_x, sps, S, L, d_w)) for _ in range(2)]
        out.append((x, want, got))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("j", range(len(LINE_CASES)), ids=[f"nfft{c[0]}-nseg{c[1]}-S{c[2]}-sps{c[3]}{'-noise' if c[4] else ''}" for c in LINE_CASES])
def test_coarse_lines_against_the_host_statement(line_cases, j):
    """|ΔP[b]| <= 1e-12 Σ_b P[b] per line: a radix-2 fp64 FFT's bin error is a small multiple of log2(L) 2^-53 ||x||, and by
    Parseval Σ_b P = L Σ ||x_s||² - the bound leaves about four decades for the device's sincospi against numpy's.  Two launches
    on the same input are bitwise equal."""
    _x, want, (got, again) = line_cases[j]
    assert got.shape == want.shape == (2, LINE_CASES[j][0])
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))
    for line in range(2):
        err, total = np.abs(got[line] - want[line]).max(), want[line].sum()
        print(f"line {line}: max |ΔP| / Σ P = {err / total:.2e}")
        assert err <= 1e-12 * total, (line, err, total)


@pytest.mark.gpu
def test_coarse_lines_refuses_a_burst_one_sample_short_of_a_segment():
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    L, sps, S = 64, 8, 4
    n = L * sps + S - 1                                         # exactly one segment
    rng = np.random.default_rng(1)
    d_x, d_w = _hip.to_device(rng.standard_normal(n) + 1j * rng.standard_normal(n)), _hip.to_device(np.hanning(L))
    assert dev.coarse_lines(d_x, sps, S, L, d_w).shape == (2, L)
    scratch, out = _hip.empty(2 * L, "float64"), _hip.empty((2, L), "float64")
    args = (_hip.ctx(), _hip.ptr(d_x), n - 1, sps, S, L, _hip.ptr(d_w), _hip.ptr(scratch), _hip.ptr(out), _hip.stream())
    assert _hip.lib().wf_coarse_lines_c128(*args) == _hip.WF_ERR_VALUE
    with pytest.raises(ValueError):
        dev.coarse_lines(d_x[:n - 1], sps, S, L, d_w)


def _estimate_matches(P, found, sps, R):
    """The device's estimate on the spectra P against the host statement on the same arrays.  The kernel exports no bin indices, so
    that i* and both i_σ are the host's is checked INDIRECTLY: T[i*] is the same sum of the same two doubles, and each line's
    f_σ = i_σ + d, recovered from the two outputs (f∓ = L/2 + 2 L sps nu ± L eps / 2), lies within 1e-6 bins of the host's own - another
    bin on one line moves its f_σ by a bin less two vertices of under half a bin each.  Then |Δnu| <= 1e-13 and |Δeps| <= 1e-11: one
    ulp of a log moves the vertex of a Hann lobe, whose curvature is about -2.8, by under 1e-13 bins."""
    want = K.coarse_estimate_host(P, sps, R)
    assert found[2] == want[2] or (np.isnan(found[2]) and np.isnan(want[2])), (found, want)
    L = P.shape[1]
    _star, im, ip = K.coarse_peaks_host(P, R)
    mid, half = 0.5 * L + 2.0 * L * sps * found[0], 0.5 * L * found[1]
    assert abs((mid + half) - (im + K.vertex_host(P[0], im))) <= 1e-6 and abs((mid - half) - (ip + K.vertex_host(P[1], ip))) <= 1e-6, (found, im, ip)
    assert abs(found[0] - want[0]) <= 1e-13 and abs(found[1] - want[1]) <= 1e-11, (found, want)
    assert abs(found[3] - want[3]) <= 1e-12 * abs(want[3]) or not np.isfinite(want[3]), (found, want)


@pytest.mark.gpu
def test_coarse_estimate_against_the_host_statement_on_the_device_spectra(line_cases):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    for (L, _nseg, _S, sps, noise_only), (_x, _want, (P, _again)) in zip(LINE_CASES, line_cases):
        for R in (1, L // 2 - 2, 4):
            found = _hip.to_host(dev.coarse_estimate(_hip.to_device(P), sps, R))
            _estimate_matches(P, found, sps, R)
        if not noise_only:                                     # the line is where the burst has it: 0.011 cycles per sample, to a bin
            assert abs(found[0] - 0.011) <= 1.0 / (2.0 * L * sps), (L, found)
    for name, P, _peaks in _crafted():
        found = _hip.to_host(dev.coarse_estimate(_hip.to_device(P), SPS, 4))
        assert np.isfinite(found[:2]).all(), (name, found)
        _estimate_matches(P, found, SPS, 4)


@pytest.mark.gpu
def test_carrier_offset_dev_is_bitwise_carrier_offset():
    """The frequency read from device memory and the gain applied there: the same bits as ``carrier_offset(signal, 0.0, g * nu)``
    for the host copy of nu, at index 1e9 too, in place and out of place."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    rng = np.random.default_rng(6)
    d_found = _hip.to_device(np.array([0.0123456789, 1e-4, 3.0, 1.0]))
    nu = float(_hip.to_host(d_found)[0])
    for n in (1, 255, 4097):
        d_x = _hip.to_device(rng.standard_normal(n) + 1j * rng.standard_normal(n))
        for g in (-1.0, 1.0):
            for first in (0, 10 ** 9):
                want = _hip.to_host(dev.carrier_offset(d_x, 0.0, g * nu, first))
                got = dev.carrier_offset_dev(d_x, d_found, g, first)
                assert got.data_ptr() != d_x.data_ptr() and np.array_equal(_hip.to_host(got).view(np.uint64), want.view(np.uint64)), (n, g, first)
                buf = d_x.clone()
                assert dev.carrier_offset_dev(buf, d_found, g, first, out=buf).data_ptr() == buf.data_ptr()
                assert np.array_equal(_hip.to_host(buf).view(np.uint64), want.view(np.uint64)), (n, g, first)
    with pytest.raises(ValueError):
        dev.carrier_offset_dev(d_x, d_found, 1.0, 0, out=d_x[1:])


@pytest.mark.gpu
def test_coarse_frequency_corrects_a_noisy_burst_as_the_host_statement(burst):
    """One 8 192-bit burst at channel Eb/N0 1 dB, 0.0123 cycles per sample off: the class's spectra within the lines' bound, its
    estimate within the estimate's bounds on those spectra and within the fine limit of the truth, its samples the host's
    correction by the DEVICE's estimate to the rounding ``carrier_offset`` documents; the stage marks are kept."""
    from waveforms_amd import _hip

    sig, noise = burst
    x = C.carrier_offset_host(sig, 0.7, 0.0123) + noise
    rec = K.CoarseFrequency(SPS)
    rec.times = True
    d_x = _hip.to_device(x)
    P = _hip.to_host(rec.spectra(d_x))
    want_P = K.line_spectra_host(K.line_samples_host(x, SPS, 4), 4096)
    for line in range(2):
        assert np.abs(P[line] - want_P[line]).max() <= 1e-12 * want_P[line].sum()
    out, d_found = rec.correct(d_x)
    found = _hip.to_host(d_found)
    assert set(rec.stage_times()) == {"lines", "estimate", "correct"}
    _estimate_matches(P, found, SPS, 4)
    assert np.array_equal(_hip.to_host(rec.estimate(d_x)), found)
    host_fixed, host_found = K.correct_host(x, SPS)
    print(f"nu^ - nu: device {found[0] - 0.0123:+.2e}, host {host_found[0] - 0.0123:+.2e}; peak / mean {found[2] / found[3]:.1f}")
    assert abs(found[0] - 0.0123) <= FINE_LIMIT / 2.0 and abs(found[0] - host_found[0]) <= 1e-9
    want = C.carrier_offset_host(x, 0.0, -1.0 * float(found[0]))
    assert (np.abs(_hip.to_host(out, True) - want) <= _rot_bound(x, C.carrier_phase_host(x.size, 0.0, -1.0 * float(found[0])))).all()
    buf = d_x.clone()
    assert rec.correct(buf, out=buf)[0].data_ptr() == buf.data_ptr()
    assert np.array_equal(_hip.to_host(buf), _hip.to_host(out))
