"""Framed coded links end to end: the CPU chains from the existing restatements plus the host statements of the framing
(waveforms_amd/encoding/framing.py), and on the GPU the four link classes with ``framing=`` / ``lead_bits=``: noiseless
bursts at every lead, the iterative loops pass by pass against their CPU restatement, and the cost of framing at equal
channel σ against the unframed link."""
from __future__ import annotations

import math

import numpy as np
import pytest

import test_cpm_idd as TCI
import test_idd as TI
import test_ldpc as TL
import test_soft_detector as TS
from test_cpm_idd import apref, ref  # noqa: F401 - module-scoped fixtures (the compiled definitions of the CPM detectors)
from waveforms_amd.encoding import framing as FR
from waveforms_amd.encoding import ldpc

SPS = 8


# ------------------------------------------------------------------------------------------------ CPU
def _framed_bits(code, fr, rng, ncw, lead, lg=1, pad=16):
    u = rng.integers(0, 2, (ncw, code.k), dtype=np.uint8)
    bits = np.concatenate((rng.integers(0, 2, lead, dtype=np.uint8), fr.frame_host(code.encode_host(u))))
    bits = np.concatenate((bits, np.zeros(-bits.size % lg + pad, np.uint8)))
    return u, bits


def _decode_located(code, fr, lam, lead, u):
    (p, s, best, other), _ = fr.search_host(lam)
    assert (p, s) == (lead, 1) and best > other
    info, _post, _its = TL.decode_restatement(code, fr.gather_host(lam, p, s, u.shape[0]), 1.0, 0.75, 50)
    assert np.array_equal(info, u)


def test_cpu_framed_soqpsk_chain_noiseless(oracle):
    """4 demo codewords behind 37 lead bits, SOQPSK-TG PT without noise: the search locks (37, +) and no information bit is
    wrong."""
    code = ldpc.demo_code()
    fr = FR.Framing(code)
    rng = np.random.default_rng(11)
    u, bits = _framed_bits(code, fr, rng, 4, 37)
    res = oracle.detection_run(bits, oracle.freq_pulse_soqpsk_tg(SPS), 0.25, SPS, 0.0, rng=rng, detector="PT", timing_offset=-1)
    llr, _ = TS.soft_restatement(oracle, np.asarray(res["mf_rows"]), True)
    _decode_located(code, fr, llr[1:], 37, u)               # transmitted bit j pairs with λ_{j+1}


@pytest.mark.parametrize("waveform,lead", [("multih", 37), ("pcmfm", 1)])
def test_cpu_framed_cpm_chain_noiseless(oracle, ref, waveform, lead):  # noqa: F811
    """The same for ARTM (an odd lead: codewords start inside a symbol, the burst is padded to whole symbols at its end) and
    PCM/FM."""
    code = ldpc.demo_code()
    fr = FR.Framing(code)
    spec, ospec, pulse, mapper = TCI._wave(oracle, waveform)
    lg = spec.bits_per_symbol
    rng = np.random.default_rng(12)
    u, bits = _framed_bits(code, fr, rng, 4, lead, lg, pad=8 * lg)
    res = oracle.cpm_detection_run(mapper(bits), pulse, SPS, ospec, sigma=None, rng=rng)
    rows = np.ascontiguousarray(res["rows"], dtype=np.complex128).reshape(-1, spec.nfilt)
    inc = TCI._increments(ref, spec, rows)
    lam = TCI._siso_batch(spec, inc[None], np.zeros((1, rows.shape[0] * lg), dtype=np.float32), 0.7)[0]
    assert lam.size >= lead + 4 * fr.period
    _decode_located(code, fr, lam, lead, u)


def test_framed_link_arguments_without_a_gpu():
    """The framing keywords are checked before any device call."""
    from waveforms_amd.encoding.coded import CodedCPMLink, CodedSOQPSKLink, IterativeCPMLink, IterativeSOQPSKLink

    code = ldpc.demo_code()
    fr = FR.Framing(code)
    other = FR.Framing(ldpc.demo_code(64))
    for cls in (CodedSOQPSKLink, CodedCPMLink, IterativeSOQPSKLink, IterativeCPMLink):
        for kw in ({"lead_bits": 5}, {"framing": fr, "lead_bits": fr.period}, {"framing": fr, "lead_bits": -1}, {"framing": other}):
            with pytest.raises(ValueError):
                cls(code, 4, **kw)
    for cls in (IterativeSOQPSKLink, IterativeCPMLink):
        with pytest.raises(ValueError):
            cls(code, 4, framing=fr, marker_prior=float("nan"))


# ------------------------------------------------------------------------------------------------ GPU
LEADS = [0, 1, 37, 2111]                  # P - 1 = 2111 for the demo code behind the 64-bit marker


def _quiet(link, ncw, code, lead, blocks=2):
    for b in range(blocks):
        link.run_block(None, seed=1, stream_id=b)
    be, fe, nc, m, _its = link.result()
    assert (be, fe, nc, m) == (0, 0, 0, blocks * ncw * code.k)
    n, wrong, (p, s, best, other) = link.sync_result()
    assert (n, wrong, p, s) == (blocks, 0, lead, 1) and best > other
    return link


@pytest.mark.gpu
@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("detector", ["PT", "PAM"])
def test_gpu_framed_soqpsk_links_noiseless(detector, lead):
    from waveforms_amd.encoding.coded import CodedSOQPSKLink, IterativeSOQPSKLink

    code = ldpc.demo_code()
    fr = FR.Framing(code)
    assert fr.period - 1 == LEADS[-1]
    link = _quiet(CodedSOQPSKLink(code, 5, detector=detector, framing=fr, lead_bits=lead), 5, code, lead)
    assert link.uncoded_result() == (0, 2 * (lead + 5 * fr.period))
    for mp in (None, 0.0):
        it = _quiet(IterativeSOQPSKLink(code, 5, detector=detector, outer=3, inner=5, framing=fr, lead_bits=lead, marker_prior=mp), 5, code, lead)
        assert int(it.state.sum()) == 5
        prior = it.prior.cpu().numpy()
        want = (1.0 - 2.0 * fr.marker_host) * it.ext_sat if mp is None else np.zeros(64)
        assert np.array_equal(prior[1 + lead:1 + lead + 64], want.astype(np.float32)) and not prior[:1 + lead].any()
        assert not prior[1 + lead + 5 * fr.period:].any() and (np.abs(prior[1 + lead + 64:1 + lead + fr.period]) == it.ext_sat).all()
    plain = FR.Framing(code, marker=0x1ACFFC1D, marker_bits=32, randomize=False)
    _quiet(CodedSOQPSKLink(code, 5, detector=detector, framing=plain, lead_bits=lead % plain.period), 5, code, lead % plain.period)


@pytest.mark.gpu
@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("waveform", ["multih", "pcmfm"])
def test_gpu_framed_cpm_links_noiseless(waveform, lead):
    from waveforms_amd.encoding.coded import CodedCPMLink, IterativeCPMLink

    code = ldpc.demo_code()
    fr = FR.Framing(code)
    _quiet(CodedCPMLink(code, 5, waveform=waveform, framing=fr, lead_bits=lead), 5, code, lead)
    for mp in (None, 0.0):
        it = _quiet(IterativeCPMLink(code, 5, waveform=waveform, outer=3, inner=5, framing=fr, lead_bits=lead, marker_prior=mp), 5, code, lead)
        assert int(it.state.sum()) == 5


def _host_loop_step(code, fr, want_ext, lock, state, ext_buf, dec, iters, prior_view, link):
    """One decoder pass of the framed loop on the host: gather, decode into the contiguous buffer, scatter."""
    p, s = lock
    lam = fr.gather_host(want_ext, p, s, link.ncw)
    TI.decode_ext_restatement(code, lam, state, ext_buf, dec, iters, 1.0, link.alpha, link.inner, link.ext_clip, link.ext_sat)
    prior_view[:] = fr.scatter_host(ext_buf, p, s, prior_view, link.marker_prior)
    return lam


@pytest.mark.gpu
@pytest.mark.parametrize("marker_prior", [None, 0.0])
def test_gpu_framed_soqpsk_loop_pass_by_pass(oracle, marker_prior):
    """tests/test_idd.py's pass-by-pass comparison with a framing: 8 demo codewords behind 37 lead bits, 4 outer passes.  After
    every pass the decoder's input, the prior buffer (as uint32), the states, the decisions and the iteration counts equal the
    host chain: detector restatement -> search_host (first pass) -> gather_host -> decoder restatement -> scatter_host."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.encoding.coded import IterativeSOQPSKLink

    code = ldpc.demo_code()
    fr = FR.Framing(code)
    link = IterativeSOQPSKLink(code, 8, detector="PT", outer=4, inner=5, framing=fr, lead_bits=37, marker_prior=marker_prior)
    info = link.info_bits(0)
    rows, _ = link.front_end(dev.ldpc_encode(code, info), 4.5 + 10 * math.log10(fr.period / code.n_tx), 7, 0)
    h = _hip.to_host(rows).reshape(-1, 3, 2)
    z = h[..., 0] + 1j * h[..., 1]
    n = z.shape[0]
    prior = np.zeros(n, dtype=np.float32)
    ext_buf = np.zeros((8, code.n_tx), dtype=np.float32)
    state, iters, dec = np.zeros(8, dtype=np.uint8), np.zeros(8, dtype=np.int32), np.zeros((8, code.k), dtype=np.uint8)
    link.begin(n)
    snaps, lock = [], None
    for o in range(4):
        ext, hard = link.detect(rows, first=o == 0)
        link.decode(ext)
        want_ext, _ = TI.apriori_restatement(oracle, z, prior, link.damping, True)
        if o == 0:
            (p, s, best, other), _ = fr.search_host(want_ext[1:])
            lock = (p, s)
            assert lock == (37, 1)
        rec = link.lock.cpu().numpy()
        assert (int(rec[0]), int(rec[1])) == lock, o
        lam = _host_loop_step(code, fr, want_ext[1:], lock, state, ext_buf, dec, iters, prior[1:], link)
        assert np.array_equal(_hip.to_host(ext).view(np.uint64), lam.view(np.uint64)), o
        snaps.append(int(state.sum()))
        assert np.array_equal(_hip.to_host(link.prior).view(np.uint32), prior.view(np.uint32)), o
        assert np.array_equal(_hip.to_host(link.ext).view(np.uint32), ext_buf.view(np.uint32)), o
        assert np.array_equal(_hip.to_host(link.state), state) and np.array_equal(_hip.to_host(link.iters), iters), o
        assert np.array_equal(_hip.to_host(link.decided), dec), o
    _hip.device_check()
    assert link.sync_result()[:2] == (1, 0)
    assert not prior[:1 + 37].any() and not prior[1 + 37 + 8 * fr.period:].any()
    assert bool(prior[1 + 37:1 + 37 + 64].any()) == (marker_prior is None)
    print("frozen after each pass:", snaps)
    assert snaps[-1] > snaps[0]                              # the loop does something on this burst


@pytest.mark.gpu
@pytest.mark.parametrize("marker_prior", [None, 0.0])
@pytest.mark.parametrize("waveform,ebn0,lead", [("multih", 7.0, 37), ("pcmfm", 3.0, 1)])
def test_gpu_framed_cpm_loop_pass_by_pass(apref, waveform, ebn0, lead, marker_prior):  # noqa: F811
    """The same for the CPM loops (tests/test_cpm_idd.py's comparison with a framing; ARTM with an odd lead)."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.encoding.coded import IterativeCPMLink

    code = ldpc.demo_code()
    fr = FR.Framing(code)
    link = IterativeCPMLink(code, 8, waveform=waveform, outer=4, inner=5, framing=fr, lead_bits=lead, marker_prior=marker_prior)
    spec, lg = link.spec, link.spec.bits_per_symbol
    info = link.info_bits(0)
    rows, _ = link.front_end(dev.ldpc_encode(code, info), ebn0 + 10 * math.log10(fr.period / code.n_tx), 7, 0)
    z = _hip.to_host(rows, complex_pairs=True)
    n = z.shape[0]
    assert n == link.ncalls and n * lg >= link.nch
    prior = np.zeros(n * lg, dtype=np.float32)
    ext_buf = np.zeros((8, code.n_tx), dtype=np.float32)
    state, iters, dec = np.zeros(8, dtype=np.uint8), np.zeros(8, dtype=np.int32), np.zeros((8, code.k), dtype=np.uint8)
    link.begin(n)
    snaps, lock = [], None
    for o in range(4):
        ext, hard = link.detect(rows, first=o == 0)
        link.decode(ext)
        want_ext, want_bits = TCI.restate(apref, spec, z, prior, link.damping)
        if o == 0:
            (p, s, best, other), _ = fr.search_host(want_ext)
            lock = (p, s)
            assert lock == (lead, 1)
        assert np.array_equal(_hip.to_host(hard), want_bits[:link.nch]), o
        lam = _host_loop_step(code, fr, want_ext, lock, state, ext_buf, dec, iters, prior, link)
        assert np.array_equal(_hip.to_host(ext).view(np.uint64), lam.view(np.uint64)), o
        snaps.append(int(state.sum()))
        assert np.array_equal(_hip.to_host(link.prior).view(np.uint32), prior.view(np.uint32)), o
        assert np.array_equal(_hip.to_host(link.state), state) and np.array_equal(_hip.to_host(link.iters), iters), o
        assert np.array_equal(_hip.to_host(link.decided), dec), o
    _hip.device_check()
    assert link.sync_result()[:2] == (1, 0)
    print("frozen after each pass:", snaps)
    assert snaps[-1] > snaps[0]


@pytest.mark.gpu
def test_gpu_framing_costs_only_its_overhead():
    """One block of about 1e7 channel bits each at the SAME channel σ, information Eb/N0 5 dB for the unframed link: the framed
    ``CodedSOQPSKLink`` at 5 dB + 10 log10(P / n_tx) (4 734 frames behind 1 234 lead bits), the unframed one at 5 dB (4 882
    codewords).  No wrong lock, and the frame-error RATES (the codeword counts differ: 4 734 and 4 882) differ by at most 4
    standard deviations of the difference of two binomial rates at the pooled rate p: sqrt(p (1 - p) (1 / n_f + 1 / n_u)).
    The yardstick is the unframed class; the margin is derived, not tuned.

    Measured on one MI355X (the chain is deterministic: counter-based noise, bitwise-defined kernels): unframed 1 849 of 4 882,
    framed 1 940 of 4 734, +3.12 standard deviations, no wrong lock.  The difference is systematic (eight more seeds: 37.8 %
    against 40.1 %) and is the modem's, not the framing's: the raw error rate of the unchanged detector on the codeword bits
    depends on the differential encoder's state in front of a codeword, which the marker and the lead bits fix for a whole
    burst of even-parity codewords (INTEGRATION.md has the figures; with ``lead_bits`` 0 or 1 the framed rate is 38.9 / 38.3 %
    against 38.3 % unframed on other seeds).  ``lead_bits`` = 1 234 was chosen before anything was measured and stays."""
    from waveforms_amd.encoding.coded import CodedSOQPSKLink

    code = ldpc.demo_code()
    fr = FR.Framing(code)
    n_u, n_f = int(1e7) // code.n_tx, int(1e7) // fr.period
    assert (n_u, n_f) == (4882, 4734)
    plain = CodedSOQPSKLink(code, n_u, detector="PT", max_iter=50)
    framed = CodedSOQPSKLink(code, n_f, detector="PT", max_iter=50, framing=fr, lead_bits=1234)
    assert plain.sigma(5.0) == pytest.approx(framed.sigma(5.0 + 10 * math.log10(fr.period / code.n_tx)), rel=1e-12)
    plain.run_block(5.0, seed=9, stream_id=0)
    framed.run_block(5.0 + 10 * math.log10(fr.period / code.n_tx), seed=9, stream_id=0)
    fe_u, fe_f = plain.result()[1], framed.result()[1]
    blocks, wrong, lock = framed.sync_result()
    p = (fe_u + fe_f) / (n_u + n_f)
    sd = math.sqrt(p * (1 - p) * (1 / n_f + 1 / n_u))
    print(f"unframed {fe_u} of {n_u} frame errors, framed {fe_f} of {n_f}; rates {fe_u / n_u:.4f} {fe_f / n_f:.4f}, "
          f"difference {(fe_f / n_f - fe_u / n_u) / sd:+.2f} standard deviations; lock {lock}, wrong locks {wrong}")
    assert (blocks, wrong) == (1, 0) and lock[:2] == (1234, 1)
    assert fe_u > 0.2 * n_u                                  # the operating point is where frame errors are common
    assert abs(fe_f / n_f - fe_u / n_u) <= 4 * sd
