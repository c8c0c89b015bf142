"""The coded ARTM / PCM/FM links with a clock offset and ``CPMTimingRecovery`` (waveforms_amd/encoding/coded.py: ``clock=``,
``clock_recovery=``): framed links with the demo code read 6 samples late and drifting by half the documented limit."""
import numpy as np
import pytest

from waveforms_amd.encoding import framing as FR
from waveforms_amd.encoding import ldpc
from waveforms_amd.sync import carrier_cpm as CC
from waveforms_amd.sync import timing as T
from waveforms_amd.sync import timing_cpm as TC

NCW, LEAD, SPS = 4, 37, 8
WAVEFORMS = ["pcmfm", "multih"]
# Information Eb/N0 of the noisy comparison: above the genie's waterfall, where the framed genie link and the recovered link both
# decoded every codeword of the sweep in profiles/timing_recovery_cpm.json; the sweep, not this test, chose it.
EBN0_DB = {"pcmfm": 6.0, "multih": 10.5}


def _spec(waveform):
    from waveforms_amd.viterbi import cpm

    return cpm.ARTM_64 if waveform == "multih" else cpm.PCMFM_20


def _window(waveform):
    return TC.defaults(_spec(waveform))["window"]


def _drift(waveform):
    return 0.5 * TC.MAX_DRIFT_SAMPLES[waveform]                  # samples per window: half the documented |eps| sps W


def _clock(waveform):
    return (6.0, _drift(waveform) / (SPS * _window(waveform)))


def _shifts(waveform):
    """Where the frame search may lock: the lead, or a period of nh symbols (nh lgM bits) either side of it."""
    spec = _spec(waveform)
    step = len(spec.K) * spec.bits_per_symbol
    return (LEAD - step, LEAD, LEAD + step)


def _links(waveform, cls=None, ncw=NCW, **kw):
    from waveforms_amd.encoding.coded import CodedCPMLink

    code = ldpc.demo_code()
    fr = FR.Framing(code)
    return code, [(cls or CodedCPMLink)(code, ncw, waveform, framing=fr, lead_bits=LEAD, **k) for k in kw.values()]


def test_links_refuse_what_the_clock_recovery_cannot_do():
    """Each with a ValueError, before anything touches a device: no framing, a carrier offset or a carrier recovery beside it, a
    recovery built for another design or sps, a SOQPSK-TG TimingRecovery, a clock that is not finite.  ``timing=`` stays a
    TypeError on the CPM classes."""
    from waveforms_amd.encoding.coded import CodedCPMLink, IterativeCPMLink
    from waveforms_amd.viterbi import cpm

    code = ldpc.demo_code()
    framing = object()                                    # (never reached: every refusal comes before the framing is looked at)
    for cls in (CodedCPMLink, IterativeCPMLink):
        for waveform in WAVEFORMS:
            rec = TC.CPMTimingRecovery(_spec(waveform), SPS)
            with pytest.raises(ValueError, match="framing"):
                cls(code, 2, waveform, clock_recovery=rec)
            with pytest.raises(ValueError, match="carrier"):
                cls(code, 2, waveform, framing=framing, clock_recovery=rec, recovery=CC.CPMCarrierRecovery(_spec(waveform)))
            with pytest.raises(ValueError, match="carrier"):
                cls(code, 2, waveform, framing=framing, clock_recovery=rec, carrier=(0.1, 0.0))
            with pytest.raises(ValueError, match="sps"):
                cls(code, 2, waveform, framing=framing, clock_recovery=TC.CPMTimingRecovery(_spec(waveform), 10))
            with pytest.raises(ValueError, match="CPMTimingRecovery"):
                cls(code, 2, waveform, framing=framing, clock_recovery=T.TimingRecovery(SPS))
            with pytest.raises(ValueError, match="finite"):
                cls(code, 2, waveform, clock=(float("nan"), 0.0))
            with pytest.raises(ValueError, match="finite"):
                cls(code, 2, waveform, clock=(0.0, float("inf")))
        with pytest.raises(ValueError, match="another design"):
            cls(code, 2, "multih", framing=framing, clock_recovery=TC.CPMTimingRecovery(cpm.PCMFM_20, SPS))
        with pytest.raises(TypeError):
            cls(code, 2, timing=(0.0, 0.0))
        with pytest.raises(TypeError):
            cls(code, 2, timing_recovery=T.TimingRecovery(SPS))


# Codewords per burst of the noiseless test: NCW for PCM/FM (8 493 calls, 34 windows of 256); 16 for ARTM, whose NCW-burst is four
# windows of 1024 and a short one - too few to tell a slope from the clipped mean's lag at the ends (16 926 calls, 17 windows).
SLOPE_NCW = {"pcmfm": NCW, "multih": 16}
# The scatter of a window's own estimate about the impairment on recover_cpm_timing_host, noiseless, at TWICE this drift: the
# largest standard deviation tests/test_cpm_timing.py prints over its six cases per waveform, in samples.
SCATTER = {"pcmfm": 0.158, "multih": 0.071}


@pytest.mark.gpu
@pytest.mark.parametrize("waveform", WAVEFORMS)
def test_framed_link_recovers_the_clock_noiseless(waveform):
    clock, W, drift, ncw = _clock(waveform), _window(waveform), _drift(waveform), SLOPE_NCW[waveform]
    code, (rec, bare) = _links(waveform, ncw=ncw, rec={"clock": clock, "clock_recovery": TC.CPMTimingRecovery(_spec(waveform), SPS)},
                               bare={"clock": clock})
    for b in range(2):
        rec.run_block(None, seed=1, stream_id=b)
        bare.run_block(None, seed=1, stream_id=b)
    be, fe, nc, m, _its = rec.result()
    assert (be, fe, nc, m) == (0, 0, 0, 2 * ncw * code.k)
    blocks, _wrong, (p, sigma, best, other) = rec.sync_result()
    assert blocks == 2 and p in _shifts(waveform) and sigma in (1, -1) and best > other
    tau, choice, grid = rec.clock_result()
    assert tau.shape == choice.shape == (-(-rec.ncalls // W),) and grid in (0, 1) and tau.size >= 16
    # The slope of τ is the drift, -drift samples per window (the signal is read LATER and later, the rows must be taken earlier
    # and earlier): the least-squares line through the windows 2 .. -3 (the two at either end carry the clipped mean's lag).  With
    # independent errors of standard deviation σ = SCATTER per window the fitted slope's own is σ / sqrt(Σ (w - mean w)²); the
    # bound is three of those: 0.010 samples per window against a drift of 0.3 (PCM/FM), 0.016 against 0.125 (ARTM).  A flat
    # trajectory, one of twice the drift and one of the other sign all miss it by far.
    y = tau[2:-2]
    w = np.arange(y.size, dtype=np.float64)
    slope = float(np.polyfit(w, y, 1)[0])
    bound = 3.0 * SCATTER[waveform] / float(np.sqrt(((w - w.mean()) ** 2).sum()))
    print(f"{waveform}: fitted slope {slope:+.4f} samples per window over {y.size} windows, drift {-drift:+.4f}, bound {bound:.4f}, grid {grid}, lock {p}")
    assert bound < 0.15 * drift and abs(slope + drift) < bound
    # the same link without the recovery loses the burst: without this the test shows nothing
    assert bare.result()[0] > 0 and bare.result()[1] > 0
    with pytest.raises(RuntimeError):
        bare.clock_result()
    # a recovered link's rows may sit a period from the sent bits: it does not count channel bits, and says so
    with pytest.raises(RuntimeError, match="periods"):
        rec.uncoded_result()
    assert bare.uncoded_result()[1] == 2 * bare.nch


@pytest.mark.gpu
@pytest.mark.parametrize("waveform", WAVEFORMS)
def test_default_arguments_leave_the_cpm_link_bitwise_alone(waveform):
    """With no clock and no recovery a block is the device calls the link made before it had the keywords, restated here one by
    one (channel bits + pad -> symbol_map -> cpm_modulate -> awgn with exp(-jπ/4) -> cpm_mf_rows -> cpm_soft -> frame search and
    gather -> ldpc_decode): the link's rows are those rows bit for bit and its counts those counts.  A clock of (0, 0) runs the
    offset kernel, whose weights are then 0, 1, 0, 0: numerically equal samples, so the same rows and counts too."""
    import torch

    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.encoding.coded import CPM_WAVEFORMS, PAD_SYMS

    ebn0, seed, sid = EBN0_DB[waveform] - 3.0, 1, 3
    code, (plain, explicit, zero, helper) = _links(waveform, plain={}, explicit={"clock": None, "clock_recovery": None}, zero={"clock": (0.0, 0.0)},
                                                   helper={})
    spec = helper.spec
    # the calls, by hand (helper lends its tables, its framing and its sigma; none of them is new code)
    info = dev.lfsr_bits(23, helper._mask, (1 << 23) - 1, NCW * code.k, skip=sid * NCW * code.k)[0]
    tx = dev.ldpc_encode(code, info)
    bits = torch.cat((helper.channel_bits(tx, sid), torch.zeros(PAD_SYMS * spec.bits_per_symbol, dtype=torch.uint8, device="cuda")))
    syms = dev.symbol_map(CPM_WAVEFORMS[waveform], bits)
    sig = dev.cpm_modulate(syms, helper._d_h, helper._d_pulse, SPS)
    received = dev.awgn(sig, int(sig.shape[0]), helper.sigma(ebn0), seed, sid, 0, np.exp(-1j * np.pi / 4))
    want_rows = dev.cpm_mf_rows(received, helper._d_templates, helper.start0, SPS, helper.ncalls)
    llr, hard = dev.cpm_soft(want_rows, spec, 0, 0, d_rot=helper._d_rot)
    lam = helper.deframe(llr)
    want_counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    dev.ldpc_decode(code, lam, scale=1.0, alpha=helper.alpha, max_iter=helper.max_iter, ref_info=info, counts=want_counts)
    want_uncoded = int((hard[:helper.nch] != bits[:helper.nch]).sum())
    want_rows, want_counts = _hip.to_host(want_rows), want_counts.cpu().tolist()
    assert want_uncoded > 0 and want_counts[3] > 0                          # channel errors and decoder iterations to compare
    for lk in (plain, explicit, zero):
        rows = _hip.to_host(lk.front_end(dev.ldpc_encode(code, lk.info_bits(sid)), ebn0, seed, sid)[0])
        if lk is zero:
            assert np.array_equal(rows, want_rows)
        else:
            assert np.array_equal(rows.view(np.uint64), want_rows.view(np.uint64))
        lk.run_block(ebn0, seed=seed, stream_id=sid)
        assert lk.counts.cpu().tolist() == want_counts
        assert lk.uncoded_result() == (want_uncoded, helper.nch)
        assert lk.sync_result() == helper.sync_result()


@pytest.mark.gpu
@pytest.mark.parametrize("waveform", WAVEFORMS)
def test_recovered_cpm_link_decodes_what_the_genie_decodes(waveform):
    code, (genie, rec) = _links(waveform, genie={}, rec={"clock": _clock(waveform), "clock_recovery": TC.CPMTimingRecovery(_spec(waveform), SPS)})
    blocks = 3
    for b in range(blocks):
        genie.run_block(EBN0_DB[waveform], seed=1, stream_id=b)
        rec.run_block(EBN0_DB[waveform], seed=1, stream_id=b)
    gbe, gfe, _gnc, gm, _ = genie.result()
    rbe, rfe, _rnc, rm, _ = rec.result()
    print(f"{waveform} Eb/N0 {EBN0_DB[waveform]}: genie {gbe} bit / {gfe} codeword errors, recovered {rbe} / {rfe}, of {gm} bits")
    assert gm == rm == blocks * NCW * code.k
    assert (gbe, gfe) == (0, 0)
    assert (rbe, rfe) == (0, 0)
    assert rec.sync_result()[2][0] in _shifts(waveform)


@pytest.mark.gpu
@pytest.mark.parametrize("waveform", WAVEFORMS)
def test_iterative_cpm_link_takes_the_recovery_too(waveform):
    from waveforms_amd.encoding.coded import IterativeCPMLink

    code, (link,) = _links(waveform, IterativeCPMLink, it={"outer": 3, "inner": 5, "clock": _clock(waveform),
                                                           "clock_recovery": TC.CPMTimingRecovery(_spec(waveform), SPS)})
    link.run_block(None, seed=1, stream_id=0)
    be, fe, _nc, m, _its = link.result()
    assert (be, fe, m) == (0, 0, NCW * code.k) and link.sync_result()[2][0] in _shifts(waveform)
    tau, choice, grid = link.clock_result()
    assert tau.size == choice.size and grid in (0, 1)
