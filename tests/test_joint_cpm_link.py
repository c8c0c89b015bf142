"""The coded ARTM / PCM/FM links under a carrier offset AND a clock offset with ``CPMJointAcquisition``
(waveforms_amd/encoding/coded.py: ``joint=``): framed links with the demo code turned by 40 degrees and drifting by half the
documented carrier limit, read 6 samples late and drifting by half the documented timing limit."""
import math

import numpy as np
import pytest

from waveforms_amd.encoding import framing as FR
from waveforms_amd.encoding import ldpc
from waveforms_amd.sync import carrier_cpm as CC
from waveforms_amd.sync import joint as J
from waveforms_amd.sync import joint_cpm as JC
from waveforms_amd.sync import timing_cpm as TC

NCW, LEAD, SPS, WC = 4, 37, 8, 256
WAVEFORMS = ["pcmfm", "multih"]
# Information Eb/N0 of the noisy comparison: the lowest point of the sweep in profiles/joint_acquisition_cpm.json from which the
# framed genie link and the acquired link both decoded every one of the 2000 codewords - PCM/FM 4.5 dB (the acquired link's last
# lost codeword is at 4.0 dB, the genie's at 4.25), ARTM 11.0 dB (the acquired link still loses 3 of 2000 at 10.5 dB, the genie
# none from 8.75); the sweep, not this test, chose them.
EBN0_DB = {"pcmfm": 4.5, "multih": 11.0}


def _spec(waveform):
    from waveforms_amd.viterbi import cpm

    return cpm.ARTM_64 if waveform == "multih" else cpm.PCMFM_20


def _impairment(waveform, share=0.5, sign=1.0):
    """(carrier, clock): 40 degrees and ``share`` of the documented carrier drift, 6 samples late and ``share`` of the documented
    timing drift -> ((theta0, nu in cycles per sample), (tau0, eps))."""
    spec = _spec(waveform)
    Wt = TC.defaults(spec)["window"]
    nu = sign * share * (JC.MAX_DRIFT_PERIODS / spec.p) / (SPS * WC)
    eps = sign * share * JC.MAX_DRIFT_SAMPLES[waveform] / (SPS * Wt)
    return (math.radians(40.0), nu), (6.0, eps)


def _shifts(waveform):
    """Where the frame search may lock.  The coarse instants cover ONE period of nh sps samples centred on 0, so the first
    window's τ lies within half a period (and half a hypothesis spacing) of 0; the burst is read 6 samples late, less than a
    period of either waveform (8, 16), so the rows come out on time or ONE period of nh symbols (nh lgM bits) early or late; the
    trajectory is unwrapped from there on and slips no further period.  The phase's ambiguity never reaches the data."""
    spec = _spec(waveform)
    step = len(spec.K) * spec.bits_per_symbol
    return (LEAD - step, LEAD, LEAD + step)


def _links(waveform, cls=None, ncw=NCW, **kw):
    from waveforms_amd.encoding.coded import CodedCPMLink

    code = ldpc.demo_code()
    fr = FR.Framing(code)
    return code, [(cls or CodedCPMLink)(code, ncw, waveform, framing=fr, lead_bits=LEAD, **k) for k in kw.values()]


def test_links_refuse_what_the_joint_acquisition_cannot_do():
    """Each with a ValueError, before anything touches a device: no framing, a carrier or a clock recovery beside it, an
    acquisition built for another design or sps, a SOQPSK-TG JointAcquisition.  ``acquisition=`` stays a TypeError on the CPM
    classes, and ``joint`` stands in front of ``carrier`` and ``recovery`` in their signatures."""
    import inspect

    from waveforms_amd.encoding.coded import CodedCPMLink, IterativeCPMLink
    from waveforms_amd.viterbi import cpm

    code = ldpc.demo_code()
    framing = object()                                    # (never reached: every refusal comes before the framing is looked at)
    for cls in (CodedCPMLink, IterativeCPMLink):
        names = list(inspect.signature(cls.__init__).parameters)
        assert "joint" in names and names[-2:] == ["carrier", "recovery"] and callable(cls.joint_result)
        for waveform in WAVEFORMS:
            acq = JC.CPMJointAcquisition(_spec(waveform), SPS)
            with pytest.raises(ValueError, match="framing"):
                cls(code, 2, waveform, joint=acq)
            with pytest.raises(ValueError, match="excludes"):
                cls(code, 2, waveform, framing=framing, joint=acq, recovery=CC.CPMCarrierRecovery(_spec(waveform)))
            with pytest.raises(ValueError, match="excludes"):
                cls(code, 2, waveform, framing=framing, joint=acq, clock_recovery=TC.CPMTimingRecovery(_spec(waveform), SPS))
            with pytest.raises(ValueError, match="sps"):
                cls(code, 2, waveform, framing=framing, joint=JC.CPMJointAcquisition(_spec(waveform), 10))
            with pytest.raises(ValueError, match="CPMJointAcquisition"):
                cls(code, 2, waveform, framing=framing, joint=J.JointAcquisition(SPS))
            with pytest.raises(ValueError, match="CPMJointAcquisition"):
                cls(code, 2, waveform, framing=framing, joint=TC.CPMTimingRecovery(_spec(waveform), SPS))
            # what the links refused before, in the same words
            with pytest.raises(ValueError, match="joint timing and carrier acquisition is not implemented"):
                cls(code, 2, waveform, framing=framing, clock_recovery=TC.CPMTimingRecovery(_spec(waveform), SPS), carrier=(0.1, 0.0))
        with pytest.raises(ValueError, match="another design"):
            cls(code, 2, "multih", framing=framing, joint=JC.CPMJointAcquisition(cpm.PCMFM_20, SPS))
        with pytest.raises(TypeError):
            cls(code, 2, acquisition=JC.CPMJointAcquisition(cpm.ARTM_64, SPS))


@pytest.mark.gpu
@pytest.mark.parametrize("waveform", WAVEFORMS)
def test_framed_link_acquires_carrier_and_clock_noiseless(waveform):
    carrier, clock = _impairment(waveform)
    code, (acq, bare) = _links(waveform, acq={"carrier": carrier, "clock": clock, "joint": JC.CPMJointAcquisition(_spec(waveform), SPS)},
                               bare={"carrier": carrier, "clock": clock})
    for b in range(2):
        acq.run_block(None, seed=1, stream_id=b)
        bare.run_block(None, seed=1, stream_id=b)
    be, fe, nc, m, _its = acq.result()
    assert (be, fe, nc, m) == (0, 0, 0, 2 * NCW * code.k)
    blocks, _wrong, (p, sigma, best, other) = acq.sync_result()
    print(f"{waveform}: lock {p} (lead {LEAD}), sigma {sigma}")
    assert blocks == 2 and p in _shifts(waveform) and sigma in (1, -1) and best > other
    tau, phase, tch, cch = acq.joint_result()
    Wt = TC.defaults(_spec(waveform))["window"]
    assert tau.shape == tch.shape == (-(-acq.ncalls // Wt),) and phase.shape == cch.shape == (-(-acq.ncalls // WC),)
    # the same link without the acquisition loses the burst: without this the test shows nothing
    assert bare.result()[0] > 0 and bare.result()[1] > 0
    with pytest.raises(RuntimeError):
        bare.joint_result()
    # an acquired link's rows may sit a period from the sent bits: it does not count channel bits, and says so
    with pytest.raises(RuntimeError, match="periods"):
        acq.uncoded_result()
    assert bare.uncoded_result()[1] == 2 * bare.nch


@pytest.mark.gpu
@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("waveform", WAVEFORMS)
def test_framed_link_acquires_at_both_documented_limits(waveform, sign):
    carrier, clock = _impairment(waveform, 1.0, sign)
    code, (acq,) = _links(waveform, acq={"carrier": carrier, "clock": clock, "joint": JC.CPMJointAcquisition(_spec(waveform), SPS)})
    acq.run_block(None, seed=1, stream_id=0)
    be, fe, nc, m, _its = acq.result()
    assert (be, fe, nc, m) == (0, 0, 0, NCW * code.k) and acq.sync_result()[2][0] in _shifts(waveform)


@pytest.mark.gpu
@pytest.mark.parametrize("waveform", WAVEFORMS)
def test_joint_none_leaves_the_cpm_link_bitwise_alone(waveform):
    """With ``joint=None`` (and no other recovery) a block under both impairments is the device calls the link made before it had
    the keyword, restated here one by one (channel bits + pad -> symbol_map -> cpm_modulate -> carrier_offset -> timing_offset ->
    awgn with exp(-jπ/4) -> cpm_mf_rows -> cpm_soft -> frame search and gather -> ldpc_decode): the link's rows are those rows bit
    for bit and its counts those counts."""
    import torch

    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.encoding.coded import CPM_WAVEFORMS, PAD_SYMS

    ebn0, seed, sid = EBN0_DB[waveform] - 3.0, 1, 3
    carrier, clock = _impairment(waveform, 0.05)                 # (small enough that the decoder still has something to count)
    code, (plain, explicit, helper) = _links(waveform, plain={"carrier": carrier, "clock": clock},
                                             explicit={"carrier": carrier, "clock": clock, "joint": None, "clock_recovery": None, "recovery": None},
                                             helper={})
    spec = helper.spec
    # the calls, by hand (helper lends its tables, its framing and its sigma; none of them is new code)
    info = dev.lfsr_bits(23, helper._mask, (1 << 23) - 1, NCW * code.k, skip=sid * NCW * code.k)[0]
    tx = dev.ldpc_encode(code, info)
    bits = torch.cat((helper.channel_bits(tx, sid), torch.zeros(PAD_SYMS * spec.bits_per_symbol, dtype=torch.uint8, device="cuda")))
    syms = dev.symbol_map(CPM_WAVEFORMS[waveform], bits)
    sig = dev.cpm_modulate(syms, helper._d_h, helper._d_pulse, SPS)
    dev.carrier_offset(sig, carrier[0], carrier[1], 0, out=sig)
    sig = dev.timing_offset(sig, clock[0], clock[1], 0)
    received = dev.awgn(sig, int(sig.shape[0]), helper.sigma(ebn0), seed, sid, 0, np.exp(-1j * np.pi / 4))
    want_rows = dev.cpm_mf_rows(received, helper._d_templates, helper.start0, SPS, helper.ncalls)
    llr, hard = dev.cpm_soft(want_rows, spec, 0, 0, d_rot=helper._d_rot)
    lam = helper.deframe(llr)
    want_counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    dev.ldpc_decode(code, lam, scale=1.0, alpha=helper.alpha, max_iter=helper.max_iter, ref_info=info, counts=want_counts)
    want_uncoded = int((hard[:helper.nch] != bits[:helper.nch]).sum())
    want_rows, want_counts = _hip.to_host(want_rows), want_counts.cpu().tolist()
    assert want_uncoded > 0 and want_counts[3] > 0                          # channel errors and decoder iterations to compare
    for lk in (plain, explicit):
        assert lk.joint is None
        rows = _hip.to_host(lk.front_end(dev.ldpc_encode(code, lk.info_bits(sid)), ebn0, seed, sid)[0])
        assert np.array_equal(rows.view(np.uint64), want_rows.view(np.uint64))
        lk.run_block(ebn0, seed=seed, stream_id=sid)
        assert lk.counts.cpu().tolist() == want_counts
        assert lk.uncoded_result() == (want_uncoded, helper.nch)
        assert lk.sync_result() == helper.sync_result()
        with pytest.raises(RuntimeError):
            lk.joint_result()


@pytest.mark.gpu
@pytest.mark.parametrize("waveform", WAVEFORMS)
def test_acquired_cpm_link_decodes_what_the_genie_decodes(waveform):
    carrier, clock = _impairment(waveform)
    code, (genie, acq) = _links(waveform, genie={}, acq={"carrier": carrier, "clock": clock, "joint": JC.CPMJointAcquisition(_spec(waveform), SPS)})
    blocks = 3
    for b in range(blocks):
        genie.run_block(EBN0_DB[waveform], seed=1, stream_id=b)
        acq.run_block(EBN0_DB[waveform], seed=1, stream_id=b)
    gbe, gfe, _gnc, gm, _ = genie.result()
    abe, afe, _anc, am, _ = acq.result()
    print(f"{waveform} Eb/N0 {EBN0_DB[waveform]}: genie {gbe} bit / {gfe} codeword errors, acquired {abe} / {afe}, of {gm} bits")
    assert gm == am == blocks * NCW * code.k
    assert (gbe, gfe) == (0, 0)
    assert (abe, afe) == (0, 0)
    assert acq.sync_result()[2][0] in _shifts(waveform)


@pytest.mark.gpu
@pytest.mark.parametrize("waveform", WAVEFORMS)
def test_iterative_cpm_link_takes_the_joint_acquisition_too(waveform):
    from waveforms_amd.encoding.coded import IterativeCPMLink

    carrier, clock = _impairment(waveform)
    code, (link,) = _links(waveform, IterativeCPMLink, it={"outer": 3, "inner": 5, "carrier": carrier, "clock": clock,
                                                           "joint": JC.CPMJointAcquisition(_spec(waveform), SPS)})
    link.run_block(None, seed=1, stream_id=0)
    be, fe, _nc, m, _its = link.result()
    assert (be, fe, m) == (0, 0, NCW * code.k) and link.sync_result()[2][0] in _shifts(waveform)
    tau, phase, tch, cch = link.joint_result()
    assert tau.size == tch.size and phase.size == cch.size


# Codewords per burst of the anchored test: NCW for PCM/FM (34 timing windows); 16 for ARTM, whose NCW-burst is four timing
# windows and a short one - too few for a drift search over segments of K = 33 windows to tell a drift from none.
ANCHOR_NCW = {"pcmfm": NCW, "multih": 16}


@pytest.mark.gpu
@pytest.mark.parametrize("waveform", WAVEFORMS)
def test_anchored_joint_acquisition_finds_the_drifts_with_their_signs(waveform):
    carrier, clock = _impairment(waveform)
    ncw = ANCHOR_NCW[waveform]
    code, (link,) = _links(waveform, ncw=ncw, acq={"carrier": carrier, "clock": clock, "joint": JC.CPMJointAcquisition(_spec(waveform), SPS, anchor=33)})
    link.run_block(None, seed=1, stream_id=0)
    be, fe, _nc, m, _its = link.result()
    assert (be, fe, m) == (0, 0, ncw * code.k)
    tau, phase, tch, cch, tdrift, trej, cdrift, crej = link.joint_result()
    print(f"{waveform}: timing drift found {tdrift:+.4f} samples per window ({trej} windows rejected), carrier {cdrift:+.5f} rad per window ({crej})")
    # the signal is read later and later, so the rows are taken earlier and earlier: τ falls where eps > 0; the phase rises with nu
    assert tdrift < 0.0 < cdrift
