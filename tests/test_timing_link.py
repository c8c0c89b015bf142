"""The coded SOQPSK-TG links with a timing offset and ``TimingRecovery`` (waveforms_amd/encoding/coded.py: ``timing=``,
``timing_recovery=``): a framed link with the demo code read 6 samples late and drifting by half the documented limit."""
import numpy as np
import pytest

from waveforms_amd.encoding import framing as FR
from waveforms_amd.encoding import ldpc
from waveforms_amd.sync import carrier as C
from waveforms_amd.sync import timing as T

NCW, LEAD, SPS = 4, 37, 8
DRIFT = 0.5 * T.MAX_DRIFT_SAMPLES                                 # samples per window: half the documented |eps| sps W
TIMING = (6.0, DRIFT / (SPS * C.DEFAULT_WINDOW))                  # eps = 3.9e-4
# Information Eb/N0 of the noisy comparison: above the genie's waterfall, where the framed genie link decoded every codeword
# of the sweep in profiles/timing_recovery.json (tools/coded_ber.py --recover-timing, 2000 codewords per point) and so did the
# recovered link; the sweep, not this test, chose it.
EBN0_DB = 8.0


def _links(**kw):
    from waveforms_amd.encoding.coded import CodedSOQPSKLink

    code = ldpc.demo_code()
    fr = FR.Framing(code)
    return code, [CodedSOQPSKLink(code, NCW, framing=fr, lead_bits=LEAD, **k) for k in kw.values()]


def test_links_refuse_what_the_timing_recovery_cannot_do():
    """Each with a ValueError, before anything touches a device: no framing, a carrier offset or a carrier recovery beside it,
    a recovery built for another sps, something that is no TimingRecovery, a timing that is not finite.  The CPM classes do
    not have the keywords."""
    from waveforms_amd.encoding.coded import CodedCPMLink, CodedSOQPSKLink, IterativeCPMLink, IterativeSOQPSKLink

    code = ldpc.demo_code()
    framing = object()                                    # (never reached: every refusal comes before the framing is looked at)
    for cls in (CodedSOQPSKLink, IterativeSOQPSKLink):
        with pytest.raises(ValueError, match="framing"):
            cls(code, 2, timing_recovery=T.TimingRecovery(SPS))
        with pytest.raises(ValueError, match="carrier"):
            cls(code, 2, framing=framing, timing_recovery=T.TimingRecovery(SPS), recovery=C.CarrierRecovery())
        with pytest.raises(ValueError, match="carrier"):
            cls(code, 2, framing=framing, timing_recovery=T.TimingRecovery(SPS), carrier=(0.1, 0.0))
        with pytest.raises(ValueError, match="sps"):
            cls(code, 2, framing=framing, timing_recovery=T.TimingRecovery(10))
        with pytest.raises(ValueError, match="TimingRecovery"):
            cls(code, 2, framing=framing, timing_recovery=C.CarrierRecovery())
        with pytest.raises(ValueError, match="finite"):
            cls(code, 2, timing=(float("nan"), 0.0))
    for cls in (CodedCPMLink, IterativeCPMLink):
        with pytest.raises(TypeError):
            cls(code, 2, timing=(0.0, 0.0))
        with pytest.raises(TypeError):
            cls(code, 2, timing_recovery=T.TimingRecovery(SPS))


@pytest.mark.gpu
def test_framed_link_recovers_the_timing_noiseless():
    code, (rec, bare) = _links(rec={"timing": TIMING, "timing_recovery": T.TimingRecovery(SPS)}, bare={"timing": TIMING})
    for b in range(2):
        rec.run_block(None, seed=1, stream_id=b)
        bare.run_block(None, seed=1, stream_id=b)
    be, fe, nc, m, _its = rec.result()
    assert (be, fe, nc, m) == (0, 0, 0, 2 * NCW * code.k)
    blocks, _wrong, (p, sigma, best, other) = rec.sync_result()
    assert blocks == 2 and p in (LEAD - 2, LEAD, LEAD + 2) and sigma in (1, -1) and best > other      # (±2: the two symbols the recovery leaves to the frame search)
    tau, choice = rec.timing_result()
    assert tau.shape == choice.shape and abs(tau.size - rec.nsym / C.DEFAULT_WINDOW) <= 1
    # The slope is the drift, -DRIFT samples per window (the signal is read LATER and later, the rows must be taken earlier and
    # earlier).  A window's own estimate stays within 0.055 samples of the impairment on recover_timing_host, noiseless, at
    # twice this drift (tests/test_timing.py prints it for six bursts), so the difference of two neighbours within 0.11; the
    # four windows at either end carry the clipped mean's lag and are left out.
    slope = np.diff(tau)[4:-4]
    print(f"slope per window: {slope.min():+.3f} .. {slope.max():+.3f}, drift {-DRIFT:+.3f}")
    assert np.abs(slope + DRIFT).max() < 0.11
    # the same link without the recovery loses the burst: without this the test shows nothing
    assert bare.result()[0] > 0 and bare.result()[1] > 0
    with pytest.raises(RuntimeError):
        bare.timing_result()
    # a recovered link's rows may sit two rows from the sent bits: it does not count channel bits, and says so
    with pytest.raises(RuntimeError, match="two rows"):
        rec.uncoded_result()
    assert bare.uncoded_result()[1] == 2 * bare.nch


@pytest.mark.gpu
def test_default_arguments_leave_the_link_bitwise_alone():
    """With no timing and no recovery a block is the device calls the link made before it had the keywords, restated here one
    by one (channel bits + pad -> fsm_encode -> cpm_modulate -> awgn_mf_bank with exp(-jπ/4) -> viterbi_soft -> frame search and
    gather -> ldpc_decode): the link's rows are those rows bit for bit and its counts those counts.  A timing of (0, 0) runs the
    offset kernel, whose weights are then 0, 1, 0, 0: numerically equal samples, so the same rows and counts too."""
    import torch

    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.encoding.coded import PAD_BITS, TIMING_OFFSET

    ebn0, seed, sid = 6.0, 1, 3
    code, (plain, explicit, zero, helper) = _links(plain={}, explicit={"timing": None, "timing_recovery": None}, zero={"timing": (0.0, 0.0)}, helper={})
    # the calls, by hand (helper lends its tables, its framing and its sigma; none of them is new code)
    info = dev.lfsr_bits(23, helper._mask, (1 << 23) - 1, NCW * code.k, skip=sid * NCW * code.k)[0]
    tx = dev.ldpc_encode(code, info)
    bits = torch.cat((helper.channel_bits(tx, sid), torch.zeros(PAD_BITS, dtype=torch.uint8, device="cuda")))
    syms, _ = dev.fsm_encode(*helper._tables, bits)
    sig = dev.cpm_modulate(syms, helper._d_h, helper._d_pulse, SPS)
    first, ncols = dev.decimation(int(sig.shape[0]), SPS, 2, TIMING_OFFSET["PT"])
    want_rows = dev.awgn_mf_bank(sig, helper._d_taps, first, SPS, ncols, helper.sigma(ebn0), seed, sid, 0, np.exp(-1j * np.pi / 4))
    llr, hard = dev.viterbi_soft(want_rows, True)
    lam = helper.deframe(llr[1:])
    want_counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    dev.ldpc_decode(code, lam, scale=1.0, alpha=helper.alpha, max_iter=helper.max_iter, ref_info=info, counts=want_counts)
    want_uncoded = int((hard[1:1 + helper.nch] != bits[:helper.nch]).sum())
    want_rows, want_counts = _hip.to_host(want_rows), want_counts.cpu().tolist()
    assert want_uncoded > 0 and want_counts[3] > 0                          # 6 dB: channel errors and decoder iterations to compare
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
def test_recovered_link_decodes_what_the_genie_decodes():
    code, (genie, rec) = _links(genie={}, rec={"timing": TIMING, "timing_recovery": T.TimingRecovery(SPS)})
    blocks = 3
    for b in range(blocks):
        genie.run_block(EBN0_DB, seed=1, stream_id=b)
        rec.run_block(EBN0_DB, seed=1, stream_id=b)
    gbe, gfe, _gnc, gm, _ = genie.result()
    rbe, rfe, _rnc, rm, _ = rec.result()
    print(f"Eb/N0 {EBN0_DB}: genie {gbe} bit / {gfe} codeword errors, recovered {rbe} / {rfe}, of {gm} bits")
    assert gm == rm == blocks * NCW * code.k
    assert (gbe, gfe) == (0, 0)
    assert (rbe, rfe) == (0, 0)
    assert rec.sync_result()[2][0] in (LEAD - 2, LEAD, LEAD + 2)


@pytest.mark.gpu
def test_iterative_link_takes_the_recovery_too():
    from waveforms_amd.encoding.coded import IterativeSOQPSKLink

    code = ldpc.demo_code()
    fr = FR.Framing(code)
    link = IterativeSOQPSKLink(code, NCW, outer=3, inner=5, framing=fr, lead_bits=LEAD, timing=TIMING, timing_recovery=T.TimingRecovery(SPS))
    link.run_block(None, seed=1, stream_id=0)
    be, fe, _nc, m, _its = link.result()
    assert (be, fe, m) == (0, 0, NCW * code.k) and link.sync_result()[2][0] in (LEAD - 2, LEAD, LEAD + 2)
    assert link.timing_result()[0].size == link.timing_result()[1].size
