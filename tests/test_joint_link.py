"""The coded SOQPSK-TG links under a carrier AND a timing offset with ``JointAcquisition`` (waveforms_amd/encoding/coded.py:
``acquisition=``): a framed link with the demo code, rotated by 40 degrees and 0.025 turns per window, read 6 samples late and
drifting by 0.8 samples per window - and the same at both documented limits."""
import math

import numpy as np
import pytest

from waveforms_amd.encoding import framing as FR
from waveforms_amd.encoding import ldpc
from waveforms_amd.sync import carrier as C
from waveforms_amd.sync import joint as J
from waveforms_amd.sync import timing as T

NCW, LEAD, SPS = 4, 37, 8
PER_WINDOW = SPS * C.DEFAULT_WINDOW
CARRIER = (math.radians(40.0), 0.025 / PER_WINDOW)
TIMING = (6.0, 0.8 / PER_WINDOW)
# both documented limits at once: MAX_DRIFT_TURNS and MAX_DRIFT_SAMPLES per window
CARRIER_LIMIT = (math.radians(-70.0), -C.MAX_DRIFT_TURNS / PER_WINDOW)
TIMING_LIMIT = (-5.3, -T.MAX_DRIFT_SAMPLES / PER_WINDOW)
EBN0_DB = 8.0                                                     # as tests/test_timing_link.py: above the genie's waterfall
LOCKS = tuple(range(LEAD - 3, LEAD + 4))                          # the lattice leaves the rows a few rows early or late, odd or even


def _links(**kw):
    from waveforms_amd.encoding.coded import CodedSOQPSKLink

    code = ldpc.demo_code()
    fr = FR.Framing(code)
    return code, [CodedSOQPSKLink(code, NCW, framing=fr, lead_bits=LEAD, **k) for k in kw.values()]


def test_links_refuse_what_the_acquisition_cannot_do():
    """Each with a ValueError, before anything touches a device: no framing, a carrier or a timing recovery beside it, an
    acquisition built for another sps, something that is no JointAcquisition.  The existing refusals stay: a timing recovery
    beside a carrier offset still names the carrier.  The CPM classes do not have the keyword."""
    from waveforms_amd.encoding.coded import CodedCPMLink, CodedSOQPSKLink, IterativeCPMLink, IterativeSOQPSKLink

    code = ldpc.demo_code()
    framing = object()                                    # (never reached: every refusal comes before the framing is looked at)
    for cls in (CodedSOQPSKLink, IterativeSOQPSKLink):
        with pytest.raises(ValueError, match="framing"):
            cls(code, 2, acquisition=J.JointAcquisition(SPS))
        with pytest.raises(ValueError, match="excludes"):
            cls(code, 2, framing=framing, acquisition=J.JointAcquisition(SPS), recovery=C.CarrierRecovery())
        with pytest.raises(ValueError, match="excludes"):
            cls(code, 2, framing=framing, acquisition=J.JointAcquisition(SPS), timing_recovery=T.TimingRecovery(SPS))
        with pytest.raises(ValueError, match="sps"):
            cls(code, 2, framing=framing, acquisition=J.JointAcquisition(10))
        with pytest.raises(ValueError, match="JointAcquisition"):
            cls(code, 2, framing=framing, acquisition=T.TimingRecovery(SPS))
        with pytest.raises(ValueError, match="carrier"):
            cls(code, 2, framing=framing, timing_recovery=T.TimingRecovery(SPS), carrier=(0.1, 0.0))
        with pytest.raises(ValueError, match="carrier"):
            cls(code, 2, framing=framing, timing_recovery=T.TimingRecovery(SPS), recovery=C.CarrierRecovery())
    for cls in (CodedCPMLink, IterativeCPMLink):
        with pytest.raises(TypeError):
            cls(code, 2, acquisition=J.JointAcquisition(SPS))


@pytest.mark.gpu
def test_framed_link_acquires_carrier_and_timing_noiseless():
    code, (acq, bare) = _links(acq={"carrier": CARRIER, "timing": TIMING, "acquisition": J.JointAcquisition(SPS)},
                               bare={"carrier": CARRIER, "timing": TIMING})
    for b in range(2):
        acq.run_block(None, seed=1, stream_id=b)
        bare.run_block(None, seed=1, stream_id=b)
    be, fe, nc, m, _its = acq.result()
    assert (be, fe, nc, m) == (0, 0, 0, 2 * NCW * code.k)
    blocks, _wrong, (p, sigma, best, other) = acq.sync_result()
    print(f"lock {p} (lead {LEAD}), polarity {sigma}")
    assert blocks == 2 and p in LOCKS and sigma in (1, -1) and best > other
    tau, phase, tchoice, cchoice = acq.acquisition_result()
    assert tau.shape == phase.shape == tchoice.shape == cchoice.shape and abs(tau.size - acq.nsym / C.DEFAULT_WINDOW) <= 1
    # (the slopes are the impairment's, -0.8 samples and +0.025 turns per window: tests/test_joint.py holds the bounds)
    print(f"slopes per window: tau {np.diff(tau)[2:-2].mean():+.4f} samples, phase {np.diff(phase)[2:-2].mean() / (2.0 * math.pi):+.5f} turns")
    # the same link without the acquisition loses the burst: without this the test shows nothing
    assert bare.result()[0] > 0 and bare.result()[1] > 0
    with pytest.raises(RuntimeError):
        bare.acquisition_result()
    with pytest.raises(RuntimeError, match="acquisition"):
        acq.uncoded_result()
    assert bare.uncoded_result()[1] == 2 * bare.nch


@pytest.mark.gpu
def test_framed_link_acquires_at_both_documented_limits_noiseless():
    code, (acq,) = _links(acq={"carrier": CARRIER_LIMIT, "timing": TIMING_LIMIT, "acquisition": J.JointAcquisition(SPS)})
    acq.run_block(None, seed=1, stream_id=0)
    be, fe, nc, m, _its = acq.result()
    assert (be, fe, nc, m) == (0, 0, 0, NCW * code.k)
    assert acq.sync_result()[2][0] in LOCKS


@pytest.mark.gpu
def test_acquired_link_decodes_what_the_genie_decodes():
    code, (genie, acq) = _links(genie={}, acq={"carrier": CARRIER, "timing": TIMING, "acquisition": J.JointAcquisition(SPS)})
    blocks = 3
    for b in range(blocks):
        genie.run_block(EBN0_DB, seed=1, stream_id=b)
        acq.run_block(EBN0_DB, seed=1, stream_id=b)
    gbe, gfe, _gnc, gm, _ = genie.result()
    abe, afe, _anc, am, _ = acq.result()
    print(f"Eb/N0 {EBN0_DB}: genie {gbe} bit / {gfe} codeword errors, acquired {abe} / {afe}, of {gm} bits")
    assert gm == am == blocks * NCW * code.k
    assert (gbe, gfe) == (0, 0)
    assert (abe, afe) == (0, 0)
    assert acq.sync_result()[2][0] in LOCKS


@pytest.mark.gpu
def test_default_arguments_leave_the_link_bitwise_alone():
    """With ``acquisition=None`` a block is the device calls the link made before it had the keyword, restated one by one as in
    tests/test_timing_link.py: the same rows bit for bit and the same counts."""
    import torch

    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.encoding.coded import PAD_BITS, TIMING_OFFSET

    ebn0, seed, sid = 6.0, 1, 3
    code, (plain, explicit, helper) = _links(plain={}, explicit={"acquisition": None}, helper={})
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
    assert want_uncoded > 0 and want_counts[3] > 0
    for lk in (plain, explicit):
        assert lk.acquisition is None
        rows = _hip.to_host(lk.front_end(dev.ldpc_encode(code, lk.info_bits(sid)), ebn0, seed, sid)[0])
        assert np.array_equal(rows.view(np.uint64), want_rows.view(np.uint64))
        lk.run_block(ebn0, seed=seed, stream_id=sid)
        assert lk.counts.cpu().tolist() == want_counts
        assert lk.uncoded_result() == (want_uncoded, helper.nch)
        assert lk.sync_result() == helper.sync_result()
        with pytest.raises(RuntimeError):
            lk.acquisition_result()


@pytest.mark.gpu
def test_iterative_link_takes_the_acquisition_too():
    from waveforms_amd.encoding.coded import IterativeSOQPSKLink

    code = ldpc.demo_code()
    fr = FR.Framing(code)
    link = IterativeSOQPSKLink(code, NCW, outer=3, inner=5, framing=fr, lead_bits=LEAD, carrier=CARRIER, timing=TIMING,
                               acquisition=J.JointAcquisition(SPS))
    link.run_block(None, seed=1, stream_id=0)
    be, fe, _nc, m, _its = link.result()
    assert (be, fe, m) == (0, 0, NCW * code.k) and link.sync_result()[2][0] in LOCKS
    assert len(link.acquisition_result()) == 4
