"""The coded SOQPSK-TG links with a carrier offset and ``CarrierRecovery`` (waveforms_amd/encoding/coded.py: ``carrier=``,
``recovery=``): a framed link with the demo code under 40 degrees and a frequency offset of half the documented limit."""
import math

import numpy as np
import pytest

from waveforms_amd.encoding import framing as FR
from waveforms_amd.encoding import ldpc
from waveforms_amd.sync import carrier as C

NCW, LEAD, SPS = 4, 37, 8
NU = 0.5 * C.MAX_DRIFT_TURNS / (SPS * C.DEFAULT_WINDOW)          # cycles per sample: half the documented |nu| sps W
CARRIER = (math.radians(40.0), NU)
# Information Eb/N0 of the noisy comparison: above the genie's waterfall, where the framed genie link decoded every codeword
# of the sweep in profiles/carrier_recovery.json (tools/coded_ber.py --recover, 2000 codewords per point) and so did the
# recovered link; the sweep, not this test, chose it.
EBN0_DB = 8.0


def _links(**kw):
    from waveforms_amd.encoding.coded import CodedSOQPSKLink

    code = ldpc.demo_code()
    fr = FR.Framing(code)
    return code, [CodedSOQPSKLink(code, NCW, framing=fr, lead_bits=LEAD, **k) for k in kw.values()]


@pytest.mark.gpu
def test_framed_link_recovers_the_carrier_noiseless():
    code, (rec, bare) = _links(rec={"carrier": CARRIER, "recovery": C.CarrierRecovery()}, bare={"carrier": CARRIER})
    for b in range(2):
        rec.run_block(None, seed=1, stream_id=b)
        bare.run_block(None, seed=1, stream_id=b)
    be, fe, nc, m, _its = rec.result()
    assert (be, fe, nc, m) == (0, 0, 0, 2 * NCW * code.k)
    blocks, _wrong, (p, sigma, best, other) = rec.sync_result()
    assert (blocks, p) == (2, LEAD) and sigma in (1, -1) and best > other       # (σ = -1 is the π the recovery leaves to the frame search)
    phase, choice = rec.carrier_result()
    nrows = rec.nsym
    assert phase.shape == choice.shape and abs(phase.size - nrows / C.DEFAULT_WINDOW) <= 1
    slope = np.diff(phase)[2:-2] / (2.0 * math.pi)                              # turns per window: nu sps W = 0.025
    assert np.abs(slope - NU * SPS * C.DEFAULT_WINDOW).max() < 0.02
    # the same link without the recovery loses the burst: without this the test shows nothing
    assert bare.result()[0] > 0 and bare.result()[1] > 0
    with pytest.raises(RuntimeError):
        bare.carrier_result()


@pytest.mark.gpu
def test_default_arguments_leave_the_link_bitwise_alone():
    """With no carrier and no recovery a block is the device calls the link made before it had the keywords, restated here one
    by one (channel bits + pad -> fsm_encode -> cpm_modulate -> awgn_mf_bank with exp(-jπ/4) -> viterbi_soft -> frame search and
    gather -> ldpc_decode): the link's rows are those rows bit for bit and its counts those counts.  A carrier of (0, 0) runs
    the offset kernel and must give the same rows too (a product with exactly 1 + 0j)."""
    import torch

    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.encoding.coded import PAD_BITS, TIMING_OFFSET

    ebn0, seed, sid = 6.0, 1, 3
    code, (plain, explicit, zero, helper) = _links(plain={}, explicit={"carrier": None, "recovery": None}, zero={"carrier": (0.0, 0.0)}, helper={})
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
        assert np.array_equal(rows.view(np.uint64), want_rows.view(np.uint64))
        lk.run_block(ebn0, seed=seed, stream_id=sid)
        assert lk.counts.cpu().tolist() == want_counts
        assert lk.uncoded_result() == (want_uncoded, helper.nch)
        assert lk.sync_result() == helper.sync_result()


@pytest.mark.gpu
def test_recovered_link_decodes_what_the_genie_decodes():
    code, (genie, rec) = _links(genie={}, rec={"carrier": CARRIER, "recovery": C.CarrierRecovery()})
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
    assert rec.sync_result()[2][0] == LEAD


@pytest.mark.gpu
def test_iterative_link_takes_the_recovery_too():
    from waveforms_amd.encoding.coded import IterativeSOQPSKLink

    code = ldpc.demo_code()
    fr = FR.Framing(code)
    link = IterativeSOQPSKLink(code, NCW, outer=3, inner=5, framing=fr, lead_bits=LEAD, carrier=CARRIER, recovery=C.CarrierRecovery())
    link.run_block(None, seed=1, stream_id=0)
    be, fe, _nc, m, _its = link.result()
    assert (be, fe, m) == (0, 0, NCW * code.k) and link.sync_result()[2][0] == LEAD
    assert link.carrier_result()[0].size == link.carrier_result()[1].size
