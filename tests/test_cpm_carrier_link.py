"""The coded ARTM / PCM/FM links with a carrier offset and ``CPMCarrierRecovery`` (waveforms_amd/encoding/coded.py:
``carrier=``, ``recovery=``): unframed links with the demo code under 40 degrees and a frequency offset of half the documented
limit.  No framing is needed: the phase comes back modulo 2π/p, which relabels phase states and leaves the data alone."""
import math

import numpy as np
import pytest

from waveforms_amd.encoding import ldpc
from waveforms_amd.sync import carrier as C
from waveforms_amd.sync import carrier_cpm as CC

NCW, SPS = 4, 8
WAVEFORMS = ["multih", "pcmfm"]


def _spec(waveform):
    from waveforms_amd.viterbi import cpm

    return cpm.ARTM_64 if waveform == "multih" else cpm.PCMFM_20


def _carrier(waveform):
    """40 degrees and half the documented drift: nu sps W = MAX_DRIFT_PERIODS / (2 p) turns per window."""
    nu = 0.5 * CC.MAX_DRIFT_PERIODS / (_spec(waveform).p * SPS * CC.DEFAULT_WINDOW)
    return (math.radians(40.0), nu)


def _links(waveform, cls=None, **kw):
    from waveforms_amd.encoding.coded import CodedCPMLink

    code = ldpc.demo_code()
    return code, [(cls or CodedCPMLink)(code, NCW, waveform, **k) for k in kw.values()]


# ------------------------------------------------------------------------------------------------ CPU
def test_links_refuse_the_other_waveforms_recovery():
    """The checks run before anything touches the device."""
    from waveforms_amd.encoding.coded import CodedCPMLink, CodedSOQPSKLink, IterativeCPMLink, IterativeSOQPSKLink
    from waveforms_amd.viterbi import cpm

    code = ldpc.demo_code()
    for cls in (CodedCPMLink, IterativeCPMLink):
        for waveform in WAVEFORMS:
            with pytest.raises(ValueError, match="CPMCarrierRecovery"):
                cls(code, 2, waveform, recovery=C.CarrierRecovery())
        with pytest.raises(ValueError, match="another design"):
            cls(code, 2, "multih", recovery=CC.CPMCarrierRecovery(cpm.PCMFM_20))
        with pytest.raises(ValueError):
            cls(code, 2, "multih", carrier=(float("nan"), 0.0))
    for cls in (CodedSOQPSKLink, IterativeSOQPSKLink):
        with pytest.raises(ValueError, match="sync.carrier.CarrierRecovery"):
            cls(code, 2, recovery=CC.CPMCarrierRecovery(cpm.ARTM_64))
        with pytest.raises(ValueError, match="framing"):
            cls(code, 2, recovery=C.CarrierRecovery())


def test_link_defaults_are_unchanged():
    import inspect

    from waveforms_amd.encoding.coded import CodedCPMLink, IterativeCPMLink

    for cls in (CodedCPMLink, IterativeCPMLink):
        par = inspect.signature(cls.__init__).parameters
        assert par["carrier"].default is None and par["recovery"].default is None
        assert list(par)[-2:] == ["carrier", "recovery"]


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("waveform", WAVEFORMS)
def test_coded_link_recovers_the_carrier_noiseless(waveform):
    """With the recovery: no bit and no codeword error, and the channel errors outside the burst's end symbols are the genie
    link's.  Without it the same link makes more channel errors than the genie: without this the test shows nothing."""
    from waveforms_amd import _hip

    spec = _spec(waveform)
    code, (genie, rec, bare) = _links(waveform, genie={}, rec={"carrier": _carrier(waveform), "recovery": CC.CPMCarrierRecovery(spec)},
                                      bare={"carrier": _carrier(waveform)})
    lg, hard = spec.bits_per_symbol, {}
    for name, lk in (("genie", genie), ("rec", rec), ("bare", bare)):
        info = lk.info_bits(0)
        tx = lk.encode(info)
        rows, _syms = lk.front_end(tx, None, 1, 0)
        _llr, bits = lk.soft(lk._recovered(rows))
        hard[name] = (_hip.to_host(bits), _hip.to_host(tx.reshape(-1)))
        lk.run_block(None, seed=1, stream_id=0)
    be, fe, nc, m, _its = rec.result()
    assert (be, fe, nc, m) == (0, 0, 0, NCW * code.k)
    inner = slice(8 * lg, NCW * code.n_tx - 8 * lg)
    errs = {name: int(np.count_nonzero(b[inner] != t[inner])) for name, (b, t) in hard.items()}
    print(f"{waveform}: channel bit errors outside the end symbols {errs}; whole burst: genie {genie.uncoded_result()}, "
          f"recovered {rec.uncoded_result()}, no recovery {bare.uncoded_result()}")
    assert errs["rec"] == errs["genie"]
    assert bare.uncoded_result()[0] > genie.uncoded_result()[0]
    phase, choice = rec.carrier_result()
    assert phase.shape == choice.shape and abs(phase.size - rec.ncalls / CC.DEFAULT_WINDOW) <= 1
    slope = np.diff(phase)[3:-3] / CC.period(spec)                              # periods per window: half the documented drift
    assert np.abs(slope - 0.5 * CC.MAX_DRIFT_PERIODS).max() < 0.25 * CC.MAX_DRIFT_PERIODS, slope
    with pytest.raises(RuntimeError):
        bare.carrier_result()


@pytest.mark.gpu
@pytest.mark.parametrize("waveform", WAVEFORMS)
def test_iterative_link_takes_the_recovery(waveform):
    from waveforms_amd.encoding.coded import IterativeCPMLink

    spec = _spec(waveform)
    code, (rec,) = _links(waveform, IterativeCPMLink, rec={"carrier": _carrier(waveform), "recovery": CC.CPMCarrierRecovery(spec), "outer": 2})
    rec.run_block(None, seed=1, stream_id=0)
    be, fe, nc, m, _its = rec.result()
    assert (be, fe, nc, m) == (0, 0, 0, NCW * code.k)
    assert rec.carrier_result()[0].size == -(-rec.ncalls // CC.DEFAULT_WINDOW)


@pytest.mark.gpu
@pytest.mark.parametrize("waveform", WAVEFORMS)
def test_default_arguments_leave_the_cpm_link_bitwise_alone(waveform):
    """With no carrier and no recovery a block is the device calls the link made before it had the keywords, restated here one
    by one (coded bits + pad -> symbol_map -> cpm_modulate -> awgn with exp(-jπ/4) -> cpm_mf_rows -> cpm_soft -> ldpc_decode):
    the link's rows are those rows bit for bit and its counts those counts.  A carrier of (0, 0) runs the offset kernel and
    must give the same rows too (a product with exactly 1 + 0j)."""
    import torch

    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.encoding.coded import CPM_WAVEFORMS, PAD_SYMS

    ebn0, seed, sid = 6.0, 1, 3
    code, (plain, explicit, zero, helper) = _links(waveform, plain={}, explicit={"carrier": None, "recovery": None}, zero={"carrier": (0.0, 0.0)},
                                                   helper={})
    spec = helper.spec
    lg = spec.bits_per_symbol
    # the calls, by hand (helper lends its tables and its sigma; none of them is new code)
    info = dev.lfsr_bits(23, helper._mask, (1 << 23) - 1, NCW * code.k, skip=sid * NCW * code.k)[0]
    tx = dev.ldpc_encode(code, info)
    bits = torch.cat((tx.reshape(-1), torch.zeros(PAD_SYMS * lg, dtype=torch.uint8, device="cuda")))
    syms = dev.symbol_map(CPM_WAVEFORMS[waveform], bits)
    sig = dev.cpm_modulate(syms, helper._d_h, helper._d_pulse, SPS)
    received = dev.awgn(sig, int(sig.shape[0]), helper.sigma(ebn0), seed, sid, 0, np.exp(-1j * np.pi / 4))
    want_rows = dev.cpm_mf_rows(received, helper._d_templates, helper.start0, SPS, helper.ncalls)
    llr, hard = dev.cpm_soft(want_rows, spec, 0, 0, d_rot=helper._d_rot)
    nbits = NCW * code.n_tx
    want_counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    dev.ldpc_decode(code, llr[:nbits].view(NCW, code.n_tx), scale=1.0, alpha=helper.alpha, max_iter=helper.max_iter, ref_info=info, counts=want_counts)
    want_uncoded = int((hard[:nbits] != bits[:nbits]).sum())
    want_rows, want_counts = _hip.to_host(want_rows), want_counts.cpu().tolist()
    assert want_uncoded > 0 and want_counts[3] > 0                          # 6 dB: channel errors and decoder iterations to compare
    for lk in (plain, explicit, zero):
        rows = _hip.to_host(lk.front_end(dev.ldpc_encode(code, lk.info_bits(sid)), ebn0, seed, sid)[0])
        assert np.array_equal(rows.view(np.uint64), want_rows.view(np.uint64))
        lk.run_block(ebn0, seed=seed, stream_id=sid)
        assert lk.counts.cpu().tolist() == want_counts
        assert lk.uncoded_result() == (want_uncoded, nbits)
