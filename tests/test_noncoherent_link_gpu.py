"""``NoncoherentPCMFMLink`` (waveforms_amd/encoding/noncoherent.py): the demo code, framed and unframed, under a carrier phase of
1 rad and a frequency offset of 1e-3 cycles per sample - 160 times what the coherent links' recoveries follow - with nothing
beside it; its λ against the host statement on the link's own samples; its refusals."""
import numpy as np
import pytest

from test_noncoherent import lam_tolerance
from waveforms_amd.encoding import framing as FR
from waveforms_amd.encoding import ldpc
from waveforms_amd.viterbi import noncoherent as nc

NCW, LEAD, CARRIER = 3, 37, (1.0, 1e-3)


def _link(framed: bool, **kw):
    from waveforms_amd.encoding.noncoherent import NoncoherentPCMFMLink

    code = ldpc.demo_code()
    if framed:
        kw.update(framing=FR.Framing(code), lead_bits=LEAD)
    return NoncoherentPCMFMLink(code, NCW, **kw)


def test_refusals_name_their_reasons():
    """Checked before anything touches the device."""
    from waveforms_amd.encoding.noncoherent import NO_PHASE, NO_TIMING, NoncoherentPCMFMLink

    code = ldpc.demo_code()
    with pytest.raises(ValueError, match="no phase to recover") as e:
        NoncoherentPCMFMLink(code, 2, recovery=object())
    assert str(e.value) == f"recovery: {NO_PHASE}"
    for name in ("clock", "clock_recovery", "joint"):
        with pytest.raises(ValueError, match="timing recovery for the noncoherent detector is not built") as e:
            NoncoherentPCMFMLink(code, 2, **{name: (0.25, 1e-5)})
        assert str(e.value) == f"{name}: {NO_TIMING}"
    for bad in ({"observe": 4}, {"observe": 9}, {"observe": 1}, {"offset": 9}, {"offset": -1}):
        with pytest.raises(ValueError):
            NoncoherentPCMFMLink(code, 2, **bad)


@pytest.mark.gpu
@pytest.mark.parametrize("framed", [False, True])
def test_noiseless_under_a_carrier_offset(framed):
    link = _link(framed, carrier=CARRIER)
    for sid in (0, 1):
        link.run_block(None, seed=1, stream_id=sid)
    be, fe, nc_, compared, _its = link.result()
    assert (be, fe, nc_) == (0, 0, 0) and compared == 2 * NCW * link.code.k
    errs, n = link.uncoded_result()
    assert n == 2 * link.nch and errs <= 2 * 2 * ((link.observe - 1) // 2)        # (at most the burst's end bits, whose windows hold zeros)
    if framed:
        blocks, wrong, (p, sigma, _best, _other) = link.sync_result()
        assert (blocks, wrong, p, sigma) == (2, 0, LEAD, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("framed", [False, True])
def test_channel_llrs_are_the_host_statements(framed):
    from waveforms_amd import _hip
    from waveforms_amd.cpm.pcmfm import freq_pulse_pcmfm

    link = _link(framed, carrier=CARRIER)
    ebn0, seed, sid = 6.0, 3, 2
    llr, info = link.channel_llrs(ebn0, seed, sid)
    received, _at, _syms = link.samples(link.encode(link.info_bits(sid)), ebn0, seed, sid)
    received = _hip.to_host(received, complex_pairs=True)
    pulse = freq_pulse_pcmfm(link.sps)
    T = nc.noncoherent_templates_host(pulse, 0.7, link.sps, link.observe, link.offset)
    assert link.start == nc.burst_start(pulse.size, link.sps, nc.DEFAULT_OFFSET) and link.offset == nc.DEFAULT_OFFSET
    want, _hard = nc.noncoherent_soft_host(received, T, link.sps, link.start, link.nsym)
    tol = lam_tolerance(received, link.observe, link.sps, link.start, link.nsym)
    if framed:
        (p, sigma, _best, _other), _folded = link.framing.search_host(want)
        assert (p, sigma) == (LEAD, 1) and int(link.lock.cpu()[0]) == LEAD
        want, tol = link.framing.gather_host(want, p, sigma, NCW), np.abs(link.framing.gather_host(tol, p, 1, NCW))
    else:
        want, tol = want[:link.nbits].reshape(NCW, -1), tol[:link.nbits].reshape(NCW, -1)
    got = _hip.to_host(llr)
    assert got.shape == want.shape == (NCW, link.code.n_tx) and tuple(info.shape) == (NCW, link.code.k)
    assert (np.abs(got - want) <= tol).all(), float((np.abs(got - want) / tol).max())
