"""The coded SOQPSK-TG links with a coarse frequency acquisition in front of the fine synchronisers
(waveforms_amd/encoding/coded.py: ``coarse=``): a framed link with the demo code, 40 degrees and 0.02 cycles per sample off - 0.16
of the bit rate, 800 times what ``CarrierRecovery`` and ``JointAcquisition`` follow."""
import math

import numpy as np
import pytest

from waveforms_amd.encoding import framing as FR
from waveforms_amd.encoding import ldpc
from waveforms_amd.sync import carrier as C
from waveforms_amd.sync import coarse as K
from waveforms_amd.sync import joint as J
from waveforms_amd.sync import timing as T

LEAD, SPS, NFFT = 37, 8, 1024
PER_WINDOW = SPS * C.DEFAULT_WINDOW
NU = 0.02
CARRIER = (math.radians(40.0), NU)
# the joint test's first impairment (tests/test_joint.py: 40 degrees, 0.025 turns, 6 samples, 0.8 samples per window) plus NU
JOINT_CARRIER = (math.radians(40.0), NU + 0.025 / PER_WINDOW)
JOINT_TIMING = (6.0, 0.8 / PER_WINDOW)


def _ncw(code, fr) -> int:
    """The fewest codewords whose burst (lead bits, frames, pad) holds four segments of NFFT bits."""
    from waveforms_amd.encoding.coded import PAD_BITS

    return -(-(4 * NFFT - LEAD - PAD_BITS) // fr.period)


def _links(cls=None, **kw):
    from waveforms_amd.encoding.coded import CodedSOQPSKLink

    code = ldpc.demo_code()
    fr = FR.Framing(code)
    return code, [(cls or CodedSOQPSKLink)(code, _ncw(code, fr), framing=fr, lead_bits=LEAD, **k) for k in kw.values()]


def test_links_refuse_what_the_coarse_acquisition_cannot_do():
    """Each with a ValueError, before anything touches a device: no recovery and no acquisition behind it (the residual phase is
    unknown), a timing recovery alone (that path excludes a carrier), another sps, something that is no CoarseFrequency.  The CPM
    classes do not have the keyword: PCM/FM and ARTM have no usable lines."""
    from waveforms_amd.encoding.coded import CodedCPMLink, CodedSOQPSKLink, IterativeCPMLink, IterativeSOQPSKLink

    code = ldpc.demo_code()
    framing = object()                                    # (never reached: every refusal comes before the framing is looked at)
    for cls in (CodedSOQPSKLink, IterativeSOQPSKLink):
        with pytest.raises(ValueError, match="needs a recovery or an acquisition"):
            cls(code, 2, framing=framing, coarse=K.CoarseFrequency(SPS))
        with pytest.raises(ValueError, match="excludes timing_recovery"):
            cls(code, 2, framing=framing, coarse=K.CoarseFrequency(SPS), timing_recovery=T.TimingRecovery(SPS))
        with pytest.raises(ValueError, match="sps"):
            cls(code, 2, framing=framing, coarse=K.CoarseFrequency(10), acquisition=J.JointAcquisition(SPS))
        with pytest.raises(ValueError, match="CoarseFrequency"):
            cls(code, 2, framing=framing, coarse=C.CarrierRecovery(), acquisition=J.JointAcquisition(SPS))
    for cls in (CodedCPMLink, IterativeCPMLink):
        with pytest.raises(TypeError):
            cls(code, 2, coarse=K.CoarseFrequency(SPS))


@pytest.mark.gpu
def test_framed_link_with_recovery_needs_the_coarse_stage_noiseless():
    """``recovery=`` alone loses every codeword at 0.02 cycles per sample; with ``coarse=`` beside it the link loses none."""
    code, (fine, both) = _links(fine={"carrier": CARRIER, "recovery": C.CarrierRecovery()},
                                both={"carrier": CARRIER, "recovery": C.CarrierRecovery(), "coarse": K.CoarseFrequency(SPS, nfft=NFFT)})
    assert both.nsym >= 4 * NFFT > both.nsym - both.framing.period
    for lk in (fine, both):
        lk.run_block(None, seed=1, stream_id=0)
    be, fe, nc, m, _its = both.result()
    assert (be, fe, nc, m) == (0, 0, 0, both.ncw * code.k)
    assert both.sync_result()[2][0] == LEAD
    nu, eps, peak, mean = both.coarse_result()
    print(f"nu^ - nu = {nu - NU:+.2e}, eps^ = {eps:+.2e}, peak / mean = {peak / mean:.0f}")
    assert abs(nu - NU) <= C.MAX_DRIFT_TURNS / PER_WINDOW and peak > 10.0 * mean
    assert fine.result()[1] == fine.ncw                       # without this the test shows nothing
    with pytest.raises(RuntimeError):
        fine.coarse_result()


@pytest.mark.gpu
def test_framed_link_with_acquisition_needs_the_coarse_stage_noiseless():
    """The same beside ``JointAcquisition(8, anchor=33)`` under the joint test's first impairment plus 0.02 cycles per sample."""
    imp = {"carrier": JOINT_CARRIER, "timing": JOINT_TIMING}
    code, (fine, both) = _links(fine={**imp, "acquisition": J.JointAcquisition(SPS, anchor=33)},
                                both={**imp, "acquisition": J.JointAcquisition(SPS, anchor=33), "coarse": K.CoarseFrequency(SPS, nfft=NFFT)})
    for lk in (fine, both):
        lk.run_block(None, seed=1, stream_id=0)
    be, fe, nc, m, _its = both.result()
    assert (be, fe, nc, m) == (0, 0, 0, both.ncw * code.k)
    assert abs(both.sync_result()[2][0] - LEAD) <= 3          # (the joint lattice: tests/test_joint_link.py)
    nu, eps, _peak, _mean = both.coarse_result()
    true_nu = JOINT_CARRIER[1] * (1.0 + JOINT_TIMING[1])      # the clock reads the rotated signal: cycles per RECEIVED sample
    print(f"nu^ - nu = {nu - true_nu:+.2e}, eps^ - eps = {eps - JOINT_TIMING[1]:+.2e}")
    assert abs(nu - true_nu) <= C.MAX_DRIFT_TURNS / PER_WINDOW
    assert len(both.acquisition_result()) >= 4
    assert fine.result()[1] == fine.ncw


@pytest.mark.gpu
def test_iterative_link_takes_the_coarse_stage_too():
    from waveforms_amd.encoding.coded import IterativeSOQPSKLink

    code, (link,) = _links(IterativeSOQPSKLink, both={"outer": 3, "inner": 5, "carrier": CARRIER, "recovery": C.CarrierRecovery(),
                                                      "coarse": K.CoarseFrequency(SPS, nfft=NFFT)})
    link.run_block(None, seed=1, stream_id=0)
    be, fe, _nc, m, _its = link.result()
    assert (be, fe, m) == (0, 0, link.ncw * code.k) and link.sync_result()[2][0] == LEAD
    assert abs(link.coarse_result()[0] - NU) <= C.MAX_DRIFT_TURNS / PER_WINDOW


@pytest.mark.gpu
def test_default_arguments_leave_the_link_bitwise_alone():
    """A link with ``coarse=None`` produces the rows, bit for bit, and the counts of a link built without the argument - with a
    recovery, with an acquisition and with neither."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    ebn0, seed, sid = 6.0, 1, 3
    for kw in ({}, {"carrier": (0.3, 1e-5), "recovery": C.CarrierRecovery()}, {"carrier": (0.3, 1e-5), "acquisition": J.JointAcquisition(SPS)}):
        code, (plain, explicit) = _links(plain=dict(kw), explicit={**kw, "coarse": None})
        rows = []
        for lk in (plain, explicit):
            assert lk.coarse is None
            rows.append(_hip.to_host(lk.front_end(dev.ldpc_encode(code, lk.info_bits(sid)), ebn0, seed, sid)[0]))
            lk.run_block(ebn0, seed=seed, stream_id=sid)
            with pytest.raises(RuntimeError):
                lk.coarse_result()
        assert np.array_equal(rows[0].view(np.uint64), rows[1].view(np.uint64))
        assert plain.counts.cpu().tolist() == explicit.counts.cpu().tolist() and plain.sync_result() == explicit.sync_result()
