"""TurboSOQPSKLink (waveforms_amd/encoding/pccc.py): a turbo code behind differentially precoded SOQPSK-TG, decoded in one
launch per pass.  The link's decisions must equal ``device.turbo_decode`` applied by hand to the link's own detector outputs."""
import numpy as np
import pytest

from waveforms_amd.encoding import turbo


def link_code():
    return turbo.TurboCode.qpp(512, 31, 64)


def test_link_python_validation_without_a_gpu():
    from waveforms_amd.encoding.pccc import TurboSOQPSKLink

    code = turbo.TurboCode.qpp(40, 3, 10)
    for kw in ({"framing": object()}, {"outer": 0}, {"iters": 0}, {"iters": 33}, {"damping": 0.0}, {"damping": float("nan")}, {"ext_scale": 0.0},
               {"ext_scale": float("inf")}, {"ext_clip": 0.0}, {"ext_clip": -1.0}):
        with pytest.raises(ValueError):
            TurboSOQPSKLink(code, 4, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("detector", ["PT", "PAM"])
def test_gpu_noiseless_blocks_and_outer_1_is_turbo_decode_on_channel_llrs(detector):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.encoding.pccc import TurboSOQPSKLink

    code = link_code()
    for outer in (1, 3):
        quiet = TurboSOQPSKLink(code, 21, detector=detector, outer=outer, iters=2, per_pass=True)
        quiet.run_block(None, seed=1, stream_id=0)
        quiet.run_block(None, seed=1, stream_id=1)
        assert quiet.result() == (0, 0, 2 * 21 * code.k)
        assert quiet.pass_results() == [(0, 0)] * outer and quiet.uncoded_result() == (0, 2 * 21 * code.n_tx)
        assert quiet.half_iterations() == 2.0                         # every codeword stops after its first iteration

    one = TurboSOQPSKLink(code, 21, detector=detector, outer=1, iters=4)
    one.run_block(5.0, seed=5, stream_id=2)
    llr, info = one.channel_llrs(5.0, seed=5, stream_id=2)
    want = dev.turbo_decode(code, llr, half_iters=8, ext_scale=0.75, early_stop=True, ref_info=info)
    assert _hip.torch().equal(one.decided, want["info_bits"])
    be, fe, halves = (int(v) for v in _hip.to_host(want["counts"]))
    assert one.result() == (be, fe, 21 * code.k) and one.uncoded_result()[0] > 0
    assert one.half_iterations() == halves / 21
    _hip.device_check()


@pytest.mark.gpu
def test_gpu_loop_pass_by_pass_and_gain():
    """A burst of 12 codewords at 6.0 dB, 3 passes of one iteration each: after every pass the decisions, constituent 1's prior
    and the burst's prior buffer equal ``device.turbo_decode`` applied by hand to the detector output of that pass; row 0 and
    the tail rows keep prior 0; the codeword errors do not grow from pass to pass."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.encoding.pccc import TurboSOQPSKLink

    code = link_code()
    ncw = 12
    link = TurboSOQPSKLink(code, ncw, detector="PT", outer=3, iters=1, per_pass=True)
    assert link.ext_clip == 50.0 and link.damping == 0.7 and link.ext_scale == 0.75
    info = link.info_bits(0)
    rows, _ = link.front_end(dev.turbo_encode(code, info), 6.0, 7, 0)
    n = int(rows.shape[0])
    link.begin(n)
    torch = _hip.torch()
    a1 = torch.zeros((ncw, code.k), dtype=torch.float32, device="cuda")
    for o in range(3):
        ext, _ = link.detect(rows, first=o == 0)
        mine = torch.zeros(n, dtype=torch.float32, device="cuda")
        want = dev.turbo_decode(code, ext.contiguous(), half_iters=2, ext_scale=0.75, early_stop=True, a1=a1, ext=mine[1:1 + link.nbits],
                                ext_stride=code.n_tx, ext_clip=50.0)
        link.decode(ext)
        assert torch.equal(link.decided, want["info_bits"]), o
        assert torch.equal(link.a1.view(torch.int32), a1.view(torch.int32)), o
        assert torch.equal(link.prior.view(torch.int32), mine.view(torch.int32)), o
    prior = _hip.to_host(link.prior)
    assert prior[0] == 0 and (prior[1 + link.nbits:] == 0).all() and np.abs(prior).max() <= 50.0 and np.abs(prior).max() > 0

    link.run_block(6.0, seed=7, stream_id=0)
    be, fe, m = link.result()
    passes = link.pass_results()
    print("per pass (information bit errors, codeword errors):", passes)
    assert passes[-1] == (be, fe) and m == ncw * code.k
    assert torch.equal(link.decided, want["info_bits"])               # the block run is the loop walked by hand above
    assert all(b[1] <= a[1] for a, b in zip(passes, passes[1:]))
    _hip.device_check()

