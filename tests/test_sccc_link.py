"""ConvSOQPSKLink (waveforms_amd/encoding/sccc.py): a convolutional code, its interleaver and differentially precoded SOQPSK-TG
decoded iteratively.  The GPU loop must equal, pass by pass and bit for bit, the host chain of the two restatements
(tests/test_idd.py: ``apriori_restatement``; tests/test_conv.py: ``siso_restatement``) fed the GPU's rows."""
import numpy as np
import pytest

import test_conv as TC
import test_idd as TI
from waveforms_amd.encoding import conv


def sccc_code():
    """The (7, 5) code with k = 1022 behind the QPP interleaver (31 t + 64 t^2) mod 2048."""
    return conv.nasa_k3(1022, tx_order=conv.qpp_order(2048, 31, 64))


def test_link_python_validation_without_a_gpu():
    from waveforms_amd.encoding.sccc import ConvSOQPSKLink

    code = conv.nasa_k3(30)
    for kw in ({"framing": object()}, {"outer": 0}, {"damping": 0.0}, {"damping": float("nan")}, {"ext_clip": 0.0}, {"ext_clip": -1.0}):
        with pytest.raises(ValueError):
            ConvSOQPSKLink(code, 4, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("detector", ["PT", "PAM"])
def test_gpu_noiseless_blocks_and_outer_1_is_conv_siso_on_channel_llrs(detector):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.encoding.sccc import ConvSOQPSKLink

    code = sccc_code()
    for outer in (1, 3):
        quiet = ConvSOQPSKLink(code, 37, detector=detector, outer=outer, per_pass=True)
        quiet.run_block(None, seed=1, stream_id=0)
        quiet.run_block(None, seed=1, stream_id=1)
        assert quiet.result() == (0, 0, 2 * 37 * code.k)
        assert quiet.pass_results() == [(0, 0)] * outer and quiet.uncoded_result() == (0, 2 * 37 * code.n_tx)

    k7 = conv.ccsds_k7(1018)
    for c in (code, k7):
        one = ConvSOQPSKLink(c, 61, detector=detector, outer=1)
        one.run_block(3.0, seed=5, stream_id=2)
        llr, info = one.channel_llrs(3.0, seed=5, stream_id=2)
        want = dev.conv_siso(c, llr, ref_info=info)
        assert _hip.torch().equal(one.decided, want["info_bits"])
        be, fe = (int(v) for v in _hip.to_host(want["counts"]))
        assert one.result() == (be, fe, 61 * c.k) and be > 0
    _hip.device_check()


@pytest.mark.gpu
def test_gpu_loop_pass_by_pass(oracle):
    """A burst of 8 codewords at 4.0 dB, 4 passes: the prior buffer and the decisions after every pass equal the host chain
    made of the two restatements, fed the GPU's rows; row 0 and the tail rows keep prior 0."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.encoding.sccc import ConvSOQPSKLink

    code = sccc_code()
    link = ConvSOQPSKLink(code, 8, detector="PT", outer=4)
    assert link.ext_clip == 50.0 and link.damping == 0.7
    info = link.info_bits(0)
    rows, _ = link.front_end(dev.conv_encode(code, info), 4.0, 7, 0)
    h = _hip.to_host(rows).reshape(-1, 3, 2)
    z = h[..., 0] + 1j * h[..., 1]
    n = z.shape[0]
    u = _hip.to_host(info).reshape(8, code.k)
    prior = np.zeros(n, dtype=np.float32)
    link.begin(n)
    errs = []
    for o in range(4):
        ext, _ = link.detect(rows, first=o == 0)
        link.decode(ext)
        want_ext, _ = TI.apriori_restatement(oracle, z, prior, link.damping, True)
        assert np.array_equal(_hip.to_host(ext).reshape(-1).view(np.uint64), want_ext[1:1 + link.nbits].view(np.uint64)), o
        bits, _lam, e, _P = TC.siso_restatement(code, want_ext[1:1 + link.nbits].reshape(8, code.n_tx), None, 1.0, link.ext_clip)
        prior[1:1 + link.nbits] = e.reshape(-1)
        assert np.array_equal(_hip.to_host(link.prior).view(np.uint32), prior.view(np.uint32)), o
        assert np.array_equal(_hip.to_host(link.decided), bits), o
        errs.append(int((bits != u).sum()))
    _hip.device_check()
    assert prior[0] == 0 and (prior[1 + link.nbits:] == 0).all() and np.abs(prior).max() <= 50.0
    print("information bit errors after each pass:", errs)
    assert errs[-1] < errs[0]                                # the loop does something on this burst


@pytest.mark.gpu
def test_gpu_iterative_gain_on_a_full_block():
    """One 1e7-channel-bit block (4 882 codewords of the interleaved (7, 5) code, k = 1022, in ONE burst) at 4.0 dB, 8 passes.
    Measured on one MI355X: frame errors per pass 4 882, 4 440, 790, 35, 6, 0, 0, 0 (information bit errors 420 433, 68 818, 3 843,
    159, 8, 0, 0, 0 of 4 989 404)."""
    from waveforms_amd.encoding.sccc import ConvSOQPSKLink

    code = sccc_code()
    ncw = int(1e7) // code.n_tx
    assert ncw == 4882
    link = ConvSOQPSKLink(code, ncw, detector="PT", outer=8, damping=0.7, per_pass=True)
    link.run_block(4.0, seed=9, stream_id=0)
    be, fe, m = link.result()
    passes = link.pass_results()
    print(f"per pass (information bit errors, frame errors): {passes}; final {be} of {m} bits, {fe} of {ncw} frames")
    assert passes[-1] == (be, fe) and m == ncw * code.k
    assert passes[0][1] >= 4
    assert 4 * fe <= passes[0][1]


@pytest.mark.gpu
@pytest.mark.parametrize("code, outer", [("conv-k3", 3), ("conv-k7", 1)])
def test_gpu_coded_ber_tool_conv_forms(code, outer):
    """tools/coded_ber.py --code conv-*: runs to the end on a small block and prints ONE JSON line whose counts are those of a
    ConvSOQPSKLink run on the same blocks (the tool is what this test is about: one process per form)."""
    import json
    import subprocess
    import sys
    from pathlib import Path

    from waveforms_amd.encoding.sccc import ConvSOQPSKLink

    root = Path(__file__).resolve().parent.parent
    K = 3 if code == "conv-k3" else 7
    k = 256 - (K - 1)                                                 # n = 512: the QPP interleaver needs a power of two
    cmd = [sys.executable, str(root / "tools" / "coded_ber.py"), "--code", code, "--info-bits", str(k), "--outer", str(outer), "--ebn0", "3.0",
           "--codewords", "24", "--block-codewords", "12", "--steps", "1"] + (["--interleave"] if code == "conv-k3" else [])
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert (out["code"], out["K"], out["k"], out["n_tx"], out["outer"], out["block_codewords"]) == (code, K, k, 512, outer, 12)
    assert out["geometry"]["codewords_per_wave"] == 64 >> (K - 1) and out["geometry"]["waves"] == -(-12 // (64 >> (K - 1)))
    (p,) = out["points"]
    ms = p["ms_per_block"]
    assert p["codewords"] == 24 and len(p["per_pass"]) == len(ms["detector_passes"]) == len(ms["siso_passes"]) == outer
    assert all(v > 0 for v in ms["detector_passes"] + ms["siso_passes"]) and p["siso_info_gbps"] > 0
    order = conv.qpp_order(out["n"], 31, 64) if code == "conv-k3" else None
    link = ConvSOQPSKLink((conv.nasa_k3 if K == 3 else conv.ccsds_k7)(k, tx_order=order), 12, outer=outer, per_pass=True)
    for b in range(2):
        link.run_block(3.0, seed=1, stream_id=b)
    be, fe, m = link.result()
    assert (p["info_bit_errors"], p["codeword_errors"]) == (be, fe) and p["coded_ber"] == be / m and p["fer"] == fe / 24
    assert [(q["info_bit_errors"], q["codeword_errors"]) for q in p["per_pass"]] == link.pass_results()
