"""RSConvSOQPSKLink (waveforms_amd/encoding/rsconv.py): the CCSDS RS(255, 223) code, interleaved, in front of the K = 7
(171, 133) convolutional code over SOQPSK-TG.

Everything is exact: the RS decoder's message, statuses and counts on a block must equal ``RSCode.decode_host`` applied to the
inner decoder's decisions of that block (``link.decided``), and ``result()`` must be the parent's count on the same bits.
"""
import numpy as np
import pytest

from waveforms_amd.encoding import conv, rs

NCW = 3                                    # frames (= convolutional codewords) per block
# The noisy block: user Eb/N0 in dB, chosen on an MI355X (a scan from 5 to 9 dB in steps of 0.5) so that the inner decoder leaves
# errors and the RS decoder meets corrections AND failures.  Seen there with seed 5, block 0, by (depth, outer): the inner code's
# information bit errors, and the RS statuses (the run is deterministic: the noisy test asserts them).
NOISY_DB = 6.0
NOISY_SEEN = {(1, 1): (155, [15, -1, 16]), (1, 3): (102, [8, 16, 9]), (2, 1): (290, [15, -1, -1, -1, 11, 9]), (2, 3): (167, [9, 9, 8, 9, 8, 9])}


def make(depth, outer=1, ncw=NCW):
    from waveforms_amd.encoding.rsconv import RSConvSOQPSKLink

    code = rs.RSCode.ccsds(16, depth)
    inner = conv.ccsds_k7(8 * code.n * depth)
    return code, inner, RSConvSOQPSKLink(code, inner, ncw, detector="PT", outer=outer)


def test_python_validation_without_a_gpu():
    from waveforms_amd.encoding.rsconv import RSConvSOQPSKLink

    code = rs.RSCode.ccsds(16, 2)
    with pytest.raises(ValueError):
        RSConvSOQPSKLink(code, conv.ccsds_k7(8 * 255), 2)                 # one codeword of the two of a frame
    with pytest.raises(ValueError):
        RSConvSOQPSKLink(code, conv.ccsds_k7(8 * 255 * 2 + 8), 2)
    with pytest.raises(ValueError):
        RSConvSOQPSKLink(code, conv.ccsds_k7(8 * 255 * 2), 2, framing=object())


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("outer", [1, 3])
def test_gpu_noiseless_blocks_are_clean(depth, outer):
    from waveforms_amd import _hip

    code, inner, link = make(depth, outer)
    assert link.user_bits_per_block == NCW * depth * 223 * 8
    assert abs(link._rate_db() - 10 * np.log10(inner.k / inner.n_tx * 223 / 255)) < 1e-12
    for b in range(2):
        link.run_block(None, seed=1, stream_id=b)
        assert not _hip.to_host(link.rs_status).any() and link.rs_status.numel() == NCW * depth
        assert _hip.torch().equal(link.rs_msg.view(-1), link.user)
    assert link.rs_result() == (0, 0, 0, 0, 0, 2 * link.user_bits_per_block)
    assert link.result() == (0, 0, 2 * NCW * inner.k)
    # the user bits are PN23, block after block, and the inner code's message is their RS frames
    u0, u1 = _hip.to_host(link.info_bits(0)), _hip.to_host(link.info_bits(1))
    user1 = _hip.to_host(link.user)
    assert np.array_equal(u1.reshape(NCW, -1), code.encode_host(user1.reshape(NCW, -1), bits=True)) and not np.array_equal(u0, u1)
    link.reset_counts()
    assert link.rs_result() == (0, 0, 0, 0, 0, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("outer", [1, 3])
def test_gpu_noisy_block_equals_the_host_decoder(depth, outer):
    """One block at NOISY_DB: the inner decoder leaves errors, and what the RS decoder makes of them is decode_host's result."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.encoding.sccc import ConvSOQPSKLink

    code, inner, link = make(depth, outer)
    link.run_block(NOISY_DB, seed=5, stream_id=0)
    decided = _hip.to_host(link.decided).reshape(NCW, inner.k)
    user = _hip.to_host(link.user).reshape(NCW, -1)
    got_msg, got_status = _hip.to_host(link.rs_msg), _hip.to_host(link.rs_status)
    rs_res, res = link.rs_result(), link.result()
    # result() is the parent class's own, on the same counters, and counts the inner code's errors on the RS-coded bits
    assert res == ConvSOQPSKLink.result(link)
    info = _hip.to_host(dev.rs_encode(code, link.user, bits=True)).reshape(NCW, inner.k)
    wrong = decided != info
    print(f"depth {depth}, outer {outer}: inner errors {int(wrong.sum())} bits in {int(wrong.any(axis=1).sum())} codewords; RS: {rs_res}; "
          f"statuses {got_status.tolist()}")
    assert res == (int(wrong.sum()), int(wrong.any(axis=1).sum()), NCW * inner.k)
    # the operating point: the run is deterministic, so the block is the one the level was chosen on
    assert (res[0], got_status.tolist()) == NOISY_SEEN[(depth, outer)]
    want_msg, want_status = code.decode_host(decided, bits=True)
    assert np.array_equal(got_msg, want_msg) and np.array_equal(got_status, want_status)
    assert list(rs_res[:5]) == code.counts_host(want_msg, want_status, user, bits=True) and rs_res[5] == link.user_bits_per_block


@pytest.mark.gpu
def test_gpu_coded_ber_tool_rs_form():
    """tools/coded_ber.py --code conv-k7 --rs 16: ONE JSON line whose counts are those of an RSConvSOQPSKLink run on the same
    blocks (the tool is what this test is about)."""
    import json
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    cmd = [sys.executable, str(root / "tools" / "coded_ber.py"), "--code", "conv-k7", "--rs", "16", "--rs-depth", "2", "--ebn0", str(NOISY_DB),
           "--codewords", "4", "--block-codewords", "2", "--steps", "1"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert (out["code"], out["k"], out["block_codewords"]) == ("conv-k7", 8 * 255 * 2, 2)
    assert (out["rs"]["n"], out["rs"]["k"], out["rs"]["depth"], out["rs"]["user_bits_per_block"]) == (255, 223, 2, 2 * 2 * 223 * 8)
    (p,) = out["points"]
    r = p["rs"]
    assert r["ms_per_block"]["rs_decode"] > 0 and r["ms_per_block"]["rs_encode"] > 0 and r["rs_decode_over_siso"] > 0
    _code, _inner, link = make(2, 1, ncw=2)
    for b in range(2):
        link.run_block(NOISY_DB, seed=1, stream_id=b)
    be, ce, fl, cor, fe, m = link.rs_result()
    assert (r["user_bit_errors"], r["codeword_errors"], r["flagged_failures"], r["symbols_corrected"], r["frame_errors"], r["user_bits"]) == (be, ce, fl, cor, fe, m)
    assert r["miscorrections"] == ce - fl and r["user_ber"] == be / m and r["fer"] == fe / 4
    ibe, ife, im = link.result()
    assert (p["info_bit_errors"], p["codeword_errors"]) == (ibe, ife) and p["coded_ber"] == ibe / im
