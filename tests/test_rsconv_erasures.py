"""RSConvSOQPSKLink with erasures (waveforms_amd/encoding/rsconv.py): the last inner pass keeps its Λ, ``rs_mark_erasures``
declares the least reliable symbols of every RS codeword erased, and the RS decoder runs as an errors-and-erasures decoder.

Everything is exact: the declared erasures, the statuses, the message and the six counts of a block must equal the host
statements (``RSCode.mark_erasures_host``, ``decode_host(erasures=)``, ``counts_host(erasures=)``) applied to the Λ and the
decisions read back from the device.  With ``erasures=0`` the link is the link it always was.
"""
import numpy as np
import pytest

from waveforms_amd.encoding import conv, rs

NCW = 3                                    # frames (= convolutional codewords) per block
# The level of tests/test_rsconv_link.py: user Eb/N0 at which the inner decoder leaves errors and the errors-only RS decoder meets
# corrections AND failures.  Seen on an MI355X with seed 5, block 0, erasures = 8 (no threshold), by depth: the inner code's
# information bit errors, the RS statuses, and (erasures declared, erasures filled).  The run is deterministic.
NOISY_DB = 6.0
F_MAX = 8
NOISY_SEEN = {1: (155, [9, -1, 12], (24, 16)), 5: (635, [10, 9, 8, -1, 10, 10, -1, 10, 7, 12, 6, 5, 5, 5, 7], (120, 104))}


def make(depth, erasures, below=float("inf"), outer=1):
    from waveforms_amd.encoding.rsconv import RSConvSOQPSKLink

    code = rs.RSCode.ccsds(16, depth)
    inner = conv.ccsds_k7(8 * code.n * depth)
    return code, inner, RSConvSOQPSKLink(code, inner, NCW, detector="PT", outer=outer, erasures=erasures, erase_below=below)


def test_python_validation_without_a_gpu():
    from waveforms_amd.encoding.rsconv import RSConvSOQPSKLink

    code = rs.RSCode.ccsds(16, 1)
    inner = conv.ccsds_k7(8 * 255)
    for bad in (-1, 33):
        with pytest.raises(ValueError):
            RSConvSOQPSKLink(code, inner, 2, erasures=bad)
    with pytest.raises(ValueError):
        RSConvSOQPSKLink(code, inner, 2, erasures=4, erase_below=float("nan"))


@pytest.mark.gpu
@pytest.mark.parametrize("depth,outer", [(1, 1), (2, 3)])
def test_gpu_no_erasures_is_the_existing_link(depth, outer):
    """``erasures=0``: the same ``rs_result()``, ``result()``, statuses and message as a link built without the argument, on
    the same block; nothing is declared and Λ is not kept."""
    from waveforms_amd import _hip
    from waveforms_amd.encoding.rsconv import RSConvSOQPSKLink

    code, inner, link = make(depth, 0, outer=outer)
    old = RSConvSOQPSKLink(code, inner, NCW, detector="PT", outer=outer)
    for lk in (link, old):
        lk.run_block(NOISY_DB, seed=5, stream_id=0)
    assert link.rs_result() == old.rs_result() and link.result() == old.result() and link.rs_result()[3] > 0
    assert _hip.torch().equal(link.rs_status, old.rs_status) and _hip.torch().equal(link.rs_msg, old.rs_msg)
    assert link.rs_erasure_result() == (0, 0) and link.post is None and link.rs_erased is None and link.rs_counts.numel() == 5


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 5])
def test_gpu_noisy_block_with_erasures_equals_the_host_statements(depth):
    from waveforms_amd import _hip

    code, inner, link = make(depth, F_MAX)
    link.run_block(NOISY_DB, seed=5, stream_id=0)
    post = _hip.to_host(link.post).reshape(NCW, inner.k)
    decided = _hip.to_host(link.decided).reshape(NCW, inner.k)
    user = _hip.to_host(link.user).reshape(NCW, -1)
    got_era, got_msg, got_status = _hip.to_host(link.rs_erased), _hip.to_host(link.rs_msg), _hip.to_host(link.rs_status)
    rs_res, res, era_res = link.rs_result(), link.result(), link.rs_erasure_result()
    six = [int(v) for v in link.rs_counts.cpu().tolist()]
    assert post.dtype == np.float32 and np.isfinite(post).all() and np.array_equal(decided, (post < 0).astype(np.uint8))
    want_era = code.mark_erasures_host(post, F_MAX)
    f = code._split(want_era, code.n).sum(axis=1)
    print(f"depth {depth}: inner errors {res[0]} bits; statuses {got_status.tolist()}; declared / filled {era_res}; six counts {six}; f {f.tolist()}")
    assert np.array_equal(got_era, want_era)
    want_msg, want_status = code.decode_host(decided, bits=True, erasures=want_era)
    assert np.array_equal(got_status, want_status) and np.array_equal(got_msg, want_msg)
    assert six == code.counts_host(want_msg, want_status, user, bits=True, erasures=want_era)
    assert list(rs_res[:5]) == six[:5] and rs_res[5] == link.user_bits_per_block and era_res == (int(want_era.sum()), six[5])
    # the erasure decoder meets a codeword with f > 0 that succeeds and one that fails
    assert ((want_status >= 0) & (f > 0)).any() and ((want_status < 0) & (f > 0)).any()
    # the operating point: the run is deterministic, so the block is the one the level was chosen on
    assert (res[0], got_status.tolist(), era_res) == NOISY_SEEN[depth]
    # the errors-only decoder on the same decisions, for the record
    _m, plain = code.decode_host(decided, bits=True)
    print(f"depth {depth}: errors-only statuses on the same decisions {plain.tolist()}")
