"""The coded SOQPSK-TG chain (waveforms_amd/encoding/coded.py): LDPC encode -> SOQPSK-TG + AWGN + PT / PAM bank ->
viterbi_soft -> LDPC decode, every stage on the GPU.

Operating point of the bound test: information Eb/N0 = 7 dB (channel 3.99 dB per coded bit, rate-1/2 demo code).
Measured on one MI355X (the test's own blocks, 2 000 codewords): PT uncoded BER 5.90e-2, 0 information bit errors, 0
codeword errors, mean 2.44 iterations; PAM uncoded 4.36e-2, 0 errors, mean 2.03 iterations.  tools/coded_ber.py over
24 410 PT codewords: 0 errors at 7 dB, and 1.35e-5 BER / 0.20 % FER at 6 dB.  So the bounds (uncoded > 1e-2, coded BER
<= 1e-4, FER <= 1 %) hold with a margin of about 1 dB; the first cut of the demo code (girth 6) missed the FER bound here
(52 of 2 000), which is why the demo code's search also avoids 6-cycles.
"""
import numpy as np
import pytest

from waveforms_amd.encoding import ldpc


@pytest.mark.gpu
@pytest.mark.parametrize("detector", ["PT", "PAM"])
def test_noiseless_chain_is_error_free_at_iteration_zero(detector):
    """Checks the alignment (bit j <-> λ_{j+1}), the interleaver and the tail padding end to end."""
    from waveforms_amd.encoding.coded import CodedSOQPSKLink

    link = CodedSOQPSKLink(ldpc.demo_code(), 37, detector=detector)
    link.run_block(None, seed=1, stream_id=0)
    link.run_block(None, seed=1, stream_id=1)
    be, fe, nc, m, mean_it = link.result()
    assert (be, fe, nc, mean_it) == (0, 0, 0, 0.0) and m == 2 * 37 * 1024
    ue, um = link.uncoded_result()
    assert ue == 0 and um == 2 * 37 * 2048


@pytest.mark.gpu
@pytest.mark.parametrize("detector", ["PT", "PAM"])
def test_coded_chain_at_7db(detector):
    from waveforms_amd.encoding.coded import CodedSOQPSKLink

    link = CodedSOQPSKLink(ldpc.demo_code(), 500, detector=detector)
    for b in range(4):
        link.run_block(7.0, seed=11, stream_id=b)
    be, fe, nc, m, mean_it = link.result()
    ue, um = link.uncoded_result()
    print(f"{detector}: uncoded {ue / um:.3e}, coded BER {be / m:.3e}, FER {fe / 2000:.3e}, not converged {nc}, mean iters {mean_it:.2f}")
    assert m == 2000 * 1024
    assert ue / um > 1e-2
    assert be / m <= 1e-4 and fe <= 20
