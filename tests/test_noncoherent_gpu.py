"""``device.noncoherent_soft`` (wf_noncoherent_soft_c128) against the host statement on RANDOM complex input: every observation
length at sps 8 and 4, windows that begin in front of the burst and run past its end, 1 and 2 bits, one below, at and above the
kernel's tile, and several workgroups; the all-zero edge; ``out=`` and repeated calls into the same buffers.  The kernel
re-associates the sums, so λ is compared within the rounding bound of ``lam_tolerance`` and decisions wherever |λ| exceeds it;
at most 1e-3 of the bits may fall below it, not counting the windows that tie by the definition itself (``structural_ties``)."""
import numpy as np
import pytest

from test_noncoherent import H, lam_tolerance
from waveforms_amd.viterbi import noncoherent as nc

NSAMP = 2600


def _tile(N, sps):
    from waveforms_amd import device as dev

    return dev.noncoherent_geometry(N, sps, 1)["tile_bits"]


@pytest.fixture(scope="module")
def random_input():
    rng = np.random.Generator(np.random.PCG64(seed=77))
    return rng.normal(size=(NSAMP, 2)).view(np.complex128).reshape(-1) * rng.uniform(0.2, 3.0, size=NSAMP)


def structural_ties(n: int, pulse, N: int, sps: int, offset: int, start: int, nbits: int) -> np.ndarray:
    """bool[nbits]: the bits whose window holds no sample of the burst that the MIDDLE bit moves.  Flipping window bit c changes
    template sample k by a phase 4π h q[k + offset - c sps]: nothing in front of its pulse (q = 0) and one constant factor behind
    it (q at its final value), which a magnitude does not see.  A window that meets the burst only there - one that hangs over
    the burst's first or last samples by a few - has λ = 0 by the definition itself, whatever the input: it is a tie of the
    detector, not a near-tie of the data, and the count of bits left out of the decision comparison does not include it."""
    K, c = N * sps, (N - 1) // 2
    q = np.cumsum(pulse) / sps
    m = np.arange(K) + offset - c * sps
    qm = np.where(m < 0, 0.0, q[np.clip(m, 0, q.size - 1)])
    moved = (qm != 0.0) & (qm != q[-1])
    idx = start - c * sps + np.arange(nbits)[:, None] * sps + np.arange(K)[None, :]
    return ~(((idx >= 0) & (idx < n)) & moved[None, :]).any(axis=1)


def _compare(received, d_received, T, d_T, N, sps, start, nbits, out=None, ties=None):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    lam_d, bits_d = dev.noncoherent_soft(d_received, d_T, sps, start, nbits, out=out)
    lam, hard = _hip.to_host(lam_d), _hip.to_host(bits_d)
    want, want_hard = nc.noncoherent_soft_host(received, T, sps, start, nbits)
    tol = lam_tolerance(received, N, sps, start, nbits)
    err = np.abs(lam - want)
    assert lam.shape == (nbits,) and hard.shape == (nbits,) and hard.dtype == np.uint8
    assert (err <= tol).all(), (N, sps, start, nbits, int(np.argmax(err - tol)), float(err.max()), float(tol.max()))
    sure = np.abs(want) > tol
    left_out = ~sure if ties is None else ~sure & ~ties
    assert np.count_nonzero(left_out) <= 1e-3 * nbits, (N, sps, start, nbits, int(np.count_nonzero(left_out)))
    assert np.array_equal(hard[sure], want_hard[sure]), (N, sps, start, nbits)
    assert np.array_equal(hard, (lam < 0).astype(np.uint8))
    return lam_d, bits_d


@pytest.mark.gpu
@pytest.mark.parametrize("sps", [8, 4])
@pytest.mark.parametrize("N", nc.OBSERVATIONS)
def test_parity_with_the_host_statement(oracle, random_input, N, sps):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    tile = _tile(N, sps)
    assert tile == 256
    offset = min(nc.DEFAULT_OFFSET, sps)
    pulse = oracle.freq_pulse_pcmfm(sps)
    T = nc.noncoherent_templates_host(pulse, H, sps, N, offset)
    d_T = dev.noncoherent_templates(pulse, H, sps, N, offset)
    assert np.array_equal(_hip.to_host(d_T, complex_pairs=True), T)
    received = random_input[:NSAMP if sps == 8 else NSAMP // 2]
    d_received = _hip.to_device(received)
    whole = received.size // sps
    # (start, nbits): in front of the burst, inside it, past its end (start + nbits sps > n), far outside on either side
    cases = [(0, 1), (-1, 2), (-5 * sps - 3, tile - 1), (3, tile), (-sps, tile + 1), (received.size - 100 * sps, tile + 1),
             (-2 * N * sps, 3 * tile + 19), (7, whole + N), (-(N + 3) * sps, 5), (received.size + sps, 3)]
    assert any(s < 0 for s, _ in cases) and any(s + nb * sps > received.size for s, nb in cases) and max(nb for _, nb in cases) > 3 * tile
    for start, nbits in cases:
        ties = structural_ties(received.size, pulse, N, sps, offset, start, nbits)
        hangs = ties & (lam_tolerance(received, N, sps, start, nbits) > 0.0)     # (the other ties miss the burst: λ is +0 exactly)
        assert np.count_nonzero(hangs) <= 2 * N                         # (only windows that hang over an end of the burst)
        _compare(received, d_received, T, d_T, N, sps, start, nbits, ties=ties)


@pytest.mark.gpu
def test_random_tables_too(random_input):
    """The kernel takes any table as it is: unit-modulus rows with random phases, N = 5 at sps 8."""
    from waveforms_amd import _hip

    rng = np.random.Generator(np.random.PCG64(seed=5))
    T = np.exp(2j * np.pi * rng.uniform(size=(32, 40)))
    _compare(random_input[:2000], _hip.to_device(random_input[:2000]), T, _hip.to_device(T), 5, 8, 16, 240)      # (every window inside the burst)
    _compare(random_input, _hip.to_device(random_input), T, _hip.to_device(T), 5, 8, 2 * 8 + 3, 300)


@pytest.mark.gpu
@pytest.mark.parametrize("N", nc.OBSERVATIONS)
def test_all_zero_input_gives_plus_zero(oracle, N):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    d_T = dev.noncoherent_templates(oracle.freq_pulse_pcmfm(8), H, 8, N)
    lam, hard = dev.noncoherent_soft(_hip.zeros((3000, 2), "float64"), d_T, 8, -3, 300)
    lam, hard = _hip.to_host(lam), _hip.to_host(hard)
    assert not lam.any() and not np.signbit(lam).any() and not hard.any()


@pytest.mark.gpu
def test_out_buffers_and_reuse(oracle, random_input):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    N, sps, nbits = 5, 8, 300
    pulse = oracle.freq_pulse_pcmfm(sps)
    T = nc.noncoherent_templates_host(pulse, H, sps, N, nc.DEFAULT_OFFSET)
    d_T, d_received = dev.noncoherent_templates(pulse, H, sps, N), _hip.to_device(random_input)
    out = (_hip.empty(nbits, "float64"), _hip.empty(nbits, "uint8"))
    first = None
    for start in (-3, 40, -3):
        lam_d, bits_d = _compare(random_input, d_received, T, d_T, N, sps, start, nbits, out=out)
        assert lam_d.data_ptr() == out[0].data_ptr() and bits_d.data_ptr() == out[1].data_ptr()
        if first is None:
            first = (_hip.to_host(lam_d), _hip.to_host(bits_d))
    assert np.array_equal(_hip.to_host(out[0]), first[0]) and np.array_equal(_hip.to_host(out[1]), first[1])      # same input, same bits
    with pytest.raises(ValueError, match="out must be"):
        dev.noncoherent_soft(d_received, d_T, sps, 0, nbits + 1, out=out)
    with pytest.raises(ValueError, match="nbits"):
        dev.noncoherent_soft(d_received, d_T, sps, 0, 0)
    with pytest.raises(ValueError, match="templates"):
        dev.noncoherent_soft(d_received, d_T[:16].contiguous(), sps, 0, 4)
    with pytest.raises(ValueError, match="sps"):
        dev.noncoherent_soft(d_received, _hip.to_device(np.ones((8, 15), dtype=np.complex128)), 5, 0, 4)          # no instantiation for sps 5
