"""tests/golden/noncoherent_scan.json: the host scan behind ``DEFAULT_OFFSET`` and ``MAX_OFFSET_CYCLES`` of
waveforms_amd/viterbi/noncoherent.py (no GPU).

The signal is the oracle's PCM/FM signal (h = 0.7, sps 8) of 100 000 random bits, the noise numpy's from the same fixed seed, at a
channel Eb/N0 of 7 dB; the detector is the host statement.  Bits c .. nbits - 1 - c are compared (c = (N - 1) / 2).

    offsets            errors of N = 5 per window offset 0 .. sps; default_offset = the fewest, the smallest on a tie
    grid               errors per N and per frequency offset ν (cycles per sample) at default_offset
    max_offset_cycles  per N the largest ν of the grid with at most twice the errors at ν = 0

    python tests/golden/make_noncoherent_scan.py
"""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

import oracle  # noqa: E402
from waveforms_amd.viterbi.noncoherent import OBSERVATIONS, burst_start, noncoherent_soft_host, noncoherent_templates_host  # noqa: E402

SEED, NBITS, SPS, EBN0_DB, H = 20261, 100000, 8, 7.0, 0.7
GRID = (0.0, 5e-4, 1e-3, 2e-3, 3e-3, 4e-3, 6e-3, 8e-3)


def burst(seed: int = SEED, nbits: int = NBITS, sps: int = SPS, ebn0_db: float | None = EBN0_DB):
    """(bits, noisy samples, pulse) of the scan's burst; ``ebn0_db=None``: noiseless."""
    rng = np.random.Generator(np.random.PCG64(seed=seed))
    bits = rng.integers(0, 2, size=nbits).astype(np.uint8)
    pulse = oracle.freq_pulse_pcmfm(sps)
    _t, sig = oracle.cpm_modulate(oracle.pcmfm_mapper(bits), H, pulse, sps)
    if ebn0_db is not None:
        sig = sig + oracle.numpy_awgn(oracle.sigma_for_ebn0(ebn0_db, sps), sig.size, rng)
    return bits, sig, pulse


def errors(bits, received, pulse, N: int, offset: int, sps: int = SPS, nu: float = 0.0):
    """(bit errors, bits compared) of the host statement on ``received`` turned by ν cycles per sample."""
    if nu:
        received = received * np.exp(2j * np.pi * nu * np.arange(received.size))
    T = noncoherent_templates_host(pulse, H, sps, N, offset)
    _lam, hard = noncoherent_soft_host(received, T, sps, burst_start(pulse.size, sps, offset), bits.size)
    c = (N - 1) // 2
    return int(np.count_nonzero(hard[c:bits.size - c] != bits[c:bits.size - c])), int(bits.size - 2 * c)


def main() -> None:
    bits, received, pulse = burst()
    offsets = {str(o): list(errors(bits, received, pulse, 5, o)) for o in range(SPS + 1)}
    best = min(range(SPS + 1), key=lambda o: (offsets[str(o)][0], o))
    grid = {str(N): {repr(nu): errors(bits, received, pulse, N, best, nu=nu)[0] for nu in GRID} for N in OBSERVATIONS}
    limit = {N: max(nu for nu in GRID if grid[N][repr(nu)] <= 2 * grid[N][repr(0.0)]) for N in grid}
    out = {"seed": SEED, "nbits": NBITS, "sps": SPS, "ebn0_db": EBN0_DB, "h": H, "offsets": offsets, "default_offset": best, "grid": grid,
           "max_offset_cycles": limit}
    (Path(__file__).resolve().parent / "noncoherent_scan.json").write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
