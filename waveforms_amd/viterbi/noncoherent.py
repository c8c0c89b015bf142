"""The multi-symbol noncoherent soft detector for PCM/FM (Osborne and Luntz): the definition, stated on the host in numpy.

For each bit the detector correlates N symbols of samples against the noise-free signal of every N-bit hypothesis and compares
correlation MAGNITUDES: it needs no carrier phase, no recovery stage, and it tolerates frequency offsets hundreds of times what
the coherent trellis detectors take (``MAX_OFFSET_CYCLES``).  ``device.noncoherent_soft`` (``wf_noncoherent_soft_c128``,
include/wfhip.h) runs the same definition on the GPU; the sums there are re-associated, so the two agree to rounding, not bit
for bit.  The reference has no such detector: this is the build's own.

    T = noncoherent_templates_host(pulse, h, sps, N, offset)          complex128[2^N, N sps]
    λ, bits = noncoherent_soft_host(received, T, sps, start, nbits)   float64[nbits], uint8[nbits]

Conventions.  Hypothesis p holds window bit i at bit N - 1 - i (MSB first, as ``cpm_soft`` numbers a symbol's bits); the decided
bit is the window's middle one, c = (N - 1) / 2, which is also bit c of p.  λ > 0 favours bit 0 and ``bits = λ < 0``, the sign of
``cpm_soft``.  The magnitude is compared, not its square: the max-log form of ln I₀(2 |z| / N₀).  The window of bit j begins at
sample ``start + (j - c) sps``; for a burst from ``cpm_modulate``, whose symbol j is an impulse at sample (j + 1) sps in front of
a centred pulse, ``burst_start`` gives the ``start`` that puts the templates on the signal.

``DEFAULT_OFFSET`` is a hand-placed instant like the coherent chains' ``TIMING_OFFSET``: the fewest bit errors of a committed
host scan (tests/golden/make_noncoherent_scan.py -> tests/golden/noncoherent_scan.json).  Timing recovery for this detector does
not exist.  ``MAX_OFFSET_CYCLES[N]`` is the documented frequency tolerance: the largest ν of the scan's grid, in cycles per
sample, at which the host statement makes at most twice the bit errors it makes at ν = 0 (about 0.3 dB on this curve) - a
definition, read off the same scan.
"""
from __future__ import annotations

import math

import numpy as np

__all__ = ["DEFAULT_OFFSET", "MAX_OFFSET_CYCLES", "OBSERVATIONS", "burst_start", "check_window", "noncoherent_templates_host", "noncoherent_soft_host"]

OBSERVATIONS = (3, 5, 7)                       # N: odd, the table has 2^N rows
DEFAULT_OFFSET = 4                             # tests/golden/noncoherent_scan.json: "default_offset"
MAX_OFFSET_CYCLES = {3: 4e-3, 5: 2e-3, 7: 1e-3}   # ... "max_offset_cycles"


def _check_observe(N: int) -> int:
    if int(N) != N or int(N) not in OBSERVATIONS:
        raise ValueError(f"N = {N} must be odd and 3 .. 7")
    return int(N)


def check_window(N: int, sps: int, offset: int) -> tuple[int, int, int]:
    """(N, sps, offset) as ints: N odd and 3 .. 7, sps at least 1, 0 <= offset <= sps, else ValueError."""
    N = _check_observe(N)
    if int(sps) != sps or int(sps) < 1:
        raise ValueError(f"sps = {sps} must be a whole number of at least 1")
    if int(offset) != offset or not 0 <= int(offset) <= int(sps):
        raise ValueError(f"offset = {offset} outside 0 .. sps = {sps}")
    return N, int(sps), int(offset)


def burst_start(ntaps: int, sps: int, offset: int) -> int:
    """``start`` for the samples of ``cpm_modulate(symbols, h, pulse, sps)`` with a pulse of ``ntaps`` taps: bit j's pulse begins
    at sample (j + 1) sps - (ntaps - 1) // 2, and window bit c's template begins ``offset`` samples behind its own pulse's
    first tap.  Negative for the PCM/FM pulse (-3 + offset at sps 8): the first windows read zeros in front of the burst."""
    return int(sps) - (int(ntaps) - 1) // 2 + int(offset)


def noncoherent_templates_host(pulse, h: float, sps: int, N: int, offset: int) -> np.ndarray:
    """complex128[2^N, N sps]: row p = samples offset .. offset + N sps - 1 of the modulator's noise-free output for the N bits of
    p alone (mapped ±1, every symbol outside the window contributing nothing), without the initial phase:
    exp(j 2π h Σ_i a_i q[k + offset - i sps]), q the running sum of ``pulse`` / sps (0 in front of the pulse, its final value
    behind it).  N odd and 3 .. 7, 0 <= offset <= sps; anything else is a ValueError."""
    N, sps, offset = check_window(N, sps, offset)
    pulse = np.asarray(pulse, dtype=np.float64).reshape(-1)
    if pulse.size < 1 or not math.isfinite(float(h)):
        raise ValueError("the pulse must not be empty and h must be finite")
    q = np.cumsum(pulse) / sps
    idx = np.arange(N * sps)[None, :] + offset - (np.arange(N) * sps)[:, None]           # [N, N sps]
    qv = np.where(idx < 0, 0.0, q[np.clip(idx, 0, q.size - 1)])
    p = np.arange(1 << N)
    a = 2.0 * ((p[:, None] >> (N - 1 - np.arange(N))[None, :]) & 1) - 1.0                       # [2^N, N]
    return np.exp(2j * np.pi * float(h) * (a @ qv))


def _table(templates, sps: int) -> tuple[np.ndarray, int]:
    """(the table as complex128[2^N, N sps], N) or ValueError."""
    T = np.asarray(templates, dtype=np.complex128)
    if T.ndim != 2 or int(sps) < 1 or T.shape[1] % int(sps):
        raise ValueError("templates must be complex128[2^N, N sps]")
    N = _check_observe(T.shape[1] // int(sps))
    if T.shape[0] != 1 << N:
        raise ValueError(f"{T.shape[0]} template rows for N = {N}: the table has 2^N")
    return T, N


def noncoherent_soft_host(received, templates, sps: int, start: int, nbits: int, chunk: int = 2048):
    """(λ float64[nbits], bits uint8[nbits]).  Bit j's window begins at sample start + (j - c) sps, c = (N - 1) / 2, and samples
    outside [0, n) read as zero;  z_p = Σ_k r[· + k] conj(T[p, k]), k increasing;
    λ_j = max_{p: bit c of p is 0} |z_p| - max_{p: bit c of p is 1} |z_p|;  bits = λ < 0.  An all-zero window gives λ = +0 and
    bit 0.  ``chunk``: bits per pass of the sums (memory only)."""
    T, N = _table(templates, sps)
    sps, start, nbits = int(sps), int(start), int(nbits)
    if nbits < 1:
        raise ValueError("nbits must be at least 1")
    r = np.asarray(received, dtype=np.complex128).reshape(-1)
    c, K = (N - 1) // 2, N * sps
    ones = ((np.arange(1 << N) >> c) & 1).astype(bool)
    Tc = np.conj(T)
    lam = np.empty(nbits, dtype=np.float64)
    for j0 in range(0, nbits, int(chunk)):
        m = min(int(chunk), nbits - j0)
        first = start + (j0 - c) * sps
        idx = first + np.arange((m - 1) * sps + K)
        ok = (idx >= 0) & (idx < r.size)
        seg = np.where(ok, r[np.clip(idx, 0, max(r.size - 1, 0))] if r.size else 0.0, 0.0)
        win = np.lib.stride_tricks.sliding_window_view(seg, K)[::sps]                          # [m, K]
        z = np.zeros((m, 1 << N), dtype=np.complex128)
        for k in range(K):
            z += win[:, k, None] * Tc[None, :, k]
        mag = np.abs(z)
        lam[j0:j0 + m] = mag[:, ~ones].max(axis=1) - mag[:, ones].max(axis=1)
    return lam, (lam < 0).astype(np.uint8)
