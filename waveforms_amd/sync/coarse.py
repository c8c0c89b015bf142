"""Coarse carrier frequency acquisition for the SOQPSK-TG receiver: feed-forward, one pass over the noisy samples, no
sequential loop (include/wfhip.h states the device operations: ``wf_coarse_lines_c128``, ``wf_coarse_estimate``,
``wf_carrier_offset_dev_c128``).  The reference has no synchroniser; every definition here is this package's own.

Why.  ``CarrierRecovery`` and ``JointAcquisition`` follow a carrier that is already within |nu| sps W <= ``MAX_DRIFT_TURNS`` of
the right frequency: 2.4e-5 cycles per sample at sps 8, 2e-4 of the bit rate.  This stage brings a burst that is a few per cent
of the bit rate off into that range; the fine recoveries then run as they are.

How it works.  SOQPSK-TG is a CPM with h = 1/2, so the SQUARE of the received signal carries two discrete spectral lines, at
2 nu ± (1 + eps) / (2 sps) cycles per sample (eps: the clock drift of ``timing=(tau0, eps)``).  Each line is shifted to 2 nu by
exp(∓jπ k / sps), integrated and dumped to one sample per bit, and its periodogram (``nfft`` bits per segment, the burst's
segments added up) has a peak at bin nfft/2 + 2 nu sps nfft.  A boxcar of ``smooth`` samples in front of the squarer keeps the
noise x noise term down.  The joint peak is found on the SUM of the two periodograms (robust), then each line's own peak
within ``search`` bins of it: a clock drift moves the two lines apart by eps nfft bins, which biases the vertex of the sum and
not the mean of the two vertices.  Their difference is eps, for nothing.

The ``*_host`` functions are the HOST statements of the definitions, written straight from them in numpy: the device's
spectra equal them to the rounding of an fp64 FFT, the estimate to the rounding of three logarithms, the correction is bitwise
``carrier_offset`` with the same value passed from the host.  ``CoarseFrequency`` is the device-resident composition.

Limits.  |nu| sps <= ``MAX_OFFSET_BITS``; at least ``MIN_BITS`` bits (tools/coarse_study.py has the measurements behind both);
one frequency per burst (a change across the burst beyond what the fine tracker follows is out of scope); segments do not
overlap and the tail beyond the last whole segment is not read.  The third and fourth outputs (the peak of the summed
periodogram and its mean) are a lock indicator for the caller: nothing here thresholds them.  eps is reported and not yet fed
to the timing trackers.  PCM/FM and ARTM have no usable lines of this kind (their 10th to 32nd power lines drown in the noise
at any useful Eb/N0): this class is for SOQPSK-TG only.
"""
from __future__ import annotations

import math

import numpy as np

from . import _stages

DEFAULT_NFFT = 4096
DEFAULT_SEARCH = 4
MAX_OFFSET_BITS = 0.2                     # |nu| sps: the band ends at 0.25 (the dumped line aliases at half the bit rate, and the other
                                          # line's image, 1 bit rate away, is only sinc-attenuated: equal at 0.25); the host statement with
                                          # the prefilter stays within 4.6e-6 cycles per sample up to 0.24 from two segments and channel
                                          # Eb/N0 -1 dB on (tools/coarse_study.py; profiles/coarse_frequency.json), without it it does not
MIN_BITS = 2 * DEFAULT_NFFT               # two segments of the default nfft: ONE segment has outliers at -1 dB (2 of 8 bursts at |nu| sps
                                          # 0.22) and none from 1 dB on; two segments had none anywhere in the study


def check_nfft(nfft) -> int:
    nfft = int(nfft)
    if not (64 <= nfft <= 4096 and nfft & (nfft - 1) == 0):
        raise ValueError(f"nfft = {nfft} must be a power of two from 64 to 4096")
    return nfft


def check_search(search, nfft: int) -> int:
    if not 1 <= int(search) < nfft // 2 - 1:
        raise ValueError(f"search = {search} outside 1 .. nfft / 2 - 2 = {nfft // 2 - 2}")
    return int(search)


def check_smooth(smooth, sps: int) -> int:
    smooth = sps // 2 if smooth is None else int(smooth)
    if not 1 <= smooth <= 1024:
        raise ValueError(f"smooth = {smooth} outside 1 .. 1024")
    return smooth


def line_rotations_host(sps: int) -> np.ndarray:
    """The table of the 2 sps rotations exp(jπ q / sps), q < 2 sps (σ = +1; σ = -1 takes the conjugate): the quotient, then
    cos and sin of π times it."""
    a = math.pi * (np.arange(2 * int(sps), dtype=np.float64) / float(sps))
    return np.cos(a) + 1j * np.sin(a)


def line_samples_host(received, sps: int, smooth: int) -> np.ndarray:
    """Step 1 of include/wfhip.h -> complex128[2, nb], row 0 the line σ = -1 (the upper line brought down to 2 nu), row 1 σ = +1:
    y_k = Σ_{j < S} r_{k+j} (j increasing), z_k = y_k², u_σ[m] = Σ_{i < sps} z_{m sps + i} exp(jσπ ((m sps + i) mod 2 sps) / sps)
    (i increasing), m < nb = (n - S + 1) // sps."""
    r = np.asarray(received, dtype=np.complex128).reshape(-1)
    sps, S = int(sps), int(smooth)
    nb = (r.size - S + 1) // sps if r.size >= S else 0
    if nb < 1:
        return np.zeros((2, 0), dtype=np.complex128)
    nz = nb * sps
    y = np.zeros(nz, dtype=np.complex128)
    for j in range(S):
        y = y + r[j:j + nz]
    z = (y * y).reshape(nb, sps)
    rot = line_rotations_host(sps)[(np.arange(nz, dtype=np.int64) % (2 * sps))].reshape(nb, sps)
    u = np.zeros((2, nb), dtype=np.complex128)
    for i in range(sps):
        u[0] = u[0] + z[:, i] * np.conj(rot[:, i])
        u[1] = u[1] + z[:, i] * rot[:, i]
    return u


def line_spectra_host(lines, nfft: int, window=None) -> np.ndarray:
    """Step 2 -> float64[2, nfft] in fftshift order: P_σ[b] = Σ_{s < nseg} |FFT(w ⊙ u_σ[s L : (s + 1) L])[b]|², nseg = nb // L (the
    tail is dropped; no whole segment: ValueError).  ``window``: L doubles (None: np.hanning(L))."""
    u = np.asarray(lines, dtype=np.complex128)
    L = check_nfft(nfft)
    w = np.hanning(L) if window is None else np.asarray(window, dtype=np.float64).reshape(-1)
    if w.size != L:
        raise ValueError(f"window must hold nfft = {L} values")
    nseg = u.shape[1] // L
    if nseg < 1:
        raise ValueError(f"{u.shape[1]} bits do not fill one segment of nfft = {L}")
    P = np.zeros((2, L))
    for s in range(nseg):
        X = np.fft.fft(u[:, s * L:(s + 1) * L] * w, axis=1)
        P = P + (X.real * X.real + X.imag * X.imag)
    return np.fft.fftshift(P, axes=1)


def _first_max(v, lo: int, hi: int) -> int:
    """The first of the largest v[lo .. hi]; a NaN never wins."""
    seg = np.asarray(v[lo:hi + 1], dtype=np.float64)
    return lo + int(np.argmax(np.where(np.isnan(seg), -np.inf, seg)))


def vertex_host(p, i: int) -> float:
    """d = ½ (a - c) / ((a - b) + (c - b)) on a, b, c = ln p[i - 1], ln p[i], ln p[i + 1]; 0 where the denominator is not negative
    and finite, or where any of the three bins is <= 0 or not finite."""
    three = np.asarray(p[i - 1:i + 2], dtype=np.float64)
    if not (np.isfinite(three).all() and (three > 0.0).all()):
        return 0.0
    a, b, c = (float(v) for v in np.log(three))
    den = (a - b) + (c - b)
    if not (math.isfinite(den) and den < 0.0):
        return 0.0
    return (0.5 * (a - c)) / den


def coarse_peaks_host(spectra, search: int = DEFAULT_SEARCH):
    """(i*, i₋, i₊) of step 3: the first maximum of T = P₋ + P₊ over the bins R + 1 .. L - R - 2, then per line the first maximum
    over i* - R .. i* + R."""
    P = np.asarray(spectra, dtype=np.float64)
    L = check_nfft(P.shape[1])
    R = check_search(search, L)
    T = P[0] + P[1]
    star = _first_max(T, R + 1, L - R - 2)
    return star, _first_max(P[0], star - R, star + R), _first_max(P[1], star - R, star + R)


def coarse_estimate_host(spectra, sps: int, search: int = DEFAULT_SEARCH) -> np.ndarray:
    """``wf_coarse_estimate``: float64[2, L] -> float64[4] = (nu in cycles per sample, eps, T[i*], the mean of T)."""
    P = np.asarray(spectra, dtype=np.float64)
    L = P.shape[1]
    star, im, ip = coarse_peaks_host(P, search)
    fm, fp = float(im) + vertex_host(P[0], im), float(ip) + vertex_host(P[1], ip)
    T = P[0] + P[1]
    nu = (0.5 * (fm + fp) - 0.5 * float(L)) / (2.0 * float(L) * float(sps))
    return np.array([nu, (fm - fp) / float(L), T[star], float(np.sum(T)) / float(L)])


def summed_vertex_host(spectra, sps: int, search: int = DEFAULT_SEARCH) -> float:
    """nu from the vertex of the SUMMED periodogram alone: what the per-line step replaces (biased under a clock drift)."""
    P = np.asarray(spectra, dtype=np.float64)
    L = P.shape[1]
    T = P[0] + P[1]
    star = coarse_peaks_host(P, search)[0]
    return ((float(star) + vertex_host(T, star)) - 0.5 * float(L)) / (2.0 * float(L) * float(sps))


def estimate_host(received, sps: int, nfft: int = DEFAULT_NFFT, smooth=None, search: int = DEFAULT_SEARCH) -> np.ndarray:
    """``CoarseFrequency.estimate`` on the host: steps 1 to 3 with the Hann window."""
    return coarse_estimate_host(line_spectra_host(line_samples_host(received, sps, check_smooth(smooth, sps)), nfft), sps, search)


def correct_host(received, sps: int, nfft: int = DEFAULT_NFFT, smooth=None, search: int = DEFAULT_SEARCH, first_index: int = 0):
    """``CoarseFrequency.correct`` on the host -> (samples complex128[n] with the estimate taken off, found float64[4])."""
    from .carrier import carrier_offset_host

    found = estimate_host(received, sps, nfft, smooth, search)
    return carrier_offset_host(received, 0.0, -1.0 * float(found[0]), first_index), found


class CoarseFrequency(_stages.Synchroniser):
    """Coarse carrier frequency acquisition of a burst of noisy SOQPSK-TG samples, everything on the device:

    1. ``coarse_lines``: one pass over the samples -> the two line periodograms float64[2, nfft],
    2. ``coarse_estimate``: one workgroup -> float64[4] = (nu in cycles per sample, eps, the peak of the summed periodogram, its
       mean),
    3. ``carrier_offset_dev`` (``correct`` only): the samples turned back by nu, read from device memory.

    ``smooth=None`` is sps // 2.  Nothing comes back to the host.  ``times=True`` keeps device events around every stage of the last
    call (``stage_times``).  Documented for |nu| sps <= ``MAX_OFFSET_BITS`` and bursts of at least ``MIN_BITS`` bits at the default
    ``nfft``; a smaller ``nfft`` has wider bins and less processing gain per segment: it is for bursts that are short AND clean
    (tests/test_coarse_link.py runs noiseless bursts of four segments of 1024 bits) and is not covered by the study."""

    def __init__(self, sps: int, nfft: int = DEFAULT_NFFT, smooth=None, search: int = DEFAULT_SEARCH) -> None:
        super().__init__()
        self.sps = _stages.check_range("sps", sps, 2, 64)
        self.nfft = check_nfft(nfft)
        self.smooth = check_smooth(smooth, self.sps)
        self.search = check_search(search, self.nfft)
        self._window = None

    def _hann(self):
        from .. import _hip

        if self._window is None or self._window.device.index != _hip.torch().cuda.current_device():
            self._window = _hip.to_device(np.hanning(self.nfft))
        return self._window

    def spectra(self, received, ctx=None):
        """The two line periodograms of ``received`` (contiguous device float64[n, 2]) -> device float64[2, nfft]."""
        from .. import device as dev

        return dev.coarse_lines(received, self.sps, self.smooth, self.nfft, self._hann(), ctx=ctx)

    def estimate(self, received, ctx=None):
        from .. import device as dev

        self._events = []
        self._mark("start")
        return self._estimate(received, dev, ctx)

    def _estimate(self, received, dev, ctx):
        P = self.spectra(received, ctx)
        self._mark("lines")
        found = dev.coarse_estimate(P, self.sps, self.search, ctx=ctx)
        self._mark("estimate")
        return found

    def correct(self, received, out=None, ctx=None):
        """-> (the samples with the estimate taken off, found); ``out=received`` works in place."""
        from .. import device as dev

        self._events = []
        self._mark("start")
        found = self._estimate(received, dev, ctx)
        out = dev.carrier_offset_dev(received, found, -1.0, 0, out=out, ctx=ctx)
        self._mark("correct")
        return out, found
