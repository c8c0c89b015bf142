"""Framed coded links: an attached sync marker in front of every codeword, a pseudo-random sequence over the codeword's
bits, and the receiver's soft frame search (include/wfhip.h states the four device operations: ``wf_frame_build``,
``wf_frame_search``, ``wf_frame_gather``, ``wf_frame_scatter``).

Frame: ``marker_bits`` marker bits (MSB first) followed by the code's ``n_tx`` transmitted bits, bit t exclusive-ored with
``pn[t]``, t counted from the start of the codeword; the marker is not randomised.  ``DEFAULT_MARKER`` is the package's
default marker, a parameter everywhere.

``Framing`` holds the period, the device tables and the HOST statements of the four operations (``frame_host``,
``search_host``, ``gather_host``, ``scatter_host``), written straight from the definitions: they are what the tests compare
the GPU against, bit for bit.
"""
from __future__ import annotations

import numpy as np

DEFAULT_MARKER = 0x034776C7272895B0       # the package's default marker, 64 bits
SLICE_FRAMES = 32                         # frames per slice of the search's sum over frames (part of the definition)


def randomizer_bits(n: int) -> np.ndarray:
    """pn[0..7] = 1, pn[n+8] = pn[n] ^ pn[n+3] ^ pn[n+5] ^ pn[n+7]: period 255, the first 40 bits read as bytes (MSB first)
    are FF 48 0E C0 9A."""
    n = int(n)
    pn = np.ones(max(n, 8), dtype=np.uint8)
    for i in range(n - 8):
        pn[i + 8] = pn[i] ^ pn[i + 3] ^ pn[i + 5] ^ pn[i + 7]
    return pn[:n].copy()


class Framing:
    """Framing of ``code`` (anything with ``n_tx``): ``marker`` (the low ``marker_bits`` bits, sent MSB first), the
    randomiser restarted at every codeword (``randomize=False``: none).  ``period`` = marker_bits + n_tx."""

    def __init__(self, code, marker: int = DEFAULT_MARKER, marker_bits: int = 64, randomize: bool = True) -> None:
        if not 1 <= int(marker_bits) <= 64:
            raise ValueError(f"marker_bits = {marker_bits} outside 1 .. 64")
        self.code, self.n_tx, self.L = code, int(code.n_tx), int(marker_bits)
        self.marker = int(marker) & ((1 << self.L) - 1)
        self.period = self.L + self.n_tx
        self.marker_host = np.array([(self.marker >> (self.L - 1 - i)) & 1 for i in range(self.L)], dtype=np.uint8)
        self.pn_host = randomizer_bits(self.n_tx) if randomize else None
        self._d_pn = None

    @property
    def pn(self):
        """The randomiser as a device table (u8[n_tx]), or None."""
        if self.pn_host is not None and self._d_pn is None:
            from .. import _hip

            self._d_pn = _hip.to_device(self.pn_host)
        return self._d_pn

    # ---------------------------------------------------------------- host statements
    def _r(self) -> np.ndarray:
        return np.ones(self.n_tx) if self.pn_host is None else 1.0 - 2.0 * self.pn_host

    def frame_host(self, tx) -> np.ndarray:
        """Coded bits (ncw x n_tx) -> the ncw frames as one u8 stream."""
        tx = np.asarray(tx, dtype=np.uint8).reshape(-1, self.n_tx) & 1
        body = tx if self.pn_host is None else tx ^ self.pn_host
        return np.concatenate((np.broadcast_to(self.marker_host, (tx.shape[0], self.L)), body), axis=1).reshape(-1)

    def search_host(self, llr):
        """-> ((p̂, σ, best, other), folded float64[2, P]) by the definition: every sum from +0, C and A over i increasing,
        frames in slices of ``SLICE_FRAMES`` added in order, then the slice sums in order; the maximum with ties to + before
        -, then to the smallest p."""
        lam = np.ascontiguousarray(llr, dtype=np.float64).reshape(-1)
        L, P = self.L, self.period
        F = (lam.size - L) // P
        if F < 1:
            raise ValueError(f"{lam.size} values hold no whole frame of period {P} behind a marker of {L}")
        N = F * P
        s = 1.0 - 2.0 * self.marker_host                        # ±1: the product is a sign flip, exact
        C, A = np.zeros(N), np.zeros(N)
        for i in range(L):
            w = lam[i:i + N]
            C += s[i] * w
            A += np.abs(w)
        M = np.stack(((C - A).reshape(F, P), ((-C) - A).reshape(F, P)))      # [polarity, frame, p]
        G = np.zeros((2, P))
        for f0 in range(0, F, SLICE_FRAMES):
            S = np.zeros((2, P))
            for f in range(f0, min(f0 + SLICE_FRAMES, F)):
                S += M[:, f]
            G += S
        flat = G.reshape(-1)
        q = int(np.argmax(flat))                                # first maximum: + before -, then the smallest p
        other = float(np.max(np.delete(flat, q)))
        return (q % P, 1 if q < P else -1, float(flat[q]), other), G

    def gather_host(self, llr, p: int, sigma: int, ncw: int) -> np.ndarray:
        """out[b, t] = σ r_t λ[p + b P + L + t]; a position at or beyond the burst gives +0."""
        lam = np.ascontiguousarray(llr, dtype=np.float64).reshape(-1)
        pos = int(p) + np.arange(int(ncw))[:, None] * self.period + self.L + np.arange(self.n_tx)[None, :]
        ok = pos < lam.size
        vals = lam[np.where(ok, pos, 0)] * (float(sigma) * self._r())[None, :]
        return np.where(ok, vals, 0.0)

    def scatter_host(self, ext, p: int, sigma: int, prior, marker_prior: float = 0.0, ext_stride: int | None = None) -> np.ndarray:
        """A copy of ``prior`` (float32) with prior[p + b P + L + t] = σ r_t ext[b ext_stride + t] and, unless ``marker_prior``
        is 0, prior[p + b P + i] = σ s_i marker_prior; positions at or beyond the buffer are skipped."""
        out = np.array(prior, dtype=np.float32).reshape(-1)
        ext = np.ascontiguousarray(ext, dtype=np.float32).reshape(-1)
        stride = self.n_tx if ext_stride is None else int(ext_stride)
        ncw = (ext.size - self.n_tx) // stride + 1
        r = (float(sigma) * self._r()).astype(np.float32)
        sm = (float(sigma) * (1.0 - 2.0 * self.marker_host)).astype(np.float32) * np.float32(marker_prior)
        for b in range(ncw):
            at = int(p) + b * self.period
            if np.float32(marker_prior) != 0:
                n = max(0, min(self.L, out.size - at))
                out[at:at + n] = sm[:n]
            n = max(0, min(self.n_tx, out.size - (at + self.L)))
            out[at + self.L:at + self.L + n] = r[:n] * ext[b * stride:b * stride + n]
        return out

    # ---------------------------------------------------------------- device operations
    def build(self, tx):
        from .. import device as dev

        return dev.frame_build(tx, self.n_tx, self.marker, self.L, self.pn)

    def search(self, llr, lock=None, want_folded: bool = False):
        from .. import device as dev

        return dev.frame_search(llr, self.marker, self.L, self.period, lock, want_folded)

    def gather(self, llr, lock, ncw: int, out=None):
        from .. import device as dev

        return dev.frame_gather(llr, lock, self.L, self.n_tx, ncw, self.pn, out)

    def scatter(self, ext, lock, prior, marker_prior: float = 0.0, ext_stride: int | None = None):
        from .. import device as dev

        return dev.frame_scatter(ext, lock, self.marker, self.L, self.n_tx, prior, self.pn, marker_prior, ext_stride)
