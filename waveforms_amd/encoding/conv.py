"""Convolutional codes: the code object, its host encoder, and the GPU encoder / max-log-MAP decoder behind it.

A code is terminated, feed-forward and of rate 1 / n_out (``wf_conv_code_create`` in include/wfhip.h states the code, the
trellis and the decoder's arithmetic).  The generators are K-bit masks whose MSB taps the current input bit, so octal 171 / 133
read in the usual way; every generator must have both end taps.  The message is followed by K - 1 zero tail bits: T = k + K - 1
steps, variable ``n_out i + j`` is output j of step i, n = n_out T variables.

* ``puncture``: an n_out x P pattern of 0 / 1 repeated over the steps (1 = sent): variable n_out i + j is sent when
  ``puncture[j][i % P]`` is 1.
* ``tx_order``: a permutation of the SURVIVING variables' ranks: transmitted position t carries the ``tx_order[t]``-th surviving
  variable (in increasing order).  Together they make ``tx_var``, the one table that is the interleaver and the puncturing
  map, exactly as ``LDPCCode.tx_order`` is.

No tables are needed: ``nasa_k3`` is the (7, 5) code, ``ccsds_k7`` the (171, 133) code of the telemetry standards.
"""
from __future__ import annotations

import numpy as np

from ._code import DeviceCode, transmit_table

MAX_N = 32768


def qpp_order(N: int, f1: int, f2: int) -> np.ndarray:
    """The quadratic permutation polynomial interleaver (f1 t + f2 t^2) mod N, t = 0 .. N - 1; raises ``ValueError`` unless
    it is a bijection."""
    N, f1, f2 = int(N), int(f1), int(f2)
    if N < 1:
        raise ValueError("N must be at least 1")
    t = np.arange(N, dtype=object)
    out = np.array([int(v) for v in (f1 * t + f2 * t * t) % N], dtype=np.int64)
    if np.unique(out).size != N:
        raise ValueError(f"({f1} t + {f2} t^2) mod {N} is not a bijection")
    return out


class ConvCode(DeviceCode):
    """A terminated feed-forward convolutional code of rate 1 / n_out with its puncturing and transmit order.

    Attributes: ``k`` information bits, ``K`` constraint length, ``n_out`` outputs per step, ``T`` = k + K - 1 steps, ``n`` =
    n_out T variables, ``n_tx`` transmitted bits, ``tx_var`` (n_tx variables), ``generators``, ``rate`` = k / n_tx."""

    def __init__(self, generators, k: int, K: int | None = None, puncture=None, tx_order=None) -> None:
        gens = [int(g) for g in generators]
        if K is None:
            K = max(gens).bit_length() if gens else 0
        self.K, self.k, self.n_out = int(K), int(k), len(gens)
        if not 3 <= self.K <= 7:
            raise ValueError(f"K = {self.K} outside 3 .. 7")
        if not 2 <= self.n_out <= 4:
            raise ValueError(f"{self.n_out} generators: n_out must be 2 .. 4")
        nu = self.K - 1
        for g in gens:
            if not (0 < g < (1 << self.K) and (g >> nu) & 1 and g & 1):
                raise ValueError(f"generator 0o{g:o} must be a {self.K}-bit mask with its first and last tap set")
        if self.k < 1:
            raise ValueError("k must be at least 1")
        self.generators = tuple(gens)
        self.T = self.k + nu
        self.n = self.n_out * self.T
        if self.n > MAX_N:
            raise ValueError(f"n = n_out (k + K - 1) = {self.n} exceeds {MAX_N}")
        sent = np.ones((self.T, self.n_out), dtype=bool)              # T x n_out, variable order
        if puncture is not None:
            pat = np.asarray(puncture)
            if pat.ndim != 2 or pat.shape[0] != self.n_out or pat.shape[1] < 1 or not np.isin(pat, (0, 1)).all():
                raise ValueError(f"puncture must be an n_out x P pattern of 0 / 1 (n_out = {self.n_out})")
            sent = pat[:, np.arange(self.T) % pat.shape[1]].T.astype(bool)
        self.tx_var = transmit_table(sent, tx_order)
        self.n_tx = int(self.tx_var.size)
        self.rate = self.k / self.n_tx

    # ------------------------------------------------------------------ presets
    @classmethod
    def nasa_k3(cls, k: int, **kw) -> "ConvCode":
        """The K = 3 (7, 5) code, rate 1/2, free distance 5."""
        return cls((0o7, 0o5), k, 3, **kw)

    @classmethod
    def ccsds_k7(cls, k: int, **kw) -> "ConvCode":
        """The K = 7 (171, 133) code, rate 1/2, free distance 10.  Output j of a step is the plain parity of generator j: there
        is NO inversion of the second output (the CCSDS transmitter inverts it for symbol synchronisation; a user who
        needs that flips the sign of those channel values)."""
        return cls((0o171, 0o133), k, 7, **kw)

    # ------------------------------------------------------------------ host forms
    def codeword_host(self, info: np.ndarray) -> np.ndarray:
        """Codewords by VARIABLE (ncw x n, uint8) from messages (ncw x k): the host statement of the encoder."""
        u = self._messages(info) & 1
        nu = self.K - 1
        pad = np.zeros((u.shape[0], self.T + nu), dtype=np.uint8)
        pad[:, nu:nu + self.k] = u                                    # pad[:, nu + i] = u_i, zeros in front and behind
        c = np.zeros((u.shape[0], self.T, self.n_out), dtype=np.uint8)
        for j, g in enumerate(self.generators):
            for d in range(self.K):                                   # bit nu - d of the mask taps u_{i-d}
                if (g >> (nu - d)) & 1:
                    c[:, :, j] ^= pad[:, nu - d:nu - d + self.T]
        return c.reshape(u.shape[0], self.n)

    def c_tables(self) -> dict:
        """The arguments of ``wf_conv_code_create``."""
        return dict(K=self.K, n_out=self.n_out, gen=np.array(self.generators, dtype=np.uint32), k=self.k, n_tx=self.n_tx,
                    tx_var=self.tx_var.astype(np.int32))

    # ------------------------------------------------------------------ device
    _free, _encode = "wf_conv_code_free", "conv_encode"

    def _create(self, lib, ctx, out) -> int:
        t = self.c_tables()
        return lib.wf_conv_code_create(ctx, t["K"], t["n_out"], t["gen"].ctypes.data, t["k"], t["n_tx"], t["tx_var"].ctypes.data, out)

    def siso(self, llr: np.ndarray, prior=None, scale: float = 1.0, ext_clip: float = float("inf")) -> dict:
        """λ (ncw x n_tx) and an optional information prior (ncw x k) -> {"info_bits", "info_post", "ext"} as host arrays,
        decoded on the GPU (``waveforms_amd.device.conv_siso``)."""
        from .. import _hip
        from .. import device as dev

        a = np.ascontiguousarray(np.atleast_2d(np.asarray(llr, dtype=np.float64)))
        if a.shape[1] != self.n_tx:
            raise ValueError(f"LLRs must have n_tx = {self.n_tx} columns")
        p = None
        if prior is not None:
            p = np.ascontiguousarray(np.atleast_2d(np.asarray(prior, dtype=np.float32)))
            if p.shape != (a.shape[0], self.k):
                raise ValueError(f"the prior must be ncw x k = {a.shape[0]} x {self.k}")
            p = _hip.to_device(p)
        out = dev.conv_siso(self, _hip.to_device(a), scale=scale, prior=p, ext_clip=ext_clip)
        return {key: _hip.to_host(out[key]) for key in ("info_bits", "info_post", "ext")}


def nasa_k3(k: int, **kw) -> ConvCode:
    """``ConvCode.nasa_k3``."""
    return ConvCode.nasa_k3(k, **kw)


def ccsds_k7(k: int, **kw) -> ConvCode:
    """``ConvCode.ccsds_k7`` (no output inversion)."""
    return ConvCode.ccsds_k7(k, **kw)
