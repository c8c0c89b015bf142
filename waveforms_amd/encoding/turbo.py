"""Turbo codes: two terminated recursive systematic convolutional (RSC) constituents joined by an interleaver, the host encoder,
and the GPU encoder / one-launch max-log-MAP turbo decoder behind it.

``wf_turbo_code_create`` in include/wfhip.h states the constituent, the code and the decoder's arithmetic.  The feedback mask
and the parity generators are K-bit masks whose MSB taps the current register input, so octal 13 / 15 read in the usual way;
every mask must have both end taps and no parity generator may equal the feedback mask.  Each constituent runs T = k + K - 1
steps (its own K - 1 tail bits empty its register) with m = 1 + n_par outputs per step, output 0 the systematic one.  Variable
``2 m i + j`` is output j of constituent 1 at step i, ``2 m i + m + j`` output j of constituent 2, n = 2 m T variables.

* The default transmission drops constituent 2's systematic output at the message steps i < k (the receiver has it already,
  interleaved) and sends everything else in increasing variable order: n_tx = (2 m - 1) k + 2 m (K - 1).
* ``puncture``: a 2 m x P pattern of 0 / 1 repeated over the steps (1 = sent), applied ON TOP of the default: variable
  ``2 m i + r`` is sent when the default sends it and ``puncture[r][i % P]`` is 1.
* ``tx_order``: a permutation of the SURVIVING variables' ranks, exactly as in ``ConvCode``.  Together they make ``tx_var``.

No table of standard interleaver parameters is shipped: ``TurboCode.qpp(k, f1, f2)`` builds the K = 4 (13, 15) constituents
around ``qpp_order(k, f1, f2)`` and the CALLER supplies (f1, f2) for the block length at hand (any pair that makes the
polynomial a bijection is accepted; how good the code is depends on the pair).
"""
from __future__ import annotations

import numpy as np

from ._code import DeviceCode, transmit_table
from .conv import MAX_N, qpp_order


def _parity(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, dtype=np.uint32).copy()
    for sh in (16, 8, 4, 2, 1):
        x ^= x >> sh
    return (x & 1).astype(np.uint8)


class TurboCode(DeviceCode):
    """A parallel concatenation of two identical terminated RSC codes with its interleaver, puncturing and transmit order.

    Attributes: ``k`` information bits, ``K`` constraint length, ``n_par`` parity outputs per constituent, ``T`` = k + K - 1
    steps, ``n`` = 2 (1 + n_par) T variables, ``n_tx`` transmitted bits, ``tx_var`` (n_tx variables), ``rate`` = k / n_tx,
    ``interleaver`` (constituent 2 encodes u[interleaver]), ``feedback`` and ``parity`` (the masks)."""

    def __init__(self, k: int, interleaver, feedback: int = 0o13, parity=(0o15,), K: int | None = None, puncture=None, tx_order=None) -> None:
        fb, gens = int(feedback), [int(g) for g in parity]
        if K is None:
            K = max([fb] + gens).bit_length()
        self.K, self.k, self.n_par = int(K), int(k), len(gens)
        if not 3 <= self.K <= 5:
            raise ValueError(f"K = {self.K} outside 3 .. 5")
        if not 1 <= self.n_par <= 3:
            raise ValueError(f"{self.n_par} parity generators: n_par must be 1 .. 3")
        nu = self.K - 1
        for g in [fb] + gens:
            if not (0 < g < (1 << self.K) and (g >> nu) & 1 and g & 1):
                raise ValueError(f"mask 0o{g:o} must be a {self.K}-bit mask with its first and last tap set")
        if fb in gens:
            raise ValueError(f"a parity generator equal to the feedback mask 0o{fb:o} repeats the systematic output")
        if self.k < 1:
            raise ValueError("k must be at least 1")
        self.feedback, self.parity = fb, tuple(gens)
        m = 1 + self.n_par
        self.T = self.k + nu
        self.n = 2 * m * self.T
        if self.n > MAX_N:
            raise ValueError(f"n = 2 (1 + n_par) (k + K - 1) = {self.n} exceeds {MAX_N}")
        perm = np.asarray(interleaver, dtype=np.int64).ravel()
        if perm.size != self.k or not np.array_equal(np.sort(perm), np.arange(self.k)):
            raise ValueError(f"the interleaver must be a permutation of 0 .. k - 1 = {self.k - 1}")
        self.interleaver = np.ascontiguousarray(perm)
        sent = np.ones((self.T, 2 * m), dtype=bool)
        sent[:self.k, m] = False                                      # constituent 2's systematic output at the message steps
        if puncture is not None:
            pat = np.asarray(puncture)
            if pat.ndim != 2 or pat.shape[0] != 2 * m or pat.shape[1] < 1 or not np.isin(pat, (0, 1)).all():
                raise ValueError(f"puncture must be a 2 m x P pattern of 0 / 1 (2 m = {2 * m})")
            sent &= pat[:, np.arange(self.T) % pat.shape[1]].T.astype(bool)
        self.tx_var = transmit_table(sent, tx_order)
        self.n_tx = int(self.tx_var.size)
        self.rate = self.k / self.n_tx

    # ------------------------------------------------------------------ presets
    @classmethod
    def qpp(cls, k: int, f1: int, f2: int, **kw) -> "TurboCode":
        """The K = 4 constituents with feedback 13 and parity 15 (octal) around the QPP interleaver (f1 t + f2 t^2) mod k.  The
        caller supplies (f1, f2) for this k: no table of standard values is shipped."""
        return cls(k, qpp_order(k, f1, f2), 0o13, (0o15,), 4, **kw)

    # ------------------------------------------------------------------ host forms
    def _constituent_host(self, u: np.ndarray) -> np.ndarray:
        """One terminated RSC constituent: messages (ncw x k) -> outputs (ncw x T x m), output 0 the bit sent as systematic
        (u_i, then the tail bits)."""
        nu, m = self.K - 1, 1 + self.n_par
        S = 1 << nu
        fbl = self.feedback & (S - 1)
        masks = (self.feedback,) + self.parity
        s = np.zeros(u.shape[0], dtype=np.uint32)
        out = np.zeros((u.shape[0], self.T, m), dtype=np.uint8)
        for i in range(self.T):
            f = _parity(s & fbl)
            a = (u[:, i] ^ f) if i < self.k else np.zeros_like(f)
            reg = (a.astype(np.uint32) << nu) | s
            for j, g in enumerate(masks):
                out[:, i, j] = _parity(reg & g)
            s = reg >> 1
        assert not s.any()
        return out

    def codeword_host(self, info: np.ndarray) -> np.ndarray:
        """Codewords by VARIABLE (ncw x n, uint8) from messages (ncw x k): the host statement of the encoder."""
        u = self._messages(info) & 1
        c = np.concatenate([self._constituent_host(u), self._constituent_host(u[:, self.interleaver])], axis=2)
        return c.reshape(u.shape[0], self.n)

    def c_tables(self) -> dict:
        """The arguments of ``wf_turbo_code_create``."""
        return dict(K=self.K, n_par=self.n_par, fb=self.feedback, gen=np.array(self.parity, dtype=np.uint32), k=self.k,
                    perm=self.interleaver.astype(np.int32), n_tx=self.n_tx, tx_var=self.tx_var.astype(np.int32))

    # ------------------------------------------------------------------ device
    _free, _encode = "wf_turbo_code_free", "turbo_encode"

    def _create(self, lib, ctx, out) -> int:
        t = self.c_tables()
        return lib.wf_turbo_code_create(ctx, t["K"], t["n_par"], t["fb"], t["gen"].ctypes.data, t["k"], t["perm"].ctypes.data, t["n_tx"],
                                        t["tx_var"].ctypes.data, out)

    def decode(self, llr: np.ndarray, half_iters: int = 12, scale: float = 1.0, ext_scale: float = 0.75, early_stop: bool = True, a1=None,
               want_ext: bool = False, ext_clip: float = float("inf")) -> dict:
        """λ (ncw x n_tx) -> {"info_bits", "info_post", "iters", "a1", "ext"} as host arrays, decoded on the GPU in one launch
        (``waveforms_amd.device.turbo_decode``).  ``a1``: the prior of constituent 1 carried over from an earlier call."""
        from .. import _hip
        from .. import device as dev

        a = np.ascontiguousarray(np.atleast_2d(np.asarray(llr, dtype=np.float64)))
        if a.shape[1] != self.n_tx:
            raise ValueError(f"LLRs must have n_tx = {self.n_tx} columns")
        p = None
        if a1 is not None:
            p = np.ascontiguousarray(np.atleast_2d(np.asarray(a1, dtype=np.float32)))
            if p.shape != (a.shape[0], self.k):
                raise ValueError(f"a1 must be ncw x k = {a.shape[0]} x {self.k}")
            p = _hip.to_device(p)
        out = dev.turbo_decode(self, _hip.to_device(a), half_iters=half_iters, scale=scale, ext_scale=ext_scale, early_stop=early_stop, a1=p,
                               want_a1=True, want_ext=want_ext, ext_clip=ext_clip)
        return {key: None if out[key] is None else _hip.to_host(out[key]) for key in ("info_bits", "info_post", "iters", "a1", "ext")}
