"""Parallel concatenated (turbo) code over SOQPSK-TG on the GPU (``TurboSOQPSKLink``): information bits -> turbo encoder ->
differentially precoded SOQPSK-TG -> AWGN + PT / PAM bank -> soft detector -> one-launch turbo decoder, optionally with the
detector inside the loop.

The front end, the PN23 information bits, the noise keys, the Eb/N0-per-information-bit convention, ``PAD_BITS`` and the
uncoded count are the SOQPSK-TG base's (coded.py) and the loop is ``_ClippedLoop`` (sccc.py); the code is a :class:`waveforms_amd.encoding.turbo.TurboCode` and its decoder
``turbo_decode`` (include/wfhip.h, wf_turbo_decode).  Nothing leaves the GPU inside a block.

Over THIS waveform the serially concatenated scheme (``ConvSOQPSKLink``) is the stronger one: there the recursive precoder of
SOQPSK-TG is the inner code of the concatenation; here it only doubles the channel's errors in front of a code that was made
for a memoryless channel, and a single detector pass needs roughly 6 dB per information bit at rate 1/3.  Putting the detector
into the loop (``outer > 1``) wins some of that back.
"""
from __future__ import annotations

import math

from .. import _hip
from .. import device as dev
from .sccc import _ClippedLoop


class TurboSOQPSKLink(_ClippedLoop):
    """``_ClippedLoop`` (sccc.py) with a turbo ``code``: ``outer=1`` is the plain soft detector once, then ONE ``turbo_decode`` of
    2 ``iters`` half-iterations; ``outer>1`` is ``outer`` passes of soft detector <-> ``turbo_decode`` of 2 ``iters``
    half-iterations, constituent 1's prior carried from pass to pass (``a1``).

    ``ext_scale`` is the usual 0.75 of max-log turbo decoding.  With ``early_stop`` a codeword whose two constituents agree
    stops inside the launch.  ``counts`` holds THREE device counters (information bit errors, codeword errors, half-iterations
    run) and ``result()`` returns the 3-tuple of ``ConvSOQPSKLink``; ``half_iterations()`` gives the mean number of
    half-iterations per codeword and pass.  ``per_pass=True`` also accumulates the counts after every pass (``pass_results``)."""

    _ncounts = 3

    def __init__(self, code, ncw: int, sps: int = 8, detector: str = "PT", iters: int = 6, outer: int = 1, damping: float = 0.7,
                 ext_scale: float = 0.75, ext_clip: float | None = None, early_stop: bool = True, per_pass: bool = False, framing=None) -> None:
        if not 1 <= int(iters) <= 32:
            raise ValueError("iters must be 1 .. 32")
        if not (math.isfinite(ext_scale) and ext_scale > 0.0):
            raise ValueError("ext_scale must be finite and positive")
        self.iters, self.ext_scale, self.early_stop = int(iters), float(ext_scale), bool(early_stop)
        super().__init__(code, ncw, sps, detector, outer, damping, ext_clip, per_pass, framing)
        self.a1 = None

    def encode(self, info):
        return dev.turbo_encode(self.code, info)

    def begin(self, nrows: int) -> None:
        """Fresh loop state of one block: prior 0 on every row, constituent 1's prior 0."""
        fresh = self.prior is None or self.prior.numel() != nrows
        super().begin(nrows)
        if fresh:
            self.a1 = _hip.zeros((self.ncw, self.code.k), "float32")
        else:
            self.a1.zero_()

    def _decode_once(self, llr, info) -> None:
        out = dev.turbo_decode(self.code, llr, half_iters=2 * self.iters, scale=self.llr_scale, ext_scale=self.ext_scale,
                               early_stop=self.early_stop, ref_info=info, counts=self._last, want_post=False, want_iters=False)
        self.decided = out["info_bits"]

    def decode(self, ext, ref_info=None, counts=None) -> None:
        """One decoder pass of the loop: the decisions (``decided``), constituent 1's prior and the coded bits' next prior, in
        place; with ``ref_info`` the three counts are added to ``counts``."""
        out = dev.turbo_decode(self.code, ext, half_iters=2 * self.iters, scale=self.llr_scale, ext_scale=self.ext_scale,
                               early_stop=self.early_stop, a1=self.a1, ext=self._prior_coded(), ext_stride=self.code.n_tx,
                               ext_clip=self.ext_clip, ref_info=ref_info, counts=counts, want_post=False, want_iters=False)
        self.decided = out["info_bits"]

    def half_iterations(self) -> float:
        """Mean half-iterations per codeword in the LAST pass of a block, over the blocks run - synchronises."""
        _hip.check(_hip.lib().wf_ctx_check(_hip.ctx(), _hip.stream()))
        n = self.blocks * self.ncw
        return int(self.counts.cpu()[2]) / n if n else 0.0
