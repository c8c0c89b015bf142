"""Parallel concatenated (turbo) code over SOQPSK-TG on the GPU (``TurboSOQPSKLink``): information bits -> turbo encoder ->
differentially precoded SOQPSK-TG -> AWGN + PT / PAM bank -> soft detector -> one-launch turbo decoder, optionally with the
detector inside the loop.

The front end, the PN23 information bits, the noise keys, the Eb/N0-per-information-bit convention, ``PAD_BITS`` and the
uncoded count are ``CodedSOQPSKLink``'s; the code is a :class:`waveforms_amd.encoding.turbo.TurboCode` and its decoder
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
from .coded import CodedSOQPSKLink


class TurboSOQPSKLink(CodedSOQPSKLink):
    """One block = ``ncw`` codewords of the turbo ``code`` sent back to back as ONE SOQPSK-TG burst (plus ``PAD_BITS`` zero
    bits).  Eb/N0 is per INFORMATION bit (the tail bits and the puncturing are in ``code.rate`` = k / n_tx).

    ``outer=1``: the plain soft detector (``viterbi_soft``) once, then ONE ``turbo_decode`` of 2 ``iters`` half-iterations.
    ``outer>1``: the front end runs once per block, then ``outer`` passes of

        soft detector with the burst's prior buffer (``viterbi_soft_apriori``, apriori_scale = ``damping``)
        -> ``turbo_decode`` of 2 ``iters`` half-iterations, constituent 1's prior carried from pass to pass (``a1``), writing
           the next prior of the coded bits at offset +1, stride n_tx, clipped to ±``ext_clip``

    Row 0 and the tail rows keep prior 0.  ``ext_clip`` is in the detector's metric units, which grow linearly with ``sps``:
    default 6.25 sps (50 at sps 8), as for the other loops.  Max-log-MAP on both sides is scale-invariant, so no noise-variance
    scale is needed (``llr_scale`` stays 1); ``ext_scale`` is the usual 0.75 of max-log turbo decoding.  With ``early_stop`` a
    codeword whose two constituents agree stops inside the launch.  ``outer`` is fixed and nothing synchronises with the host
    inside a block.  ``per_pass=True`` also accumulates the counts after every pass (``pass_results``).  Framing is not
    supported.

    What differs from the parent class: ``alpha`` and ``max_iter`` are inherited attributes that mean nothing here, ``counts``
    holds THREE device counters (information bit errors, codeword errors, half-iterations run), and ``result()`` returns the
    3-tuple of ``ConvSOQPSKLink``; ``half_iterations()`` gives the mean number of half-iterations per codeword and pass."""

    def __init__(self, code, ncw: int, sps: int = 8, detector: str = "PT", iters: int = 6, outer: int = 1, damping: float = 0.7,
                 ext_scale: float = 0.75, ext_clip: float | None = None, early_stop: bool = True, per_pass: bool = False, framing=None) -> None:
        if framing is not None:
            raise ValueError("TurboSOQPSKLink does not support framing")
        if outer < 1:
            raise ValueError("outer must be at least 1")
        if not 1 <= int(iters) <= 32:
            raise ValueError("iters must be 1 .. 32")
        if not (math.isfinite(damping) and damping > 0.0):
            raise ValueError("damping must be finite and positive")
        if not (math.isfinite(ext_scale) and ext_scale > 0.0):
            raise ValueError("ext_scale must be finite and positive")
        self.outer, self.iters, self.damping, self.ext_scale = int(outer), int(iters), float(damping), float(ext_scale)
        self.ext_clip = 6.25 * int(sps) if ext_clip is None else float(ext_clip)
        if not self.ext_clip > 0.0:
            raise ValueError("ext_clip must be positive")
        super().__init__(code, ncw, sps, detector)
        self.early_stop, self.per_pass = bool(early_stop), bool(per_pass)
        self.counts = _hip.zeros(3, "int64")
        self.pass_counts = _hip.zeros((self.outer, 3), "int64")
        self._last = _hip.zeros(3, "int64")
        self.prior = self.a1 = self.decided = None

    # ---------------------------------------------------------------- stages
    def channel_llrs(self, ebn0_db: float | None, seed: int = 1, stream_id: int = 0):
        """(λ ncw x n_tx of the plain detector, information bits ncw x k) of one block, on the device."""
        info = self.info_bits(stream_id)
        rows, _ = self.front_end(dev.turbo_encode(self.code, info), ebn0_db, seed, stream_id)
        llr, _ = self.soft(rows)
        return llr.contiguous(), info.view(self.ncw, self.code.k)

    def begin(self, nrows: int) -> None:
        """Fresh loop state of one block: prior 0 on every row, constituent 1's prior 0."""
        if self.prior is None or self.prior.numel() != nrows:
            self.prior = _hip.zeros(nrows, "float32")
            self.a1 = _hip.zeros((self.ncw, self.code.k), "float32")
        else:
            self.prior.zero_()
            self.a1.zero_()

    def detect(self, rows, first: bool = False):
        """One detector pass -> (extrinsic λ of the coded bits, ncw x n_tx view; hard decisions of λ + π).  The first pass of
        a block has prior 0 everywhere and takes the plain detector (bitwise the same result)."""
        ext, bits = dev.viterbi_soft_apriori(rows, None if first else self.prior, self.damping)
        return ext[1:1 + self.nbits].view(self.ncw, self.code.n_tx), bits[1:1 + self.nbits]

    def decode(self, ext, ref_info=None, counts=None) -> None:
        """One decoder pass of the loop: the decisions (``decided``), constituent 1's prior and the coded bits' next prior, in
        place; with ``ref_info`` the three counts are added to ``counts``."""
        out = dev.turbo_decode(self.code, ext, half_iters=2 * self.iters, scale=self.llr_scale, ext_scale=self.ext_scale,
                               early_stop=self.early_stop, a1=self.a1, ext=self.prior[1:1 + self.nbits], ext_stride=self.code.n_tx,
                               ext_clip=self.ext_clip, ref_info=ref_info, counts=counts, want_post=False, want_iters=False)
        self.decided = out["info_bits"]

    # ---------------------------------------------------------------- blocks
    def run_block(self, ebn0_db: float | None, seed: int = 1, stream_id: int = 0) -> None:
        """Queue one block on the current stream; the counts accumulate on the device."""
        info = self.info_bits(stream_id)
        rows, syms = self.front_end(dev.turbo_encode(self.code, info), ebn0_db, seed, stream_id)
        self._last.zero_()
        if self.outer == 1:
            llr, hard = self.soft(rows)
            dev.count_errors(syms, syms, hard, self.sent, self.nch, self.uncoded)
            out = dev.turbo_decode(self.code, llr, half_iters=2 * self.iters, scale=self.llr_scale, ext_scale=self.ext_scale,
                                   early_stop=self.early_stop, ref_info=info, counts=self._last, want_post=False, want_iters=False)
            self.decided = out["info_bits"]
        else:
            self.begin(int(rows.shape[0]))
            for o in range(self.outer):
                ext, hard = self.detect(rows, first=o == 0)
                if o == 0:
                    dev.count_errors(syms, syms, hard, self.sent, self.nch, self.uncoded)
                if o == self.outer - 1:
                    self.decode(ext, info, self._last)
                elif self.per_pass:
                    self.decode(ext, info, self.pass_counts[o])
                else:
                    self.decode(ext)
        self.counts += self._last
        if self.per_pass:
            self.pass_counts[self.outer - 1] += self._last
        self.blocks += 1

    def reset_counts(self) -> None:
        self.counts.zero_()
        self.uncoded.zero_()
        self.pass_counts.zero_()
        self.blocks = 0

    def result(self) -> tuple[int, int, int]:
        """(information bit errors, codeword errors, information bits compared) - synchronises."""
        _hip.check(_hip.lib().wf_ctx_check(_hip.ctx(), _hip.stream()))
        be, fe, _halves = (int(v) for v in self.counts.cpu().tolist())
        return be, fe, self.blocks * self.ncw * self.code.k

    def half_iterations(self) -> float:
        """Mean half-iterations per codeword in the LAST pass of a block, over the blocks run - synchronises."""
        _hip.check(_hip.lib().wf_ctx_check(_hip.ctx(), _hip.stream()))
        n = self.blocks * self.ncw
        return int(self.counts.cpu()[2]) / n if n else 0.0

    def pass_results(self) -> list[tuple[int, int]]:
        """Per outer pass (``per_pass=True``): (information bit errors, codeword errors) over the blocks run - synchronises."""
        if not self.per_pass:
            raise RuntimeError("pass_results needs per_pass=True")
        _hip.check(_hip.lib().wf_ctx_check(_hip.ctx(), _hip.stream()))
        return [(int(be), int(fe)) for be, fe, _h in self.pass_counts.cpu().tolist()]
