"""Serially concatenated convolutional code over SOQPSK-TG on the GPU (``ConvSOQPSKLink``): information bits -> convolutional
encoder (with its interleaver) -> differentially precoded SOQPSK-TG, the recursive inner code -> AWGN + PT / PAM bank -> soft
detector <-> max-log-MAP decoder of the outer code, iterated.

The front end, the PN23 information bits, the noise keys, the Eb/N0-per-information-bit convention, ``PAD_BITS`` and the
uncoded count are ``CodedSOQPSKLink``'s; the outer code is a :class:`waveforms_amd.encoding.conv.ConvCode` and its decoder
``conv_siso`` (include/wfhip.h, wf_conv_siso).  Nothing leaves the GPU inside a block.
"""
from __future__ import annotations

import math

from .. import _hip
from .. import device as dev
from .coded import CodedSOQPSKLink


class ConvSOQPSKLink(CodedSOQPSKLink):
    """One block = ``ncw`` codewords of the convolutional ``code`` sent back to back as ONE SOQPSK-TG burst (plus ``PAD_BITS``
    zero bits).  Eb/N0 is per INFORMATION bit (the tail bits and any puncturing are in ``code.rate`` = k / n_tx).

    ``outer=1``: one pass, the plain soft detector (``viterbi_soft``) and one ``conv_siso``.  ``outer>1``: the front end runs
    once per block, then ``outer`` passes of

        soft detector with the burst's prior buffer (``viterbi_soft_apriori``, apriori_scale = ``damping``)
        -> ``conv_siso`` writing the next prior at offset +1, stride n_tx, clipped to ±``ext_clip``

    Row 0 and the tail rows keep prior 0.  The decoder's extrinsic output MUST be clipped: unclipped, its magnitude grows
    from pass to pass without bound (a convolutional decoder has no syndrome to stop at, and there is no freeze state here).
    ``ext_clip`` is in the detector's metric units, which grow linearly with ``sps``: default 6.25 sps (50 at sps 8), the
    loops' ``ext_sat`` default.  Max-log-MAP on both sides is scale-invariant, so no noise-variance scale is needed
    (``llr_scale`` stays 1).  ``outer`` is fixed and nothing synchronises with the host inside a block.  ``per_pass=True``
    also accumulates the two counts after every pass (``pass_results``).  Framing is not supported.

    What differs from the parent class: ``alpha`` and ``max_iter`` are inherited attributes that mean nothing here (there is no
    LDPC decoder), ``counts`` holds TWO device counters instead of four, and ``result()`` returns a 3-tuple, not the parent's
    5-tuple (a convolutional decoder has no "not converged" and no iteration count)."""

    def __init__(self, code, ncw: int, sps: int = 8, detector: str = "PT", outer: int = 1, damping: float = 0.7, ext_clip: float | None = None,
                 per_pass: bool = False, framing=None) -> None:
        if framing is not None:
            raise ValueError("ConvSOQPSKLink does not support framing")
        if outer < 1:
            raise ValueError("outer must be at least 1")
        if not (math.isfinite(damping) and damping > 0.0):
            raise ValueError("damping must be finite and positive")
        self.outer, self.damping = int(outer), float(damping)
        self.ext_clip = 6.25 * int(sps) if ext_clip is None else float(ext_clip)
        if not self.ext_clip > 0.0:
            raise ValueError("ext_clip must be positive")
        super().__init__(code, ncw, sps, detector)
        self.per_pass = bool(per_pass)
        self.counts = _hip.zeros(2, "int64")
        self.pass_counts = _hip.zeros((self.outer, 2), "int64")
        self._last = _hip.zeros(2, "int64")
        self.prior = self.decided = self.post = None
        self.keep_post = False                 # a subclass that needs the last pass's Λ (conv_siso's info_post) sets it: ``post``

    # ---------------------------------------------------------------- stages
    def channel_llrs(self, ebn0_db: float | None, seed: int = 1, stream_id: int = 0):
        """(λ ncw x n_tx of the plain detector, information bits ncw x k) of one block, on the device."""
        info = self.info_bits(stream_id)
        rows, _ = self.front_end(dev.conv_encode(self.code, info), ebn0_db, seed, stream_id)
        llr, _ = self.soft(rows)
        return llr.contiguous(), info.view(self.ncw, self.code.k)

    def begin(self, nrows: int) -> None:
        """Fresh loop state of one block: prior 0 on every row."""
        if self.prior is None or self.prior.numel() != nrows:
            self.prior = _hip.zeros(nrows, "float32")
        else:
            self.prior.zero_()

    def detect(self, rows, first: bool = False):
        """One detector pass -> (extrinsic λ of the coded bits, ncw x n_tx view; hard decisions of λ + π).  The first pass of
        a block has prior 0 everywhere and takes the plain detector (bitwise the same result)."""
        ext, bits = dev.viterbi_soft_apriori(rows, None if first else self.prior, self.damping)
        return ext[1:1 + self.nbits].view(self.ncw, self.code.n_tx), bits[1:1 + self.nbits]

    def decode(self, ext, ref_info=None, counts=None, want_post: bool = False) -> None:
        """One decoder pass: the decisions (``decided``) and the next prior, in place; with ``ref_info`` the two counts are
        added to ``counts``; with ``want_post`` the pass's Λ is kept as ``post``."""
        out = dev.conv_siso(self.code, ext, scale=self.llr_scale, ext=self.prior[1:1 + self.nbits], ext_stride=self.code.n_tx,
                            ext_clip=self.ext_clip, ref_info=ref_info, counts=counts, want_post=want_post)
        self.decided, self.post = out["info_bits"], out["info_post"]

    # ---------------------------------------------------------------- blocks
    def run_block(self, ebn0_db: float | None, seed: int = 1, stream_id: int = 0) -> None:
        """Queue one block on the current stream; the counts accumulate on the device."""
        info = self.info_bits(stream_id)
        rows, syms = self.front_end(dev.conv_encode(self.code, info), ebn0_db, seed, stream_id)
        self._last.zero_()
        if self.outer == 1:
            llr, hard = self.soft(rows)
            dev.count_errors(syms, syms, hard, self.sent, self.nch, self.uncoded)
            out = dev.conv_siso(self.code, llr, scale=self.llr_scale, ref_info=info, counts=self._last, want_post=self.keep_post, want_ext=False)
            self.decided, self.post = out["info_bits"], out["info_post"]
        else:
            self.begin(int(rows.shape[0]))
            for o in range(self.outer):
                ext, hard = self.detect(rows, first=o == 0)
                if o == 0:
                    dev.count_errors(syms, syms, hard, self.sent, self.nch, self.uncoded)
                if o == self.outer - 1:
                    self.decode(ext, info, self._last, want_post=self.keep_post)
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
        be, fe = (int(v) for v in self.counts.cpu().tolist())
        return be, fe, self.blocks * self.ncw * self.code.k

    def pass_results(self) -> list[tuple[int, int]]:
        """Per outer pass (``per_pass=True``): (information bit errors, codeword errors) over the blocks run - synchronises."""
        if not self.per_pass:
            raise RuntimeError("pass_results needs per_pass=True")
        _hip.check(_hip.lib().wf_ctx_check(_hip.ctx(), _hip.stream()))
        return [(int(be), int(fe)) for be, fe in self.pass_counts.cpu().tolist()]
