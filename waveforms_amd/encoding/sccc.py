"""Serially concatenated convolutional code over SOQPSK-TG on the GPU (``ConvSOQPSKLink``): information bits -> convolutional
encoder (with its interleaver) -> differentially precoded SOQPSK-TG, the recursive inner code -> AWGN + PT / PAM bank -> soft
detector <-> max-log-MAP decoder of the outer code, iterated.

The front end, the PN23 information bits, the noise keys, the Eb/N0-per-information-bit convention, ``PAD_BITS`` and the
uncoded count are the SOQPSK-TG base's, shared with ``CodedSOQPSKLink`` (coded.py); the loop without a freeze state is
``_ClippedLoop``, shared with ``TurboSOQPSKLink`` (pccc.py); the outer code is a
:class:`waveforms_amd.encoding.conv.ConvCode` and its decoder ``conv_siso`` (include/wfhip.h, wf_conv_siso).  Nothing leaves the
GPU inside a block.
"""
from __future__ import annotations

from .. import _hip
from .. import device as dev
from .coded import _SOQPSK


class _ClippedLoop(_SOQPSK):
    """A code whose decoder has no freeze state, behind SOQPSK-TG: one block = ``ncw`` codewords of ``code`` sent back to back as
    ONE burst (plus ``PAD_BITS`` zero bits), Eb/N0 per INFORMATION bit (tail bits and puncturing are in ``code.rate`` = k / n_tx).

    ``outer=1``: the plain soft detector (``viterbi_soft``) once and the class's one-shot decode (``_decode_once``).
    ``outer>1``: the front end runs once per block, then ``outer`` passes of

        soft detector with the burst's prior buffer (``viterbi_soft_apriori``, apriori_scale = ``damping``)
        -> the class's ``decode`` writing the next prior at ``_prior_coded`` (offset +1), stride n_tx, clipped to ±``ext_clip``

    Row 0 and the tail rows keep prior 0.  ``ext_clip`` is in the detector's metric units, which grow linearly with ``sps``:
    default 6.25 sps (50 at sps 8), the LDPC loops' ``ext_sat`` default.  Max-log-MAP on both sides is scale-invariant, so no
    noise-variance scale is needed (``llr_scale`` stays 1).  ``outer`` is fixed and nothing synchronises with the host inside a
    block.  The last pass counts into ``_last``, which is added to ``counts`` and, with ``per_pass=True``, to the last row of
    ``pass_counts``; the earlier passes then count into their own rows (``pass_results``).  Framing is not supported.

    A class supplies ``_ncounts`` (the first two are information bit errors and codeword errors), ``encode``, ``_decode_once``
    and ``decode(ext, ref_info, counts, ...)``, and extends ``begin`` by what else it carries from pass to pass."""

    def __init__(self, code, ncw: int, sps: int, detector: str, outer: int, damping: float, ext_clip: float | None, per_pass: bool, framing) -> None:
        if framing is not None:
            raise ValueError(f"{type(self).__name__} does not support framing")
        self._loop_args(damping, outer=outer)
        self.ext_clip = 6.25 * int(sps) if ext_clip is None else float(ext_clip)
        if not self.ext_clip > 0.0:
            raise ValueError("ext_clip must be positive")
        super().__init__(code, ncw, sps, detector)
        self.per_pass = bool(per_pass)
        self.pass_counts = _hip.zeros((self.outer, self._ncounts), "int64")
        self._last = _hip.zeros(self._ncounts, "int64")
        self.prior = self.decided = None

    # ---------------------------------------------------------------- stages
    def begin(self, nrows: int) -> None:
        """Fresh loop state of one block: prior 0 on every row."""
        if self.prior is None or self.prior.numel() != nrows:
            self.prior = _hip.zeros(nrows, "float32")
        else:
            self.prior.zero_()

    def _decode_last(self, ext, info) -> None:
        self.decode(ext, info, self._last)

    # ---------------------------------------------------------------- blocks
    def run_block(self, ebn0_db: float | None, seed: int = 1, stream_id: int = 0) -> None:
        """Queue one block on the current stream; the counts accumulate on the device."""
        info = self.info_bits(stream_id)
        tx = self.encode(info)
        rows, syms = self.front_end(tx, ebn0_db, seed, stream_id)
        self._last.zero_()
        if self.outer == 1:
            llr, hard = self.soft(rows)
            self.count_uncoded(hard, tx, syms)
            self._decode_once(llr, info)
        else:
            self.begin(int(rows.shape[0]))
            for o in range(self.outer):
                ext, hard = self.detect(rows, first=o == 0)
                if o == 0:
                    self.count_uncoded(hard, tx, syms)
                if o == self.outer - 1:
                    self._decode_last(ext, info)
                elif self.per_pass:
                    self.decode(ext, info, self.pass_counts[o])
                else:
                    self.decode(ext)
        self.counts += self._last
        if self.per_pass:
            self.pass_counts[self.outer - 1] += self._last
        self.blocks += 1

    def reset_counts(self) -> None:
        super().reset_counts()
        self.pass_counts.zero_()

    def result(self) -> tuple[int, int, int]:
        """(information bit errors, codeword errors, information bits compared) - synchronises."""
        _hip.check(_hip.lib().wf_ctx_check(_hip.ctx(), _hip.stream()))
        be, fe = (int(v) for v in self.counts.cpu().tolist()[:2])
        return be, fe, self.blocks * self.ncw * self.code.k

    def pass_results(self) -> list[tuple[int, int]]:
        """Per outer pass (``per_pass=True``): (information bit errors, codeword errors) over the blocks run - synchronises."""
        if not self.per_pass:
            raise RuntimeError("pass_results needs per_pass=True")
        _hip.check(_hip.lib().wf_ctx_check(_hip.ctx(), _hip.stream()))
        return [(int(row[0]), int(row[1])) for row in self.pass_counts.cpu().tolist()]


class ConvSOQPSKLink(_ClippedLoop):
    """``_ClippedLoop`` with a convolutional ``code`` (:class:`waveforms_amd.encoding.conv.ConvCode`): ``outer=1`` is one
    ``conv_siso``, ``outer>1`` is ``outer`` passes of soft detector <-> ``conv_siso``.

    The decoder's extrinsic output MUST be clipped: unclipped, its magnitude grows from pass to pass without bound (a
    convolutional decoder has no syndrome to stop at, and there is no freeze state here).  ``counts`` holds TWO device counters
    and ``result()`` returns a 3-tuple (a convolutional decoder has no "not converged" and no iteration count);
    ``per_pass=True`` also accumulates the two counts after every pass (``pass_results``)."""

    _ncounts = 2

    def __init__(self, code, ncw: int, sps: int = 8, detector: str = "PT", outer: int = 1, damping: float = 0.7, ext_clip: float | None = None,
                 per_pass: bool = False, framing=None) -> None:
        super().__init__(code, ncw, sps, detector, outer, damping, ext_clip, per_pass, framing)
        self.post = None
        self.keep_post = False                 # a subclass that needs the last pass's Λ (conv_siso's info_post) sets it: ``post``

    def encode(self, info):
        return dev.conv_encode(self.code, info)

    def _decode_once(self, llr, info) -> None:
        out = dev.conv_siso(self.code, llr, scale=self.llr_scale, ref_info=info, counts=self._last, want_post=self.keep_post, want_ext=False)
        self.decided, self.post = out["info_bits"], out["info_post"]

    def decode(self, ext, ref_info=None, counts=None, want_post: bool = False) -> None:
        """One decoder pass: the decisions (``decided``) and the next prior, in place; with ``ref_info`` the two counts are
        added to ``counts``; with ``want_post`` the pass's Λ is kept as ``post``."""
        out = dev.conv_siso(self.code, ext, scale=self.llr_scale, ext=self._prior_coded(), ext_stride=self.code.n_tx,
                            ext_clip=self.ext_clip, ref_info=ref_info, counts=counts, want_post=want_post)
        self.decided, self.post = out["info_bits"], out["info_post"]

    def _decode_last(self, ext, info) -> None:
        self.decode(ext, info, self._last, want_post=self.keep_post)
