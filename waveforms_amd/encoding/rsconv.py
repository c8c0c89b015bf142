"""The concatenated telemetry link on the GPU (``RSConvSOQPSKLink``): user bits -> Reed-Solomon encoder, symbol-interleaved to
depth I -> convolutional encoder -> differentially precoded SOQPSK-TG -> AWGN + PT / PAM bank -> soft detector <-> max-log-MAP
decoder of the convolutional code -> Reed-Solomon decoder.

Everything up to the convolutional decoder's decisions is ``ConvSOQPSKLink`` (waveforms_amd/encoding/sccc.py), whose
"information bits" are here the RS frames in bit form: one convolutional codeword carries one RS frame (``code.k == 8 rs.n
rs.depth``), so the inner decoder's decisions feed ``rs_decode(bits=True)`` with no packing pass.  Nothing leaves the GPU inside
a block.

With ``erasures=F`` the two halves talk: the last inner pass keeps its Λ, ``rs_mark_erasures`` declares per RS codeword the at
most F symbols of smallest reliability (below ``erase_below``) erased, and the RS decoder runs as an errors-and-erasures decoder.
"""
from __future__ import annotations

import math

from .. import _hip
from .. import device as dev
from .sccc import ConvSOQPSKLink


class RSConvSOQPSKLink(ConvSOQPSKLink):
    """One block = ``ncw`` convolutional codewords, each carrying one RS frame of ``rs.depth`` interleaved codewords.

    Eb/N0 is per USER information bit: ``_rate_db`` pays for the RS parity, the tail bits and any puncturing.  The user bits are
    PN23 (from the all-ones state), block b = ``stream_id`` taking the segment that starts at bit b ncw depth rs.k 8.
    ``result()`` stays the parent's: the inner code's errors, counted on the RS-coded bits.  ``rs_result()`` is the link's
    own count after the RS decoder.  Every ``outer`` value works as in the parent; framing is not supported.

    ``erasures=0``: the errors-only decoder, the calls and counts as they always were.  ``erasures=F`` (1 .. 2t): the last inner
    pass also keeps Λ (``post``); ``rs_mark_erasures(F, erase_below)`` writes ``rs_erased`` and ``rs_decode(erasures=...)`` decodes
    errors and erasures.  ``rs_result()`` keeps its tuple; ``rs_erasure_result()`` adds (erasures declared, erasures filled)."""

    def __init__(self, rs, code, ncw: int, sps: int = 8, detector: str = "PT", outer: int = 1, damping: float = 0.7,
                 ext_clip: float | None = None, per_pass: bool = False, framing=None, erasures: int = 0,
                 erase_below: float = float("inf")) -> None:
        if framing is not None:
            raise ValueError("RSConvSOQPSKLink does not support framing")
        if not 0 <= int(erasures) <= 2 * rs.t:
            raise ValueError(f"erasures = {erasures} outside 0 .. 2t = {2 * rs.t}")
        if math.isnan(float(erase_below)):
            raise ValueError("erase_below must not be NaN")
        if code.k != 8 * rs.n * rs.depth:
            raise ValueError(f"the inner code must carry one RS frame: code.k = {code.k}, 8 rs.n rs.depth = {8 * rs.n * rs.depth}")
        self.rs = rs
        super().__init__(code, ncw, sps, detector, outer, damping, ext_clip, per_pass)
        self.user_bits_per_block = self.ncw * rs.depth * rs.k * 8
        self.erasures, self.erase_below = int(erasures), float(erase_below)
        self.keep_post = self.erasures > 0
        self.rs_counts = _hip.zeros(6 if self.erasures else 5, "int64")
        self.rs_declared = _hip.zeros(1, "int64")
        self.user = self.rs_msg = self.rs_status = self.rs_erased = None
        rs.handle()

    def _rate_db(self) -> float:
        return super()._rate_db() + 10.0 * math.log10(self.rs.k / self.rs.n)

    def user_bits(self, stream_id: int = 0):
        """The PN23 user bits of one block."""
        n = self.user_bits_per_block
        return dev.lfsr_bits(23, self._mask, (1 << 23) - 1, n, skip=int(stream_id) * n)[0]

    def info_bits(self, stream_id: int = 0):
        """The inner code's message of one block: the RS frames (bit form) of the block's user bits (kept in ``user``)."""
        self.user = self.user_bits(stream_id)
        return dev.rs_encode(self.rs, self.user, bits=True).view(-1)

    def run_block(self, ebn0_db: float | None, seed: int = 1, stream_id: int = 0) -> None:
        """Queue one block on the current stream: the parent's block, then the RS decoder on its decisions."""
        super().run_block(ebn0_db, seed, stream_id)
        if self.erasures:
            self.rs_erased = dev.rs_mark_erasures(self.rs, self.post, self.erasures, self.erase_below)
            self.rs_declared += self.rs_erased.sum()
        out = dev.rs_decode(self.rs, self.decided, bits=True, ref_msg=self.user, counts=self.rs_counts, erasures=self.rs_erased)
        self.rs_msg, self.rs_status = out["msg"], out["status"]

    def reset_counts(self) -> None:
        super().reset_counts()
        self.rs_counts.zero_()
        self.rs_declared.zero_()

    def rs_result(self) -> tuple[int, int, int, int, int, int]:
        """(user bit errors, RS codeword errors, flagged failures, symbols corrected, frame errors, user bits compared) after
        the RS decoder - synchronises.  Miscorrections are codeword errors - flagged failures."""
        _hip.check(_hip.lib().wf_ctx_check(_hip.ctx(), _hip.stream()))
        be, ce, fl, cor, fe = (int(v) for v in self.rs_counts[:5].cpu().tolist())
        return be, ce, fl, cor, fe, self.blocks * self.user_bits_per_block

    def rs_erasure_result(self) -> tuple[int, int]:
        """(erasures declared, erasures filled: those of the codewords that decoded) over the blocks run - synchronises.
        (0, 0) with ``erasures=0``."""
        _hip.check(_hip.lib().wf_ctx_check(_hip.ctx(), _hip.stream()))
        return int(self.rs_declared.item()), int(self.rs_counts[5].item()) if self.erasures else 0
