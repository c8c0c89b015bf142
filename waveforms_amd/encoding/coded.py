"""Coded SOQPSK-TG chain on the GPU: info bits -> LDPC encode -> SOQPSK-TG modulate + AWGN + PT / PAM bank -> max-log-MAP
soft detector (``viterbi_soft``) -> LDPC decode -> error counts.

Every stage is an existing device entry point (waveforms_amd.device); nothing leaves the GPU inside a block.  The fused
``SOQPSKLink`` is not used and not changed.
"""
from __future__ import annotations

import math

import numpy as np

from .. import _hip
from .. import device as dev
from ..cpm.soqpsk import freq_pulse_soqpsk_tg
from ..cpm.trellis.model import SOQPSKTrellis4x2DiffEncoded
from ..filters.matched import pam_matched_filter_taps, pt_matched_filter_taps
from ..glfsr.pn import generate_mask
from ..link import sigma_for_ebn0

TIMING_OFFSET = {"PT": -1, "PAM": 0}      # SOQPSK-TG (examples/soqpsk_detection.py)
PAD_BITS = 16                             # tail after the burst's last codeword: every coded bit gets its λ


class CodedSOQPSKLink:
    """One block = ``ncw`` codewords of ``code`` sent back to back as ONE SOQPSK-TG burst (plus ``PAD_BITS`` zero bits).

    Eb/N0 is per INFORMATION bit: the channel's σ is ``sigma_for_ebn0(ebn0_db + 10 log10(k / n_tx), sps)``, i.e. the
    channel runs at Eb/N0 + 10 log10(rate) per transmitted bit (-3.01 dB for the rate-1/2 demo code).

    The information bits are PN23 (from the all-ones state), block b = ``stream_id`` taking the segment that starts at
    bit b ncw k.  The noise is the library's counter-based AWGN keyed by (``seed``, ``stream_id``).  Transmitted bit j
    is paired with the soft detector's λ_{j+1} (include/wfhip.h, wf_viterbi4_soft).  ``ebn0_db=None`` is noiseless."""

    def __init__(self, code, ncw: int, sps: int = 8, detector: str = "PT", alpha: float = 0.75, max_iter: int = 50) -> None:
        if detector not in TIMING_OFFSET:
            raise ValueError(f"unknown detector {detector!r}")
        if ncw < 1:
            raise ValueError("ncw must be at least 1")
        self.code, self.ncw, self.sps, self.detector = code, int(ncw), int(sps), detector
        self.alpha, self.max_iter = float(alpha), int(max_iter)
        self.llr_scale = 1.0                    # (normalized min-sum does not depend on it)
        self.nbits = self.ncw * code.n_tx
        self.nsym = self.nbits + PAD_BITS
        pulse = freq_pulse_soqpsk_tg(self.sps)
        taps = (pt_matched_filter_taps if detector == "PT" else pam_matched_filter_taps)(pulse, 0.25, self.sps)
        self._d_h = _hip.to_device(np.array([0.25]))
        self._d_pulse = _hip.to_device(pulse)
        self._d_taps = _hip.to_device(np.ascontiguousarray(taps))
        self._tables = SOQPSKTrellis4x2DiffEncoded.dense_tables()
        self._pad = _hip.zeros(PAD_BITS, "uint8")
        self._mask = generate_mask(23)
        self.counts = _hip.zeros(4, "int64")
        self.uncoded = _hip.zeros(2, "int64")
        self.blocks = 0
        code.handle()

    def sigma(self, ebn0_db: float | None) -> float:
        if ebn0_db is None:
            return 0.0
        return sigma_for_ebn0(float(ebn0_db) + 10.0 * math.log10(self.code.k / self.code.n_tx), self.sps)

    # ---------------------------------------------------------------- stages
    def info_bits(self, stream_id: int = 0):
        n = self.ncw * self.code.k
        bits, _ = dev.lfsr_bits(23, self._mask, (1 << 23) - 1, n, skip=int(stream_id) * n)
        return bits

    def front_end(self, tx, ebn0_db: float | None, seed: int = 1, stream_id: int = 0):
        """Coded bits (device ncw x n_tx) -> matched-filter rows of the burst."""
        torch = _hip.torch()
        bits = torch.cat((tx.reshape(-1), self._pad))
        syms, _ = dev.fsm_encode(*self._tables, bits)
        sig = dev.cpm_modulate(syms, self._d_h, self._d_pulse, self.sps)
        first, ncols = dev.decimation(int(sig.shape[0]), self.sps, 2, TIMING_OFFSET[self.detector])
        if ncols < self.nbits + 1:
            raise RuntimeError(f"{ncols} detector rows for {self.nbits} coded bits")
        rows = dev.awgn_mf_bank(sig, self._d_taps, first, self.sps, ncols, self.sigma(ebn0_db), seed, stream_id, 0,
                                np.exp(-1j * np.pi / 4))
        return rows, syms

    def soft(self, rows):
        """Rows -> (λ of the coded bits, ncw x n_tx view; hard decisions of the same λ)."""
        llr, bits = dev.viterbi_soft(rows, True)
        return llr[1:1 + self.nbits].view(self.ncw, self.code.n_tx), bits[1:1 + self.nbits]

    def channel_llrs(self, ebn0_db: float | None, seed: int = 1, stream_id: int = 0):
        """(λ ncw x n_tx, information bits ncw x k) of one block, on the device."""
        info = self.info_bits(stream_id)
        tx = dev.ldpc_encode(self.code, info)
        rows, _ = self.front_end(tx, ebn0_db, seed, stream_id)
        llr, _ = self.soft(rows)
        return llr.contiguous(), info.view(self.ncw, self.code.k)

    # ---------------------------------------------------------------- blocks
    def run_block(self, ebn0_db: float | None, seed: int = 1, stream_id: int = 0) -> None:
        """Queue one block on the current stream; the counts accumulate on the device."""
        info = self.info_bits(stream_id)
        tx = dev.ldpc_encode(self.code, info)
        rows, syms = self.front_end(tx, ebn0_db, seed, stream_id)
        llr, hard = self.soft(rows)
        dev.count_errors(syms, syms, hard, tx.reshape(-1), self.nbits, self.uncoded)
        dev.ldpc_decode(self.code, llr, scale=self.llr_scale, alpha=self.alpha, max_iter=self.max_iter, ref_info=info,
                        counts=self.counts)
        self.blocks += 1

    def reset_counts(self) -> None:
        self.counts.zero_()
        self.uncoded.zero_()
        self.blocks = 0

    def result(self) -> tuple[int, int, int, int, float]:
        """(information bit errors, codeword errors, codewords not converged, information bits compared, mean
        iterations) - synchronises."""
        _hip.check(_hip.lib().wf_ctx_check(_hip.ctx(), _hip.stream()))
        be, fe, nc, its = (int(v) for v in self.counts.cpu().tolist())
        ncw = self.blocks * self.ncw
        return be, fe, nc, ncw * self.code.k, (its / ncw if ncw else 0.0)

    def uncoded_result(self) -> tuple[int, int]:
        """(bit errors of λ < 0 against the coded bits, coded bits compared) over the same blocks."""
        return int(self.uncoded.cpu()[1]), self.blocks * self.nbits
