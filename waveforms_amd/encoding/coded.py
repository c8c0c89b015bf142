"""Coded SOQPSK-TG chain on the GPU: info bits -> LDPC encode -> SOQPSK-TG modulate + AWGN + PT / PAM bank -> max-log-MAP
soft detector (``viterbi_soft``) -> LDPC decode -> error counts (``CodedSOQPSKLink``), and the same chain closed into a
loop: soft detector with a prior <-> LDPC decoder with extrinsic output (``IterativeSOQPSKLink``).

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


class IterativeSOQPSKLink(CodedSOQPSKLink):
    """``CodedSOQPSKLink`` with iterative detection and decoding: same block layout, PN23 information bits, noise keys,
    Eb/N0 convention and result tuples; the front end runs once per block, then ``outer`` passes of

        soft detector with the burst's prior buffer (``viterbi_soft_apriori``, apriori_scale = ``damping``)
        -> ``ldpc_decode_ext`` (``inner`` iterations from a cold start) writing the next prior at offset +1, stride n_tx

    and one ``ldpc_count``.  A codeword whose syndrome is zero is FROZEN: its prior becomes ±``ext_sat`` by its decisions and
    later passes leave it alone (without this a converged codeword would hand back zero extrinsic and be decoded from
    scratch on the next pass, and the loop oscillates).  Row 0 and the tail rows keep prior 0.  Max-log-MAP and
    normalized min-sum are both scale-invariant, so the loop needs no noise-variance scale (``llr_scale`` stays 1).

    ``ext_sat`` / ``ext_clip`` are in the detector's metric units, which grow linearly with ``sps`` (the matched filters
    sum sps + 1 unit-magnitude taps): the defaults are ext_sat = 6.25 sps (50 at sps 8, where mean |λ| is about 11 at
    4.5 dB) and no clip.  ``outer`` is fixed per block and nothing synchronises with the host inside one; every pass is
    queued even when every codeword is already frozen (the decoder's workgroups then retire at once, the detector
    still runs).  ``per_pass=True`` also accumulates the four counts after every pass (``pass_results``)."""

    def __init__(self, code, ncw: int, sps: int = 8, detector: str = "PT", alpha: float = 0.75, outer: int = 8, inner: int = 5,
                 damping: float = 0.7, ext_clip: float | None = None, ext_sat: float | None = None, per_pass: bool = False) -> None:
        if outer < 1 or inner < 1:
            raise ValueError("outer and inner must be at least 1")
        if not (math.isfinite(damping) and damping > 0.0):
            raise ValueError("damping must be finite and positive")
        self.outer, self.inner, self.damping = int(outer), int(inner), float(damping)
        self.ext_sat = 6.25 * int(sps) if ext_sat is None else float(ext_sat)
        self.ext_clip = math.inf if ext_clip is None else float(ext_clip)
        if not (math.isfinite(self.ext_sat) and self.ext_sat > 0.0 and self.ext_clip > 0.0):
            raise ValueError("ext_sat must be finite and positive, ext_clip positive")
        super().__init__(code, ncw, sps, detector, alpha, max_iter=inner)
        self.per_pass = bool(per_pass)
        self.pass_counts = _hip.zeros((self.outer, 4), "int64")
        self.prior = self.state = self.iters = self.decided = None

    # ---------------------------------------------------------------- stages
    def begin(self, nrows: int) -> None:
        """Fresh loop state of one block: prior 0 on every row, every codeword open, no iterations."""
        if self.prior is None or self.prior.numel() != nrows:
            self.prior = _hip.zeros(nrows, "float32")
            self.state = _hip.zeros(self.ncw, "uint8")
            self.iters = _hip.zeros(self.ncw, "int32")
            self.decided = _hip.zeros((self.ncw, self.code.k), "uint8")
        else:
            for t in (self.prior, self.state, self.iters, self.decided):
                t.zero_()

    def detect(self, rows, first: bool = False):
        """One detector pass -> (extrinsic λ of the coded bits, ncw x n_tx view; hard decisions of λ + π).  The first pass
        of a block has prior 0 everywhere and takes the plain detector (bitwise the same result)."""
        ext, bits = dev.viterbi_soft_apriori(rows, None if first else self.prior, self.damping)
        return ext[1:1 + self.nbits].view(self.ncw, self.code.n_tx), bits[1:1 + self.nbits]

    def decode(self, ext) -> None:
        """One decoder pass over the open codewords: decisions, iterations, states and the next prior, in place."""
        dev.ldpc_decode_ext(self.code, ext, self.state, self.prior[1:1 + self.nbits], self.code.n_tx, scale=self.llr_scale, alpha=self.alpha,
                            max_iter=self.inner, ext_clip=self.ext_clip, ext_sat=self.ext_sat, info_bits=self.decided, iters=self.iters)

    # ---------------------------------------------------------------- blocks
    def run_block(self, ebn0_db: float | None, seed: int = 1, stream_id: int = 0) -> None:
        info = self.info_bits(stream_id)
        tx = dev.ldpc_encode(self.code, info)
        rows, syms = self.front_end(tx, ebn0_db, seed, stream_id)
        self.begin(int(rows.shape[0]))
        for o in range(self.outer):
            ext, hard = self.detect(rows, first=o == 0)
            if o == 0:
                dev.count_errors(syms, syms, hard, tx.reshape(-1), self.nbits, self.uncoded)
            self.decode(ext)
            if self.per_pass:
                dev.ldpc_count(self.code, self.decided, info, self.state, self.iters, self.pass_counts[o])
        dev.ldpc_count(self.code, self.decided, info, self.state, self.iters, self.counts)
        self.blocks += 1

    def reset_counts(self) -> None:
        super().reset_counts()
        self.pass_counts.zero_()

    def pass_results(self) -> list[tuple[int, int, int, float]]:
        """Per outer pass (``per_pass=True``): (information bit errors, codeword errors, codewords still open, mean
        iterations so far) over the blocks run - synchronises."""
        _hip.check(_hip.lib().wf_ctx_check(_hip.ctx(), _hip.stream()))
        ncw = self.blocks * self.ncw
        return [(int(be), int(fe), int(nc), (int(its) / ncw if ncw else 0.0)) for be, fe, nc, its in self.pass_counts.cpu().tolist()]
