"""A coded PCM/FM link on the multi-symbol noncoherent detector: the one receiver here that needs no carrier recovery.

``NoncoherentPCMFMLink`` is ``CodedCPMLink`` for ``waveform="pcmfm"`` (coded.py: the same burst, modulator, impairments, channel,
σ, counters, framing and LDPC decoder) with the detector exchanged: its "rows" are the noisy samples themselves and its soft
detector is ``device.noncoherent_soft`` (waveforms_amd/viterbi/noncoherent.py states the definition).  Magnitudes do not see a
phase, and a frequency offset costs only what it turns within one window of ``observe`` symbols: ``carrier=(theta0, nu)`` needs
nothing beside it up to ``MAX_OFFSET_CYCLES[observe]`` cycles per sample, hundreds of times what the coherent links' recoveries
follow.  The price is the detector's own loss against the coherent trellis at ν = 0 (HISTORY.md and profiles/noncoherent_pcmfm.json have the curves).

There is no loop: the detector takes no prior.  The window's instant ``offset`` is hand-placed (``DEFAULT_OFFSET``), as the
coherent chains' ``TIMING_OFFSET`` is; timing recovery for this detector is not built, so ``clock`` (the impairment) is refused
with its two synchronisers.
"""
from __future__ import annotations

from .. import device as dev
from ..viterbi import noncoherent as nc
from .coded import _CPM, _LDPC

NO_PHASE = "the noncoherent detector compares correlation magnitudes: there is no phase to recover"
NO_TIMING = "timing recovery for the noncoherent detector is not built (offset is a hand-placed instant)"


class NoncoherentPCMFMLink(_LDPC, _CPM):
    """One block = ``ncw`` codewords of ``code`` sent back to back as ONE PCM/FM burst from symbol 0, plus ``PAD_SYMS`` zero
    symbols (``CodedCPMLink``'s burst):

    coded bits -> ``symbol_map`` -> ``cpm_modulate`` (h = 0.7) -> ``carrier_offset`` if ``carrier`` -> ``awgn`` ->
    ``noncoherent_soft`` over ``observe`` symbols -> ``ldpc_decode``.  Transmitted bit j pairs with λ[j]; every symbol of the
    burst, the pad included, gets a λ (framed, the search runs over all of them).

    ``observe``: N, odd and 3 .. 7; ``offset``: the window's instant, 0 .. sps (None: ``DEFAULT_OFFSET``).  Eb/N0, information
    bits, noise keys and result tuples are ``CodedCPMLink``'s.  Refused with a ValueError: ``recovery`` (there is no phase to
    recover), ``clock``, ``clock_recovery`` and ``joint`` (no timing recovery exists for this detector)."""

    def __init__(self, code, ncw: int, sps: int = 8, observe: int = 5, offset: int | None = None, framing=None, lead_bits: int = 0, carrier=None, *,
                 alpha: float = 0.75, max_iter: int = 50, recovery=None, clock=None, clock_recovery=None, joint=None) -> None:
        if recovery is not None:
            raise ValueError(f"recovery: {NO_PHASE}")
        for name, value in (("clock", clock), ("clock_recovery", clock_recovery), ("joint", joint)):
            if value is not None:
                raise ValueError(f"{name}: {NO_TIMING}")
        self.alpha, self.max_iter = float(alpha), int(max_iter)
        self.observe, self.offset = int(observe), nc.DEFAULT_OFFSET if offset is None else int(offset)
        nc.check_window(observe, sps, self.offset)                                    # (refused before anything touches the device)
        super().__init__(code, ncw, "pcmfm", sps, framing=framing, lead_bits=lead_bits, carrier=carrier)

    def _wave_init(self) -> None:
        from ..cpm.pcmfm import PCMFM_DENOM, PCMFM_NUMER, freq_pulse_pcmfm

        super()._wave_init()
        pulse = freq_pulse_pcmfm(self.sps)
        self.start = nc.burst_start(pulse.size, self.sps, self.offset)
        self._d_table = dev.noncoherent_templates(pulse, PCMFM_NUMER / PCMFM_DENOM, self.sps, self.observe, self.offset)

    def front_end(self, tx, ebn0_db: float | None, seed: int = 1, stream_id: int = 0):
        """Coded bits (device ncw x n_tx) -> (the burst's noisy samples, which are this detector's rows; its symbols)."""
        received, _at, syms = self.samples(tx, ebn0_db, seed, stream_id)
        return received, syms

    def _soft(self, rows):
        return dev.noncoherent_soft(rows, self._d_table, self.sps, self.start, self.nsym)

    def _soft_apriori(self, rows, prior):
        raise NotImplementedError("the noncoherent detector takes no prior")
