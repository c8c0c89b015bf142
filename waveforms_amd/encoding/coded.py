"""Coded chains on the GPU: info bits -> encoder -> modulate + AWGN + matched filters -> max-log-MAP soft detector -> decoder ->
error counts, and the same chains closed into a loop, soft detector with a prior <-> decoder with extrinsic output.  Every
stage is an existing device entry point (waveforms_amd.device); nothing leaves the GPU inside a block.  The fused ``SOQPSKLink``
and ``CPMLink`` are not used and not changed.

A link class is a waveform, a code and a kind of loop, each stated once:

    ``_Framed``   the burst around the codewords: sync marker, randomiser, frame search; the synchroniser slots and their results
    ``_Link``     what every link does: PN23 information bits, ``channel_llrs`` through the ``encode`` hook, the counters, the
                  view of the detector's output as codewords (``_coded``) and of the prior buffer (``_prior_coded``), ``detect``,
                  and the front end: modulated signal (``modulated``) -> impairments (``impaired``; of a block: ``signal``) ->
                  noisy samples (``noisy``; of a block: ``samples``) -> rows
    ``_SOQPSK``   SOQPSK-TG: pad, tables, PT / PAM bank, ``viterbi_soft`` (``_apriori``), the uncoded count, λ offset 1
    ``_CPM``      ARTM multi-h and PCM/FM on the generic CPM trellis: the same list with ``cpm_soft`` (``_apriori``), λ offset 0
    ``_LDPC``     one ``ldpc_decode`` per block: ``CodedSOQPSKLink`` = ``_LDPC`` on ``_SOQPSK``, ``CodedCPMLink`` = ``_LDPC`` on ``_CPM``
    ``_LDPCLoop`` the loop with frozen codewords: ``IterativeSOQPSKLink`` (adds ``live_only``), ``IterativeCPMLink`` (``prior_warmup``)

The clipped loops without a freeze state (``ConvSOQPSKLink``, ``TurboSOQPSKLink``, ``RSConvSOQPSKLink``) are in sccc.py, pccc.py
and rsconv.py, on ``_SOQPSK``.

The four classes here take ``framing`` (a :class:`waveforms_amd.encoding.framing.Framing`) and ``lead_bits``: the burst is then
``lead_bits`` pseudo-random bits, ``ncw`` frames (sync marker + randomised codeword) and the pad, and the receiver finds the
codewords itself: ``frame_search`` over the whole burst's λ, ``frame_gather`` into the decoder's input and, in the loops,
``frame_scatter`` of the decoder's extrinsic output (and the marker as a known-bits prior) back into the detector's prior
buffer (``_Framed``).  With ``framing=None`` every class does exactly what it did without the keyword.

They also take two impairments of the modulated signal, applied in this order in front of the unchanged channel, and the
synchronisers that undo them.  Every keyword defaults to None: the same calls as without it.

    ``carrier=(theta0, nu)``   all four: rotated by theta0 + 2π nu k (``carrier_offset``, in place; nu in cycles per sample)
    ``timing=(tau0, eps)``     SOQPSK-TG: read at n + tau0 + eps n (``timing_offset``; symbol timing offset and drift, in samples)
    ``clock=(tau0, eps)``      CPM: the same impairment

A synchroniser sits at one of three places: it corrects the noisy samples, makes the detector's rows from them in place of the
plain bank, or turns the bank's rows in front of the detector.  As soon as one reads samples they are materialised (``awgn``,
the same rotation and the same noise coordinates as the fused front end's); SOQPSK-TG's fused ``awgn_mf_bank`` is used only
when none does.  Each must be built for the link's sps (the CPM ones for its design too; ``CarrierRecovery`` has no sps), and
one that leaves the rows shifted needs a ``framing`` whose search absorbs what it leaves open.  ``_SOQPSK._slots`` and
``_CPM._slots`` state the same as data.

    keyword, waveform             class under waveforms_amd.sync     place     excludes                   comes back modulo
    ``recovery``         SOQPSK   carrier.CarrierRecovery            turns     -                          π: framing (its polarity)
    ``recovery``         CPM      carrier_cpm.CPMCarrierRecovery     turns     -                          2π/p: no framing needed
    ``timing_recovery``  SOQPSK   timing.TimingRecovery              rows      carrier, recovery          two symbols: framing
    ``acquisition``      SOQPSK   joint.JointAcquisition             rows      recovery, timing_recovery  (sps, π/2) and (0, π): framing
    ``coarse``           SOQPSK   coarse.CoarseFrequency             samples   timing_recovery            - (needs recovery or acquisition)
    ``clock_recovery``   CPM      timing_cpm.CPMTimingRecovery       rows      carrier, recovery          nh symbols: framing
    ``joint``            CPM      joint_cpm.CPMJointAcquisition      rows      recovery, clock_recovery   (nh sps, P/2) and (0, P): framing

``recovery``: 2π/p is a rotation that relabels the trellis's phase states and leaves the data alone.  Either waveform refuses
the other's recovery.  ``timing_recovery``: the rows may be two early or late.  ``acquisition`` / ``joint`` work under BOTH
impairments (``carrier=`` and ``timing=`` / ``clock=`` may be given beside them); the SOQPSK-TG rows may be a few rows early or
late, and inverted, the CPM rows a whole number of periods of nh symbols early or late, as ``clock_recovery``'s.  ``coarse``
takes a carrier frequency offset far outside the fine recoveries' pull-in range off the noisy samples before anything else reads
them: beside ``recovery`` the front end becomes ``awgn`` -> ``coarse.correct`` -> ``mf_bank`` -> ``recovery``, beside
``acquisition`` it becomes ``awgn`` -> ``coarse.correct`` -> ``acquisition.recover``.  It needs one of the two (the residual phase
is unknown) and excludes ``timing_recovery`` (that path excludes a carrier).

A keyword of the other waveform is a TypeError.  That is why the CPM names are ``clock`` / ``clock_recovery`` and ``joint``, not
``timing`` / ``timing_recovery`` and ``acquisition`` (and a ``TimingRecovery`` passed as ``clock_recovery`` is refused).  ``coarse``
stays a TypeError on the CPM classes: PCM/FM and ARTM have no usable spectral lines of this kind (their 10th to 32nd power lines
drown in the noise at any useful Eb/N0) and need another estimator.
"""
from __future__ import annotations

import importlib
import math
from typing import NamedTuple

import numpy as np

from .. import _hip
from .. import device as dev
from .live import DEFAULT_GUARD
from ..cpm.soqpsk import freq_pulse_soqpsk_tg
from ..cpm.trellis.model import SOQPSKTrellis4x2DiffEncoded
from ..filters.matched import pam_matched_filter_taps, pt_matched_filter_taps
from ..glfsr.pn import generate_mask
from ..link import sigma_for_ebn0

TIMING_OFFSET = {"PT": -1, "PAM": 0}      # SOQPSK-TG (examples/soqpsk_detection.py)
PAD_BITS = 16                             # tail after the burst's last codeword: every coded bit gets its λ
PAD_SYMS = 8                              # CPM chains: zero symbols after the burst's last codeword
CPM_WAVEFORMS = {"multih": 1, "pcmfm": 2}  # -> symbol_map kind (the reference's natural-binary mappers)
DEROTATION = np.exp(-1j * np.pi / 4)      # of the channel's output, in ``awgn`` and in the fused ``awgn_mf_bank``


class _Slot(NamedTuple):
    """One synchroniser keyword of a waveform's links (``_SOQPSK._slots``, ``_CPM._slots``): what ``_sync_init`` checks, in this
    order, where ``front_end`` puts it and what its ``*_result`` hands back."""

    name: str                     # the keyword and the attribute
    a: str                        # "<name>_result needs <a> and a block that ran"
    noun: str                     # what the refusals call it
    stage: str                    # "samples": corrects the noisy samples; "rows": makes the rows from them; "turns": turns the bank's rows
    returns: tuple                # what recover / correct returns beyond the rows (the samples), by ``_HOST``
    found: tuple = ()             # which of timing_found / carrier_found the result appends
    cls: str | None = None        # module.Class under waveforms_amd.sync, imported when the keyword is used; None: ``_check_recovery``
    excludes: tuple = ()          # keywords it cannot stand beside,
    why: str = ""                 # and why
    needs: tuple = ()             # the keywords one of which it needs beside it,
    needs_what: str = ""          # and the refusal's words for them and for why
    design: bool = False          # built for the link's design (``spec``) beside its sps
    framing: str | None = None    # why it needs a framing: what comes back modulo what
    shifted: str | None = None    # how it leaves the rows, where that keeps the channel bits from being counted (``uncoded_result``'s words)


_HOST = {"array": lambda t: (_hip.to_host(t),), "int": lambda t: (int(t.cpu()),), "floats": lambda t: tuple(float(v) for v in _hip.to_host(t))}
_ACQUIRES = "it recovers the carrier and the timing itself"
_NOT_JOINT = "joint timing and carrier acquisition is not implemented"


def _pair(name: str, parts: str, value):
    """An impairment ``name=(a, b)`` as two finite floats, or None."""
    if value is None:
        return None
    a, b = (float(v) for v in value)
    if not (math.isfinite(a) and math.isfinite(b)):
        raise ValueError(f"{name} = ({parts}) must be finite")
    return a, b


class _Framed:
    """What a framed link adds to a coded link (``framing=None``: nothing).  ``nch`` is the number of channel bits in front
    of the pad: ``lead_bits + ncw period`` (``ncw n_tx`` unframed).  The receiver side never reads ``lead_bits``: it is used
    only to count, on the device, the blocks whose lock differs from it."""

    def _frame_init(self, framing, lead_bits: int, bits_per_symbol: int = 1) -> None:
        self.framing, self.lead_bits = framing, int(lead_bits)
        self.nch, self._fill = self.nbits, None
        if framing is None:
            if self.lead_bits:
                raise ValueError("lead_bits needs a framing")
            return
        if framing.n_tx != self.code.n_tx:
            raise ValueError(f"the framing is for n_tx = {framing.n_tx}, the code has {self.code.n_tx}")
        if not 0 <= self.lead_bits < framing.period:
            raise ValueError(f"lead_bits = {lead_bits} outside 0 .. {framing.period - 1}")
        self.nch = self.lead_bits + self.ncw * framing.period
        fill = -self.nch % int(bits_per_symbol)                  # whole symbols: zero bits at the END of the burst
        self._fill = _hip.zeros(fill, "uint8") if fill else None
        self.lock = _hip.zeros(4, "int64")
        self.sync = _hip.zeros(2, "int64")                       # blocks searched, wrong locks
        self._true_lock = _hip.to_device(np.array([self.lead_bits, 1], dtype=np.int64))
        self._llr_in = _hip.empty((self.ncw, self.code.n_tx), "float64")

    def _sync_init(self, sps: int, given: dict) -> None:
        """The waveform's own keywords out of ``given`` (every keyword of the constructor by name), checked in the order of
        ``_slots`` before anything touches the device: the timing impairment ``_drift``, then per slot the class, what it excludes,
        what it needs, the link's design and sps, the framing.  ``recovery`` is not checked here: ``_Link.__init__`` does that
        behind the framing (``_check_recovery``).  Nothing is left of a last block."""
        setattr(self, self._drift, _pair(self._drift, "tau0, eps", given[self._drift]))
        for slot in (s for s in self._slots if s.cls):
            sync = given[slot.name]
            if sync is not None:
                module, cls = slot.cls.split(".")
                if not isinstance(sync, getattr(importlib.import_module(f"..sync.{module}", __package__), cls)):
                    raise ValueError(f"{slot.name} is a waveforms_amd.sync.{slot.cls}")
                if any(given.get(k) is not None for k in slot.excludes):
                    raise ValueError(f"{slot.name} excludes {' and '.join(slot.excludes)}: {slot.why}")
                if slot.needs and all(given.get(k) is None for k in slot.needs):
                    raise ValueError(f"{slot.name} needs {slot.needs_what}")
                if slot.design and sync.spec != self.spec:
                    raise ValueError(f"the {slot.noun} is for another design than the link's full-phase trellis")
                if sync.sps != sps:
                    raise ValueError(f"the {slot.noun} is for sps = {sync.sps}, the link has {sps}")
                if slot.framing and given.get("framing") is None:
                    raise ValueError(f"{slot.name} needs a framing: {slot.framing}")
            setattr(self, slot.name, sync)
        used = [s for s in self._slots if s.cls and getattr(self, s.name) is not None]
        self._correctors = [s for s in used if s.stage == "samples"]
        self._row_maker = next((s for s in used if s.stage == "rows"), None)     # (at most one: they exclude each other)
        self._shifts = next((s for s in used if s.shifted), None)
        self._sync_last = {}                                                           # slot name -> what its last recover / correct returned

    @staticmethod
    def _found(*found):
        """What the anchored coarse tracks of a synchroniser's last ``recover`` found, for the ``*_result`` methods: per track
        (the drift in the tracker's unit per window, the number of rejected windows); nothing without an anchor."""
        return tuple(v for f in found if f is not None for v in (float(f[0].cpu()), int(f[1].sum().cpu())))

    def _sync_result(self, name: str, asked: str):
        """What the slot ``name`` left of the last block, on the host, plus what its anchored tracks found; a synchroniser and a
        block that ran, else RuntimeError."""
        sync = getattr(self, name)
        slot = next(s for s in self._slots if s.name == name)
        last = None if sync is None else self._sync_last.get(name)
        if last is None:
            raise RuntimeError(f"{asked} needs {slot.a} and a block that ran")
        return tuple(v for kind, t in zip(slot.returns, last) for v in _HOST[kind](t)) + self._found(*(getattr(sync, f) for f in slot.found))

    def carrier_result(self):
        """(phase float64[nwin] in radians, modulo π - modulo 2π/p on the CPM links; choice uint8[nwin]) of the last block's
        recovery - synchronises.  A recovery with an ``anchor`` adds (the drift found in radians per window, the number of
        rejected windows) of its coarse track."""
        return self._sync_result("recovery", "carrier_result")

    def timing_result(self):
        """(tau float64[nwin] in samples, modulo two symbols; choice uint8[nwin]) of the last block's timing recovery -
        synchronises.  A recovery with an ``anchor`` adds (the drift found in samples per window, the number of rejected windows)
        of its coarse track."""
        return self._sync_result("timing_recovery", "timing_result")

    def acquisition_result(self):
        """(tau float64[nwin] in samples, phase float64[nwin] in radians - both modulo the lattice of waveforms_amd/sync/joint.py;
        timing choice uint8[nwin]; carrier choice uint8[nwin]) of the last block's acquisition - synchronises.  An acquisition with
        an ``anchor`` adds (the timing drift found in samples per window, the rejected windows of the coarse timing track, the carrier
        drift found in radians per window, the rejected windows of the coarse carrier track)."""
        return self._sync_result("acquisition", "acquisition_result")

    def coarse_result(self):
        """(nu in cycles per sample, eps, the peak of the summed line periodogram, its mean) of the last block's coarse
        acquisition, as floats - synchronises."""
        return self._sync_result("coarse", "coarse_result")

    def clock_result(self):
        """(tau float64[nwin] in samples, modulo nh symbols; choice uint8[nwin]; grid 0 / 1) of the last block's clock recovery -
        synchronises.  A recovery with an ``anchor`` adds (the drift found in samples per window, the number of rejected windows)
        of its coarse track."""
        return self._sync_result("clock_recovery", "clock_result")

    def joint_result(self):
        """(tau float64[nwt] in samples per timing window, phase float64[nwc] in radians per carrier window - both modulo the
        lattice of waveforms_amd/sync/joint_cpm.py; timing choice uint8[nwt]; carrier choice uint8[nwc]) of the last block's joint
        acquisition - synchronises.  An acquisition with an ``anchor`` adds (the timing drift found in samples per window, the
        rejected windows of the coarse timing track, the carrier drift found in radians per window, the rejected windows of the
        coarse carrier track)."""
        return self._sync_result("joint", "joint_result")

    def _recovered(self, rows):
        """The bank's rows through ``recovery``, the slot that turns rows."""
        if self.recovery is None:
            return rows
        rows, *self._sync_last["recovery"] = self.recovery.recover(rows, *self._differential)
        return rows

    def _rate_db(self) -> float:
        """10 log10 of information bits per channel bit: Eb/N0 is per information bit and pays for the marker."""
        return 10.0 * math.log10(self.code.k / (self.code.n_tx if self.framing is None else self.framing.period))

    def channel_bits(self, tx, stream_id: int = 0):
        """Coded bits (device ncw x n_tx) -> the burst's bits in front of the pad: the coded bits themselves, or lead bits
        (the PN23 bits that follow the block's information bits) + ``ncw`` frames (+ a zero bit to whole symbols)."""
        if self.framing is None:
            return tx.reshape(-1)
        parts = [self.framing.build(tx).reshape(-1)]
        if self.lead_bits:
            n = self.ncw * self.code.k
            parts.insert(0, dev.lfsr_bits(23, self._mask, (1 << 23) - 1, self.lead_bits, skip=(int(stream_id) + 1) * n)[0])
        if self._fill is not None:
            parts.append(self._fill)
        return _hip.torch().cat(parts) if len(parts) > 1 else parts[0]

    def deframe(self, llr, search: bool = True):
        """The whole burst's λ (aligned: λ[j] is channel bit j) -> the decoder's ncw x n_tx input.  ``search`` locks first
        (once per block: the loops keep the lock of their first pass) and counts a lock that is not (lead_bits, +)."""
        if search:
            self.framing.search(llr, self.lock)
            self.sync[0] += 1
            self.sync[1] += (self.lock[:2] != self._true_lock).any()
        return self.framing.gather(llr, self.lock, self.ncw, out=self._llr_in)

    def sync_result(self) -> tuple[int, int, tuple[int, int, float, float]]:
        """(blocks searched, wrong locks, the last lock record (p̂, σ, best value, best of the others)) - synchronises."""
        if self.framing is None:
            raise RuntimeError("sync_result needs a framing")
        _hip.check(_hip.lib().wf_ctx_check(_hip.ctx(), _hip.stream()))
        blocks, wrong = (int(v) for v in self.sync.cpu().tolist())
        rec = self.lock.cpu().numpy()
        best, other = (float(v) for v in rec[2:].view(np.float64))
        return blocks, wrong, (int(rec[0]), int(rec[1]), best, other)


class _Link(_Framed):
    """What every coded link does, whatever its waveform, its code and its loop: one block = ``ncw`` codewords of ``code`` sent
    back to back as ONE burst, PN23 information bits by ``stream_id``, Eb/N0 per INFORMATION bit (``_rate_db``).

    The waveform base under this class supplies ``bits_per_symbol``, ``_wave_init`` (pad, ``nsym``, device tables, the bank's
    filters ``_d_bank``), its synchroniser keywords (``_slots``, ``_drift``, ``_differential``, ``_check_recovery``), its part of
    the front end (``_symbols``, ``_geometry``, ``_bank``, ``_fused_bank`` where it has one), ``sigma``, the detector calls
    ``_soft`` / ``_soft_apriori``, ``_compare`` and ``_lam0``: transmitted bit j pairs with the detector's λ[j + _lam0], and
    ``_coded`` / ``_prior_coded`` are the only two places that use it.  The code supplies ``encode`` and ``_ncounts``, the
    width of ``counts``."""

    _ncounts = 4
    _fused_bank = None

    def __init__(self, code, ncw: int, sps: int, framing=None, lead_bits: int = 0, carrier=None, recovery=None) -> None:
        if ncw < 1:
            raise ValueError("ncw must be at least 1")
        self.code, self.ncw, self.sps = code, int(ncw), int(sps)
        self.llr_scale = 1.0                    # (max-log-MAP and normalized min-sum do not depend on it)
        self.nbits = self.ncw * code.n_tx
        self._frame_init(framing, lead_bits, self.bits_per_symbol)
        self.carrier = _pair("carrier", "theta0, nu", carrier)
        if recovery is not None:
            self._check_recovery(recovery)
        self.recovery = recovery
        self._wave_init()
        self._mask = generate_mask(23)
        self.counts = _hip.zeros(self._ncounts, "int64")
        self.uncoded = _hip.zeros(2, "int64")
        self.blocks = 0
        code.handle()

    def _loop_args(self, damping: float, **passes: int) -> None:
        """A loop's pass counts (``outer``, and ``inner`` where there is one) and ``damping``, checked before anything touches the
        device, and kept as attributes."""
        if min(passes.values()) < 1:
            raise ValueError(" and ".join(passes) + " must be at least 1")
        if not (math.isfinite(damping) and damping > 0.0):
            raise ValueError("damping must be finite and positive")
        self.damping = float(damping)
        for name, n in passes.items():
            setattr(self, name, int(n))

    # ---------------------------------------------------------------- stages
    def info_bits(self, stream_id: int = 0):
        n = self.ncw * self.code.k
        bits, _ = dev.lfsr_bits(23, self._mask, (1 << 23) - 1, n, skip=int(stream_id) * n)
        return bits

    def impaired(self, sig):
        """A modulated signal -> the signal under the link's impairments: ``carrier_offset`` in place, then ``timing_offset``."""
        if self.carrier is not None:
            dev.carrier_offset(sig, self.carrier[0], self.carrier[1], 0, out=sig)
        drift = getattr(self, self._drift)
        if drift is not None:
            sig = dev.timing_offset(sig, drift[0], drift[1], 0)
        return sig

    def noisy(self, sig, ebn0_db: float | None, seed: int = 1, stream_id: int = 0):
        """A signal -> the channel's noisy samples, derotated."""
        return dev.awgn(sig, int(sig.shape[0]), self.sigma(ebn0_db), seed, stream_id, 0, DEROTATION)

    def modulated(self, bits):
        """A burst's bits, pad included -> (its modulated signal, its symbols)."""
        syms = self._symbols(bits)
        return dev.cpm_modulate(syms, self._d_h, self._d_pulse, self.sps), syms

    def signal(self, tx, stream_id: int = 0):
        """Coded bits -> (the burst's impaired signal, where the bank reads it: the waveform's ``_geometry``, its symbols); ``sent``
        keeps the burst's bits."""
        bits = self.sent = _hip.torch().cat((self.channel_bits(tx, stream_id), self._pad))
        sig, syms = self.modulated(bits)
        sig = self.impaired(sig)
        return sig, self._geometry(sig), syms

    def samples(self, tx, ebn0_db: float | None, seed: int = 1, stream_id: int = 0):
        """Coded bits (device ncw x n_tx) -> (the noisy samples of the burst, where the bank reads them, its symbols)."""
        sig, at, syms = self.signal(tx, stream_id)
        return self.noisy(sig, ebn0_db, seed, stream_id), at, syms

    def front_end(self, tx, ebn0_db: float | None, seed: int = 1, stream_id: int = 0):
        """Coded bits (device ncw x n_tx) -> (matched-filter rows of the burst, its symbols): the plain bank's rows, or those a
        synchroniser makes from the samples, behind those that correct the samples."""
        sig, at, syms = self.signal(tx, stream_id)
        if self._fused_bank is not None and not self._correctors and self._row_maker is None:      # (nothing reads samples)
            return self._fused_bank(sig, *at, self.sigma(ebn0_db), seed, stream_id), syms
        received = self.noisy(sig, ebn0_db, seed, stream_id)
        for slot in self._correctors:
            received, *self._sync_last[slot.name] = getattr(self, slot.name).correct(received, out=received)
        if self._row_maker is None:
            return self._bank(received, *at), syms
        slot = self._row_maker
        rows, *self._sync_last[slot.name] = getattr(self, slot.name).recover(received, self._d_bank, *at, *self._differential)
        return rows, syms

    def _coded(self, lam, bits, search: bool = True):
        """A detector's (λ, bits) of the whole burst -> (λ of the coded bits, ncw x n_tx view; hard decisions of the channel bits
        in front of the pad).  Framed, the view is ``deframe``'s (``search``: lock first)."""
        j = self._lam0
        if self.framing is not None:
            return self.deframe(lam[j:], search), bits[j:j + self.nch]
        return lam[j:j + self.nbits].view(self.ncw, self.code.n_tx), bits[j:j + self.nbits]

    def _prior_coded(self):
        """The prior buffer's slice of the coded bits, where a decoder writes the next prior at stride n_tx; framed, the slice
        from channel bit 0 on that ``frame_scatter`` writes at the lock's position."""
        j = self._lam0
        return self.prior[j:] if self.framing is not None else self.prior[j:j + self.nbits]

    def soft(self, rows):
        """Rows -> (λ of the coded bits, ncw x n_tx view; hard decisions of the same λ)."""
        return self._coded(*self._soft(rows))

    def detect(self, rows, first: bool = False, o: int | None = None):
        """One detector pass of a loop -> (extrinsic λ of the coded bits, ncw x n_tx view; hard decisions of λ + π).  The first
        pass of a block has prior 0 everywhere and takes the plain detector (bitwise the same result)."""
        return self._coded(*self._soft_apriori(rows, None if first else self.prior), search=first)

    def channel_llrs(self, ebn0_db: float | None, seed: int = 1, stream_id: int = 0):
        """(λ ncw x n_tx of the plain detector, information bits ncw x k) of one block, on the device."""
        info = self.info_bits(stream_id)
        rows, _ = self.front_end(self.encode(info), ebn0_db, seed, stream_id)
        llr, _ = self.soft(self._recovered(rows))
        return llr.contiguous(), info.view(self.ncw, self.code.k)

    # ---------------------------------------------------------------- counts
    def reset_counts(self) -> None:
        self.counts.zero_()
        self.uncoded.zero_()
        self.blocks = 0
        if self.framing is not None:
            self.sync.zero_()

    def count_uncoded(self, hard, tx, syms=None) -> None:
        """The detector's hard decisions against the channel bits in front of the pad, into ``uncoded`` - unless a synchroniser
        leaves the rows shifted against the sent bits: there is then nothing to compare at."""
        if self._shifts is None:
            self._compare(hard, tx, syms)

    def uncoded_result(self) -> tuple[int, int]:
        """(bit errors of λ < 0 against the channel bits in front of the pad, bits compared) over the same blocks."""
        if self._shifts is not None:
            raise RuntimeError(f"uncoded_result: {self._shifts.shifted}; "
                               "the channel bits are not counted (the decoder's counts hold)")
        return int(self.uncoded.cpu()[1]), self.blocks * self.nch


class _SOQPSK(_Link):
    """The SOQPSK-TG side of a link: the channel bits plus ``PAD_BITS`` zero bits, differentially precoded, through the PT or PAM
    bank and ``viterbi_soft`` (``CodedSOQPSKLink`` states the conventions)."""

    bits_per_symbol, _lam0 = 1, 1
    _drift, _differential = "timing", (True,)                 # (the synchronisers' ``differential`` argument)
    _slots = (
        _Slot("timing_recovery", "a timing_recovery", "timing recovery", "rows", ("array", "array"), ("timing_found",), "timing.TimingRecovery",
              excludes=("carrier", "recovery"), why=_NOT_JOINT,
              framing="the instant is recovered modulo two symbols and the frame search absorbs the shift",
              shifted="a timing recovery leaves the rows two rows early or late in some bursts"),
        _Slot("acquisition", "an acquisition", "acquisition", "rows", ("array",) * 4, ("timing_found", "carrier_found"), "joint.JointAcquisition",
              excludes=("recovery", "timing_recovery"), why=_ACQUIRES,
              framing="the instant and the phase are recovered modulo (sps, π/2) and (0, π), and the frame search absorbs the shift and the polarity",
              shifted="an acquisition leaves the rows a few rows early or late, and inverted, in some bursts"),
        _Slot("coarse", "a coarse acquisition", "coarse acquisition", "samples", ("floats",), (), "coarse.CoarseFrequency",
              excludes=("timing_recovery",), why="that path has no carrier recovery behind it",
              needs=("recovery", "acquisition"),
              needs_what="a recovery or an acquisition: it leaves the residual frequency and the phase to them"),
        _Slot("recovery", "a recovery", "recovery", "turns", ("array", "array"), ("carrier_found",)),
    )

    def __init__(self, code, ncw: int, sps: int = 8, detector: str = "PT", *, timing=None, timing_recovery=None, acquisition=None, coarse=None,
                 **burst) -> None:
        if detector not in TIMING_OFFSET:
            raise ValueError(f"unknown detector {detector!r}")
        self.detector = detector
        self._sync_init(int(sps), dict(burst, timing=timing, timing_recovery=timing_recovery, acquisition=acquisition, coarse=coarse))
        super().__init__(code, ncw, sps, **burst)

    def _wave_init(self) -> None:
        self.nsym = self.nch + PAD_BITS
        pulse = freq_pulse_soqpsk_tg(self.sps)
        taps = (pt_matched_filter_taps if self.detector == "PT" else pam_matched_filter_taps)(pulse, 0.25, self.sps)
        self._d_h = _hip.to_device(np.array([0.25]))
        self._d_pulse = _hip.to_device(pulse)
        self._d_taps = self._d_bank = _hip.to_device(np.ascontiguousarray(taps))
        self._tables = SOQPSKTrellis4x2DiffEncoded.dense_tables()
        self._pad = _hip.zeros(PAD_BITS, "uint8")

    def sigma(self, ebn0_db: float | None) -> float:
        if ebn0_db is None:
            return 0.0
        return sigma_for_ebn0(float(ebn0_db) + self._rate_db(), self.sps)

    def _symbols(self, bits):
        return dev.fsm_encode(*self._tables, bits)[0]

    def _geometry(self, sig, nsym: int | None = None):
        """Where the bank reads ``sig``: the link's own burst, or (``nsym``) a burst of another length."""
        first, ncols = dev.decimation(int(sig.shape[0]), self.sps, 2, TIMING_OFFSET[self.detector])
        if nsym is None and ncols < self.nch + 1:
            raise RuntimeError(f"{ncols} detector rows for {self.nch} channel bits")
        return first, ncols

    def _bank(self, received, first: int, ncols: int):
        return dev.mf_bank(received, self._d_taps, first, self.sps, ncols)

    def _fused_bank(self, sig, first: int, ncols: int, sigma: float, seed: int, stream_id: int):
        return dev.awgn_mf_bank(sig, self._d_taps, first, self.sps, ncols, sigma, seed, stream_id, 0, DEROTATION)

    def _check_recovery(self, recovery) -> None:
        from ..sync.carrier import CarrierRecovery

        if not isinstance(recovery, CarrierRecovery):
            raise ValueError("an SOQPSK-TG link's recovery is a waveforms_amd.sync.carrier.CarrierRecovery")
        if self.framing is None:
            raise ValueError("recovery needs a framing: the phase is recovered modulo π and the frame search's polarity resolves the rest")

    def _soft(self, rows):
        return dev.viterbi_soft(rows, True)

    def _soft_apriori(self, rows, prior):
        return dev.viterbi_soft_apriori(rows, prior, self.damping)

    def _compare(self, hard, tx, syms) -> None:
        dev.count_errors(syms, syms, hard, self.sent, self.nch, self.uncoded)


class _CPM(_Link):
    """The ARTM multi-h / PCM/FM side of a link: the channel bits from call 0 plus ``PAD_SYMS`` zero symbols, through the generic
    CPM trellis and ``cpm_soft`` (``CodedCPMLink`` states the chain and the conventions)."""

    _lam0 = 0
    bits_per_symbol = property(lambda self: self.spec.bits_per_symbol)
    _drift, _differential = "clock", ()
    _slots = (
        _Slot("clock_recovery", "a clock_recovery", "clock recovery", "rows", ("array", "array", "int"), ("timing_found",),
              "timing_cpm.CPMTimingRecovery", excludes=("carrier", "recovery"), why=_NOT_JOINT, design=True,
              framing="the instant is recovered modulo nh symbols and the frame search absorbs the shift",
              shifted="a clock recovery leaves the rows a whole number of periods early or late in some bursts"),
        _Slot("joint", "a joint acquisition", "joint acquisition", "rows", ("array",) * 4, ("timing_found", "carrier_found"),
              "joint_cpm.CPMJointAcquisition", excludes=("recovery", "clock_recovery"), why=_ACQUIRES, design=True,
              framing="the instant and the phase are recovered modulo (nh sps, P/2) and (0, P), and the frame search absorbs the shift",
              shifted="a joint acquisition leaves the rows a whole number of periods early or late in some bursts"),
        _Slot("recovery", "a recovery", "recovery", "turns", ("array", "array"), ("carrier_found",)),
    )

    def __init__(self, code, ncw: int, waveform: str = "multih", sps: int = 8, *, clock=None, clock_recovery=None, joint=None, **burst) -> None:
        from ..viterbi import cpm

        if waveform not in CPM_WAVEFORMS:
            raise ValueError(f"unknown waveform {waveform!r}")
        if waveform == "multih" and code.n_tx % 2:
            raise ValueError(f"ARTM sends two bits per symbol: a code with an odd n_tx = {code.n_tx} is refused")
        self.waveform, self.spec = waveform, cpm.ARTM_64 if waveform == "multih" else cpm.PCMFM_20
        self._sync_init(int(sps), dict(burst, clock=clock, clock_recovery=clock_recovery, joint=joint))
        super().__init__(code, ncw, sps, **burst)

    def _wave_init(self) -> None:
        from ..viterbi import cpm

        if self.waveform == "multih":
            from ..cpm.multih import freq_pulse_multih_irig as freq_pulse
        else:
            from ..cpm.pcmfm import freq_pulse_pcmfm as freq_pulse
        spec, lg = self.spec, self.spec.bits_per_symbol
        self.nsym = (self.nch + lg - 1) // lg + PAD_SYMS
        pulse = np.asarray(freq_pulse(self.sps), dtype=np.float64)
        geo = cpm.filter_geometry(pulse.size, self.sps, spec, self.nsym)
        self.start0, self.ncalls = int(geo["start0"]), int(geo["ncalls"])
        if self.ncalls * lg < self.nch:
            raise RuntimeError(f"{self.ncalls} detector calls for {self.nch} channel bits")
        self._d_h = _hip.to_device(spec.mod_index)
        self._d_pulse = _hip.to_device(pulse)
        self._d_templates = self._d_bank = _hip.to_device(cpm.matched_filter_templates(pulse, self.sps, cpm.full_phase(spec)))
        self._d_rot = _hip.to_device(cpm.rotation_table(spec))
        self._pad = _hip.zeros(PAD_SYMS * lg, "uint8")

    def sigma(self, ebn0_db: float | None) -> float:
        from ..viterbi.cpm import sigma_for_ebn0 as cpm_sigma

        if ebn0_db is None:
            return 0.0
        return cpm_sigma(float(ebn0_db) + self._rate_db(), self.sps, self.spec.bits_per_symbol)

    def _symbols(self, bits):
        return dev.symbol_map(CPM_WAVEFORMS[self.waveform], bits)

    def _geometry(self, sig, nsym: int | None = None):
        if nsym is None:
            return self.start0, self.ncalls
        from ..viterbi import cpm

        geo = cpm.filter_geometry(int(self._d_pulse.numel()), self.sps, self.spec, int(nsym))
        return int(geo["start0"]), int(geo["ncalls"])

    def _bank(self, received, start0: int, ncalls: int):
        """Rows float64[ncalls, nfilt, 2]."""
        return dev.cpm_mf_rows(received, self._d_templates, start0, self.sps, ncalls)

    def _check_recovery(self, recovery) -> None:
        from ..sync.carrier_cpm import CPMCarrierRecovery

        if not isinstance(recovery, CPMCarrierRecovery):
            raise ValueError("a CPM link's recovery is a waveforms_amd.sync.carrier_cpm.CPMCarrierRecovery")
        if recovery.spec != self.spec:
            raise ValueError(f"the recovery is for another design than the link's {self.waveform!r} full-phase trellis")

    def _soft(self, rows):
        return dev.cpm_soft(rows, self.spec, 0, 0, d_rot=self._d_rot)

    def _soft_apriori(self, rows, prior):
        return dev.cpm_soft_apriori(rows, self.spec, prior, self.damping, 0, 0 if prior is None else self.prior_warmup, d_rot=self._d_rot)

    def _compare(self, hard, tx, syms) -> None:
        flat = tx.reshape(-1) if self.framing is None else self.sent
        dev.count_errors(hard, flat, hard, flat, self.nch, self.uncoded)     # (bits in both pairs: [1] is what is read)


class _LDPC:
    """An LDPC code on a link: ``ldpc_encode``, and per block one ``ldpc_decode`` (normalized min-sum with ``alpha``, at most
    ``max_iter`` iterations) that also counts."""

    def encode(self, info):
        return dev.ldpc_encode(self.code, info)

    def run_block(self, ebn0_db: float | None, seed: int = 1, stream_id: int = 0) -> None:
        """Queue one block on the current stream; the counts accumulate on the device."""
        info = self.info_bits(stream_id)
        tx = self.encode(info)
        rows, syms = self.front_end(tx, ebn0_db, seed, stream_id)
        llr, hard = self.soft(self._recovered(rows))
        self.count_uncoded(hard, tx, syms)
        dev.ldpc_decode(self.code, llr, scale=self.llr_scale, alpha=self.alpha, max_iter=self.max_iter, ref_info=info,
                        counts=self.counts)
        self.blocks += 1

    def result(self) -> tuple[int, int, int, int, float]:
        """(information bit errors, codeword errors, codewords not converged, information bits compared, mean
        iterations) - synchronises."""
        _hip.check(_hip.lib().wf_ctx_check(_hip.ctx(), _hip.stream()))
        be, fe, nc, its = (int(v) for v in self.counts.cpu().tolist())
        ncw = self.blocks * self.ncw
        return be, fe, nc, ncw * self.code.k, (its / ncw if ncw else 0.0)


class CodedSOQPSKLink(_LDPC, _SOQPSK):
    """One block = ``ncw`` codewords of ``code`` sent back to back as ONE SOQPSK-TG burst (plus ``PAD_BITS`` zero bits).

    Eb/N0 is per INFORMATION bit: the channel's σ is ``sigma_for_ebn0(ebn0_db + 10 log10(k / n_tx), sps)``, i.e. the
    channel runs at Eb/N0 + 10 log10(rate) per transmitted bit (-3.01 dB for the rate-1/2 demo code).

    The information bits are PN23 (from the all-ones state), block b = ``stream_id`` taking the segment that starts at
    bit b ncw k.  The noise is the library's counter-based AWGN keyed by (``seed``, ``stream_id``).  Transmitted bit j
    is paired with the soft detector's λ_{j+1} (include/wfhip.h, wf_viterbi4_soft).  ``ebn0_db=None`` is noiseless."""

    def __init__(self, code, ncw: int, sps: int = 8, detector: str = "PT", alpha: float = 0.75, max_iter: int = 50, framing=None,
                 lead_bits: int = 0, carrier=None, recovery=None, timing=None, timing_recovery=None, acquisition=None, coarse=None) -> None:
        self.alpha, self.max_iter = float(alpha), int(max_iter)
        super().__init__(code, ncw, sps, detector, timing=timing, timing_recovery=timing_recovery, acquisition=acquisition, coarse=coarse,
                         framing=framing, lead_bits=lead_bits, carrier=carrier, recovery=recovery)


class CodedCPMLink(_LDPC, _CPM):
    """``CodedSOQPSKLink`` for ARTM multi-h (``waveform="multih"``) and PCM/FM (``"pcmfm"``): one block = ``ncw`` codewords of
    ``code`` sent back to back as ONE burst from call 0, plus ``PAD_SYMS`` zero symbols.

    coded bits -> ``symbol_map`` -> ``cpm_modulate`` with the waveform's modulation indices -> ``awgn`` (with the e^{-jπ/4}
    derotation of the CPM chains) -> ``cpm_mf_rows`` with the waveform's matched-filter templates -> ``cpm_soft`` on the
    full-phase trellis (``ARTM_64``: 64 states, ``PCMFM_20``: 20 states) -> ``ldpc_decode``.  Transmitted bit j pairs with
    λ[j] (include/wfhip.h, wf_cpm_soft).

    Eb/N0 is per INFORMATION bit: σ = ``viterbi.cpm.sigma_for_ebn0(ebn0_db + 10 log10(k / n_tx), sps, bits_per_symbol)``.
    Information bits, noise keys and result tuples are ``CodedSOQPSKLink``'s: PN23 by ``stream_id``, counter-based AWGN keyed
    by (``seed``, ``stream_id``); ``ebn0_db=None`` is noiseless.  ARTM carries two bits per symbol, so a code whose ``n_tx`` is
    odd is refused for it (a codeword would end inside a symbol).  The burst is detected from a free start, before any symbol
    has been sent: the λ of its FIRST symbol is weak and can have the wrong sign even without noise, which costs the burst's
    first codeword at most lgM channel errors (one decoder iteration when there is no noise)."""

    def __init__(self, code, ncw: int, waveform: str = "multih", sps: int = 8, alpha: float = 0.75, max_iter: int = 50, framing=None,
                 lead_bits: int = 0, clock=None, clock_recovery=None, joint=None, carrier=None, recovery=None) -> None:
        self.alpha, self.max_iter = float(alpha), int(max_iter)
        super().__init__(code, ncw, waveform, sps, framing=framing, lead_bits=lead_bits, clock=clock, clock_recovery=clock_recovery,
                         joint=joint, carrier=carrier, recovery=recovery)


class _LDPCLoop:
    """Iterative detection and decoding over a ``Coded*Link`` (which it precedes in the bases): the front end runs once per
    block, then ``outer`` passes of

        the waveform's soft detector with the burst's prior buffer (apriori_scale = ``damping``)
        -> ``ldpc_decode_ext`` (``inner`` iterations from a cold start) writing the next prior at ``_prior_coded``, stride n_tx

    and one ``ldpc_count``.  A codeword whose syndrome is zero is FROZEN: its prior becomes ±``ext_sat`` by its decisions and
    later passes leave it alone (without this a converged codeword would hand back zero extrinsic and be decoded from
    scratch on the next pass, and the loop oscillates).  The rows or calls outside the coded bits keep prior 0.  Max-log-MAP and
    normalized min-sum are both scale-invariant, so the loop needs no noise-variance scale (``llr_scale`` stays 1).

    ``ext_sat`` / ``ext_clip`` are in the detector's metric units, which grow linearly with ``sps`` (the matched filters
    sum sps + 1 unit-magnitude taps): the defaults are ext_sat = 6.25 sps (50 at sps 8) and no clip.  ``outer`` is fixed per
    block and nothing synchronises with the host inside one; every pass is queued even when every codeword is already frozen
    (the decoder's workgroups then retire at once, the detector still runs).  ``per_pass=True`` also accumulates the four
    counts after every pass (``pass_results``).  Framed, ``marker_prior`` (default ``ext_sat``) is the known-bits prior on the
    marker rows."""

    def __init__(self, code, ncw: int, *, sps: int, outer: int, inner: int, damping: float, ext_clip: float | None, ext_sat: float | None,
                 per_pass: bool, marker_prior: float | None, **link) -> None:
        self._loop_args(damping, outer=outer, inner=inner)
        self.ext_sat = 6.25 * int(sps) if ext_sat is None else float(ext_sat)
        self.ext_clip = math.inf if ext_clip is None else float(ext_clip)
        if not (math.isfinite(self.ext_sat) and self.ext_sat > 0.0 and self.ext_clip > 0.0):
            raise ValueError("ext_sat must be finite and positive, ext_clip positive")
        self.marker_prior = self.ext_sat if marker_prior is None else float(marker_prior)
        if not math.isfinite(self.marker_prior):
            raise ValueError("marker_prior must be finite")
        super().__init__(code, ncw, sps=sps, max_iter=inner, **link)
        self.per_pass = bool(per_pass)
        self.pass_counts = _hip.zeros((self.outer, 4), "int64")
        self.prior = self.state = self.iters = self.decided = self.ext = None

    # ---------------------------------------------------------------- stages
    def _begin(self, n: int) -> None:
        """Fresh loop state of one block for a prior of ``n`` values: prior 0, every codeword open, no iterations."""
        if self.prior is None or self.prior.numel() != n:
            self.prior = _hip.zeros(n, "float32")
            self.state = _hip.zeros(self.ncw, "uint8")
            self.iters = _hip.zeros(self.ncw, "int32")
            self.decided = _hip.zeros((self.ncw, self.code.k), "uint8")
            self.ext = None if self.framing is None else _hip.zeros((self.ncw, self.code.n_tx), "float32")
        else:
            for t in (self.prior, self.state, self.iters, self.decided, self.ext):
                if t is not None:
                    t.zero_()

    def decode(self, ext) -> None:
        """One decoder pass over the open codewords: decisions, iterations, states and the next prior, in place.  Framed: the
        extrinsic values go to the contiguous ``ext`` buffer (frozen codewords keep theirs) and ``frame_scatter`` puts all of
        them, and ±``marker_prior`` on the marker rows, into the prior at the lock's position."""
        dev.ldpc_decode_ext(self.code, ext, self.state, self._prior_coded() if self.framing is None else self.ext, self.code.n_tx,
                            scale=self.llr_scale, alpha=self.alpha, max_iter=self.inner, ext_clip=self.ext_clip, ext_sat=self.ext_sat,
                            info_bits=self.decided, iters=self.iters)
        if self.framing is not None:
            self.framing.scatter(self.ext, self.lock, self._prior_coded(), self.marker_prior)

    # ---------------------------------------------------------------- blocks
    def run_block(self, ebn0_db: float | None, seed: int = 1, stream_id: int = 0) -> None:
        info = self.info_bits(stream_id)
        tx = self.encode(info)
        rows, syms = self.front_end(tx, ebn0_db, seed, stream_id)
        rows = self._recovered(rows)
        self.begin(int(rows.shape[0]))
        for o in range(self.outer):
            ext, hard = self.detect(rows, first=o == 0, o=o)
            if o == 0:
                self.count_uncoded(hard, tx, syms)
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


class IterativeSOQPSKLink(_LDPCLoop, CodedSOQPSKLink):
    """``CodedSOQPSKLink`` with iterative detection and decoding (``_LDPCLoop``): same block layout, PN23 information bits, noise
    keys, Eb/N0 convention and result tuples; the detector is ``viterbi_soft_apriori`` and the next prior is written at offset
    +1: row 0 and the tail rows keep prior 0.  At the default ``ext_sat`` of 50 at sps 8, mean |λ| is about 11 at 4.5 dB.

    ``live_only=True`` is the answer to the loop's remark that the detector runs even when every codeword is frozen: pass 1 is
    unchanged, every later pass first turns the states the
    previous decoder pass left into the burst's live windows (``idd_windows``: the rows of the open codewords and ``guard``
    rows on either side, on the device) and runs the detector on those rows only (``viterbi_soft_apriori_windows``), into the
    ONE ext / bits buffer the block keeps: rows outside the windows hold an earlier pass's values, and the decoder never
    reads a frozen codeword's input.  Still no host synchronisation and a fixed ``outer``; a pass with nothing open costs
    launches that find nothing.  A window's edges start from free metrics instead of the burst's history, so this is the
    full loop exactly only when the metrics merge within the guard; the frozen neighbours' saturated priors pin the trellis
    within a few rows, and INTEGRATION.md has the counts behind the default of 128 rows (``guard >= nrows`` makes any open
    codeword's window the whole burst: the full loop bit for bit).  ``live_results`` returns what each pass worked on."""

    def __init__(self, code, ncw: int, sps: int = 8, detector: str = "PT", alpha: float = 0.75, outer: int = 8, inner: int = 5,
                 damping: float = 0.7, ext_clip: float | None = None, ext_sat: float | None = None, per_pass: bool = False, framing=None,
                 lead_bits: int = 0, marker_prior: float | None = None, live_only: bool = False, guard: int = DEFAULT_GUARD, carrier=None,
                 recovery=None, timing=None, timing_recovery=None, acquisition=None, coarse=None) -> None:
        if int(guard) < 0:
            raise ValueError(f"guard = {guard} must not be negative")
        self.live_only, self.guard = bool(live_only), int(guard)
        super().__init__(code, ncw, sps=sps, detector=detector, alpha=alpha, outer=outer, inner=inner, damping=damping, ext_clip=ext_clip,
                         ext_sat=ext_sat, per_pass=per_pass, framing=framing, lead_bits=lead_bits, marker_prior=marker_prior, carrier=carrier,
                         recovery=recovery, timing=timing, timing_recovery=timing_recovery, acquisition=acquisition, coarse=coarse)
        self.live_counts = _hip.zeros((self.outer, 3), "int64") if self.live_only else None
        self.windows = _hip.zeros(4 + 2 * self.ncw, "int64") if self.live_only else None
        self._live_out, self._live_first = None, 0          # the block's ext / bits buffers; first passes run

    # ---------------------------------------------------------------- stages
    def begin(self, nrows: int) -> None:
        """Fresh loop state of one block: prior 0 on every row, every codeword open, no iterations."""
        self._live_out = None
        self._begin(nrows)

    def live_windows(self, nrows: int):
        """The live windows of the burst's ``nrows`` rows for the states as they are now -> the device table of ``idd_windows``
        (kept in ``windows``).  Coded bit j is row j + 1; framed, codeword 0 starts behind the lock's p̂ and one marker."""
        if self.framing is None:
            return dev.idd_windows(self.state, nrows, self.code.n_tx, guard=self.guard, out=self.windows)
        return dev.idd_windows(self.state, nrows, self.code.n_tx, self.framing.period, 1, self.lock, self.framing.L, self.guard, out=self.windows)

    def detect(self, rows, first: bool = False, o: int | None = None):
        """One detector pass, as every loop's.  ``live_only``: every later pass works on the live windows only and writes into
        the first pass's buffers; ``o`` is the pass whose entry of ``live_results`` gets the table's counts (None: nobody's)."""
        if not self.live_only:
            return super().detect(rows, first)
        if first:
            ext, bits = self._live_out = self._soft_apriori(rows, None)
            self._live_first += o is not None
        else:
            if self._live_out is None:
                raise RuntimeError("live_only: the block's first pass (first=True) has not run")
            table = self.live_windows(int(self._live_out[0].numel()))
            if o is not None:
                self.live_counts[o] += table[:3]
            ext, bits = dev.viterbi_soft_apriori_windows(rows, self.prior, table, self.damping, out=self._live_out)
        return self._coded(ext, bits, search=first)

    # ---------------------------------------------------------------- blocks
    def reset_counts(self) -> None:
        super().reset_counts()
        if self.live_only:
            self.live_counts.zero_()
            self._live_first = 0

    def live_results(self) -> list[tuple[int, int, int]]:
        """Per outer pass (``live_only=True``): (windows, live rows, codewords open on entry), summed over the blocks
        run since ``reset_counts`` - synchronises.  Pass 1 is the plain detector on the whole burst: one
        window of every row, every codeword open.  The later entries are the words [0 .. 2] of the passes' window tables,
        added up on the device."""
        if not self.live_only:
            raise RuntimeError("live_results needs live_only=True")
        _hip.check(_hip.lib().wf_ctx_check(_hip.ctx(), _hip.stream()))
        rest = [tuple(int(v) for v in row) for row in self.live_counts.cpu().tolist()[1:]]
        nrows = 0 if self.prior is None else int(self.prior.numel())
        return [(self._live_first, self._live_first * nrows, self._live_first * self.ncw)] + rest


class IterativeCPMLink(_LDPCLoop, CodedCPMLink):
    """``CodedCPMLink`` with iterative detection and decoding, the loop of ``IterativeSOQPSKLink`` (``_LDPCLoop``) on the generic
    CPM trellis: the detector is ``cpm_soft_apriori`` and the next prior is written at offset 0.  The detector's output is
    extrinsic per BIT: for ARTM the prior of the other bit of the same
    quaternary symbol stays in, a bit's own never does.  Frozen codewords, ``per_pass``, ``ext_clip`` and the result tuples
    are ``IterativeSOQPSKLink``'s; the tail calls keep prior 0.  The phase state makes a CPM modulator a recursive inner code,
    which is where iterating pays most.

    ``ext_sat`` is in the detector's metric units, which grow linearly with ``sps``.  Default, both waveforms: 6.25 sps (50
    at sps 8), the SOQPSK loop's value.  It was chosen from the mean |λ| of one plain pass at sps 8 — about 4 for ARTM at
    7 dB and about 16 for PCM/FM at 3 dB information Eb/N0, against 11 for SOQPSK-TG at 4.5 dB — as the value that is at
    least three times every one of them (a frozen codeword's bits must outweigh the channel in the neighbouring sections)
    and with which the CPU restatement of the loop reaches no frame error in 40 at both operating points
    (tests/test_cpm_idd.py).

    ``prior_warmup``: the detector's warm-up, in calls, on the passes that carry a prior (0: the library's 64).  The warm-up
    never changes a result, only how many chunks the proof sends to the repair; a saturated prior pins the inputs, paths
    from different phase states then stop merging, and with 64 calls EVERY chunk of a frozen block failed its proof in both
    directions (16 232 repairs on 8 117 chunks, a pass at 1.8 - 1.9 times the plain one).  With 512 calls none did (1.04 -
    1.09 times; INTEGRATION.md has the measurement)."""

    def __init__(self, code, ncw: int, waveform: str = "multih", sps: int = 8, alpha: float = 0.75, outer: int = 8, inner: int = 5,
                 damping: float = 0.7, ext_clip: float | None = None, ext_sat: float | None = None, per_pass: bool = False,
                 prior_warmup: int = 512, framing=None, lead_bits: int = 0, marker_prior: float | None = None, clock=None,
                 clock_recovery=None, joint=None, carrier=None, recovery=None) -> None:
        if prior_warmup < 0:
            raise ValueError("prior_warmup must not be negative")
        self.prior_warmup = int(prior_warmup)
        super().__init__(code, ncw, waveform=waveform, sps=sps, alpha=alpha, outer=outer, inner=inner, damping=damping, ext_clip=ext_clip,
                         ext_sat=ext_sat, per_pass=per_pass, framing=framing, lead_bits=lead_bits, marker_prior=marker_prior, clock=clock,
                         clock_recovery=clock_recovery, joint=joint, carrier=carrier, recovery=recovery)

    def begin(self, ncalls: int | None = None) -> None:
        """Fresh loop state of one block: prior 0 on every bit of every call, every codeword open, no iterations."""
        self._begin((self.ncalls if ncalls is None else int(ncalls)) * self.spec.bits_per_symbol)
