"""Coded BER / FER curve of the LDPC-coded SOQPSK-TG, ARTM multi-h or PCM/FM chain (waveforms_amd/encoding/coded.py) and the
decoder's speed; prints ONE JSON line.

    python tools/coded_ber.py [--waveform soqpsk|multih|pcmfm] [--code demo|demo16k] [--ebn0 4 5 6 7 8] [--codewords N]
                              [--detector PT] [--steps 5] [--outer N --inner M --damping D]
                              [--framed [--lead-bits J] [--marker-prior X]] [--live-only [--guard G]]
    python tools/coded_ber.py --code conv-k3|conv-k7 [--info-bits K] [--interleave] [--outer N --damping D] [--ebn0 ...]
    python tools/coded_ber.py --code conv-k3|conv-k7 --rs 16|8 [--rs-depth I] [--rs-n N] [--rs-erasures F [--rs-erase-below X]] ...
    python tools/coded_ber.py --carrier-phase DEG --carrier-freq NU --recover [--carrier-window W --carrier-hyp H] [--ebn0 ...]
    python tools/coded_ber.py [--waveform multih|pcmfm] --timing-offset TAU --timing-drift EPS --recover-timing [--timing-window W --timing-hyp H --timing-refine R]
    python tools/coded_ber.py --carrier-phase DEG --carrier-freq NU --timing-offset TAU --timing-drift EPS --acquire
                              [--acq-timing-hyp Ht --acq-carrier-hyp Hc [Hc2 ...] --acq-stack N --acq-time-rows N1 N2 --acq-out PATH]

``--waveform soqpsk`` (default) is CodedSOQPSKLink / IterativeSOQPSKLink with ``--detector``; ``multih`` and ``pcmfm`` are
CodedCPMLink / IterativeCPMLink on the full-phase trellis (``--detector`` is not used).

Eb/N0 is per information bit.  Per point: coded BER and FER, codewords not converged, mean iterations, and the soft
detector's uncoded BER (λ < 0 against the coded bits) on the same channel bits.  Each block is one burst of
``--block-codewords`` codewords; blocks run until ``--codewords`` have been decoded.  Timing: ``--steps`` more blocks at the
point, each stage bracketed by device events (encode, front end = PRBS + precoder + modulator + channel + matched filters,
soft detector, decode); the decoder's throughput is information bits / decode time.

With ``--outer N`` (> 0) every point also runs the iterative chain (IterativeSOQPSKLink: N outer passes of ``--inner`` decoder
iterations, prior scaled by ``--damping``) on the SAME blocks, next to the one-pass curve: BER / FER and open codewords after
every pass, total inner iterations, and the time per block split into the detector passes and the decoder passes (each pass
bracketed by device events; the first detector pass is the plain detector).

With ``--framed`` every point also runs the FRAMED link (waveforms_amd/encoding/framing.py: the default marker and the
randomiser in front of every codeword, ``--lead-bits`` pseudo-random bits in front of the burst) on the same number of
codewords per burst, next to the unframed curve and at the same information Eb/N0 (which now pays for the marker): the same
counts, the wrong locks, the last lock record, and the times of ``frame_search``, ``frame_gather`` and ``frame_scatter`` on
the burst (device events).  With ``--outer`` the framed iterative link runs too, the marker rows carrying
``--marker-prior`` (default: ext_sat; 0 = no marker prior).

With ``--live-only`` (SOQPSK-TG, with ``--outer``) every iterative link, framed or not, gets a twin with ``live_only=True`` and
``--guard`` rows of guard, run on the SAME blocks: its counts after every pass, what every pass worked on (windows, live rows,
codewords open on entry, summed over the blocks), the number of codewords whose FINAL decisions differ from the full loop's,
and the per-pass detector and decoder times of both loops from the same run: ``--steps`` timed blocks after one warm-up
block, full and windowed alternating (device events; a windowed detector pass includes the window table, a framed one the
gather, a framed decoder pass the scatter).

``--code conv-k3`` / ``conv-k7`` (SOQPSK-TG only) is ConvSOQPSKLink (waveforms_amd/encoding/sccc.py) with the (7, 5) or the
(171, 133) convolutional code of ``--info-bits`` information bits (default: n = 2048) and, with ``--interleave``, the QPP
interleaver (31 t + 64 t^2) mod n: ``--outer`` passes (0 or 1: one pass with the plain detector) of soft detector and
max-log-MAP decoder.  Per point: BER / FER (after every pass), the uncoded BER, and the time per block of the encoder, the
front end and every detector and decoder pass (device events; the same device calls ``run_block`` makes, so with one pass
the plain detector and a decoder that writes no extrinsic output), with the decoder's information bits per second of one pass.

With ``--rs E`` the link is RSConvSOQPSKLink (waveforms_amd/encoding/rsconv.py): the CCSDS Reed-Solomon code correcting E = 16 or 8
symbols (``--rs-n``: shortened), interleaved to ``--rs-depth``, in front of the convolutional code, whose ``--info-bits`` are then
fixed at one RS frame (8 n I).  Eb/N0 is per USER bit.  Every point gains an ``"rs"`` entry: BER and FER after the RS decoder
next to the inner code's, flagged failures, miscorrections, symbols corrected, and the time per block of ``rs_encode`` and of
``rs_decode`` (device events around those two calls alone, the same ``--steps`` blocks) with its ratio to the ``conv_siso`` passes
of the block.  Without ``--rs`` the output is unchanged.

With ``--rs-erasures F`` the link also declares erasures (``rs_mark_erasures``: per RS codeword the at most F symbols of smallest
reliability below ``--rs-erase-below``, from the last inner pass's Λ) and decodes errors and erasures; the errors-only decoder
runs on the SAME decisions of the same blocks, and stays the ``"rs"`` entry.  Every point gains ``"rs_erasures"``: BER and FER,
flagged failures, miscorrections, symbols corrected, erasures declared / filled, and from the same timed blocks the device-event
times of ``rs_mark_erasures``, of ``rs_decode`` with erasures and of ``rs_decode`` without, with their ratio.

With ``--carrier-phase DEG`` / ``--carrier-freq NU`` (cycles per sample) and ``--recover`` (LDPC codes) the tool runs
three FRAMED CodedSOQPSKLink on the same blocks and prints three curves: ``genie`` (no carrier offset: today's link),
``impaired`` (the offset, no recovery) and ``recovered`` (the offset and ``CarrierRecovery`` with ``--carrier-window`` rows per
window, ``--carrier-hyp`` hypotheses, ``--carrier-span``, ``--carrier-refine``).  With ``--waveform multih|pcmfm`` the three are
unframed CodedCPMLink and the recovery is ``CPMCarrierRecovery`` (``--carrier-hyp`` defaults to the class's 2).  It also prints the recovery's kernel times per
block (device events around every stage, summed over the passes, ``--steps`` blocks after one warm-up) beside one plain soft
detection of the same rows, and ``loss_db_at_fer_1e-2``: recovered minus genie, both interpolated in log FER (null where a
curve does not cross 1e-2 inside the sweep).  ``--coarse [--coarse-nfft N --coarse-smooth S]`` (SOQPSK-TG) adds two curves on the
same blocks: ``coarse``, a ``CoarseFrequency`` in front of the same recovery, and ``reference``, that recovery at ``--carrier-freq
0`` - with the estimates' statistics over the bursts, the bursts in which the coarse link loses codewords the reference keeps
(with the burst's frequency error), the coarse stage's times and ``coarse_cost_db_at_fer_1e-2``: coarse minus reference.  Beside
``--acquire`` it does the same around the acquisition (the anchored one with ``--anchor``), the reference under the same timing
offset; the estimates are held against the frequency in cycles per RECEIVED sample, NU (1 + EPS), and against EPS.

With ``--timing-offset TAU`` (samples) / ``--timing-drift EPS`` (samples per sample) and ``--recover-timing`` the tool does the
same for the symbol timing of the framed SOQPSK-TG link: ``genie`` (no offset), ``impaired`` (``timing=(TAU, EPS)``, no recovery)
and ``recovered`` (the offset and ``TimingRecovery`` with ``--timing-window``, ``--timing-hyp``, ``--timing-span``,
``--timing-refine``, ``--timing-delta``) on the same blocks, the recovery's stage times beside the fused front end and one
soft detection, and the same ``loss_db_at_fer_1e-2``.  With ``--waveform multih|pcmfm`` the three links are ``CodedCPMLink``s with
``clock=(TAU, EPS)`` and a ``CPMTimingRecovery`` whose window, hypotheses and delta default per waveform; the front end beside
the recovery is then ``awgn`` + ``cpm_mf_rows``, the detection ``cpm_soft``, and every point also has the ``grid`` decision.

With ``--acquire`` both impairments are applied at once (``--carrier-*`` and ``--timing-*``) and the third link runs a
``JointAcquisition`` (``--acq-timing-hyp`` instants over one symbol, ``--acq-carrier-hyp`` rotations; window, span, refine and
delta from the ``--timing-*`` flags): ``genie``, ``impaired`` and ``acquired`` on the same blocks, one more acquired curve per
further value of ``--acq-carrier-hyp``, ``loss_db_at_fer_1e-2`` per acquired curve, and under ``one_acquisition`` the time of
one acquisition of a burst of each ``--acq-time-rows`` length - device events around the whole call after a warm-up, ``stack=1``
(the existing entry points per hypothesis) against the default stacking, with the launch counts, the stage times and the
time in units of one plain soft detection of as many rows.  The result is also written to ``--acq-out``
(profiles/joint_acquisition.json).

``--anchor K`` (with ``--recover-timing`` or ``--acquire``) adds an ``anchored`` link whose synchroniser has ``anchor=K`` (the
anchored unwrapping of include/wfhip.h) beside the unanchored one on the same blocks: its curve, the windows its coarse tracks
rejected per point, its loss, and with ``--acquire`` one more timed acquisition (``stack_default_anchored``).
"""
import argparse
import json
import sys
from pathlib import Path
from typing import NamedTuple

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def time_loops(links, code, ebn0, first_block, steps):
    """Per-pass detector and decoder times (ms per block, device events) of several loops on the same blocks, the loops
    alternating block by block; one warm-up block each, not timed -> (det[len(links), outer], dec[...])."""
    import torch

    from waveforms_amd import device as dev

    outer = links[0].outer
    pev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * outer + 1)]
    det, dec = np.zeros((len(links), outer)), np.zeros((len(links), outer))
    for s in range(steps + 1):
        for i, lk in enumerate(links):
            tx = dev.ldpc_encode(code, lk.info_bits(first_block + s))
            rows, _ = lk.front_end(tx, ebn0, 1, first_block + s)
            lk.begin(int(rows.shape[0]))
            pev[0].record()
            for o in range(outer):
                ext, _ = lk.detect(rows, first=o == 0)
                pev[2 * o + 1].record()
                lk.decode(ext)
                pev[2 * o + 2].record()
            torch.cuda.synchronize()
            if s:
                det[i] += [pev[2 * o].elapsed_time(pev[2 * o + 1]) for o in range(outer)]
                dec[i] += [pev[2 * o + 1].elapsed_time(pev[2 * o + 2]) for o in range(outer)]
    return det / max(steps, 1), dec / max(steps, 1)


def live_point(full, lv, differ, code, ebn0, first_block, steps, ncw):
    """The windowed loop's part of a point: its counts (it has run the point's blocks beside ``full``), what its passes worked
    on, the decisions that differ, and both loops' times from one alternating run."""
    ibe, ife, inc, im, imean = lv.result()
    det, dec = time_loops([full, lv], code, ebn0, first_block, steps)

    def ms(i):
        return {"detector_passes": [round(v, 4) for v in det[i]], "decoder_passes": [round(v, 4) for v in dec[i]],
                "detector_total": round(float(det[i].sum()), 4), "decoder_total": round(float(dec[i].sum()), 4)}

    return {"guard": lv.guard, "coded_ber": ibe / im, "fer": ife / ncw, "info_bit_errors": ibe, "codeword_errors": ife, "open": inc,
            "total_inner_iters_mean": round(imean, 3),
            "per_pass": [{"info_bit_errors": p[0], "codeword_errors": p[1], "open": p[2], "iters_mean": round(p[3], 3)} for p in lv.pass_results()],
            "live_per_pass": [{"windows": w, "live_rows": r, "open_on_entry": n} for w, r, n in lv.live_results()],
            "burst_rows": int(lv.prior.numel()), "final_decisions_differ": int(differ),
            "ms_per_block": ms(1), "full_loop_ms_per_block_same_run": ms(0)}


def _ebn0_at_fer(points, key, target=1e-2):
    """Eb/N0 where the curve ``key`` crosses ``target``, interpolated in log10 FER between the sweep's points (None: no crossing)."""
    pts = sorted((p["ebn0_info_db"], p[key]["fer"]) for p in points)
    for (e0, f0), (e1, f1) in zip(pts, pts[1:]):
        if f0 >= target > f1:
            if f1 <= 0.0:
                f1 = 0.1 * target / max(1, points[0]["codewords"])       # (no error seen: the crossing is bounded, not located)
            return e0 + (e1 - e0) * (np.log10(f0) - np.log10(target)) / (np.log10(f0) - np.log10(f1))
    return None


def _coarse_point(found, lost, true_nu, true_eps):
    """A point's part of the ``--coarse`` forms: the statistics of the bursts' estimates ``found`` (``coarse_result()`` per burst)
    against the truth, and the bursts in which the coarse link loses codewords that the reference keeps (``lost``: the running
    codeword errors after every burst, per link), each with its burst's frequency error."""
    nu, eps = np.array([f[0] for f in found]) - true_nu, np.array([f[1] for f in found]) - true_eps
    per_burst = {k: np.diff([0] + v) for k, v in lost.items()}
    return {"coarse_estimates": {"bursts": len(found), "nu_error_mean": float(nu.mean()), "nu_error_max_abs": float(np.abs(nu).max()),
                                 "eps_error_mean": float(eps.mean()), "eps_error_max_abs": float(np.abs(eps).max()),
                                 "peak_over_mean_min": float(min(f[2] / f[3] for f in found))},
            "coarse_lost_beyond_reference": [{"burst": i, "coarse": int(c), "reference": int(r), "nu_error": float(nu[i])}
                                             for i, (c, r) in enumerate(zip(per_burst["coarse"], per_burst["reference"])) if c > r]}


def _setup(args):
    """What every LDPC form starts from: the device, the code and the codewords per burst."""
    import torch

    from waveforms_amd.encoding import ldpc

    torch.cuda.set_device(0)
    code = ldpc.demo_code(128 if args.code == "demo" else 1024)
    return code, min(args.block_codewords or max(1, int(1e7) // code.n_tx), args.codewords)


def _rounds(steps, nev, body):
    """``body(ev)`` ``steps`` + 1 times, the first a warm-up: it records the ``nev`` device events ``ev`` in order and may return
    its stage times (name -> ms) -> (the ms between consecutive events, the stage times), summed over the ``steps`` timed rounds."""
    import torch

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(nev)]
    ms, stages = [0.0] * max(nev - 1, 0), {}
    for s in range(steps + 1):
        t = body(ev)
        if ev:
            torch.cuda.synchronize()
        if s:                                                             # (the first round warms up)
            ms = [m + a.elapsed_time(b) for m, a, b in zip(ms, ev, ev[1:])]
            for k, v in (t or {}).items():
                stages[k] = stages.get(k, 0.0) + v
    return ms, stages


def _mean(total, steps):
    return round(total / max(steps, 1), 4)


def _stage_means(sync, steps, body, nev=0, total=True):
    """``_rounds`` with ``sync.times`` on -> (the mean ms between the events, the mean stage times per block with their total)."""
    sync.times = True
    ms, tot = _rounds(steps, nev, body)
    sync.times = False
    stages = {k: _mean(v, steps) for k, v in tot.items()}
    if total:
        stages["total"] = _mean(sum(tot.values()), steps)
    return [_mean(v, steps) for v in ms], stages


class _Form(NamedTuple):
    """One synchroniser form of the tool, as ``main_sync`` runs it."""

    s: object                     # ``_sync_setup``'s
    links: dict                   # curve name -> link, in the order they run and print: genie, impaired, the synchronised ones
    out: dict                     # the header, ending in "points": [] (and "coarse")
    entry: tuple                  # a curve's entries beyond the counts (``_curve_entry``)
    compared: list                # the curves whose Eb/N0 at FER 1e-2 is interpolated,
    losses: object                # and loss(name) -> the header's loss entries
    truth: tuple = ()             # --coarse: the true (nu, eps) the estimates are held against
    point: object = None          # (point, ebn0, first free burst): the form's timed sections and finds, into the point
    after: object = None          # () -> entries behind the summary (the timed acquisitions); the result then goes to --acq-out,
    acq_key: str | None = None    # under this key of the file (None: it is the file)
    rejected: object = None       # anchored link -> the windows its coarse tracks rejected in the last burst,
    rejected_windows: object = None   # and the list of those per burst -> the curve's "rejected_windows"


def _sync_setup(args, framed=True):
    """What the synchroniser forms share: ``_setup``, the framing, the two impairments from the flags, the waveform's link class
    with the keywords every link of the form gets (``link``), and the names of its links' synchroniser keywords and results."""
    import math
    from types import SimpleNamespace

    from waveforms_amd.encoding.coded import CodedCPMLink, CodedSOQPSKLink
    from waveforms_amd.encoding.framing import Framing

    code, per = _setup(args)
    cpm = args.waveform != "soqpsk"
    fr = Framing(code)
    kw = dict(alpha=args.alpha, max_iter=args.max_iter, **(dict(framing=fr, lead_bits=args.lead_bits) if framed else {}))
    if cpm:
        from waveforms_amd.viterbi import cpm as vc

        cls, kw["waveform"], spec = CodedCPMLink, args.waveform, vc.ARTM_64 if args.waveform == "multih" else vc.PCMFM_20
        names = dict(drift="clock", timing_slot=("clock_recovery", "clock_result", ("grid",)), joint_slot=("joint", "joint_result"), unit="calls")
    else:
        cls, kw["detector"], spec = CodedSOQPSKLink, args.detector, None
        names = dict(drift="timing", timing_slot=("timing_recovery", "timing_result", ()), joint_slot=("acquisition", "acquisition_result"), unit="rows")
    return SimpleNamespace(code=code, per=per, sps=8, cpm=cpm, spec=spec, link=lambda **sync: cls(code, per, **sync, **kw),
                           carrier=(math.radians(args.carrier_phase), args.carrier_freq), timing=(args.timing_offset, args.timing_drift),
                           head=lambda form, **first: {"tool": "coded_ber", "form": form, **first, "code": args.code, "n": code.n, "k": code.k, "n_tx": code.n_tx},
                           framed={"marker_bits": fr.L, "period": fr.period, "lead_bits": args.lead_bits} if framed else None, **names)


def _coarse_links(args, s, links, carrier, **fine):
    """``--coarse``: the coarse stage in front of the SAME fine synchroniser ``fine`` (``links["coarse"]``), and that synchroniser at
    --carrier-freq 0 as the reference curve -> (the ``CoarseFrequency``, its header entry)."""
    from waveforms_amd.sync.coarse import CoarseFrequency

    coarse = CoarseFrequency(s.sps, nfft=args.coarse_nfft, smooth=args.coarse_smooth or None)
    links["reference"] = s.link(carrier=(carrier[0], 0.0), **fine)
    links["coarse"] = s.link(carrier=carrier, coarse=coarse, **fine)
    return coarse, {"nfft": coarse.nfft, "smooth": coarse.smooth, "search": coarse.search}


def _carrier_form(args):
    """The ``--recover`` form: genie, impaired and recovered links on the same blocks (SOQPSK-TG: framed; ARTM, PCM/FM: not)."""
    s = _sync_setup(args, framed=args.waveform == "soqpsk")
    if s.cpm:
        from waveforms_amd.sync.carrier_cpm import DEFAULT_HYPOTHESES, MAX_DRIFT_PERIODS, CPMCarrierRecovery

        rec = CPMCarrierRecovery(s.spec, args.carrier_window, args.carrier_span, args.carrier_hyp or DEFAULT_HYPOTHESES, args.carrier_refine)
        limit = MAX_DRIFT_PERIODS / s.spec.p
    else:
        from waveforms_amd.sync.carrier import MAX_DRIFT_TURNS as limit, CarrierRecovery

        rec = CarrierRecovery(args.carrier_window, args.carrier_span, args.carrier_hyp or 8, args.carrier_refine)
    links = {"genie": s.link(), "impaired": s.link(carrier=s.carrier), "recovered": s.link(carrier=s.carrier, recovery=rec)}
    out = {**s.head("carrier", waveform=args.waveform), "detector": None if s.cpm else args.detector, "block_codewords": s.per,
           "framed": s.framed,
           "carrier": {"phase_deg": args.carrier_phase, "nu_cycles_per_sample": args.carrier_freq,
                       "drift_turns_per_window": abs(args.carrier_freq) * s.sps * rec.window, "documented_limit_turns_per_window": limit},
           "recovery": {"window": rec.window, "span": rec.span, "hypotheses": rec.hypotheses, "refine": rec.refine}, "points": []}
    coarse = None
    if args.coarse:
        coarse, out["coarse"] = _coarse_links(args, s, links, s.carrier, recovery=rec)

    def point(p, e, b):
        """The coarse stage's times over the front end of its link, then the recovery's stages on one burst, each bracketed by
        device events, beside one plain soft detection of the same rows."""
        if coarse is not None:
            ck = links["coarse"]

            def front_end(ev):
                ck.front_end(ck.encode(ck.info_bits(b)), e, 1, b)
                return coarse.stage_times()

            _, p["coarse_ms_per_block"] = _stage_means(coarse, args.steps, front_end, total=False)
        lk = links["recovered"]
        rows, _ = lk.front_end(lk.encode(lk.info_bits(b)), e, 1, b)

        def body(ev):
            rec.recover(rows, *lk._differential)
            t = rec.stage_times()
            ev[0].record()
            lk._soft(rows)
            ev[1].record()
            return t

        (soft_ms,), stages = _stage_means(rec, args.steps, body, 2)
        p.update({"recovery_ms_per_block": stages, "soft_detector_ms": soft_ms, "burst_rows": int(rows.shape[0])})

    return _Form(s=s, links=links, out=out, entry=("uncoded_ber", "wrong_locks"), truth=(args.carrier_freq, 0.0), point=point,
                 compared=["genie", "recovered"], losses=lambda loss: {"loss_db_at_fer_1e-2": loss("recovered")})


def _timing_form(args):
    """The ``--recover-timing`` form: genie, impaired and recovered FRAMED links on the same blocks - SOQPSK-TG with a
    ``TimingRecovery``, ARTM and PCM/FM (``--waveform multih|pcmfm``) with a ``CPMTimingRecovery``; the anchored one with ``--anchor``."""
    from functools import partial

    s = _sync_setup(args)
    if s.cpm:
        from waveforms_amd.sync.timing_cpm import MAX_DRIFT_SAMPLES, CPMTimingRecovery

        make = partial(CPMTimingRecovery, s.spec, s.sps, args.timing_window, args.timing_span, args.timing_hyp, args.timing_refine, args.timing_delta)
        limit = MAX_DRIFT_SAMPLES[args.waveform]
    else:
        from waveforms_amd.sync.timing import MAX_DRIFT_SAMPLES as limit, TimingRecovery

        make = partial(TimingRecovery, s.sps, args.timing_window or 256, args.timing_span, args.timing_hyp or 8, args.timing_refine,
                       args.timing_delta or 2.0)
    keyword, result, beyond = s.timing_slot
    rec = make()
    syncs = {"recovered": rec, **({"anchored": make(anchor=args.anchor)} if args.anchor else {})}
    links = {"genie": s.link(), "impaired": s.link(**{s.drift: s.timing})}
    links.update((name, s.link(**{s.drift: s.timing, keyword: sync})) for name, sync in syncs.items())
    out = {**s.head("timing", waveform=args.waveform), "detector": None if s.cpm else args.detector, "block_codewords": s.per,
           "framed": s.framed,
           "timing": {"tau0_samples": args.timing_offset, "eps": args.timing_drift, "drift_samples_per_window": abs(args.timing_drift) * s.sps * rec.window,
                      "documented_limit_samples_per_window": limit},
           "recovery": {"window": rec.window, "span": rec.span, "hypotheses": rec.hypotheses, "refine": rec.refine, "delta": rec.delta,
                        "anchor": args.anchor}, "points": []}

    def point(p, e, b):
        """The recovery's stages on one burst's noisy samples, each bracketed by device events, beside the plain front end (channel
        + bank, what the genie link runs) and one plain soft detection of its rows; then what the last burst's recovery found."""
        lk = links["recovered"]
        sig, at, _ = lk.signal(lk.encode(lk.info_bits(b)), b)
        received = lk.noisy(sig, e, 1, b)

        def body(ev):
            rec.recover(received, lk._d_bank, *at, *lk._differential)
            t = rec.stage_times()
            ev[0].record()
            if lk._fused_bank is not None:
                rows = lk._fused_bank(sig, *at, lk.sigma(e), 1, b)
            else:
                rows = lk._bank(lk.noisy(sig, e, 1, b), *at)
            ev[1].record()
            lk._soft(rows)
            ev[2].record()
            return t

        (front_ms, soft_ms), p["recovery_ms_per_block"] = _stage_means(rec, args.steps, body, 3)
        p.update({"fused_front_end_ms": front_ms, "soft_detector_ms": soft_ms, "burst_rows": int(at[1])})
        tau, _choice, *found = getattr(lk, result)()
        p["tau_samples"] = {"first": round(float(tau[0]), 3), "last": round(float(tau[-1]), 3), "windows": int(tau.size)}
        p.update(zip(beyond, found))

    def losses(loss):
        return {"loss_db_at_fer_1e-2": loss("recovered"), **({"anchored_loss_db_at_fer_1e-2": loss("anchored")} if args.anchor else {})}

    return _Form(s=s, links=links, out=out, entry=("uncoded_ber", "wrong_locks", "last_lock"), point=point, compared=["genie", *syncs],
                 losses=losses, rejected=lambda lk: getattr(lk, result)()[-1], rejected_windows=sum)


def _time_acquisition(lk, make, stacks, length, ebn0, steps, unit, stack_of):
    """One acquisition of a burst of about ``length`` rows or calls (PN bits, the link's own impairments and channel) per entry of
    ``stacks`` (name -> (stack, anchor)): device events around the whole call, ``steps`` calls after one warm-up, beside one plain
    soft detection of as many rows -> {unit, "soft_detector_ms", name: {"stack", "ms", "launches", "in_soft_detections", "stages_ms"}}."""
    from waveforms_amd import device as dev

    bits = dev.lfsr_bits(23, lk._mask, (1 << 23) - 1, int(length) * lk.bits_per_symbol)[0]
    sig = lk.impaired(lk.modulated(bits)[0])
    at = lk._geometry(sig, int(length))                                   # (not the link's own burst: the geometry of this length)
    received = lk.noisy(sig, ebn0, 1, 0)
    del sig
    plain = lk._bank(received, *at)

    def soft(ev):
        ev[0].record()
        lk._soft(plain)
        ev[1].record()

    (soft_ms,), _ = _rounds(steps, 2, soft)
    del plain
    n = max(steps, 1)
    out = {unit: int(at[1]), "soft_detector_ms": round(soft_ms / n, 4)}
    for name, (stack, anchor) in stacks.items():
        acq = make(stack=stack, anchor=anchor)

        def once(ev):
            acq.times = False
            ev[0].record()
            acq.recover(received, lk._d_bank, *at, *lk._differential)
            ev[1].record()

        (ms,), _ = _rounds(steps, 2, once)
        acq.times = True                                                  # (the stages from a call of their own: the events cost time)
        acq.recover(received, lk._d_bank, *at, *lk._differential)
        stages = {k: round(v, 4) for k, v in acq.stage_times().items()}
        out[name] = {"stack": stack_of(acq, stack, at[1]), "ms": round(ms / n, 4), "launches": acq.launches,
                     "in_soft_detections": round(ms / n / (soft_ms / n), 2), "stages_ms": stages}
    return out


def _acquire_form(args):
    """The ``--acquire`` form: genie, impaired and acquired FRAMED links on the same blocks under a carrier offset AND a timing
    offset, the anchored curve with ``--anchor``, and the time of one acquisition, unstacked and stacked.  SOQPSK-TG: a
    ``JointAcquisition``, one more acquired curve per further value of ``--acq-carrier-hyp``, timed on bursts of ``--acq-time-rows``
    rows.  ARTM and PCM/FM: a ``CPMJointAcquisition``, timed on the link's own burst and on bursts of ``--acq-time-rows`` calls; the
    result goes under the waveform's key of ``--acq-out``, beside what the file holds for the other waveform."""
    from functools import partial

    s = _sync_setup(args)
    stack = args.acq_stack or None
    hyp = args.acq_carrier_hyp
    if s.cpm:
        from waveforms_amd.sync.joint_cpm import MAX_DRIFT_PERIODS, MAX_DRIFT_SAMPLES, CPMJointAcquisition

        common = dict(timing_window=args.timing_window, carrier_window=args.carrier_window, span=args.timing_span, timing_hypotheses=args.timing_hyp,
                      carrier_hypotheses=args.carrier_hyp or 2, refine=args.timing_refine, delta=args.timing_delta)
        first = partial(CPMJointAcquisition, s.spec, s.sps, **common)
        further = {}
        # timed unstacked (cpm_soft_branch per table and per buffer) and stacked, on the link's own burst and on 1e6 calls
        timed = dict(stacks={"stack_1": (1, 0), "stacked": (None, 0), **({"stacked_anchored": (None, args.anchor)} if args.anchor else {})},
                     lengths=lambda lk: [lk.ncalls] + ([1_000_000] if args.acq_time_rows == [211_252, 10_000_000] else args.acq_time_rows),
                     stack_of=lambda acq, stack, n: stack)
    else:
        from waveforms_amd.sync.joint import MAX_DRIFT_SAMPLES, MAX_DRIFT_TURNS, STACK_BYTES, JointAcquisition

        common = dict(window=args.timing_window or 256, span=args.timing_span, timing_hypotheses=args.acq_timing_hyp, refine=args.timing_refine,
                      delta=args.timing_delta or 2.0)
        make = partial(JointAcquisition, s.sps, **common)
        first = partial(make, carrier_hypotheses=hyp[0])
        further = {f"acquired_hc{hc}": partial(make, carrier_hypotheses=hc) for hc in hyp[1:]}
        # timed unstacked (the existing entry points per hypothesis) and stacked
        timed = dict(stacks={"stack_1": (1, 0), "stack_default": (stack, 0), **({"stack_default_anchored": (stack, args.anchor)} if args.anchor else {})},
                     lengths=lambda lk: args.acq_time_rows, stack_of=lambda acq, stack, n: acq.stack_for(n))
    keyword, result = s.joint_slot
    acqs = {"acquired": first(stack=stack), **{name: f(stack=stack) for name, f in further.items()}}
    if args.anchor:                                                       # the anchored curve beside the first acquired one, on the same blocks
        acqs["anchored"] = first(stack=stack, anchor=args.anchor)
    both = {"carrier": s.carrier, s.drift: s.timing}
    links = {"genie": s.link(), "impaired": s.link(**both)}
    links.update((name, s.link(**both, **{keyword: acq})) for name, acq in acqs.items())
    carrier = {"phase_deg": args.carrier_phase, "nu_cycles_per_sample": args.carrier_freq}
    timing = {"tau0_samples": args.timing_offset, "eps": args.timing_drift}
    if s.cpm:
        a = acqs["acquired"]
        out = {**s.head("acquire", waveform=args.waveform), "block_codewords": s.per, "burst_calls": links["genie"].ncalls, "framed": s.framed,
               "carrier": {**carrier, "drift_turns_per_carrier_window": abs(args.carrier_freq) * s.sps * a.carrier_window,
                           "documented_limit_turns_per_carrier_window": MAX_DRIFT_PERIODS / s.spec.p},
               "timing": {**timing, "drift_samples_per_timing_window": abs(args.timing_drift) * s.sps * a.timing_window,
                          "documented_limit_samples_per_timing_window": MAX_DRIFT_SAMPLES[args.waveform]},
               "acquisition": {"timing_window": a.timing_window, "carrier_window": a.carrier_window, "span": a.span, "timing_hypotheses": a.timing_hypotheses,
                               "carrier_hypotheses": a.carrier_hypotheses, "refine": a.refine, "delta": a.delta, "stack": a.stack, "anchor": args.anchor},
               "points": []}
    else:
        W = common["window"]
        out = {**s.head("acquire"), "detector": args.detector, "block_codewords": s.per, "framed": s.framed,
               "carrier": {**carrier, "drift_turns_per_window": abs(args.carrier_freq) * s.sps * W, "documented_limit_turns_per_window": MAX_DRIFT_TURNS},
               "timing": {**timing, "drift_samples_per_window": abs(args.timing_drift) * s.sps * W, "documented_limit_samples_per_window": MAX_DRIFT_SAMPLES},
               "acquisition": {**common, "carrier_hypotheses": hyp, "stack": stack, "stack_bytes": STACK_BYTES, "anchor": args.anchor}, "points": []}
    # --coarse: the clock reads the rotated signal, so the carrier frequency in cycles per RECEIVED sample is nu (1 + eps)
    true_nu = args.carrier_freq * (1.0 + args.timing_drift)
    if args.coarse:
        fine = {s.drift: s.timing, keyword: acqs["anchored" if args.anchor else "acquired"]}
        _, out["coarse"] = _coarse_links(args, s, links, s.carrier, **fine)
        out["coarse"]["true_nu_cycles_per_received_sample"] = true_nu

    def after():
        """One acquisition in units of one plain soft detection."""
        lk = links["acquired"]
        return {"one_acquisition": [_time_acquisition(lk, first, timed["stacks"], n, args.ebn0[-1], args.steps, s.unit, timed["stack_of"])
                                    for n in timed["lengths"](lk)]}

    return _Form(s=s, links=links, out=out, entry=("wrong_locks", "last_lock"), truth=(true_nu, args.timing_drift), compared=["genie", *acqs],
                 losses=lambda loss: {"loss_db_at_fer_1e-2": {name: loss(name) for name in acqs}}, after=after,
                 rejected=lambda lk: getattr(lk, result)()[5::2],
                 rejected_windows=lambda found: dict(zip(("timing", "carrier"), map(sum, zip(*found)))),
                 acq_key=args.waveform if s.cpm else None)


def _curve_entry(lk, ncw, keys):
    """A link's counts over the point's ``ncw`` codewords, and the form's further entries ``keys``."""
    def uncoded_ber():
        try:
            ue, um = lk.uncoded_result()
        except RuntimeError:                                              # (its synchroniser leaves the rows shifted: it does not count channel bits)
            return None
        return ue / um

    further = {"uncoded_ber": uncoded_ber, "wrong_locks": lambda: None if lk.framing is None else lk.sync_result()[1],
               "last_lock": lambda: lk.sync_result()[2][0]}
    be, fe, nc, m, mean_it = lk.result()
    return {"coded_ber": be / m, "fer": fe / ncw, "info_bit_errors": be, "codeword_errors": fe, "not_converged": nc, "mean_iters": round(mean_it, 3),
            **{k: further[k]() for k in keys}}


def main_sync(args, make_form) -> None:
    """The synchroniser forms (``_carrier_form``, ``_timing_form``, ``_acquire_form``): every link of the form on the same blocks,
    point by point; per point the form's own timed sections; the Eb/N0 at FER 1e-2 of the curves the form compares, and the losses."""
    form = make_form(args)
    s, links, out = form.s, form.links, form.out
    for e in args.ebn0:
        point = {"ebn0_info_db": e}
        b = 0
        lost, found = {}, []
        for name, lk in links.items():
            lk.reset_counts()
            b, rejected = 0, []
            while b * s.per < args.codewords:
                lk.run_block(e, seed=1, stream_id=b)
                b += 1
                if name == "anchored":                                    # the windows its coarse tracks rejected in this burst
                    rejected.append(form.rejected(lk))
                if name in ("reference", "coarse"):                       # (per burst: these two synchronise after every block)
                    lost.setdefault(name, []).append(lk.result()[1])
                    if name == "coarse":
                        found.append(lk.coarse_result())
            point[name] = _curve_entry(lk, b * s.per, form.entry)
            if name == "anchored":
                point[name]["rejected_windows"] = form.rejected_windows(rejected)
        point["codewords"] = b * s.per
        if "coarse" in links:
            point.update(_coarse_point(found, lost, *form.truth))
        if form.point is not None:
            form.point(point, e, b)
        out["points"].append(point)
    at = out["ebn0_at_fer_1e-2"] = {name: _ebn0_at_fer(out["points"], name) for name in form.compared}

    def loss(name, over="genie"):
        return None if at[over] is None or at[name] is None else round(at[name] - at[over], 3)

    out.update(form.losses(loss))
    if "coarse" in links:
        # the coarse stage's cost: the distance between the coarse + fine curve and the same fine synchroniser at --carrier-freq 0
        at.update({name: _ebn0_at_fer(out["points"], name) for name in ("reference", "coarse")})
        out["coarse_cost_db_at_fer_1e-2"] = loss("coarse", "reference")
    if form.after is not None:
        out.update(form.after())
    print(json.dumps(out))
    if form.after is not None and args.acq_out:                           # --acq-out: the forms that time an acquisition
        path = Path(args.acq_out)
        if form.acq_key is not None:                                      # under the waveform's key, beside what the file holds for the other
            if path.name == "joint_acquisition.json":                     # (the SOQPSK-TG form's default)
                path = path.with_name("joint_acquisition_cpm.json")
            out = {**(json.loads(path.read_text()) if path.exists() else {}), form.acq_key: out}
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(out, indent=1) + "\n")


def main_conv(args) -> None:
    """The ``--code conv-*`` form: ConvSOQPSKLink."""
    import torch

    from waveforms_amd import device as dev
    from waveforms_amd.encoding import conv
    from waveforms_amd.encoding.sccc import ConvSOQPSKLink

    torch.cuda.set_device(0)
    K = 3 if args.code == "conv-k3" else 7
    rs = None
    if args.rs:
        from waveforms_amd.encoding.rs import RSCode
        from waveforms_amd.encoding.rsconv import RSConvSOQPSKLink

        rs = RSCode.ccsds(args.rs, args.rs_depth, args.rs_n)
        if args.info_bits and args.info_bits != 8 * rs.n * rs.depth:
            raise SystemExit(f"--rs fixes --info-bits at one RS frame: {8 * rs.n * rs.depth}")
        args.info_bits = 8 * rs.n * rs.depth
    k = args.info_bits or 1024 - (K - 1)
    n = 2 * (k + K - 1)
    order = conv.qpp_order(n, 31, 64) if args.interleave else None
    code = (conv.nasa_k3 if K == 3 else conv.ccsds_k7)(k, tx_order=order)
    per = args.block_codewords or max(1, int(1e7) // code.n_tx)
    per = min(per, args.codewords)
    outer = max(args.outer, 1)
    if rs is None:
        link = ConvSOQPSKLink(code, per, detector=args.detector, outer=outer, damping=args.damping, per_pass=True)
    else:
        link = RSConvSOQPSKLink(rs, code, per, detector=args.detector, outer=outer, damping=args.damping, per_pass=True,
                                erasures=args.rs_erasures, erase_below=args.rs_erase_below)
    out = {"tool": "coded_ber", "code": args.code, "generators": [oct(g) for g in code.generators], "K": code.K, "n": code.n, "k": code.k,
           "n_tx": code.n_tx, "interleave": bool(args.interleave), "detector": args.detector, "block_codewords": per, "outer": outer,
           "damping": link.damping, "ext_clip": link.ext_clip, "geometry": dev.conv_siso_geometry(code, per), "points": []}
    if rs is not None:
        out["rs"] = {"n": rs.n, "k": rs.k, "t": rs.t, "depth": rs.depth, "prim": hex(rs.prim), "fcr": rs.fcr, "step": rs.step,
                     "user_bits_per_block": link.user_bits_per_block, "geometry": dev.rs_decode_geometry(rs, per)}
    rs_scratch = torch.zeros(6, dtype=torch.int64, device="cuda") if rs is not None else None
    era = bool(rs is not None and args.rs_erasures)
    plain_counts = torch.zeros(5, dtype=torch.int64, device="cuda") if era else None      # the errors-only decoder on the same decisions
    if era:
        out["rs"]["erasures"] = {"f_max": link.erasures, "below": link.erase_below}
    for e in args.ebn0:
        link.reset_counts()
        b = 0
        while b * per < args.codewords:
            link.run_block(e, seed=1, stream_id=b)
            if era:
                dev.rs_decode(rs, link.decided, bits=True, ref_msg=link.user, counts=plain_counts)
            b += 1
        be, fe, m = link.result()
        ue, um = link.uncoded_result()
        passes = link.pass_results()
        ncw = b * per
        rs_counts = link.rs_result() if rs is not None else None
        if era:
            era_counts, era_marks = rs_counts, link.rs_erasure_result()
            rs_counts = tuple(int(v) for v in plain_counts.cpu().tolist()) + (rs_counts[5],)
            plain_counts.zero_()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3 + 2 * outer)]
        rev = [torch.cuda.Event(enable_timing=True) for _ in range(8)]
        ms, rs_ms = np.zeros(2 + 2 * outer), np.zeros(4)
        for s in range(args.steps + 1):
            if rs is not None:                                            # (the RS encoder alone, in front of the block: what info_bits does)
                link.user = link.user_bits(b + s)
                rev[0].record()
                info = dev.rs_encode(rs, link.user, bits=True).view(-1)
                rev[1].record()
            ev[0].record()
            tx = dev.conv_encode(code, info if rs is not None else link.info_bits(b + s))
            ev[1].record()
            rows, _ = link.front_end(tx, e, 1, b + s)
            ev[2].record()
            if outer == 1:                                                # the calls of run_block: plain detector, no ext output
                llr, _ = link.soft(rows)
                ev[3].record()
                dev.conv_siso(code, llr, scale=link.llr_scale, want_post=False, want_ext=False)
                ev[4].record()
            else:
                link.begin(int(rows.shape[0]))
                for o in range(outer):
                    ext, _ = link.detect(rows, first=o == 0)
                    ev[3 + 2 * o].record()
                    link.decode(ext, want_post=era and o == outer - 1)
                    ev[4 + 2 * o].record()
            if rs is not None:                                            # the call run_block makes on the block's decisions
                if outer > 1:
                    decided, post = link.decided, link.post
                else:
                    siso = dev.conv_siso(code, llr, scale=link.llr_scale, want_post=era, want_ext=False)
                    decided, post = siso["info_bits"], siso["info_post"]
                rev[2].record()
                dev.rs_decode(rs, decided, bits=True, ref_msg=link.user, counts=rs_scratch)
                rev[3].record()
                if era:                                                   # ... and the two calls the link makes with erasures, on the same decisions
                    rev[4].record()
                    marks = dev.rs_mark_erasures(rs, post, link.erasures, link.erase_below)
                    rev[5].record()
                    rev[6].record()
                    dev.rs_decode(rs, decided, bits=True, ref_msg=link.user, counts=rs_scratch, erasures=marks)
                    rev[7].record()
            torch.cuda.synchronize()
            if s:                                                         # (the first round warms up)
                ms += [ev[i].elapsed_time(ev[i + 1]) for i in range(2 + 2 * outer)]
                if rs is not None:
                    rs_ms[:2] += [rev[0].elapsed_time(rev[1]), rev[2].elapsed_time(rev[3])]
                if era:
                    rs_ms[2:] += [rev[4].elapsed_time(rev[5]), rev[6].elapsed_time(rev[7])]
        ms /= max(args.steps, 1)
        rs_ms /= max(args.steps, 1)
        det, dec = ms[2::2], ms[3::2]
        out["points"].append({
            "ebn0_info_db": e, "ebn0_channel_db": round(e + 10 * np.log10(code.k / code.n_tx), 3), "codewords": ncw,
            "coded_ber": be / m, "fer": fe / ncw, "info_bit_errors": be, "codeword_errors": fe, "uncoded_ber": ue / um,
            "per_pass": [{"info_bit_errors": p[0], "codeword_errors": p[1]} for p in passes],
            "ms_per_block": {"encode": round(ms[0], 4), "front_end": round(ms[1], 4), "detector_passes": [round(v, 4) for v in det],
                             "siso_passes": [round(v, 4) for v in dec], "detector_total": round(float(det.sum()), 4),
                             "siso_total": round(float(dec.sum()), 4)},
            "siso_info_gbps": round(per * code.k / (float(dec.mean()) * 1e-3) / 1e9, 4) if dec.mean() > 0 else None,
        })
        if rs is not None:
            rbe, rce, rfl, rcor, rfe, rm = rs_counts
            out["points"][-1]["ebn0_channel_db"] = round(e + link._rate_db(), 3)
            out["points"][-1]["rs"] = {
                "user_ber": rbe / rm, "fer": rfe / ncw, "user_bit_errors": rbe, "user_bits": rm, "codeword_errors": rce, "codewords": ncw * rs.depth,
                "frame_errors": rfe, "flagged_failures": rfl, "miscorrections": rce - rfl, "symbols_corrected": rcor,
                "ms_per_block": {"rs_encode": round(rs_ms[0], 4), "rs_decode": round(rs_ms[1], 4)},
                "rs_decode_over_siso": round(float(rs_ms[1] / dec.sum()), 5) if dec.sum() > 0 else None}
        if era:
            ebe, ece, efl, ecor, efe, em = era_counts
            out["points"][-1]["rs_erasures"] = {
                "user_ber": ebe / em, "fer": efe / ncw, "user_bit_errors": ebe, "user_bits": em, "codeword_errors": ece, "codewords": ncw * rs.depth,
                "frame_errors": efe, "flagged_failures": efl, "miscorrections": ece - efl, "symbols_corrected": ecor,
                "erasures_declared": era_marks[0], "erasures_filled": era_marks[1],
                "ms_per_block": {"rs_mark_erasures": round(rs_ms[2], 4), "rs_decode_erasures": round(rs_ms[3], 4), "rs_decode": round(rs_ms[1], 4)},
                "erasures_over_errors_only": round(float((rs_ms[2] + rs_ms[3]) / rs_ms[1]), 4) if rs_ms[1] > 0 else None,
                "rs_decode_erasures_over_rs_decode": round(float(rs_ms[3] / rs_ms[1]), 4) if rs_ms[1] > 0 else None}
    print(json.dumps(out))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--waveform", default="soqpsk", choices=["soqpsk", "multih", "pcmfm"])
    ap.add_argument("--code", default="demo", choices=["demo", "demo16k", "conv-k3", "conv-k7"])
    ap.add_argument("--info-bits", type=int, default=0, help="--code conv-*: information bits per codeword (0: n = 2048)")
    ap.add_argument("--interleave", action="store_true", help="--code conv-*: QPP interleaver (31 t + 64 t^2) mod n")
    ap.add_argument("--rs", type=int, default=0, choices=[0, 8, 16], help="--code conv-*: CCSDS Reed-Solomon outer code correcting E symbols")
    ap.add_argument("--rs-depth", type=int, default=1, help="--rs: symbol interleaving depth 1 .. 8")
    ap.add_argument("--rs-n", type=int, default=255, help="--rs: shortened code length")
    ap.add_argument("--rs-erasures", type=int, default=0, help="--rs: also decode errors and erasures, at most F erasures per RS codeword (0: off)")
    ap.add_argument("--rs-erase-below", type=float, default=float("inf"), help="--rs-erasures: only symbols whose reliability is below X are erased")
    ap.add_argument("--ebn0", type=float, nargs="+", default=[4.0, 5.0, 6.0, 7.0, 8.0])
    ap.add_argument("--codewords", type=int, default=20000)
    ap.add_argument("--block-codewords", type=int, default=0, help="codewords per burst (0: about 1e7 channel bits)")
    ap.add_argument("--detector", default="PT", choices=["PT", "PAM"])
    ap.add_argument("--max-iter", type=int, default=50)
    ap.add_argument("--alpha", type=float, default=0.75)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--outer", type=int, default=0, help="outer passes of the iterative chain (0: one-pass curve only)")
    ap.add_argument("--inner", type=int, default=5, help="decoder iterations per outer pass")
    ap.add_argument("--damping", type=float, default=0.7, help="scale of the prior fed back to the detector")
    ap.add_argument("--framed", action="store_true", help="also run the framed link (sync marker + randomiser + soft frame search)")
    ap.add_argument("--lead-bits", type=int, default=0, help="pseudo-random bits in front of the framed burst (0 .. period - 1)")
    ap.add_argument("--marker-prior", type=float, default=None, help="prior of the marker rows in the framed loop (default ext_sat)")
    ap.add_argument("--live-only", action="store_true", help="also run the iterative loop(s) with the detector on the live windows only")
    ap.add_argument("--guard", type=int, default=128, help="guard rows of --live-only")
    ap.add_argument("--carrier-phase", type=float, default=0.0, help="carrier phase offset of the modulated signal, degrees")
    ap.add_argument("--carrier-freq", type=float, default=0.0, help="carrier frequency offset, cycles per sample")
    ap.add_argument("--recover", action="store_true", help="genie, impaired and recovered framed links on the same blocks (CarrierRecovery)")
    ap.add_argument("--carrier-window", type=int, default=256, help="--recover: rows per window")
    ap.add_argument("--carrier-hyp", type=int, default=0, help="--recover: coarse hypotheses (0: 8 for SOQPSK-TG, the class's 2 for ARTM and PCM/FM)")
    ap.add_argument("--carrier-span", type=int, default=5, help="--recover: windows of the centred mean")
    ap.add_argument("--carrier-refine", type=int, default=1, help="--recover: refinement passes")
    ap.add_argument("--coarse", action="store_true", help="--recover / --acquire (SOQPSK-TG): also a link with a CoarseFrequency in front of the recovery "
                    "(of the acquisition: the anchored one with --anchor), and the same one at --carrier-freq 0 as its reference curve")
    ap.add_argument("--coarse-nfft", type=int, default=4096, help="--coarse: bits per segment of the line periodograms")
    ap.add_argument("--coarse-smooth", type=int, default=0, help="--coarse: samples of the boxcar in front of the squarer (0: sps // 2)")
    ap.add_argument("--timing-offset", type=float, default=0.0, help="timing offset of the modulated signal, samples")
    ap.add_argument("--timing-drift", type=float, default=0.0, help="timing drift, samples per sample")
    ap.add_argument("--recover-timing", action="store_true", help="genie, impaired and recovered framed links on the same blocks (TimingRecovery)")
    ap.add_argument("--timing-window", type=int, default=None, help="--recover-timing: rows per window (default: 256; the class's for ARTM and PCM/FM)")
    ap.add_argument("--timing-hyp", type=int, default=None, help="--recover-timing: coarse hypotheses over one period (default: 8; the class's for ARTM and PCM/FM)")
    ap.add_argument("--timing-span", type=int, default=5, help="--recover-timing: windows of the centred mean")
    ap.add_argument("--timing-refine", type=int, default=1, help="--recover-timing: refinement rounds")
    ap.add_argument("--timing-delta", type=float, default=None, help="--recover-timing: spacing of a refinement's three points, samples (default: 2.0; the class's for ARTM and PCM/FM)")
    ap.add_argument("--anchor", type=int, default=0, help="--recover-timing / --acquire: K of the anchored unwrapping (odd, 3 .. 1023); adds the "
                    "anchored curve beside the unanchored one on the same blocks (0: none)")
    ap.add_argument("--acquire", action="store_true", help="genie, impaired and acquired framed links on the same blocks under --carrier-* AND --timing-* (JointAcquisition; "
                    "--waveform multih|pcmfm: CPMJointAcquisition, with --timing-* / --carrier-window / --carrier-hyp as its arguments, into profiles/joint_acquisition_cpm.json)")
    ap.add_argument("--acq-timing-hyp", type=int, default=4, help="--acquire: timing hypotheses over one symbol")
    ap.add_argument("--acq-carrier-hyp", type=int, nargs="+", default=[8], help="--acquire: carrier hypotheses over [0, pi); further values add a curve each")
    ap.add_argument("--acq-stack", type=int, default=0, help="--acquire: carrier hypotheses per stacked launch set (0: all that fit the byte budget; 1: unstacked)")
    ap.add_argument("--acq-time-rows", type=int, nargs="*", default=[211_252, 10_000_000], help="--acquire: burst lengths one acquisition is timed at (ARTM, PCM/FM: the link's own and 1e6 calls)")
    ap.add_argument("--acq-out", default=str(ROOT / "profiles" / "joint_acquisition.json"), help="--acquire: where the result is also written ('' : nowhere)")
    args = ap.parse_args()
    if args.coarse and (not (args.recover or args.acquire) or args.waveform != "soqpsk"):
        ap.error("--coarse goes with --recover or --acquire on --waveform soqpsk (PCM/FM and ARTM have no usable lines)")
    if args.acquire:
        if args.code.startswith("conv") or args.outer or args.live_only or args.recover or args.recover_timing:
            ap.error("--acquire is the framed CodedSOQPSKLink's and CodedCPMLink's: an LDPC code, no --outer / --live-only / --recover / --recover-timing")
        return main_sync(args, _acquire_form)
    if args.recover_timing or args.timing_offset or args.timing_drift:
        if not args.recover_timing:
            ap.error("--timing-offset / --timing-drift go with --recover-timing")
        if args.code.startswith("conv") or args.outer or args.live_only or args.recover:
            ap.error("--recover-timing is the framed CodedSOQPSKLink's and CodedCPMLink's: an LDPC code, no --outer / --live-only / --recover")
        return main_sync(args, _timing_form)
    if args.recover or args.carrier_phase or args.carrier_freq:
        if not args.recover:
            ap.error("--carrier-phase / --carrier-freq go with --recover")
        if args.code.startswith("conv") or args.outer or args.live_only:
            ap.error("--recover is CodedSOQPSKLink's (framed) and CodedCPMLink's: an LDPC code, no --outer / --live-only")
        return main_sync(args, _carrier_form)
    if args.live_only and (args.waveform != "soqpsk" or args.outer < 1):
        ap.error("--live-only is the SOQPSK-TG loop's: it needs --waveform soqpsk and --outer N")
    if args.code.startswith("conv"):
        if args.waveform != "soqpsk" or args.framed or args.live_only:
            ap.error("--code conv-* is the SOQPSK-TG link's, unframed and without --live-only")
        if args.rs_erasures and not args.rs:
            ap.error("--rs-erasures goes with --rs")
        return main_conv(args)
    if args.info_bits or args.interleave or args.rs or args.rs_erasures:
        ap.error("--info-bits, --interleave, --rs and --rs-erasures go with --code conv-k3 / conv-k7")

    import torch

    from waveforms_amd import device as dev
    from waveforms_amd.encoding.coded import CodedCPMLink, CodedSOQPSKLink, IterativeCPMLink, IterativeSOQPSKLink

    code, per = _setup(args)
    cpm = args.waveform != "soqpsk"
    which = {"waveform": args.waveform} if cpm else {"detector": args.detector}
    link = (CodedCPMLink if cpm else CodedSOQPSKLink)(code, per, alpha=args.alpha, max_iter=args.max_iter, **which)
    out = {"tool": "coded_ber", "code": args.code, "n": code.n, "k": code.k, "n_tx": code.n_tx, **which,
           "alpha": args.alpha, "max_iter": args.max_iter, "block_codewords": per,
           "geometry": dev.ldpc_decode_geometry(code, per), "points": []}
    idd = None
    if args.outer > 0:
        idd = (IterativeCPMLink if cpm else IterativeSOQPSKLink)(code, per, alpha=args.alpha, outer=args.outer, inner=args.inner,
                                                                damping=args.damping, per_pass=True, **which)
        out["iterative"] = {"outer": idd.outer, "inner": idd.inner, "damping": idd.damping, "ext_sat": idd.ext_sat,
                            "ext_clip": None if np.isinf(idd.ext_clip) else idd.ext_clip}
    lidd = lfidd = None
    if args.live_only:
        lidd = IterativeSOQPSKLink(code, per, alpha=args.alpha, outer=args.outer, inner=args.inner, damping=args.damping, per_pass=True,
                                   live_only=True, guard=args.guard, **which)
    flink = fidd = None
    if args.framed:
        from waveforms_amd.encoding.framing import Framing

        fr = Framing(code)
        flink = (CodedCPMLink if cpm else CodedSOQPSKLink)(code, per, alpha=args.alpha, max_iter=args.max_iter, framing=fr,
                                                         lead_bits=args.lead_bits, **which)
        out["framed"] = {"marker": hex(fr.marker), "marker_bits": fr.L, "period": fr.period, "lead_bits": args.lead_bits}
        if args.outer > 0:
            fidd = (IterativeCPMLink if cpm else IterativeSOQPSKLink)(code, per, alpha=args.alpha, outer=args.outer, inner=args.inner,
                                                                     damping=args.damping, per_pass=True, framing=fr,
                                                                     lead_bits=args.lead_bits, marker_prior=args.marker_prior, **which)
            out["framed"]["marker_prior"] = fidd.marker_prior
            if args.live_only:
                lfidd = IterativeSOQPSKLink(code, per, alpha=args.alpha, outer=args.outer, inner=args.inner, damping=args.damping, per_pass=True,
                                            framing=fr, lead_bits=args.lead_bits, marker_prior=args.marker_prior, live_only=True,
                                            guard=args.guard, **which)
    for e in args.ebn0:
        link.reset_counts()
        b = 0
        while b * per < args.codewords:
            link.run_block(e, seed=1, stream_id=b)
            b += 1
        be, fe, nc, m, mean_it = link.result()
        ue, um = link.uncoded_result()
        ncw = b * per
        # timing: the same stages, one event pair each, over --steps further blocks
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        ms = np.zeros(4)
        for s in range(args.steps):
            ev[0].record()
            info = link.info_bits(b + s)
            tx = dev.ldpc_encode(code, info)
            ev[1].record()
            rows, _ = link.front_end(tx, e, 1, b + s)
            ev[2].record()
            llr, _ = link.soft(rows)
            ev[3].record()
            dev.ldpc_decode(code, llr, scale=link.llr_scale, alpha=args.alpha, max_iter=args.max_iter)
            ev[4].record()
            torch.cuda.synchronize()
            ms += [ev[i].elapsed_time(ev[i + 1]) for i in range(4)]
        ms /= max(args.steps, 1)
        it_point = None
        if idd is not None:
            idd.reset_counts()
            differ = torch.zeros((), dtype=torch.int64, device="cuda")
            if lidd is not None:
                lidd.reset_counts()
            for blk in range(b):
                idd.run_block(e, seed=1, stream_id=blk)
                if lidd is not None:
                    lidd.run_block(e, seed=1, stream_id=blk)
                    differ += (idd.decided != lidd.decided).any(dim=1).sum()
            ibe, ife, inc, im, imean = idd.result()
            passes = idd.pass_results()
            # timing: front end once (not timed again), then every pass bracketed
            pev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * idd.outer + 1)]
            det_ms, dec_ms = np.zeros(idd.outer), np.zeros(idd.outer)
            for s in range(args.steps):
                tx = dev.ldpc_encode(code, idd.info_bits(b + s))
                rows, _ = idd.front_end(tx, e, 1, b + s)
                idd.begin(int(rows.shape[0]))
                pev[0].record()
                for o in range(idd.outer):
                    ext, _ = idd.detect(rows, first=o == 0)
                    pev[2 * o + 1].record()
                    idd.decode(ext)
                    pev[2 * o + 2].record()
                torch.cuda.synchronize()
                det_ms += [pev[2 * o].elapsed_time(pev[2 * o + 1]) for o in range(idd.outer)]
                dec_ms += [pev[2 * o + 1].elapsed_time(pev[2 * o + 2]) for o in range(idd.outer)]
            det_ms /= max(args.steps, 1)
            dec_ms /= max(args.steps, 1)
            it_point = {
                "coded_ber": ibe / im, "fer": ife / ncw, "info_bit_errors": ibe, "codeword_errors": ife, "open": inc,
                "total_inner_iters_mean": round(imean, 3),
                "per_pass": [{"info_bit_errors": p[0], "codeword_errors": p[1], "open": p[2], "iters_mean": round(p[3], 3)} for p in passes],
                "ms_per_block": {"detector_passes": [round(v, 4) for v in det_ms], "decoder_passes": [round(v, 4) for v in dec_ms],
                                 "detector_total": round(float(det_ms.sum()), 4), "decoder_total": round(float(dec_ms.sum()), 4)},
            }
            if lidd is not None:
                it_point["live_only"] = live_point(idd, lidd, differ, code, e, b, args.steps, ncw)
        fr_point = None
        if flink is not None:
            flink.reset_counts()
            for blk in range(b):
                flink.run_block(e, seed=1, stream_id=blk)
            fbe, ffe, fnc, fm, fmean = flink.result()
            fue, fum = flink.uncoded_result()
            blocks, wrong, lock = flink.sync_result()
            # the three framing kernels on one burst's λ, each bracketed by device events
            rows, _ = flink.front_end(dev.ldpc_encode(code, flink.info_bits(b)), e, 1, b)
            lam = (dev.cpm_soft(rows, flink.spec, 0, 0, d_rot=flink._d_rot)[0] if cpm else dev.viterbi_soft(rows, True)[0][1:])
            prior = torch.zeros(lam.numel(), dtype=torch.float32, device="cuda")
            ext = torch.zeros((per, code.n_tx), dtype=torch.float32, device="cuda")
            fev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            fms = np.zeros(3)
            for s in range(args.steps + 1):
                fev[0].record()
                fr.search(lam, flink.lock)
                fev[1].record()
                fr.gather(lam, flink.lock, per)
                fev[2].record()
                fr.scatter(ext, flink.lock, prior, 50.0)
                fev[3].record()
                torch.cuda.synchronize()
                if s:                                                     # (the first round warms up)
                    fms += [fev[i].elapsed_time(fev[i + 1]) for i in range(3)]
            fms /= max(args.steps, 1)
            fr_point = {"ebn0_channel_db": round(e + 10 * np.log10(code.k / fr.period), 3), "coded_ber": fbe / fm, "fer": ffe / ncw,
                        "info_bit_errors": fbe, "codeword_errors": ffe, "not_converged": fnc, "mean_iters": round(fmean, 3),
                        "uncoded_ber": fue / fum, "blocks": blocks, "wrong_locks": wrong, "last_lock": lock, "burst_llrs": int(lam.numel()),
                        "ms": {"frame_search": round(fms[0], 4), "frame_gather": round(fms[1], 4), "frame_scatter": round(fms[2], 4)}}
            if fidd is not None:
                fidd.reset_counts()
                differ = torch.zeros((), dtype=torch.int64, device="cuda")
                if lfidd is not None:
                    lfidd.reset_counts()
                for blk in range(b):
                    fidd.run_block(e, seed=1, stream_id=blk)
                    if lfidd is not None:
                        lfidd.run_block(e, seed=1, stream_id=blk)
                        differ += (fidd.decided != lfidd.decided).any(dim=1).sum()
                ibe, ife, inc, im, imean = fidd.result()
                fr_point["iterative"] = {
                    "coded_ber": ibe / im, "fer": ife / ncw, "info_bit_errors": ibe, "codeword_errors": ife, "open": inc,
                    "total_inner_iters_mean": round(imean, 3), "wrong_locks": fidd.sync_result()[1],
                    "per_pass": [{"info_bit_errors": p[0], "codeword_errors": p[1], "open": p[2], "iters_mean": round(p[3], 3)}
                                 for p in fidd.pass_results()]}
                if lfidd is not None:
                    fr_point["iterative"]["live_only"] = live_point(fidd, lfidd, differ, code, e, b, args.steps, ncw)
        out["points"].append({
            "ebn0_info_db": e, "ebn0_channel_db": round(e + 10 * np.log10(code.k / code.n_tx), 3), "codewords": ncw,
            "coded_ber": be / m, "fer": fe / ncw, "info_bit_errors": be, "codeword_errors": fe, "not_converged": nc,
            "mean_iters": round(mean_it, 3), "uncoded_ber": ue / um,
            "ms_per_block": {"encode": round(ms[0], 4), "front_end": round(ms[1], 4), "soft_detector": round(ms[2], 4),
                             "decode": round(ms[3], 4)},
            "decode_info_gbps": round(per * code.k / (ms[3] * 1e-3) / 1e9, 3) if ms[3] > 0 else None,
            **({"iterative": it_point} if it_point is not None else {}),
            **({"framed": fr_point} if fr_point is not None else {}),
        })
    print(json.dumps(out))


if __name__ == "__main__":
    main()
