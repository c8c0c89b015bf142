#!/usr/bin/env python
"""The multi-symbol noncoherent PCM/FM detector on the MI355X: its time against the coherent pair, its uncoded BER with and
without a frequency offset, and the coded link against the genie-phase coherent link -> profiles/noncoherent_pcmfm.json.

    python tools/noncoherent_bench.py [--out profiles/noncoherent_pcmfm.json] [--parts time ber offsets coded]
        [--bits 211252 10000000] [--warmup 3] [--repeats 15] [--batch 10] [--ber-bits 1000000] [--ber-blocks 10]
        [--ncw 16] [--steps 40] [--ebn0 3.0 3.5 ...]

time     ``noncoherent_soft`` for N = 3, 5, 7 on each burst (random samples: the time does not depend on them), ``--batch`` launches
         between two device events, warm-up rounds first, median and spread over the repeats; beside it, on the same samples, the
         coherent pair ``cpm_mf_rows`` + ``cpm_soft`` (PCMFM_20), each stage and their sum.  Shares of peak: the operations and
         bytes the algorithm needs (2^N N sps complex multiply-adds of 8 flops per bit; every sample read once, 9 bytes written per
         bit) over the time, against 78.6 Tflop/s fp64 and 8 TB/s HBM; ``executed_flops`` counts the zero rows of N = 3 too.
ber      uncoded bit errors of the device chain (``symbol_map`` -> ``cpm_modulate`` -> ``awgn`` -> ``noncoherent_soft``) by channel
         Eb/N0 5 .. 10 dB for the three N at ν = 0, bits c .. nbits - 1 - c of every block compared.
offsets  the same curve for N = 5 at ν = 1e-3 and 2e-3 cycles per sample (``carrier_offset`` with a phase of 40 degrees).
coded    ``NoncoherentPCMFMLink`` (demo code, framed, 40 degrees and ν = 1e-3, N = 5) against the genie-phase ``CodedCPMLink`` at
         ν = 0 on the same information bits; the distance in dB at FER 1e-2, interpolated in log10 FER (None: a curve does not
         cross 1e-2 inside the sweep).
A part that was not run is absent from the record: nothing is estimated.
"""
from __future__ import annotations

import argparse
import json
import math
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

FP64_PEAK, HBM_PEAK = 78.6e12, 8.0e12
OBSERVATIONS = (3, 5, 7)


def _stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def _timed(calls: dict, warmup: int, repeats: int, batch: int) -> dict:
    import torch

    times = {s: [] for s in calls}
    for it in range(warmup + repeats):
        for s, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(batch):
                fn()
            e1.record()
            e1.synchronize()
            if it >= warmup:
                times[s].append(e0.elapsed_time(e1) / batch)
    return {s: _stats(v) for s, v in times.items()}


def part_time(args) -> list:
    import torch

    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.cpm.pcmfm import freq_pulse_pcmfm
    from waveforms_amd.viterbi import cpm
    from waveforms_amd.viterbi import noncoherent as nc

    sps, spec = args.sps, cpm.PCMFM_20
    pulse = np.asarray(freq_pulse_pcmfm(sps), dtype=np.float64)
    d_rot = _hip.to_device(cpm.rotation_table(spec))
    d_mf = _hip.to_device(cpm.matched_filter_templates(pulse, sps, cpm.full_phase(spec)))
    tables = {N: dev.noncoherent_templates(pulse, 0.7, sps, N) for N in OBSERVATIONS}
    start = nc.burst_start(pulse.size, sps, nc.DEFAULT_OFFSET)
    rows_out = []
    for nbits in args.bits:
        n = (nbits + 1) * sps
        x = torch.randn((n, 2), dtype=torch.float64, device="cuda")
        geo = cpm.filter_geometry(pulse.size, sps, spec, nbits)
        start0, ncalls = int(geo["start0"]), int(geo["ncalls"])
        out = (_hip.empty(nbits, "float64"), _hip.empty(nbits, "uint8"))
        rows = dev.cpm_mf_rows(x, d_mf, start0, sps, ncalls)
        calls = {f"noncoherent_N{N}": (lambda N=N: dev.noncoherent_soft(x, tables[N], sps, start, nbits, out=out)) for N in OBSERVATIONS}
        calls["cpm_mf_rows"] = lambda: dev.cpm_mf_rows(x, d_mf, start0, sps, ncalls)
        calls["cpm_soft"] = lambda: dev.cpm_soft(rows, spec, 0, 0, d_rot=d_rot)
        t = _timed(calls, args.warmup, args.repeats, args.batch)
        _hip.device_check()
        coherent = t["cpm_mf_rows"]["median_ms"] + t["cpm_soft"]["median_ms"]
        row = {"bits": nbits, "samples": n, "coherent_calls": ncalls, **t, "coherent_pair_median_ms": coherent}
        for N in OBSERVATIONS:
            ms = t[f"noncoherent_N{N}"]["median_ms"]
            flops = 8.0 * (1 << N) * N * sps * nbits
            nbytes = 16.0 * n + 9.0 * nbits
            least = max(flops / FP64_PEAK, nbytes / HBM_PEAK)
            row[f"noncoherent_N{N}"].update({
                "over_coherent_pair": ms / coherent, "flops": flops, "executed_flops": 8.0 * max(1 << N, 16) * N * sps * nbits, "bytes": nbytes,
                "tflops": flops / (ms * 1e9), "gb_per_s": nbytes / (ms * 1e6), "share_of_fp64_peak": flops / FP64_PEAK / (ms * 1e-3),
                "share_of_hbm_peak": nbytes / HBM_PEAK / (ms * 1e-3), "bound_by": "fp64" if flops / FP64_PEAK >= nbytes / HBM_PEAK else "hbm",
                "share_of_peak": least / (ms * 1e-3), "geometry": dev.noncoherent_geometry(N, sps, nbits)})
        rows_out.append(row)
        del x, rows, out
    return rows_out


def _ber_curve(args, N: int, nu: float) -> list:
    import torch

    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.cpm.pcmfm import freq_pulse_pcmfm
    from waveforms_amd.encoding.coded import DEROTATION
    from waveforms_amd.viterbi import cpm
    from waveforms_amd.viterbi import noncoherent as nc

    sps, nbits, c = args.sps, args.ber_bits, (N - 1) // 2
    pulse = np.asarray(freq_pulse_pcmfm(sps), dtype=np.float64)
    d_h, d_pulse, table = _hip.to_device(np.array([0.7])), _hip.to_device(pulse), dev.noncoherent_templates(pulse, 0.7, sps, N)
    start = nc.burst_start(pulse.size, sps, nc.DEFAULT_OFFSET)
    gen = torch.Generator(device="cuda")
    points = []
    for ebn0 in args.ber_ebn0:
        sigma, errors = cpm.sigma_for_ebn0(ebn0, sps, 1), torch.zeros((), dtype=torch.int64, device="cuda")
        for b in range(args.ber_blocks):
            gen.manual_seed(1000 + b)
            bits = torch.randint(0, 2, (nbits,), dtype=torch.uint8, device="cuda", generator=gen)
            sig = dev.cpm_modulate(dev.symbol_map(2, bits), d_h, d_pulse, sps)
            if nu:
                dev.carrier_offset(sig, math.radians(40.0), nu, 0, out=sig)
            rx = dev.awgn(sig, int(sig.shape[0]), sigma, 7, b, 0, DEROTATION)
            _lam, hard = dev.noncoherent_soft(rx, table, sps, start, nbits)
            errors += (hard[c:nbits - c] != bits[c:nbits - c]).sum()
        _hip.device_check()
        compared = args.ber_blocks * (nbits - 2 * c)
        points.append({"ebn0_db": ebn0, "errors": int(errors.cpu()), "compared": compared, "ber": int(errors.cpu()) / compared})
    return points


def _ebn0_at_fer(points, key, target=1e-2):
    """Eb/N0 where the curve ``key`` crosses ``target``, interpolated in log10 FER between the sweep's points (None: no crossing)."""
    pts = sorted((p["ebn0_info_db"], p[key]["fer"]) for p in points)
    for (e0, f0), (e1, f1) in zip(pts, pts[1:]):
        if f0 >= target > f1:
            if f1 <= 0.0:
                f1 = 0.1 * target / max(1, points[0]["codewords"])       # (no error seen: the crossing is bounded, not located)
            return e0 + (e1 - e0) * (np.log10(f0) - np.log10(target)) / (np.log10(f0) - np.log10(f1))
    return None


def part_coded(args) -> dict:
    from waveforms_amd.encoding import framing as FR
    from waveforms_amd.encoding import ldpc
    from waveforms_amd.encoding.coded import CodedCPMLink
    from waveforms_amd.encoding.noncoherent import NoncoherentPCMFMLink

    code = ldpc.demo_code()
    fr, lead, carrier = FR.Framing(code), 37, (math.radians(40.0), 1e-3)
    links = {"noncoherent": NoncoherentPCMFMLink(code, args.ncw, args.sps, 5, framing=fr, lead_bits=lead, carrier=carrier),
             "coherent_genie": CodedCPMLink(code, args.ncw, "pcmfm", args.sps, framing=fr, lead_bits=lead)}
    points = []
    for ebn0 in args.ebn0:
        point = {"ebn0_info_db": ebn0, "codewords": args.steps * args.ncw}
        for name, link in links.items():
            link.reset_counts()
            for s in range(args.steps):
                link.run_block(ebn0, seed=11, stream_id=s)
            be, fe, _nc, nb, its = link.result()
            ue, un = link.uncoded_result()
            blocks, wrong, _rec = link.sync_result()
            point[name] = {"bit_errors": be, "codeword_errors": fe, "info_bits": nb, "fer": fe / (args.steps * args.ncw), "mean_iterations": its,
                           "channel_ber": ue / un, "wrong_locks": wrong, "blocks": blocks}
        points.append(point)
    at = {name: _ebn0_at_fer(points, name) for name in links}
    gap = None if None in at.values() else at["noncoherent"] - at["coherent_genie"]
    return {"code": "demo (2048, 1024)", "ncw": args.ncw, "steps": args.steps, "carrier_deg_nu": [40.0, 1e-3], "observe": 5, "framed": True, "lead_bits": lead,
            "points": points, "ebn0_at_fer_1e-2": at, "noncoherent_minus_genie_db_at_fer_1e-2": gap}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["time", "ber", "offsets", "coded"])
    ap.add_argument("--bits", type=int, nargs="+", default=[211_252, 10_000_000])
    ap.add_argument("--sps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--ber-bits", type=int, default=1_000_000)
    ap.add_argument("--ber-blocks", type=int, default=10)
    ap.add_argument("--ber-ebn0", type=float, nargs="+", default=[5.0, 6.0, 7.0, 8.0, 9.0, 10.0])
    ap.add_argument("--ncw", type=int, default=16)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--ebn0", type=float, nargs="+", default=[3.0, 3.5, 4.0, 4.5, 5.0, 5.5, 6.0, 6.5, 7.0, 7.5, 8.0])
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    from waveforms_amd.viterbi import noncoherent as nc

    result = {"device": torch.cuda.get_device_name(0), "sps": args.sps, "default_offset": nc.DEFAULT_OFFSET,
              "max_offset_cycles": {str(k): v for k, v in nc.MAX_OFFSET_CYCLES.items()},
              "host_scan": json.loads((ROOT / "tests" / "golden" / "noncoherent_scan.json").read_text())}

    def save() -> None:
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(result, indent=1) + "\n")

    if "time" in args.parts:
        result["time"] = {"warmup": args.warmup, "repeats": args.repeats, "batch": args.batch, "fp64_peak_flops": FP64_PEAK, "hbm_peak_bytes_per_s": HBM_PEAK,
                          "bursts": part_time(args)}
        save()
    if "ber" in args.parts:
        result["uncoded_ber"] = {"bits_per_block": args.ber_bits, "blocks": args.ber_blocks,
                                 "curves": {f"N{N}": _ber_curve(args, N, 0.0) for N in OBSERVATIONS}}
        save()
    if "offsets" in args.parts:
        result["uncoded_ber_offsets_N5"] = {"bits_per_block": args.ber_bits, "blocks": args.ber_blocks, "phase_deg": 40.0,
                                            "curves": {repr(nu): _ber_curve(args, 5, nu) for nu in (1e-3, 2e-3)}}
        save()
    if "coded" in args.parts:
        result["coded_fer"] = part_coded(args)
        save()
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
