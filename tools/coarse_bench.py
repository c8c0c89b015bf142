#!/usr/bin/env python
"""The time of the coarse frequency acquisition's three stages (``coarse_lines``, ``coarse_estimate``, ``carrier_offset_dev``) on
bursts of 211 252 and 1e7 bits at sps 8, against ``carrier_offset`` over the same samples - a read-and-write pass of the same
array, the yardstick for a stage that reads every sample once.

    python tools/coarse_bench.py [--bits 211252 10000000] [--nfft 4096] [--smooth 4] [--warmup 5] [--repeats 30] [--batch 20] [--out FILE.json]

Per stage, ``--batch`` launches back to back between two device events (every buffer, the lines' scratch too, allocated beforehand),
so that the figure is a launch's share of a full queue and not the host's gap between two wrapper calls: ``estimate`` and the
correction of a short burst take about ten microseconds, which a single bracketed call cannot resolve.  Warm-up rounds first, the
median and the spread (min, max) over the repeats; one JSON result.  ``coarse_total_median_ms`` is the sum of the three stages'
medians: what the stage adds to a queue that is kept full, not the latency of one call from the host.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def _stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, nargs="+", default=[211_252, 10_000_000])
    ap.add_argument("--sps", type=int, default=8)
    ap.add_argument("--nfft", type=int, default=4096)
    ap.add_argument("--smooth", type=int, default=0, help="0: sps // 2")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--batch", type=int, default=20, help="launches of a stage between its two events")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.sync.coarse import CoarseFrequency

    rec = CoarseFrequency(args.sps, nfft=args.nfft, smooth=args.smooth or None)
    window = _hip.to_device(np.hanning(rec.nfft))
    stages = ("lines", "estimate", "correct", "carrier_offset")
    result = {"sps": rec.sps, "nfft": rec.nfft, "smooth": rec.smooth, "search": rec.search, "warmup": args.warmup, "repeats": args.repeats,
              "batch": args.batch,
              "device": torch.cuda.get_device_name(0), "bursts": []}
    for nbits in args.bits:
        n = nbits * rec.sps
        k = torch.arange(n, dtype=torch.float64, device="cuda")
        x = torch.stack((torch.cos(0.3 * k), torch.sin(0.3 * k)), dim=1).contiguous()      # any samples: the time does not depend on them
        del k
        x += 0.5 * torch.randn((n, 2), dtype=torch.float64, device="cuda")
        out = torch.empty_like(x)
        spectra, found = _hip.empty((2, rec.nfft), "float64"), _hip.empty(4, "float64")
        scratch = _hip.empty(_hip.lib().wf_coarse_scratch_doubles(n, rec.sps, rec.nfft, rec.smooth), "float64")
        calls = {"lines": lambda: dev.coarse_lines(x, rec.sps, rec.smooth, rec.nfft, window, out=spectra, scratch=scratch),
                 "estimate": lambda: dev.coarse_estimate(spectra, rec.sps, rec.search, out=found),
                 "correct": lambda: dev.carrier_offset_dev(x, found, -1.0, 0, out=out),
                 "carrier_offset": lambda: dev.carrier_offset(x, 0.0, 1e-3, 0, out=out)}
        times = {s: [] for s in stages}
        for it in range(args.warmup + args.repeats):
            for s in stages:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.batch):
                    calls[s]()
                e1.record()
                e1.synchronize()
                if it >= args.warmup:
                    times[s].append(e0.elapsed_time(e1) / args.batch)
        _hip.device_check()
        row = {"bits": nbits, "samples": n, "segments": (n - rec.smooth + 1) // rec.sps // rec.nfft, **{s: _stats(times[s]) for s in stages}}
        row["coarse_total_median_ms"] = sum(row[s]["median_ms"] for s in stages[:3])
        row["lines_over_carrier_offset"] = row["lines"]["median_ms"] / row["carrier_offset"]["median_ms"]
        row["lines_read_gb_per_s"] = 16.0 * n / (row["lines"]["median_ms"] * 1e6)
        result["bursts"].append(row)
        del x, out, scratch
    text = json.dumps(result, indent=1)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
