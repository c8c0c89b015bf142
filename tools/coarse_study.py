#!/usr/bin/env python
"""The host study behind ``MAX_OFFSET_BITS`` and ``MIN_BITS`` of waveforms_amd/sync/coarse.py: the error of
``coarse_estimate_host`` (numpy, no GPU) on SOQPSK-TG bursts of random bits from the oracle's modulator, over the carrier
offset, the burst length, the noise and the prefilter.

    python tools/coarse_study.py [--trials T] [--out FILE.json]

Per (smooth, segments of nfft 4096 bits, channel Eb/N0, |nu| sps): the largest |nu^ - nu| in cycles per sample over the trials
(random sign of nu, random phase, fresh noise) and the number of trials beyond the fine recovery's limit
MAX_DRIFT_TURNS / (sps W) = 2.4e-5.  The result is printed as JSON (and written to --out).
"""
from __future__ import annotations

import argparse
import json
import math
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from oracle import numpy_ref as ref  # noqa: E402
from waveforms_amd.sync import carrier as C  # noqa: E402
from waveforms_amd.sync import coarse as K  # noqa: E402

SPS, NFFT = 8, 4096
OFFSETS = (0.0, 0.05, 0.1, 0.15, 0.2, 0.22, 0.24)
SEGMENTS = (1, 2, 4, 50)
EBN0 = (-1.0, 1.0, 3.0, 5.0)


def burst(rng, nbits: int) -> np.ndarray:
    bits = rng.integers(0, 2, nbits).astype(np.uint8)
    symbols, _, _ = ref.fsm_encode("SOQPSKTrellis4x2DiffEncoded", bits)
    _t, sig = ref.cpm_modulate(symbols, 0.25, ref.freq_pulse_soqpsk_tg(SPS), SPS)
    return np.asarray(sig, dtype=np.complex128)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=8, help="trials per point (a quarter of it, at least 2, at 50 segments)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    limit = C.MAX_DRIFT_TURNS / (SPS * C.DEFAULT_WINDOW)
    rng = np.random.default_rng(2024)
    rows = []
    for nseg in SEGMENTS:
        trials = args.trials if nseg < 50 else max(2, args.trials // 4)
        sigs = [burst(rng, nseg * NFFT + 8) for _ in range(trials)]
        for ebn0 in EBN0:
            sigma = ref.sigma_for_ebn0(ebn0, SPS)
            for off in OFFSETS:
                worst = {1: 0.0, SPS // 2: 0.0}
                beyond = {1: 0, SPS // 2: 0}
                for sig in sigs:
                    nu = off / SPS * (1.0 if rng.integers(0, 2) else -1.0)
                    x = C.carrier_offset_host(sig, float(rng.uniform(0.0, 2.0 * math.pi)), nu)
                    x = x + sigma * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size))
                    for S in worst:
                        err = abs(float(K.estimate_host(x, SPS, NFFT, S)[0]) - nu)
                        worst[S] = max(worst[S], err)
                        beyond[S] += err > limit
                for S in worst:
                    rows.append({"smooth": S, "segments": nseg, "ebn0_db": ebn0, "offset_bits": off, "trials": trials,
                                 "max_abs_error": worst[S], "beyond_fine_limit": int(beyond[S])})
                print(f"segments {nseg:2d}  Eb/N0 {ebn0:+.0f} dB  |nu| sps {off:.2f}:  " +
                      "  ".join(f"smooth {S}: max {worst[S]:.2e} ({beyond[S]}/{trials} beyond)" for S in worst), file=sys.stderr, flush=True)
    result = {"sps": SPS, "nfft": NFFT, "search": K.DEFAULT_SEARCH, "fine_limit_cycles_per_sample": limit, "rows": rows}
    text = json.dumps(result, indent=1)
    if args.out:
        Path(args.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
