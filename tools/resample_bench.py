"""``mf_bank_resample`` next to ``mf_bank`` on the same noisy samples, the same taps and the same rows; prints ONE JSON line.

    python tools/resample_bench.py [--rows 211252 10000000] [--detector PT PAM] [--steps 20] [--warmup 3]
    python tools/resample_bench.py --waveform multih|pcmfm [--rows ...] [--steps 20] [--warmup 3]

Both kernels read ``sps`` complex128 samples and write one 48-byte row per symbol; the resampler adds the instant of every
row and four real-by-complex multiply-adds per sample a row reads.  The two alternate launch by launch, each bracketed by
device events; per shape the median times, their ratio and the bytes moved per second (samples read once + rows written).
``--tau`` picks the trajectory: ``none`` (the bank's own instants, μ = 0), ``const`` (one fraction), ``ramp`` (a drift of
0.8 samples per 256-row window: the fraction and the integer part change along the burst).

``--waveform multih|pcmfm``: ``cpm_mf_rows_resample`` next to ``cpm_mf_rows`` with the link's templates (16 / 4 filters of 9
taps, a row of 16 nfilt bytes per symbol); BOTH calls allocate their rows inside the timed region.  The ramp drifts by the
waveform's documented ``MAX_DRIFT_SAMPLES`` per window of the recovery's default length."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[211252, 10_000_000])
    ap.add_argument("--detector", nargs="+", default=["PT", "PAM"], choices=["PT", "PAM"])
    ap.add_argument("--tau", nargs="+", default=["none", "const", "ramp"], choices=["none", "const", "ramp"])
    ap.add_argument("--waveform", default="soqpsk", choices=["soqpsk", "multih", "pcmfm"])
    ap.add_argument("--sps", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch

    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.cpm.soqpsk import freq_pulse_soqpsk_tg
    from waveforms_amd.filters.matched import pam_matched_filter_taps, pt_matched_filter_taps

    torch.cuda.set_device(0)
    if args.waveform != "soqpsk":
        return main_cpm(args)
    sps, W = args.sps, 256
    out = {"tool": "resample_bench", "sps": sps, "steps": args.steps, "points": []}
    for det in args.detector:
        taps = np.ascontiguousarray((pt_matched_filter_taps if det == "PT" else pam_matched_filter_taps)(freq_pulse_soqpsk_tg(sps), 0.25, sps))
        d_taps = _hip.to_device(taps)
        for rows in args.rows:
            nsamp = (rows + 2) * sps
            received = dev.awgn(None, nsamp, 1.0, 1, 0, 0)
            nwin = -(-rows // W)
            forms = {"none": (None, 0.0), "const": (None, 0.37), "ramp": (_hip.to_device(-0.8 * np.arange(nwin, dtype=np.float64)), 0.37)}
            work = _hip.empty((rows, 3, 2), "float64")
            for name in args.tau:
                tau, tau0 = forms[name]
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                ms = [[], []]
                first = sps + (int(0.8 * nwin) + 1 if name == "ramp" else 0)       # (the ramp walks back 0.8 samples per window: the rows stay inside)
                for s in range(args.warmup + args.steps):
                    ev[0].record()
                    dev.mf_bank(received, d_taps, sps, sps, rows)
                    ev[1].record()
                    dev.mf_bank_resample(received, d_taps, first, sps, rows, W, tau, tau0, out=work)
                    ev[2].record()
                    torch.cuda.synchronize()
                    if s >= args.warmup:
                        ms[0].append(ev[0].elapsed_time(ev[1]))
                        ms[1].append(ev[1].elapsed_time(ev[2]))
                bank, res = float(np.median(ms[0])), float(np.median(ms[1]))
                moved = 16.0 * nsamp + 48.0 * rows
                out["points"].append({"detector": det, "ntaps": int(taps.shape[1]), "rows": rows, "tau": name, "mf_bank_ms": round(bank, 4),
                                      "mf_bank_resample_ms": round(res, 4), "ratio": round(res / bank, 3), "mf_bank_gb_s": round(moved / bank / 1e6, 1),
                                      "mf_bank_resample_gb_s": round(moved / res / 1e6, 1)})
    print(json.dumps(out))


def main_cpm(args) -> None:
    """``cpm_mf_rows_resample`` next to ``cpm_mf_rows``: ARTM (nh 2, 16 filters) or PCM/FM (nh 1, 4 filters), 9 taps at sps 8."""
    import torch

    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.sync.timing_cpm import MAX_DRIFT_SAMPLES, defaults
    from waveforms_amd.viterbi import cpm

    if args.waveform == "multih":
        from waveforms_amd.cpm.multih import freq_pulse_multih_irig as freq_pulse
    else:
        from waveforms_amd.cpm.pcmfm import freq_pulse_pcmfm as freq_pulse
    sps = args.sps
    spec = cpm.ARTM_64 if args.waveform == "multih" else cpm.PCMFM_20
    W, drift = defaults(spec)["window"], MAX_DRIFT_SAMPLES[args.waveform]
    d_templates = _hip.to_device(cpm.matched_filter_templates(np.asarray(freq_pulse(sps), dtype=np.float64), sps, cpm.full_phase(spec)))
    nfilt, ntm = int(d_templates.shape[1]), int(d_templates.shape[2])
    out = {"tool": "resample_bench", "waveform": args.waveform, "sps": sps, "steps": args.steps, "window": W, "points": []}
    for rows in args.rows:
        nsamp = (rows + 2) * sps
        received = dev.awgn(None, nsamp, 1.0, 1, 0, 0)
        nwin = -(-rows // W)
        forms = {"none": (None, 0.0), "const": (None, 0.37), "ramp": (_hip.to_device(-drift * np.arange(nwin, dtype=np.float64)), 0.37)}
        for name in args.tau:
            tau, tau0 = forms[name]
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ms = [[], []]
            start0 = sps + (int(drift * nwin) + 1 if name == "ramp" else 0)      # (the ramp walks back: the rows stay inside)
            for s in range(args.warmup + args.steps):
                ev[0].record()
                dev.cpm_mf_rows(received, d_templates, sps, sps, rows)
                ev[1].record()
                dev.cpm_mf_rows_resample(received, d_templates, start0, sps, rows, W, tau, tau0)
                ev[2].record()
                torch.cuda.synchronize()
                if s >= args.warmup:
                    ms[0].append(ev[0].elapsed_time(ev[1]))
                    ms[1].append(ev[1].elapsed_time(ev[2]))
            plain, res = float(np.median(ms[0])), float(np.median(ms[1]))
            moved = 16.0 * nsamp + 16.0 * nfilt * rows
            out["points"].append({"nfilt": nfilt, "ntm": ntm, "rows": rows, "tau": name, "cpm_mf_rows_ms": round(plain, 4),
                                  "cpm_mf_rows_resample_ms": round(res, 4), "ratio": round(res / plain, 3),
                                  "min_ms": [round(min(ms[0]), 4), round(min(ms[1]), 4)], "max_ms": [round(max(ms[0]), 4), round(max(ms[1]), 4)],
                                  "cpm_mf_rows_gb_s": round(moved / plain / 1e6, 1), "cpm_mf_rows_resample_gb_s": round(moved / res / 1e6, 1)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
