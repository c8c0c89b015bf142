"""Soft-output SOQPSK detector alone (wf_viterbi4_soft) on one block of link rows; prints ONE JSON line.

    python tools/soft_bench.py [--calls 1e7] [--ebn0 10] [--detector PT] [--steps 20] [--warmup-steps 3] [--soft-warmup 0]
    python tools/soft_bench.py --waveform multih|pcmfm [...]     the CPM soft detector (wf_cpm_soft): main_cpm
    python tools/soft_bench.py --waveform multih|pcmfm --apriori [--apriori-sigma 8]
                                                                 ... and one a-priori pass (wf_cpm_soft_apriori) beside it

The rows are what SOQPSKLink(calls, fuse=15) leaves in its workspace (detector-packed, 32 B per call: layout()["off_mf"],
layout()["row_bytes"]); the link's own length-2 detector runs on them once, for its bit errors; the transmitted bits are
the block's PN23 sequence.  Then the soft detector runs `--warmup-steps` untimed and `--steps` timed passes over the same
rows: device events around the timed window, and a host clock around it that ends in a synchronise.  Reported next to the time: the launch geometry
(wf_viterbi4_soft_geometry), chunk repairs per pass, the bit errors of λ < 0 (transmitted bit j against λ_{j+1}) beside the
length-2 detector's, and the effective LLR scale: the c that best fits the error rate per bin of |λ| to 1 / (1 + e^{c |λ|})
(maximum likelihood over bins 0.25 σ² wide), given as c σ² — 1 would mean λ / σ² is the exact log-likelihood ratio.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def fit_scale(abs_llr: np.ndarray, err: np.ndarray, sigma2: float, width: float = 0.25) -> float:
    """c σ² maximising the binned likelihood of the errors under P(error | |λ|) = 1 / (1 + e^{c |λ|})."""
    x = abs_llr / sigma2
    b = np.floor(x / width).astype(np.int64)
    tot = np.bincount(b)
    errs = np.bincount(b, weights=err.astype(np.float64), minlength=tot.size)
    xs = np.bincount(b, weights=x, minlength=tot.size)
    keep = tot > 0
    tot, errs, xm = tot[keep], errs[keep], xs[keep] / tot[keep]

    def nll(c):
        return float(np.sum(errs * np.logaddexp(0.0, c * xm) + (tot - errs) * np.logaddexp(0.0, -c * xm)))

    lo, hi = 0.0, 4.0                                   # golden-section search; c σ² is well inside
    g = (np.sqrt(5.0) - 1.0) / 2.0
    a, bb = hi - g * (hi - lo), lo + g * (hi - lo)
    fa, fb = nll(a), nll(bb)
    for _ in range(80):
        if fa < fb:
            hi, bb, fb = bb, a, fa
            a = hi - g * (hi - lo)
            fa = nll(a)
        else:
            lo, a, fa = a, bb, fb
            bb = lo + g * (hi - lo)
            fb = nll(bb)
    return 0.5 * (lo + hi)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=float, default=1e7)
    ap.add_argument("--ebn0", type=float, default=10.0)
    ap.add_argument("--detector", default="PT", choices=["PT", "PAM"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup-steps", type=int, default=3)
    ap.add_argument("--soft-warmup", type=int, default=0, help="warm-up rows of the soft detector (0: library default)")
    ap.add_argument("--opt", action="append", default=[], help="wf_ctx option key=value, e.g. soft_chunk_calls=64")
    ap.add_argument("--waveform", default="soqpsk", choices=["soqpsk", "multih", "pcmfm"],
                    help="soqpsk: wf_viterbi4_soft (above); multih / pcmfm: wf_cpm_soft on one CPMLink block's rows (main_cpm)")
    ap.add_argument("--apriori", action="store_true",
                    help="CPM waveforms: also time wf_cpm_soft_apriori on the same rows (random prior, and a NULL prior)")
    ap.add_argument("--apriori-sigma", type=float, default=8.0, help="standard deviation of the random prior (clipped to +-50)")
    args = ap.parse_args()
    if args.waveform != "soqpsk":
        return main_cpm(args)

    import torch

    from waveforms.glfsr import PNSequence
    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.link import SOQPSKLink, sigma_for_ebn0

    _hip.apply_option_args(args.opt)
    torch.cuda.set_device(0)
    nsym, sps = int(args.calls), 8
    link = SOQPSKLink(nsym, sps, detector=args.detector, fuse=15, private_ctx=True)
    link.run_block(args.ebn0, seed=1)
    _hse, hbe, hm = link.result()
    lay = link.layout()
    rb, ncalls = lay["row_bytes"], lay["calls"]
    rows = link.workspace[lay["off_mf"]:lay["off_mf"] + ncalls * rb].clone().view(torch.float64)
    tx = PNSequence(23).generate(nsym, device=True)          # what the block sent (seed 1, skip 0)
    del link

    ctx = _hip.new_ctx()
    try:
        geom = dev.viterbi_soft_geometry(ncalls, args.soft_warmup, ctx=ctx)
        for _ in range(args.warmup_steps):
            llr, bits = dev.viterbi_soft(rows, True, args.soft_warmup, rb, ctx=ctx)
        torch.cuda.synchronize()
        dev.viterbi_repaired(reset=True, ctx=ctx)
        dev.viterbi_unmerged(reset=True, ctx=ctx)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(args.steps):
            llr, bits = dev.viterbi_soft(rows, True, args.soft_warmup, rb, ctx=ctx)
        e1.record()
        torch.cuda.synchronize()
        host_ms = (time.perf_counter() - t0) * 1e3 / args.steps
        ev_ms = e0.elapsed_time(e1) / args.steps
        repaired = dev.viterbi_repaired(reset=True, ctx=ctx)
        unproven = dev.viterbi_unmerged(reset=True, ctx=ctx)
    finally:
        _hip.free_ctx(ctx)

    llr_h, bits_h, tx_h = _hip.to_host(llr), _hip.to_host(bits), _hip.to_host(tx)
    m = min(tx_h.size, bits_h.size - 1)
    err = bits_h[1:1 + m] != tx_h[:m]
    sigma2 = sigma_for_ebn0(args.ebn0, sps) ** 2
    scale = fit_scale(np.abs(llr_h[1:1 + m]), err, sigma2) if err.any() else None
    print(json.dumps({
        "tool": "soft_bench", "detector": args.detector, "ebn0_db": args.ebn0, "calls": ncalls, "row_bytes": rb,
        "geometry": geom, "steps": args.steps, "warmup_steps": args.warmup_steps,
        "ms_per_block_events": round(ev_ms, 4), "ms_per_block_host": round(host_ms, 4),
        "gsym_per_s": round(ncalls / (ev_ms * 1e-3) / 1e9, 3),
        "repairs_per_block": repaired / args.steps, "unproven": unproven,
        "soft_bit_errors": int(err.sum()), "soft_compared": int(m),
        "hard_len2_bit_errors": int(hbe), "hard_len2_compared": int(hm),
        "llr_scale_c_sigma2": None if scale is None else round(scale, 4),
    }))


def main_cpm(args) -> None:
    """--waveform multih | pcmfm: the CPM soft detector (wf_cpm_soft, full-phase trellis) alone on the rows one CPMLink block
    leaves in its workspace (layout()["off_rows"]: calls x M^Lp complex128).  Bit errors of λ < 0 (transmitted bit j against
    λ[j]) next to the link's own reduced detector (ARTM_16 / PCMFM_10, its counts) and the full-phase hard detector on the
    same rows, over the link's compared symbols; c σ² fitted as above, σ from cpm.sigma_for_ebn0."""
    import torch

    from waveforms_amd import _hip
    from waveforms_amd import device as dev
    from waveforms_amd.link import CPMLink
    from waveforms_amd.viterbi.cpm import CPMTrellisDetector, full_phase, rotation_table, sigma_for_ebn0

    _hip.apply_option_args(args.opt)
    torch.cuda.set_device(0)
    nsym, sps = int(args.calls), 8
    link = CPMLink(nsym, sps, waveform=args.waveform, private_ctx=True)
    link.run_block(args.ebn0, seed=1)
    _hse, hbe, hm = link.result()
    lay = link.layout()
    ncalls, spec = lay["calls"], link.spec
    rows = link.workspace[lay["off_rows"]:lay["off_rows"] + ncalls * spec.nfilt * 16].clone().view(torch.float64).view(ncalls, spec.nfilt, 2)
    alpha = link.workspace[lay["off_syms"]:lay["off_syms"] + nsym].clone().view(torch.int8)
    skip_head = int(link.cfg.skip_head)
    del link
    fspec = full_phase(spec)
    M, lg, D = fspec.M, fspec.bits_per_symbol, fspec.D

    ctx = _hip.new_ctx()
    try:
        geom = dev.cpm_soft_geometry(fspec, ncalls, args.soft_warmup, ctx=ctx)
        d_rot = _hip.to_device(rotation_table(fspec))
        for _ in range(args.warmup_steps):
            llr, bits = dev.cpm_soft(rows, fspec, 0, args.soft_warmup, ctx=ctx, d_rot=d_rot)
        torch.cuda.synchronize()
        dev.viterbi_repaired(reset=True, ctx=ctx)
        dev.viterbi_unmerged(reset=True, ctx=ctx)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(args.steps):
            llr, bits = dev.cpm_soft(rows, fspec, 0, args.soft_warmup, ctx=ctx, d_rot=d_rot)
        e1.record()
        torch.cuda.synchronize()
        host_ms = (time.perf_counter() - t0) * 1e3 / args.steps
        ev_ms = e0.elapsed_time(e1) / args.steps
        repaired = dev.viterbi_repaired(reset=True, ctx=ctx)
        unproven = dev.viterbi_unmerged(reset=True, ctx=ctx)
        ap = apriori_passes(args, dev, _hip, torch, rows, fspec, d_rot, ctx, ev_ms) if args.apriori else None
    finally:
        _hip.free_ctx(ctx)

    def to_bits(u):
        u = u.to(torch.uint8)
        return (u.view(-1) if M == 2 else torch.stack([(u >> 1) & 1, u & 1], dim=1).reshape(-1)).cpu().numpy()

    tx = to_bits((alpha.to(torch.int16) + (M - 1)) // 2)
    hard = to_bits(CPMTrellisDetector(fspec).detect_device(rows)[D - 1:])       # symbol j, decided at call j + D - 1
    lo, hi = skip_head * lg, (skip_head + int(hm)) * lg                         # the link's compared symbols
    llr_h, bits_h = _hip.to_host(llr), _hip.to_host(bits)
    err = bits_h[lo:hi] != tx[lo:hi]
    sigma2 = sigma_for_ebn0(args.ebn0, sps, lg) ** 2
    scale = fit_scale(np.abs(llr_h[lo:hi]), err, sigma2) if err.any() else None
    print(json.dumps({
        "tool": "soft_bench", "waveform": args.waveform, "spec": f"M {M} p {fspec.p} K {list(fspec.K)} Lp {fspec.Lp}: {fspec.nstates} states",
        "ebn0_db": args.ebn0, "calls": ncalls, "geometry": geom, "steps": args.steps, "warmup_steps": args.warmup_steps,
        "ms_per_block_events": round(ev_ms, 4), "ms_per_block_host": round(host_ms, 4),
        "gsym_per_s": round(ncalls / (ev_ms * 1e-3) / 1e9, 3),
        "repairs_per_block": repaired / args.steps, "unproven": unproven,
        "soft_bit_errors": int(err.sum()), "hard_full_phase_bit_errors": int((hard[lo:hi] != tx[lo:hi]).sum()),
        "hard_reduced_bit_errors": int(hbe), "compared_bits": int(hi - lo),
        "llr_scale_c_sigma2": None if scale is None else round(scale, 4),
        **({"apriori": ap} if ap is not None else {}),
    }))


def apriori_passes(args, dev, _hip, torch, rows, fspec, d_rot, ctx, plain_ms) -> dict:
    """--apriori: wf_cpm_soft_apriori on the same rows, same context and same step counts as the plain pass timed just
    before: once with a random float32 prior (normal, --apriori-sigma, clipped to +-50; scale 0.7) and once with a NULL
    prior (the plain kernels through the new entry point).  Time per pass by device events, chunk repairs per pass."""
    n = int(rows.shape[0]) * fspec.bits_per_symbol
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    prior = (args.apriori_sigma * torch.randn(n, generator=g, device="cuda", dtype=torch.float32)).clamp_(-50.0, 50.0)
    out = {"prior_sigma": args.apriori_sigma, "scale": 0.7}
    for name, p in (("random_prior", prior), ("null_prior", None)):
        for _ in range(args.warmup_steps):
            dev.cpm_soft_apriori(rows, fspec, p, 0.7, 0, args.soft_warmup, ctx=ctx, d_rot=d_rot)
        torch.cuda.synchronize()
        dev.viterbi_repaired(reset=True, ctx=ctx)
        dev.viterbi_unmerged(reset=True, ctx=ctx)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            dev.cpm_soft_apriori(rows, fspec, p, 0.7, 0, args.soft_warmup, ctx=ctx, d_rot=d_rot)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.steps
        out[name] = {"ms_per_block_events": round(ms, 4), "ratio_to_plain": round(ms / plain_ms, 4),
                     "repairs_per_block": dev.viterbi_repaired(reset=True, ctx=ctx) / args.steps,
                     "unproven": dev.viterbi_unmerged(reset=True, ctx=ctx)}
    return out


if __name__ == "__main__":
    main()
