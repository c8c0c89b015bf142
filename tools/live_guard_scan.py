"""How much guard the live windows of the SOQPSK-TG loop need (IterativeSOQPSKLink(live_only=True, guard=G)); prints one JSON
line per pass and writes them all to ``--out``.

    python tools/live_guard_scan.py [--ebn0 4.5 5] [--blocks 2] [--guards 4 8 16 32 64 128 512] [--out FILE]

Full blocks (4 882 demo codewords in one burst, PT, 8 x 5 passes, damping 0.7) go through the FULL loop.  On entry to every pass
that has a frozen codeword, the windowed detector pass is run for every guard on the same states and prior, and compared
BITWISE with the full pass on the rows of the open codewords: rows that differ, rows whose sign differs, the largest
difference.  A window's edge starts from free metrics instead of the burst's history; this counts where that shows."""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from waveforms_amd import device as dev
from waveforms_amd.encoding import ldpc
from waveforms_amd.encoding.coded import IterativeSOQPSKLink

ap = argparse.ArgumentParser()
ap.add_argument("--ebn0", type=float, nargs="+", default=[4.5, 5.0])
ap.add_argument("--blocks", type=int, default=2)
ap.add_argument("--guards", type=int, nargs="+", default=[4, 8, 16, 32, 64, 128, 512])
ap.add_argument("--out", default=None)
args = ap.parse_args()
code = ldpc.demo_code()
ncw, n_tx = int(1e7) // code.n_tx, code.n_tx
GUARDS = tuple(args.guards)
out = {"tool": "live_guard_scan", "ncw": ncw, "n_tx": n_tx, "outer": 8, "inner": 5, "damping": 0.7, "points": []}
for ebn0 in args.ebn0:
    for blk in range(args.blocks):
        link = IterativeSOQPSKLink(code, ncw, detector="PT", outer=8, inner=5)
        info = link.info_bits(blk)
        rows, _ = link.front_end(dev.ldpc_encode(code, info), ebn0, 1, blk)
        n = int(rows.shape[0])
        link.begin(n)
        for o in range(8):
            if o:
                opened = link.state == 0
                nopen = int(opened.sum())
                if 0 < nopen:
                    mask = torch.zeros(n, dtype=torch.bool, device="cuda")
                    mask[1:1 + ncw * n_tx] = opened.repeat_interleave(n_tx)
                    full_ext, _ = dev.viterbi_soft_apriori(rows, link.prior, link.damping)
                    rec = {"ebn0": ebn0, "block": blk, "pass": o + 1, "open": nopen, "rows_of_open": int(mask.sum()), "guards": {}}
                    for G in GUARDS:
                        table = dev.idd_windows(link.state, n, n_tx, guard=G)
                        ext = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
                        bits = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
                        dev.viterbi_soft_apriori_windows(rows, link.prior, table, link.damping, out=(ext, bits))
                        d = (ext.view(torch.int64) != full_ext.view(torch.int64)) & mask
                        sgn = ((ext < 0) != (full_ext < 0)) & mask
                        mx = float((ext - full_ext)[mask].abs().max())
                        hdr = table[:3].cpu().tolist()
                        rec["guards"][G] = {"windows": hdr[0], "live_rows": hdr[1], "rows_differ": int(d.sum()), "sign_flips": int(sgn.sum()), "max_abs": mx}
                    out["points"].append(rec)
                    print(json.dumps(rec), flush=True)
            ext, _ = link.detect(rows, first=o == 0)
            link.decode(ext)
        del link, rows
if args.out:
    Path(args.out).write_text(json.dumps(out))
