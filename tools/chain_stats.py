"""Figures of a pipelined SOQPSK link's kernel timeline (a listing of tools/timeline.py): front-end duration, period, the two
gaps behind a front end and what the next front end's start followed, over the longest run of periods without a drain.
    python tools/chain_stats.py <listing.txt>"""
import statistics
import sys

rows = []
for line in open(sys.argv[1]):
    f = line.split(None, 4)
    if len(f) == 5 and f[3].startswith("q") and not line.startswith("#"):
        try:
            rows.append((float(f[0]), float(f[1]), f[4]))
        except ValueError:
            pass
fe = [r for r in rows if "mod_chan_bank_kernel" in r[2]]
det = [r for r in rows if "viterbi_batch_kernel" in r[2]]
scan = [r for r in rows if "mod_tile_scan_kernel" in r[2]]
runs, cur = [], []
for a, b in zip(fe, fe[1:]):              # a drain (the host synchronises) shows as a gap of more than a quarter front end
    if b[0] - a[1] < 0.25 * (a[1] - a[0]):
        cur.append((a, b))
    else:
        runs.append(cur)
        cur = []
runs.append(cur)
pairs = max(runs, key=len)
med = statistics.median
to_det, to_fe, lead, after_scan, scan_later = [], [], [], [], 0
for a, b in pairs:
    d = min((r for r in det if r[0] >= a[1] - 1.0), key=lambda r: r[0])      # block k's detector: the first to start behind front end k
    s = max((r for r in scan if r[1] <= b[0] + 0.5), key=lambda r: r[1])     # block k + 1's scan: the last to end before front end k + 1
    to_det.append(d[0] - a[1])
    to_fe.append(b[0] - a[1])
    lead.append(b[0] - d[0])
    after_scan.append(b[0] - s[1])
    scan_later += s[1] > a[1]
print(f"# periods in the longest run without a drain: {len(pairs)}")
print(f"# median front-end duration {med(a[1] - a[0] for a, _ in pairs):.1f} us; median period {med(b[0] - a[0] for a, b in pairs):.1f} us")
print(f"# front end k's end -> detector k's start: median {med(to_det):.1f} us (min {min(to_det):.1f}, max {max(to_det):.1f})")
print(f"# front end k's end -> front end k + 1's start: median {med(to_fe):.1f} us (min {min(to_fe):.1f}, max {max(to_fe):.1f})")
print(f"# detector k started before front end k + 1 in {sum(v > 0 for v in lead)} of {len(lead)} periods; lead min {min(lead):.1f} / median {med(lead):.1f} / max {max(lead):.1f} us")
print(f"# front end k + 1's start - its own scan kernel's end: median {med(after_scan):.1f} us (min {min(after_scan):.1f}); the scan ended after front end k in {scan_later} of {len(pairs)} periods")
