"""tests/golden/detect_ties.npz: what the reference's SOQPSKTrellisDetector.iteration returns on rows that TIE: 1500
integer-grid rows (components in -2 .. 2, every metric sum exact) with a 300-row gap of zeros, where every add-compare-select
of the window ties and the decision is made by list order alone (strict '<' at waveforms/viterbi/algorithm.py:79-83, the
first arg-min at :92).  Window lengths 1, 2, 3, 8, 17 and 64, both trellises.

Run where a checkout of the reference exists, from a directory outside this repository (so that `waveforms` is the
reference's package and not this repository's own), with REFERENCE the path of that checkout:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=$REFERENCE python3 <this file>

Stored: the inputs as int8 components (rows_ri[n, 3, 2]) and element [0] of both arrays every call returned (what a caller
keeps, examples/soqpsk_detection.py:196-198).  No reference source text is stored.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np

OUT = Path(__file__).resolve().parent

import waveforms  # noqa: E402  (must resolve to the reference, not to this repository's package of the same name)

assert OUT.parents[1] not in Path(waveforms.__file__).resolve().parents, waveforms.__file__

from waveforms.viterbi.algorithm import SOQPSKTrellisDetector  # noqa: E402

LENGTHS = (1, 2, 3, 8, 17, 64)
N, GAP = 1500, (600, 900)


def main():
    rng = np.random.default_rng(1)                 # tests/test_degenerate_rows.py: grid_rows
    re = rng.integers(-2, 3, (N, 3))
    im = rng.integers(-2, 3, (N, 3))
    ri = np.stack([re, im], axis=-1).astype(np.int8)
    ri[GAP[0]:GAP[1]] = 0
    rows = ri[..., 0].astype(np.float64) + 1j * ri[..., 1].astype(np.float64)
    d = {"rows_ri": ri, "lengths": np.array(LENGTHS)}
    for length in LENGTHS:
        for diff in (True, False):
            det = SOQPSKTrellisDetector(length=length, differantial_encoding=diff)
            fb, fs = [], []
            for z in rows:
                b, s = det.iteration(z)
                fb.append(b[0])
                fs.append(s[0])
            d[f"L{length}_diff{int(diff)}_bits0"] = np.array(fb, dtype=np.float64).astype(np.uint8)
            d[f"L{length}_diff{int(diff)}_syms0"] = np.array(fs, dtype=np.float64).astype(np.int8)
    np.savez_compressed(OUT / "detect_ties.npz", **d)
    print({k: v.shape for k, v in d.items()})


if __name__ == "__main__":
    main()
