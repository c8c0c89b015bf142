"""Live windows of an iterative detection and decoding loop: the rows of a burst a detector pass still has to work on, given
which codewords are open (include/wfhip.h states the device operation, ``wf_idd_windows``, and the windowed detector that
reads its table, ``wf_viterbi4_soft_apriori_windows``).

``windows_host`` is the HOST statement of the definition, written straight from it: the device table equals it bit for bit.
"""
from __future__ import annotations

import numpy as np

DEFAULT_GUARD = 128                       # rows on either side of an open codeword (INTEGRATION.md has the evidence)


def windows_host(state, nrows: int, n_tx: int, period: int | None = None, first: int = 1, guard: int = DEFAULT_GUARD):
    """-> (windows int64[W, 2] of (s, e), live rows Σ (e - s), open codewords).

    ``state``: one byte per codeword, 0 = open.  Codeword b occupies the rows [a_b, e_b), a_b = ``first`` + b ``period``,
    e_b = a_b + ``n_tx`` (``period`` default ``n_tx``: codewords back to back).  An open codeword's span is widened by
    ``guard`` rows on either side, its start rounded DOWN to an even row (row k is trellis column k % 2: a window keeps the
    burst's parity) and clipped to [0, ``nrows``); a span that starts less than ``guard`` rows behind the previous window's
    end is merged into it.  A span wholly outside the burst gives no window."""
    state = np.asarray(state).reshape(-1)
    nrows, n_tx, guard, first = int(nrows), int(n_tx), int(guard), int(first)
    period = n_tx if period is None else int(period)
    if nrows < 1 or n_tx < 1 or period < n_tx or guard < 0:
        raise ValueError("nrows and n_tx must be at least 1, period at least n_tx, guard at least 0")
    out: list[list[int]] = []
    nopen = 0
    for b in np.flatnonzero(state == 0).tolist():
        nopen += 1
        a = first + b * period
        s = max(0, a - guard) & ~1
        e = min(nrows, a + n_tx + guard)
        if e <= s:
            continue
        if out and s - out[-1][1] < guard:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e])
    win = np.array(out, dtype=np.int64).reshape(-1, 2)
    return win, int((win[:, 1] - win[:, 0]).sum()), nopen


def table_host(state, nrows: int, n_tx: int, period: int | None = None, first: int = 1, guard: int = DEFAULT_GUARD) -> np.ndarray:
    """The specified words of ``wf_idd_windows``' table: [W, live rows, open codewords, 0, s_0, e_0, s_1, e_1, ...] (int64,
    4 + 2 W words; the device table has room for 4 + 2 ncw and leaves the rest unspecified)."""
    win, live, nopen = windows_host(state, nrows, n_tx, period, first, guard)
    return np.concatenate((np.array([win.shape[0], live, nopen, 0], dtype=np.int64), win.reshape(-1)))
