"""LDPC codes: the code object, its systematic encoder, and the GPU encoder / layered min-sum decoder behind it.

A code is a parity-check matrix H (m checks x n variables) plus two maps:

* the LAYERS of the decoder: groups of checks that share no variable, decoded in order (``wf_ldpc_decode`` in
  include/wfhip.h states the decoder's definition).  For a quasi-cyclic code the layers are the block rows; for a
  general H the default is greedy: the checks in index order, each placed in the first layer that shares no variable
  with it;
* ``tx_order``: transmitted position t carries variable ``tx_order[t]``.  This one array is both the bit interleaver and
  the puncturing map: the variables it does not name are punctured (never sent; the decoder starts them at L = 0).

The systematic encoder comes from GF(2) elimination of H on the host (packed uint64 rows).  The pivot columns, which
become the parity variables, are taken in a fixed order: the punctured columns first, then the others from the last to
the first; the pivot row of a column is the first row not yet used that has a 1 there.  k = n - rank(H); the
information variables are the non-pivot columns in increasing order; parity = A u over GF(2).  A punctured column that
cannot be a pivot raises ``ValueError``.

Codes that this package does not ship.  The IRIG 106 LDPC codes for SOQPSK-TG (the CCSDS AR4JA family) are defined by
θ/φ permutation tables that are not reproduced here.  With those tables, build H as the standard's block matrix of
circulant permutations (each M x M block a permutation that the tables give, not a cyclic shift), and call
``LDPCCode.from_parity_check(H, tx_order=...)`` with ``tx_order`` naming every column but the last M, which are punctured.
"""
from __future__ import annotations

import functools

import numpy as np

from ._code import DeviceCode

MAX_N = 32768
MAX_DEG = 32

# Demo code: a regular (3, 6) quasi-cyclic code, base 8 x 16, Z = 128 (n = 2048).  Base column j has its three blocks in
# rows (j, j+1, j+3) mod 8 for j < 8 and (j, j+2, j+5) mod 8 for j >= 8: six per row.  The shifts come from
# _demo_search(Z), a deterministic greedy search without random numbers: the blocks in column-major order (column j, rows
# increasing); block number i tries s = (29 i + 7 + 37 t) mod Z for t = 0, 1, ... and keeps the first s that closes no
# 4-cycle (s(r1,c1) - s(r2,c1) + s(r2,c2) - s(r1,c2) != 0 mod Z) and no 6-cycle (the alternating sum over three rows and
# three columns != 0 mod Z) with the blocks already placed.  The girth is therefore >= 8.  (The same search with the
# 4-cycle test alone gave a girth-6 code that decoded 52 of 2 000 codewords wrongly in the coded SOQPSK-TG chain at an
# information Eb/N0 of 7 dB; this one decodes none of 24 410 there: INTEGRATION.md.)
DEMO_SHIFTS_128 = (
    (7, -1, -1, -1, -1, 58, -1, 104, 63, -1, -1, 68, -1, -1, 73, -1),
    (36, 94, -1, -1, -1, -1, 17, -1, -1, 22, -1, -1, 27, -1, -1, 32),
    (-1, 123, 53, -1, -1, -1, -1, 42, 38, -1, 109, -1, -1, 114, -1, -1),
    (65, -1, 82, 12, -1, -1, -1, -1, -1, 88, -1, 6, -1, -1, 85, -1),
    (-1, 24, -1, 78, 99, -1, -1, -1, -1, -1, 47, -1, 56, -1, -1, 44),
    (-1, -1, 111, -1, 37, 87, -1, -1, 121, -1, -1, 72, -1, 89, -1, -1),
    (-1, -1, -1, 70, -1, 25, 46, -1, -1, 80, -1, -1, 122, -1, 60, -1),
    (-1, -1, -1, -1, 29, -1, 75, 34, -1, -1, 39, -1, -1, 27, -1, 127),
)


def _demo_pattern() -> list[list[int]]:
    return [sorted((j + d) % 8 for d in ((0, 1, 3) if j < 8 else (0, 2, 5))) for j in range(16)]


def _closes_short_cycle(E: np.ndarray, r: int, j: int, s: int, Z: int) -> bool:
    """Would shift s at block (r, j) close a 4- or 6-cycle with the blocks of E already placed?"""
    mb, nb = E.shape
    for r2 in range(mb):
        if r2 == r or E[r2, j] < 0:
            continue
        for c2 in range(nb):
            if c2 == j or E[r2, c2] < 0:
                continue
            if E[r, c2] >= 0 and (s - E[r2, j] + E[r2, c2] - E[r, c2]) % Z == 0:
                return True
            for r3 in range(mb):
                if r3 in (r, r2) or E[r3, c2] < 0:
                    continue
                for c3 in range(nb):
                    if c3 in (j, c2) or E[r3, c3] < 0 or E[r, c3] < 0:
                        continue
                    if (s - E[r2, j] + E[r2, c2] - E[r3, c2] + E[r3, c3] - E[r, c3]) % Z == 0:
                        return True
    return False


def _demo_search(Z: int) -> np.ndarray:
    """The documented search behind DEMO_SHIFTS_128 (and ``demo_code(Z)`` for other Z)."""
    E = -np.ones((8, 16), dtype=np.int64)
    i = 0
    for j, rows in enumerate(_demo_pattern()):
        for r in rows:
            for t in range(Z):
                s = (29 * i + 7 + 37 * t) % Z
                if not _closes_short_cycle(E, r, j, s, Z):
                    E[r, j] = s
                    break
            else:
                raise RuntimeError(f"no shift free of 4- and 6-cycles for block ({r}, {j}) at Z = {Z}")
            i += 1
    return E


def demo_tx_order(Z: int = 128) -> np.ndarray:
    """The demo codes' default interleaver: transmitted bit t goes to base column j = t mod 16, position
    (37 (t div 16) + 11 j) mod Z inside it.  Consecutive channel bits (the SOQPSK detector's errors come in pairs) land in
    different block columns, far apart."""
    t = np.arange(16 * Z, dtype=np.int64)
    j, i = t % 16, t // 16
    return (Z * j + (37 * i + 11 * j) % Z).astype(np.int64)


@functools.lru_cache(maxsize=4)
def _demo(Z: int) -> "LDPCCode":
    E = np.array(DEMO_SHIFTS_128, dtype=np.int64) if Z == 128 else _demo_search(Z)
    return LDPCCode.from_exponent_matrix(E, Z, tx_order=demo_tx_order(Z))


def demo_code(Z: int = 128) -> "LDPCCode":
    """The package's demo code: regular (3, 6) QC, base 8 x 16, n = 16 Z (2048 at the default Z = 128, 16384 at
    Z = 1024), rate about 1/2, girth >= 8, layers = block rows, tx_order = :func:`demo_tx_order`.  Cached per Z."""
    return _demo(int(Z))


def _pack_rows(bits: np.ndarray) -> np.ndarray:
    """uint8 0/1 rows -> uint64 words, bit i of word w = column 64 w + i."""
    rows, n = bits.shape
    nw = (n + 63) // 64
    pad = np.zeros((rows, nw * 64), dtype=np.uint8)
    pad[:, :n] = bits
    return np.packbits(pad, axis=1, bitorder="little").view("<u8").reshape(rows, nw)


def _unpack_rows(words: np.ndarray, n: int) -> np.ndarray:
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=1, bitorder="little")[:, :n]


def _systematic(H: np.ndarray, punctured: np.ndarray):
    """GF(2) elimination of H (dense uint8) -> (info variables, parity variables, A packed (n - k) x ceil(k / 64))."""
    m, n = H.shape
    R = _pack_rows(H)
    used = np.zeros(m, dtype=bool)
    pcol, prow = [], []
    pset = set(int(v) for v in punctured)
    order = sorted(pset) + [c for c in range(n - 1, -1, -1) if c not in pset]
    for c in order:
        w, b = divmod(c, 64)
        col = ((R[:, w] >> np.uint64(b)) & np.uint64(1)).astype(bool)
        cand = np.flatnonzero(col & ~used)
        if cand.size == 0:
            if c in pset:
                raise ValueError(f"punctured variable {c} cannot be a parity variable of the systematic encoder")
            continue
        r = int(cand[0])
        used[r] = True
        col[r] = False
        others = np.flatnonzero(col)
        if others.size:
            R[others] ^= R[r]
        pcol.append(c)
        prow.append(r)
        if used.all():
            break
    par = np.array(sorted(pcol), dtype=np.int64)
    row_of = dict(zip(pcol, prow))
    is_par = np.zeros(n, dtype=bool)
    is_par[par] = True
    info = np.flatnonzero(~is_par).astype(np.int64)
    if info.size == 0:
        raise ValueError("H has full column rank: the code has no information bits")
    full = _unpack_rows(R[[row_of[int(c)] for c in par]], n)
    A = _pack_rows(np.ascontiguousarray(full[:, info]))
    return info, par, A


class LDPCCode(DeviceCode):
    """A binary LDPC code with its decoder layering, transmit order and systematic encoder.

    Attributes: ``n`` variables, ``m`` checks, ``k`` information bits, ``n_tx`` transmitted bits, ``info_var`` (the k
    information variables, message order), ``parity_var`` (the others, increasing), ``tx_order`` (n_tx variables),
    ``layers`` (lists of check indices of H), ``rate`` = k / n_tx."""

    def __init__(self, rows: list[np.ndarray], n: int, layers, tx_order) -> None:
        self.n, self.m = int(n), len(rows)
        if not 2 <= self.n <= MAX_N:
            raise ValueError(f"n = {self.n} outside 2 .. {MAX_N}")
        if self.m < 1:
            raise ValueError("H has no checks")
        self.check_vars = [np.asarray(r, dtype=np.int64) for r in rows]
        for c, r in enumerate(self.check_vars):
            if not 2 <= r.size <= MAX_DEG:
                raise ValueError(f"check {c} has degree {r.size} (must be 2 .. {MAX_DEG})")
        if layers is None:
            layers = self._greedy_layers()
        self.layers = [[int(c) for c in layer] for layer in layers]
        seen = np.zeros(self.m, dtype=np.int64)
        for li, layer in enumerate(self.layers):
            if not layer:
                raise ValueError(f"layer {li} is empty")
            used: set[int] = set()
            for c in layer:
                if not 0 <= c < self.m:
                    raise ValueError(f"layer {li} names check {c}, which does not exist")
                seen[c] += 1
                vs = set(int(v) for v in self.check_vars[c])
                if used & vs:
                    raise ValueError(f"checks of layer {li} share variables {sorted(used & vs)[:4]}")
                used |= vs
        if not np.all(seen == 1):
            raise ValueError("the layers must name every check exactly once")
        tx = np.arange(self.n, dtype=np.int64) if tx_order is None else np.asarray(tx_order, dtype=np.int64).ravel()
        if tx.size == 0 or tx.min() < 0 or tx.max() >= self.n or np.unique(tx).size != tx.size:
            raise ValueError("tx_order must name distinct variables of the code")
        self.tx_order = tx
        self.n_tx = int(tx.size)
        sent = np.zeros(self.n, dtype=bool)
        sent[tx] = True
        self.punctured = np.flatnonzero(~sent).astype(np.int64)
        H = np.zeros((self.m, self.n), dtype=np.uint8)
        for c, r in enumerate(self.check_vars):
            H[c, r] = 1
        self.info_var, self.parity_var, self.generator = _systematic(H, self.punctured)
        self.k = int(self.info_var.size)
        self.rate = self.k / self.n_tx

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_parity_check(cls, H, layers=None, tx_order=None) -> "LDPCCode":
        """H: dense 0/1 array or scipy.sparse matrix (m x n).  ``layers``: sequences of check indices (default: greedy);
        ``tx_order``: transmitted position -> variable (default: every variable, in order; variables it leaves out are
        punctured)."""
        try:
            import scipy.sparse as sp
        except ImportError:          # pragma: no cover - scipy is optional
            sp = None
        if sp is not None and sp.issparse(H):
            Hc = sp.csr_matrix(H)
            Hc.eliminate_zeros()
            if Hc.nnz and not np.all((Hc.data == 1)):
                raise ValueError("H must be a 0/1 matrix")
            rows = [np.sort(Hc.indices[Hc.indptr[c]:Hc.indptr[c + 1]]) for c in range(Hc.shape[0])]
            n = Hc.shape[1]
        else:
            Hd = np.asarray(H)
            if Hd.ndim != 2 or not np.isin(Hd, (0, 1)).all():
                raise ValueError("H must be a 2-D 0/1 matrix")
            rows = [np.flatnonzero(Hd[c]) for c in range(Hd.shape[0])]
            n = Hd.shape[1]
        return cls(rows, n, layers, tx_order)

    @classmethod
    def from_exponent_matrix(cls, E, Z: int, punctured_blocks=(), tx_order=None) -> "LDPCCode":
        """Quasi-cyclic code: E is mb x nb, -1 a zero block, s in [0, Z) the Z x Z identity shifted by s (row r of the
        block has its 1 in column (r + s) mod Z).  Layers = block rows.  ``punctured_blocks``: block columns that are not
        transmitted; ``tx_order`` default: the other variables in order."""
        E = np.asarray(E, dtype=np.int64)
        Z = int(Z)
        if E.ndim != 2 or Z < 1 or (E < -1).any() or (E >= Z).any():
            raise ValueError("E must be mb x nb with entries -1 or 0 .. Z-1")
        mb, nb = E.shape
        rows, layers = [], []
        for br in range(mb):
            layers.append(list(range(br * Z, (br + 1) * Z)))
            for r in range(Z):
                rows.append(np.array([bc * Z + (r + E[br, bc]) % Z for bc in range(nb) if E[br, bc] >= 0], dtype=np.int64))
        pb = sorted(set(int(b) for b in punctured_blocks))
        if any(not 0 <= b < nb for b in pb):
            raise ValueError("punctured_blocks names a block column that does not exist")
        if tx_order is None:
            keep = np.ones(nb * Z, dtype=bool)
            for b in pb:
                keep[b * Z:(b + 1) * Z] = False
            tx_order = np.flatnonzero(keep)
        else:
            tx = np.asarray(tx_order, dtype=np.int64)
            if any(((tx >= b * Z) & (tx < (b + 1) * Z)).any() for b in pb):
                raise ValueError("tx_order names a variable of a punctured block")
        return cls(rows, nb * Z, layers, tx_order)

    def _greedy_layers(self) -> list[list[int]]:
        layers: list[list[int]] = []
        vars_of: list[set[int]] = []
        for c, r in enumerate(self.check_vars):
            vs = set(int(v) for v in r)
            for li, used in enumerate(vars_of):
                if not used & vs:
                    layers[li].append(c)
                    used |= vs
                    break
            else:
                layers.append([c])
                vars_of.append(set(vs))
        return layers

    # ------------------------------------------------------------------ host forms
    def parity_check_matrix(self) -> np.ndarray:
        """Dense H (uint8, m x n) in the caller's check order."""
        H = np.zeros((self.m, self.n), dtype=np.uint8)
        for c, r in enumerate(self.check_vars):
            H[c, r] = 1
        return H

    def c_tables(self) -> dict:
        """The tables of ``wf_ldpc_code_create``: checks renumbered in layer order."""
        order = [c for layer in self.layers for c in layer]
        deg = np.array([self.check_vars[c].size for c in order], dtype=np.int32)
        check_ptr = np.zeros(self.m + 1, dtype=np.int32)
        np.cumsum(deg, out=check_ptr[1:])
        edge_var = np.concatenate([self.check_vars[c] for c in order]).astype(np.int32)
        layer_ptr = np.zeros(len(self.layers) + 1, dtype=np.int32)
        np.cumsum([len(layer) for layer in self.layers], out=layer_ptr[1:])
        return dict(n=self.n, m=self.m, check_ptr=check_ptr, edge_var=edge_var, nlayers=len(self.layers), layer_ptr=layer_ptr,
                    n_tx=self.n_tx, tx_var=self.tx_order.astype(np.int32), k=self.k, info_var=self.info_var.astype(np.int32),
                    parity_gen=np.ascontiguousarray(self.generator, dtype=np.uint64))

    def codeword_host(self, info: np.ndarray) -> np.ndarray:
        """Systematic codewords by VARIABLE (ncw x n, uint8) from messages (ncw x k): the host statement of the encoder."""
        u = self._messages(info) & 1
        up = _pack_rows(u)
        A = self.generator
        c = np.zeros((u.shape[0], self.n), dtype=np.uint8)
        c[:, self.info_var] = u
        step = max(1, (1 << 22) // max(1, A.size))
        for b0 in range(0, u.shape[0], step):
            x = np.bitwise_count(A[None, :, :] & up[b0:b0 + step, None, :]).sum(axis=2, dtype=np.int64)
            c[b0:b0 + step, self.parity_var] = (x & 1).astype(np.uint8)
        return c

    def encode_host(self, info: np.ndarray) -> np.ndarray:
        """Host encoder: messages (ncw x k) -> transmitted bits (ncw x n_tx, uint8) in transmit order."""
        return np.ascontiguousarray(self.codeword_host(info)[:, self.tx_order])

    # ------------------------------------------------------------------ device
    _free, _encode = "wf_ldpc_code_free", "ldpc_encode"

    def _create(self, lib, ctx, out) -> int:
        t = self.c_tables()
        return lib.wf_ldpc_code_create(ctx, t["n"], t["m"], t["check_ptr"].ctypes.data, t["edge_var"].ctypes.data, t["nlayers"], t["layer_ptr"].ctypes.data,
                                       t["n_tx"], t["tx_var"].ctypes.data, t["k"], t["info_var"].ctypes.data, t["parity_gen"].ctypes.data, out)

    def encode_device(self, d_info):
        """Device messages (ncw x k or flat, u8) -> device transmitted bits (ncw x n_tx, u8)."""
        from .. import device as dev

        return dev.ldpc_encode(self, d_info)

    def decode_device(self, d_llr, **kw):
        """Device λ (ncw x n_tx float64, λ > 0 favouring 0) -> :func:`waveforms_amd.device.ldpc_decode`'s dict."""
        from .. import device as dev

        return dev.ldpc_decode(self, d_llr, **kw)

    def decode(self, llr: np.ndarray, scale: float = 1.0, alpha: float = 0.75, max_iter: int = 50, want_post: bool = False) -> dict:
        """λ (ncw x n_tx) -> {"info_bits", "iters"[, "post"]} as host arrays, decoded on the GPU."""
        from .. import _hip

        a = np.ascontiguousarray(np.atleast_2d(np.asarray(llr, dtype=np.float64)))
        if a.shape[1] != self.n_tx:
            raise ValueError(f"LLRs must have n_tx = {self.n_tx} columns")
        out = self.decode_device(_hip.to_device(a), scale=scale, alpha=alpha, max_iter=max_iter, want_post=want_post)
        return {key: _hip.to_host(v) for key, v in out.items() if v is not None}
