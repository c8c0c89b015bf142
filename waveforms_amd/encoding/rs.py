"""Reed-Solomon codes over GF(2^8): the code object, its host statements, and the GPU encoder / decoder behind it.

``wf_rs_code_create`` in include/wfhip.h states the field, the code, the frame layout and the decoder's result.  In short:
GF(2^8) = GF(2)[x] / ``prim``, α the class of x, β = α^``step``; RS(n, k) with 2t = n - k has the generator
g(x) = Π_{i<2t} (x - β^(fcr+i)); a codeword c_0 .. c_{n-1} is sent c_0 first and c_0 is the HIGHEST coefficient of c(x); encoding is
systematic (message, then parity); n < 255 is the shortened code.  With ``depth`` = I, a frame is n I symbols, position p
belonging to codeword p mod I at index p div I; a message frame is k I symbols laid out the same way.

Every array here is in SYMBOLS (uint8, one per byte) unless ``bits=True`` is passed: then it is one bit per byte, eight per
symbol, MSB first (``to_bits`` / ``from_bits``), the form the convolutional encoder reads and its decoder writes.

The decoder is bounded-distance: the unique codeword within t symbols of the received word if there is one (status = the
distance), else the received message unchanged and status -1.  With ``erasures`` (f erased positions of a word, f <= 2t) it is
the unique codeword that differs from the word in e positions OUTSIDE the erased set with 2e + f <= 2t (status = e); the bytes
at erased positions decide nothing.  ``decode_host`` finds its candidate with the Euclidean algorithm (on the syndromes times
the erasure locator) and then CHECKS it against that definition (zero syndromes, the inequality, none at a virtual position);
the GPU decoder (Berlekamp-Massey) must agree with it bitwise.  ``mark_erasures_host`` is the rule that declares erasures from
the inner decoder's soft output.
"""
from __future__ import annotations

import math

import numpy as np

from ._code import DeviceCode

MAX_T, MAX_DEPTH = 16, 8


def to_bits(sym: np.ndarray) -> np.ndarray:
    """Symbols (.. x m) -> bits (.. x 8 m), MSB first."""
    s = np.ascontiguousarray(sym, dtype=np.uint8)
    return np.unpackbits(s[..., None], axis=-1).reshape(s.shape[:-1] + (8 * s.shape[-1],))


def below_f32(below: float) -> float:
    """The threshold of the erasure rule as the device takes it: rounded to float32, ±infinity replaced by the largest finite
    float32 of that sign."""
    with np.errstate(over="ignore"):
        b = np.float32(below)
    if np.isnan(b):
        raise ValueError("below must not be NaN")
    big = np.finfo(np.float32).max
    return float(min(max(b, -big), big))


def from_bits(bits: np.ndarray) -> np.ndarray:
    """Bits (.. x 8 m, only bit 0 of a byte counts) -> symbols (.. x m)."""
    b = np.ascontiguousarray(bits, dtype=np.uint8) & 1
    return np.packbits(b.reshape(b.shape[:-1] + (b.shape[-1] // 8, 8)), axis=-1).reshape(b.shape[:-1] + (b.shape[-1] // 8,))


class RSCode(DeviceCode):
    """RS(n, k) over GF(2^8), interleaved to ``depth``.

    Attributes: ``n``, ``k``, ``t``, ``prim``, ``fcr``, ``step``, ``depth``, ``rate`` = k / n, ``exp`` / ``log`` (the field's
    tables, exp doubled to 510 entries), ``gen`` (g's coefficients, gen[j] of x^j, 2t + 1 of them)."""

    def __init__(self, n: int, k: int, prim: int = 0x187, fcr: int = 112, step: int = 11, depth: int = 1) -> None:
        self.n, self.k, self.prim, self.fcr, self.step, self.depth = int(n), int(k), int(prim), int(fcr), int(step), int(depth)
        if not 0x100 <= self.prim < 0x200:
            raise ValueError(f"prim = {self.prim:#x} is not a polynomial of degree 8")
        if not 3 <= self.n <= 255:
            raise ValueError(f"n = {self.n} outside 3 .. 255")
        if self.k < 1 or (self.n - self.k) % 2 or not 1 <= (self.n - self.k) // 2 <= MAX_T:
            raise ValueError(f"n - k = {self.n - self.k} must be 2 t with t = 1 .. {MAX_T}, and k >= 1")
        if not 1 <= self.depth <= MAX_DEPTH:
            raise ValueError(f"depth = {self.depth} outside 1 .. {MAX_DEPTH}")
        if not 0 <= self.fcr <= 254:
            raise ValueError(f"fcr = {self.fcr} outside 0 .. 254")
        if not 1 <= self.step <= 254 or math.gcd(self.step, 255) != 1:
            raise ValueError(f"step = {self.step} must be 1 .. 254 and prime to 255")
        self.t = (self.n - self.k) // 2
        self.rate = self.k / self.n
        exp, log, v = np.zeros(510, dtype=np.int64), np.zeros(256, dtype=np.int64), 1
        for i in range(255):
            if i and v == 1:
                raise ValueError(f"prim = {self.prim:#x} is not primitive (x has period {i})")
            exp[i], log[v] = v, i
            v <<= 1
            if v & 0x100:
                v ^= self.prim
        if v != 1:
            raise ValueError(f"prim = {self.prim:#x} is not primitive")
        exp[255:] = exp[:255]
        self.exp, self.log = exp, log
        g = np.array([1], dtype=np.int64)
        for i in range(2 * self.t):                                   # g <- g (x - β^(fcr+i)), lowest coefficient first
            root = self.beta_pow(self.fcr + i)
            g = np.concatenate(([0], g)) ^ np.concatenate((self.mul(g, root), [0]))
        self.gen = g

    # ------------------------------------------------------------------ presets
    @classmethod
    def ccsds(cls, e: int = 16, depth: int = 1, n: int = 255) -> "RSCode":
        """The CCSDS code correcting ``e`` = 16 or 8 symbols: (255, 223) or (255, 239), prim 0x187, step 11, fcr 128 - e; ``n`` <
        255 shortens it.  Symbols are in the conventional (polynomial) basis: the standard's dual-basis map is not applied."""
        if e not in (16, 8):
            raise ValueError("e must be 16 or 8")
        return cls(n, n - 2 * e, 0x187, 128 - e, 11, depth)

    @classmethod
    def conventional(cls, n: int, k: int, depth: int = 1) -> "RSCode":
        """prim 0x11d, fcr 0, step 1."""
        return cls(n, k, 0x11d, 0, 1, depth)

    # ------------------------------------------------------------------ the field
    def mul(self, a, b):
        a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
        return np.where((a != 0) & (b != 0), self.exp[self.log[a] + self.log[b]], 0)

    def inv(self, a):
        return self.exp[(255 - self.log[np.asarray(a, dtype=np.int64)]) % 255]

    def beta_pow(self, e):
        """β^e for any integer (array) e."""
        return self.exp[(self.step * np.asarray(e, dtype=np.int64)) % 255]

    def poly_eval(self, p, x):
        """p (lowest coefficient first) at the points x."""
        x = np.asarray(x, dtype=np.int64)
        acc = np.zeros_like(x)
        for c in np.asarray(p, dtype=np.int64)[::-1]:
            acc = self.mul(acc, x) ^ int(c)
        return acc

    # ------------------------------------------------------------------ layout
    def _split(self, frames: np.ndarray, per: int) -> np.ndarray:
        """Frames (F x per I) -> codewords (F I x per): codeword b I + c takes positions c, c + I, .."""
        f = np.atleast_2d(np.asarray(frames, dtype=np.uint8))
        if f.shape[1] != per * self.depth:
            raise ValueError(f"a frame must hold {per} x depth = {per * self.depth} symbols, not {f.shape[1]}")
        return f.reshape(f.shape[0], per, self.depth).transpose(0, 2, 1).reshape(-1, per)

    def _join(self, words: np.ndarray) -> np.ndarray:
        per = words.shape[1]
        return np.ascontiguousarray(words.reshape(-1, self.depth, per).transpose(0, 2, 1).reshape(-1, per * self.depth)).astype(np.uint8)

    # ------------------------------------------------------------------ host statements
    def syndromes_host(self, words: np.ndarray) -> np.ndarray:
        """S_j = r(β^(fcr+j)), j < 2t, of codewords (B x n, c_0 first) -> B x 2t."""
        w = np.atleast_2d(np.asarray(words, dtype=np.int64))
        deg = self.n - 1 - np.arange(self.n)
        out = np.zeros((w.shape[0], 2 * self.t), dtype=np.int64)
        for j in range(2 * self.t):
            out[:, j] = np.bitwise_xor.reduce(self.mul(w, self.beta_pow((self.fcr + j) * deg)[None, :]), axis=1)
        return out

    def encode_words_host(self, msgs: np.ndarray) -> np.ndarray:
        """Messages (B x k) -> codewords (B x n): the message, then the remainder of m(x) x^(2t) by g(x) (long division)."""
        m = np.atleast_2d(np.asarray(msgs, dtype=np.int64))
        if m.shape[1] != self.k:
            raise ValueError(f"messages must have k = {self.k} symbols")
        gdesc = self.gen[:-1][::-1]                                    # g_{2t-1} .. g_0
        par = np.zeros((m.shape[0], 2 * self.t), dtype=np.int64)        # the running remainder, highest coefficient first
        for i in range(self.k):
            f = m[:, i] ^ par[:, 0]
            par = np.concatenate((par[:, 1:], np.zeros((m.shape[0], 1), dtype=np.int64)), axis=1) ^ self.mul(f[:, None], gdesc[None, :])
        return np.concatenate((m, par), axis=1).astype(np.uint8)

    def encode_host(self, msg_frames: np.ndarray, bits: bool = False) -> np.ndarray:
        """Message frames (F x k I) -> frames (F x n I)."""
        m = from_bits(msg_frames) if bits else msg_frames
        out = self._join(self.encode_words_host(self._split(m, self.k)))
        return to_bits(out) if bits else out

    def _candidate(self, S: np.ndarray, erased=()):
        """A candidate error vector by degree (255 entries) from the syndromes of one word whose symbols at the degrees
        ``erased`` were taken as 0, by the Euclidean algorithm on S Γ mod x^2t, Γ = Π (1 - β^d x) over the erased degrees, or
        None.  Its values at the erased degrees are the symbols there."""
        t2 = 2 * self.t
        f = len(erased)

        def deg(p):
            nz = np.flatnonzero(p)
            return int(nz[-1]) if nz.size else -1

        gam = np.zeros(t2 + 1, dtype=np.int64)
        gam[0] = 1
        for d in erased:                                               # Γ <- Γ (1 - β^d x)
            gam[1:] ^= self.mul(gam[:-1], self.beta_pow(d))
        r0, r1 = np.zeros(t2 + 1, dtype=np.int64), np.zeros(t2 + 1, dtype=np.int64)
        r0[t2] = 1
        for i in range(f + 1):                                         # the modified syndromes S Γ mod x^2t
            r1[i:t2] ^= self.mul(gam[i], np.asarray(S[:t2 - i], dtype=np.int64))
        u0, u1 = np.zeros(t2 + 2, dtype=np.int64), np.zeros(t2 + 2, dtype=np.int64)
        u1[0] = 1
        while 2 * deg(r1) >= t2 + f:
            d1, lead = deg(r1), self.inv(r1[deg(r1)])
            while deg(r0) >= d1:                                       # r0 <- r0 mod r1, u0 <- u0 - q u1
                d0 = deg(r0)
                q, s = int(self.mul(r0[d0], lead)), d0 - d1
                r0[s:s + d1 + 1] ^= self.mul(q, r1[:d1 + 1])
                u0[s:] ^= self.mul(q, u1[:u1.size - s])
            r0, r1, u0, u1 = r1, r0, u1, u0
        sig, om = u1, r1                                               # the error locator; Ω = S Γ σ mod x^2t
        Ls = deg(sig)
        if Ls < (0 if f else 1) or 2 * Ls + f > t2 or sig[0] == 0:
            return None
        lam = np.zeros(2 * t2 + 3, dtype=np.int64)                     # the errata locator σ Γ, of degree L
        for i in range(Ls + 1):
            lam[i:i + t2 + 1] ^= self.mul(sig[i], gam)
        L = Ls + f
        d = np.arange(255)
        x = self.beta_pow(-d)                                          # β^(-d): a root there is an error or an erasure at degree d
        roots = self.poly_eval(lam[:L + 1], x) == 0
        if int(roots.sum()) != L or roots[self.n:].any():
            return None
        dlam = lam[:L + 1].copy()
        dlam[0::2] = 0                                                 # the formal derivative: odd terms, one degree down
        den = self.poly_eval(dlam[1:], x)
        if (den[roots] == 0).any():
            return None
        e = self.mul(self.mul(self.poly_eval(om, x), self.inv(np.where(den == 0, 1, den))), self.beta_pow(d * (1 - self.fcr)))
        return np.where(roots, e, 0)

    def decode_words_host(self, words: np.ndarray, erasures=None):
        """Codewords (B x n) -> (messages B x k, status B): the definition, word by word.  ``erasures``: B x n, nonzero = erased."""
        w = np.atleast_2d(np.asarray(words, dtype=np.uint8))
        if w.shape[1] != self.n:
            raise ValueError(f"words must have n = {self.n} symbols")
        out, status = w[:, :self.k].copy(), np.zeros(w.shape[0], dtype=np.int32)
        if erasures is None:
            era = np.zeros(w.shape, dtype=bool)
        else:
            era = np.atleast_2d(np.asarray(erasures)) != 0
            if era.shape != w.shape:
                raise ValueError("erasures must have one entry per symbol")
        f = era.sum(axis=1)
        wz = np.where(era, 0, w).astype(np.uint8)                      # the bytes at erased positions are not read past this line
        S = self.syndromes_host(wz)
        status[f > 2 * self.t] = -1
        idx = self.n - 1 - np.arange(self.n)                           # the degree of position i
        for b in np.flatnonzero((S.any(axis=1) | (f > 0)) & (f <= 2 * self.t)):
            status[b] = -1
            if S[b].any():
                e = self._candidate(S[b], idx[era[b]].tolist())
                if e is None:
                    continue
                c = wz[b].astype(np.int64) ^ e[idx]
            else:
                c = wz[b].astype(np.int64)                             # the word with 0 at its erased positions is a codeword
            nerr = int(np.count_nonzero((c != wz[b]) & ~era[b]))
            # a codeword with 2 (changes outside the erased set) + f <= 2t: the one
            if (nerr >= 1 or f[b] > 0) and 2 * nerr + int(f[b]) <= 2 * self.t and not self.syndromes_host(c[None, :]).any():
                out[b], status[b] = c[:self.k], nerr
        return out, status

    def decode_host(self, frames: np.ndarray, bits: bool = False, erasures=None):
        """Frames (F x n I) -> (message frames F x k I, status F I int32, codeword b I + c at [b I + c]).  ``erasures``: uint8 in
        SYMBOL form whatever ``bits`` is, F x n I laid out like the frame, nonzero = erased (None: errors only)."""
        f = from_bits(frames) if bits else frames
        era = None if erasures is None else self._split(erasures, self.n)
        msgs, status = self.decode_words_host(self._split(f, self.n), era)
        out = self._join(msgs)
        return (to_bits(out) if bits else out), status

    def mark_erasures_host(self, post: np.ndarray, f_max: int, below: float = float("inf")) -> np.ndarray:
        """The erasure rule (``wf_rs_mark_erasures``): ``post`` F x 8 n I float32, the Λ of ``conv_siso`` for frames in bit form,
        finite -> uint8 F x n I, 1 = erased.  ρ of a symbol = min |Λ| over its eight bits; per codeword the erased symbols are
        the at most ``f_max`` symbols of smallest ρ among those with ρ < ``below`` (as ``below_f32`` makes it), ties to the
        smaller index within the codeword."""
        p = np.atleast_2d(np.asarray(post, dtype=np.float32))
        if p.shape[1] != 8 * self.n * self.depth:
            raise ValueError(f"a frame must hold 8 n depth = {8 * self.n * self.depth} values, not {p.shape[1]}")
        f_max = int(f_max)
        if not 0 <= f_max <= 2 * self.t:
            raise ValueError(f"f_max = {f_max} outside 0 .. 2t = {2 * self.t}")
        lim = np.float32(below_f32(below))
        rho = np.abs(p).reshape(p.shape[0], self.n * self.depth, 8).min(axis=2)
        rho = rho.reshape(p.shape[0], self.n, self.depth).transpose(0, 2, 1).reshape(-1, self.n)       # by codeword
        era = np.zeros(rho.shape, dtype=np.uint8)
        for b in range(rho.shape[0]):
            order = np.argsort(rho[b], kind="stable")                  # equal ρ: the smaller index first
            era[b, [i for i in order if rho[b, i] < lim][:f_max]] = 1
        return self._join(era)

    def counts_host(self, msg_out: np.ndarray, status: np.ndarray, ref: np.ndarray, bits: bool = False, erasures=None) -> list[int]:
        """The five counts of ``wf_rs_decode`` from its outputs and the reference message frames; with ``erasures`` (symbol
        form, as ``decode_host`` takes them) the six of ``wf_rs_decode_erasures``: the sixth is the erasures filled, summed over
        the successful codewords."""
        a = self._split(from_bits(msg_out) if bits else msg_out, self.k)
        r = self._split(from_bits(ref) if bits else ref, self.k)
        be = np.unpackbits((a ^ r)[..., None], axis=-1).reshape(a.shape[0], -1).sum(axis=1)
        wrong = be > 0
        out = [int(be.sum()), int(wrong.sum()), int((status < 0).sum()), int(status[status > 0].sum()),
               int(wrong.reshape(-1, self.depth).any(axis=1).sum())]
        if erasures is not None:
            f = (self._split(erasures, self.n) != 0).sum(axis=1)
            out.append(int(f[np.asarray(status) >= 0].sum()))
        return out

    # ------------------------------------------------------------------ device
    _free = "wf_rs_code_free"

    def _create(self, lib, ctx, out) -> int:
        return lib.wf_rs_code_create(ctx, self.prim, self.fcr, self.step, self.n, self.k, self.depth, out)

    def encode(self, msg_frames: np.ndarray, bits: bool = False) -> np.ndarray:
        """Message frames (F x k I symbols, or 8 times as many bits) -> frames, encoded on the GPU."""
        from .. import _hip
        from .. import device as dev

        m = np.ascontiguousarray(np.atleast_2d(np.asarray(msg_frames, dtype=np.uint8)))
        return _hip.to_host(dev.rs_encode(self, _hip.to_device(m), bits=bits))

    def decode(self, frames: np.ndarray, bits: bool = False, ref=None, erasures=None) -> dict:
        """Frames -> {"msg", "status", "counts"} as host arrays, decoded on the GPU (``waveforms_amd.device.rs_decode``);
        ``erasures`` as ``decode_host`` takes them."""
        from .. import _hip
        from .. import device as dev

        f = np.ascontiguousarray(np.atleast_2d(np.asarray(frames, dtype=np.uint8)))
        r = None if ref is None else _hip.to_device(np.ascontiguousarray(np.atleast_2d(np.asarray(ref, dtype=np.uint8))))
        era = None if erasures is None else _hip.to_device(np.ascontiguousarray(np.atleast_2d(np.asarray(erasures, dtype=np.uint8))))
        out = dev.rs_decode(self, _hip.to_device(f), bits=bits, ref_msg=r, erasures=era)
        return {"msg": _hip.to_host(out["msg"]), "status": _hip.to_host(out["status"]),
                "counts": None if out["counts"] is None else _hip.to_host(out["counts"])}


def ccsds(e: int = 16, depth: int = 1, n: int = 255) -> RSCode:
    """``RSCode.ccsds``."""
    return RSCode.ccsds(e, depth, n)
