"""Errors-and-erasures Reed-Solomon decoding: wf_rs_decode_erasures / wf_rs_mark_erasures (include/wfhip.h) and
RSCode.decode_host(erasures=) / mark_erasures_host (waveforms_amd/encoding/rs.py).

The result is defined by its outcome: with f <= 2t positions of a word erased, the codeword that differs from the word in e
positions OUTSIDE the erased set with 2e + f <= 2t if there is one (it is unique; status = e), else the received message and
status -1.  On the CPU the host statements are held to that definition on constructed words and, on a (6, 2) code, against
the enumeration of all 65 536 codewords.  On the GPU the kernels must equal the host statements BITWISE: message, status, the
six counts, and the erasures that the marking rule declares.

One reading had to be fixed where two sentences of the definition meet: on a FAILURE the output is the received message as
it came, erased positions included, so two inputs that differ only at erased positions get the same status and, on success,
the same output - on a failure each gets its own received message back (``test_erased_bytes_decide_nothing``).

The cases of a code are built once (``pool``) and shared by every test; a GPU call draws its codewords from that pool at
random, so that clean, correctable, failing and over-erased codewords sit in neighbouring waves.
"""
import ctypes
import functools
import itertools
import json
from pathlib import Path

import numpy as np
import pytest

from waveforms_amd.encoding import rs

ROOT = Path(__file__).resolve().parent.parent
CODES = {"ccsds223": (255, 223), "ccsds239": (255, 239), "short40": (40, 32), "t1": (20, 18)}
NEW_KERNELS = ("rse_decode_kernel<true>", "rse_mark_kernel")


def make_code(name, depth=1):
    n, k = CODES[name]
    return rs.RSCode(n, k, 0x187, 128 - (n - k) // 2, 11, depth)


def grid(t):
    """(e, f) with 2e + f <= 2t: the corners, one erasure, an odd f at the largest e that fits it, and points in between."""
    g = {(0, 0), (t, 0), (0, 2 * t), (0, 1), (t - 1, 1), (t - 1, 2), (1, 2 * t - 2), (t // 2, 2 * t - 2 * (t // 2)), (0, 2 * t - 1)}
    if t >= 2:
        g |= {(t - 2, 3), (1, 2 * t - 3), (t // 2, 1)}
    return sorted((e, f) for e, f in g if e >= 0 and f >= 0 and 2 * e + f <= 2 * t)


def _word(code, rng, e, f, erase_in=None, keep_erased=False):
    """A codeword with ``e`` errors and ``f`` erased positions (inside ``erase_in`` if given), the erased bytes randomised ->
    (word, erasure flags, message sent)."""
    m = rng.integers(0, 256, code.k, dtype=np.uint8)
    w = code.encode_words_host(m[None, :])[0].copy()
    era = np.zeros(code.n, dtype=np.uint8)
    ep = rng.choice(code.n if erase_in is None else np.asarray(erase_in), f, replace=False)
    era[ep] = 1
    if not keep_erased:
        w[ep] = rng.integers(0, 256, f)
    rest = np.flatnonzero(era == 0)
    pos = rng.choice(rest, e, replace=False)
    w[pos] ^= rng.integers(1, 256, e).astype(np.uint8)
    return w, era, m


def _trap(code, rng, j, f):
    """A word of the shortened code that is a FULL-length codeword with j nonzero symbols among the 255 - n dropped leading
    positions, f of its real positions erased (their bytes randomised) -> (word, erasure flags)."""
    full = rs.RSCode(255, 255 - 2 * code.t, code.prim, code.fcr, code.step)
    lead = 255 - code.n
    m = np.zeros(full.k, dtype=np.uint8)
    m[rng.choice(lead, j, replace=False)] = rng.integers(1, 256, j)
    m[lead:] = rng.integers(0, 256, code.k)
    w = full.encode_words_host(m[None, :])[0][lead:].copy()
    era = np.zeros(code.n, dtype=np.uint8)
    ep = rng.choice(code.n, f, replace=False)
    era[ep] = 1
    w[ep] = rng.integers(0, 256, f)
    return w, era


def edge_positions(n):
    """The indices whose degrees, or which themselves, sit at the ends of a lane's ownership (degree = n - 1 - index)."""
    idx = {i for i in (0, 63, 64, 127, 128, n - 1) if i < n}
    return sorted(idx | {n - 1 - i for i in idx})


@functools.lru_cache(maxsize=None)
def pool(name):
    """The cases of a code -> dict(words P x n, era P x n, ref P x k (the message sent; zeros where there is none), kind P, e P
    (errors put in outside the erased set, -1 unknown), f P, msg / status: ``decode_words_host`` of them)."""
    code = make_code(name)
    n, k, t = code.n, code.k, code.t
    rng = np.random.default_rng(sum(map(ord, name)) + 7)
    words, era, ref, kind, ne = [], [], [], [], []

    def add(w, er, m, label, e):
        words.append(w), era.append(er), ref.append(np.zeros(k, dtype=np.uint8) if m is None else m), kind.append(label), ne.append(e)

    for e, f in grid(t):
        for _ in range(2):
            add(*_word(code, rng, e, f), "ok", e)
    for e, f in ((0, 2 * t), (0, 1), (t - 1, 2), (t // 2, 2 * t - 2 * (t // 2))):
        add(*_word(code, rng, e, f, erase_in=np.arange(k, n)), "parity", e)                  # erasures in the parity only
    for e, f in ((0, 2 * t), (t - 1, 1)):
        add(*_word(code, rng, e, f, keep_erased=True), "kept", e)                            # correct symbols erased
    edges = edge_positions(n)[:2 * t]
    add(*_word(code, rng, (2 * t - len(edges)) // 2, len(edges), erase_in=edges), "edges", (2 * t - len(edges)) // 2)
    add(*_word(code, rng, 0, len(edges), erase_in=edges), "edges", 0)
    for f in (2 * t + 1, n):
        add(*_word(code, rng, 0, f), "over", -1)
    for e, f in ((t, 1), (0, 2 * t + 1 - 2 * 0), (t - 1, 3), (t // 2, 2 * t + 1 - 2 * (t // 2))):
        if f <= 2 * t:
            for _ in range(2):
                add(*_word(code, rng, e, f), "one-too-many", -1)
    for _ in range(2):
        add(*_word(code, rng, t + 1, 0), "one-too-many", -1)
    for f in (0, 1, t, 2 * t):
        er = np.zeros(n, dtype=np.uint8)
        er[rng.choice(n, f, replace=False)] = 1
        add(rng.integers(0, 256, n, dtype=np.uint8), er, None, "random", -1)
    add(*_word(code, rng, 0, 0), "ok", 0)
    if n < 255:
        for f in (1, 2, 2 * t - 2):
            for j in range(1, t - (f + 1) // 2 + 1):
                w, er = _trap(code, rng, j, f)
                add(w, er, None, "trap", -1)
    words, era, ref = np.stack(words), np.stack(era), np.stack(ref)
    msg, status = code.decode_words_host(words, era)
    return dict(words=words, era=era, ref=ref, kind=np.array(kind), e=np.array(ne), f=era.sum(axis=1), msg=msg, status=status)


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", sorted(CODES))
def test_decode_host_against_the_definition(name):
    code = make_code(name)
    P = pool(name)
    n, k, t = code.n, code.k, code.t
    seen = set()
    for b in range(P["words"].shape[0]):
        w, er, st, label, e, f = P["words"][b], P["era"][b] != 0, int(P["status"][b]), P["kind"][b], int(P["e"][b]), int(P["f"][b])
        tag = (name, label, b, e, f, st)
        if st >= 0:                                                   # the definition: a codeword, the inequality, status = changes outside E
            c = code.encode_words_host(P["msg"][b][None, :])[0]
            assert f <= 2 * t and int(np.count_nonzero((c != w) & ~er)) == st and 2 * st + f <= 2 * t, tag
        else:
            assert np.array_equal(P["msg"][b], w[:k]), tag
        if label in ("ok", "parity", "kept", "edges"):                # a codeword satisfying the inequality was put there: it is THE result
            assert st == e and np.array_equal(P["msg"][b], P["ref"][b]), tag
            seen.add((e, f))
        if label in ("over", "trap"):
            assert st == -1, tag
        if label == "one-too-many" and st >= 0:                       # (held to the definition above) never the word that was sent
            assert not np.array_equal(P["msg"][b], P["ref"][b]), tag
    assert {(0, 0), (t, 0), (0, 2 * t), (0, 1), (t - 1, 1)} <= seen
    assert set(P["f"][P["kind"] == "over"].tolist()) == {2 * t + 1, n}
    assert ((P["kind"] == "parity") & (P["f"] > 0)).sum() >= 3
    print(f"{name}: statuses of the words with one errata too many:", P["status"][P["kind"] == "one-too-many"].tolist(),
          "of the random words:", P["status"][P["kind"] == "random"].tolist())


@pytest.mark.parametrize("name", sorted(CODES))
def test_erased_bytes_decide_nothing(name):
    """Randomising the bytes at erased positions: the same status everywhere; on success the same message; on a failure the
    received message comes back, the (randomised) erased bytes with it and nothing else changed."""
    code = make_code(name)
    P = pool(name)
    rng = np.random.default_rng(11)
    w2 = P["words"].copy()
    mask = P["era"] != 0
    w2[mask] = rng.integers(0, 256, int(mask.sum()))
    msg2, status2 = code.decode_words_host(w2, P["era"])
    assert np.array_equal(status2, P["status"])
    ok = P["status"] >= 0
    assert ok.any() and (~ok).any() and np.array_equal(msg2[ok], P["msg"][ok])
    assert np.array_equal(msg2[~ok], w2[~ok, :code.k])
    assert np.array_equal(msg2[~ok][~mask[~ok, :code.k]], P["msg"][~ok][~mask[~ok, :code.k]])


def test_erasing_correct_symbols_does_not_count_as_errors():
    code = make_code("ccsds239")
    rng = np.random.default_rng(3)
    m = rng.integers(0, 256, (1, code.k), dtype=np.uint8)
    w = code.encode_words_host(m)
    w[0, [5, 100]] ^= 0x21                                            # two errors ...
    era = np.zeros((1, code.n), dtype=np.uint8)
    era[0, [7, 8, 9, 240]] = 1                                        # ... and four correct symbols erased: 2 2 + 4 <= 16
    msg, status = code.decode_words_host(w, era)
    assert status[0] == 2 and np.array_equal(msg, m)
    era[0, 5] = 1                                                     # an error inside the erased set is an erasure, not an error
    msg, status = code.decode_words_host(w, era)
    assert status[0] == 1 and np.array_equal(msg, m)
    assert code.counts_host(msg, status, m, erasures=era) == [0, 0, 0, 1, 0, 5]
    assert code.counts_host(msg, status, m) == [0, 0, 0, 1, 0]       # the five-count form stays


@pytest.mark.parametrize("name", sorted(CODES))
@pytest.mark.parametrize("depth", [1, 3])
def test_no_erasures_is_todays_decode_host(name, depth):
    code = make_code(name, depth)
    P = pool(name)
    idx = np.random.default_rng(depth).integers(0, P["words"].shape[0], 6 * depth)
    frames = code._join(P["words"][idx])
    m0, s0 = code.decode_host(frames)
    m1, s1 = code.decode_host(frames, erasures=None)
    m2, s2 = code.decode_host(frames, erasures=np.zeros_like(frames))
    assert np.array_equal(m0, m1) and np.array_equal(s0, s1) and np.array_equal(m0, m2) and np.array_equal(s0, s2)
    mb, sb = code.decode_host(rs.to_bits(frames), bits=True, erasures=np.zeros_like(frames))      # symbol form whatever `bits` is
    assert np.array_equal(mb, rs.to_bits(m0)) and np.array_equal(sb, s0)
    # with erasures, frames de-interleave like the words: codeword b I + c takes positions c, c + I, ..
    era = code._join(P["era"][idx])
    m4, s4 = code.decode_host(frames, erasures=era)
    assert np.array_equal(s4, P["status"][idx]) and np.array_equal(m4, code._join(P["msg"][idx]))
    with pytest.raises(ValueError):
        code.decode_host(frames, erasures=era[:, :-1])


def test_the_shortened_codes_trap_with_erasures():
    """A full-length codeword W with j nonzero symbols among the 255 - n dropped positions, f real positions erased.  A
    shortened codeword c with 2e + f <= 2t would, padded with zeros, be a full codeword that differs from W in at most
    j + e + f places; with j <= t - ceil(f / 2) that is at most 2t, below the minimum distance: the status must be -1, although
    the errata locator of W itself (roots at the virtual positions) is what the algorithm finds."""
    code = make_code("short40")
    rng = np.random.default_rng(41)
    seen = 0
    for f in (1, 2, 3, 4, 6):
        for j in range(1, code.t - (f + 1) // 2 + 1):
            w, era = _trap(code, rng, j, f)
            msg, status = code.decode_words_host(w[None, :], era[None, :])
            assert status[0] == -1 and np.array_equal(msg[0], w[:code.k]), (j, f)
            seen += 1
    assert seen >= 8


def test_brute_force_on_a_6_2_code():
    """RS(6, 2), t = 2: for 200 random (r, E), f = 0 .. 5, the existence of a codeword with 2e + f <= 2t, found by enumerating all
    65 536 codewords, equals status >= 0, and the message is that codeword's."""
    code = rs.RSCode(6, 2, 0x187, 126, 11)
    allm = np.stack(np.meshgrid(np.arange(256), np.arange(256), indexing="ij"), axis=-1).reshape(-1, 2).astype(np.uint8)
    allc = code.encode_words_host(allm)
    assert not code.syndromes_host(allc[::97]).any()
    rng = np.random.default_rng(62)
    hits = {True: 0, False: 0}
    for trial in range(200):
        f = trial % 6
        r = allc[rng.integers(0, 65536)].copy()
        ne = int(rng.integers(0, 4))
        r[rng.choice(6, ne, replace=False)] ^= rng.integers(1, 256, ne).astype(np.uint8)
        era = np.zeros(6, dtype=np.uint8)
        era[rng.choice(6, f, replace=False)] = 1
        e = ((allc != r[None, :]) & (era == 0)[None, :]).sum(axis=1)
        good = np.flatnonzero(2 * e + f <= 4) if f <= 4 else np.array([], dtype=np.int64)
        assert good.size <= 1                                          # the uniqueness argument
        msg, status = code.decode_words_host(r[None, :], era[None, :])
        assert (status[0] >= 0) == (good.size == 1), (trial, f, ne, status)
        if good.size:
            assert status[0] == e[good[0]] and np.array_equal(msg[0], allm[good[0]]), (trial, f, ne)
        else:
            assert np.array_equal(msg[0], r[:2])
        hits[bool(good.size)] += 1
    assert hits[True] >= 40 and hits[False] >= 40, hits


def _post_from_rho(code, rho_words, rng):
    """A Λ (F x 8 n I float32) whose symbol reliabilities are ``rho_words`` (F I x n, by codeword): one bit of a symbol, at a
    random place and with a random sign, carries ρ, the others something larger."""
    rho = np.asarray(rho_words, dtype=np.float32)
    sym = rho.reshape(-1, code.depth, code.n).transpose(0, 2, 1).reshape(-1, code.n * code.depth)      # frame order
    post = (sym[..., None] + rng.uniform(0.0, 3.0, sym.shape + (8,))).astype(np.float32)
    at = rng.integers(0, 8, sym.shape)
    np.put_along_axis(post, at[..., None], sym[..., None], axis=2)
    post *= rng.choice(np.array([-1.0, 1.0], dtype=np.float32), post.shape)
    return post.reshape(sym.shape[0], -1)


def test_mark_erasures_host():
    code = make_code("short40")
    rng = np.random.default_rng(9)
    rho = np.full((1, 40), 9.0, dtype=np.float32)
    rho[0, [30, 4, 17, 22]] = [1.0, 1.0, 0.5, 1.0]                     # ties: the smaller index first
    post = _post_from_rho(code, rho, rng)
    mark = lambda f_max, below=float("inf"): np.flatnonzero(code.mark_erasures_host(post, f_max, below)[0]).tolist()      # noqa: E731
    assert mark(1) == [17] and mark(2) == [4, 17] and mark(3) == [4, 17, 22] and mark(4) == [4, 17, 22, 30]
    assert mark(0) == [] and mark(8, 0.5) == [] and mark(8, -1.0) == [] and mark(8, 0.0) == []      # `below` excludes everything
    assert mark(8, 0.75) == [17] and mark(8, 1.0) == [17] and mark(8, 1.5) == [4, 17, 22, 30]      # f_max above what is under `below`
    assert len(mark(8)) == 8 and len(mark(8, 9.0)) == 4 and len(mark(8, 1e39)) == 8               # (an infinite float32: no threshold)
    out = code.mark_erasures_host(post, 3)
    assert out.dtype == np.uint8 and out.shape == (1, 40) and set(out.ravel().tolist()) == {0, 1}
    with pytest.raises(ValueError):
        code.mark_erasures_host(post, 9)
    with pytest.raises(ValueError):
        code.mark_erasures_host(post, -1)
    with pytest.raises(ValueError):
        code.mark_erasures_host(post, 2, float("nan"))
    with pytest.raises(ValueError):
        code.mark_erasures_host(post[:, :-8], 2)
    # ρ is the minimum over the symbol's EIGHT bits of |Λ|, whatever the sign and the place
    p2 = np.full((1, 320), 5.0, dtype=np.float32)
    p2[0, 8 * 3 + 7], p2[0, 8 * 9 + 0] = -0.25, 0.125
    assert np.flatnonzero(code.mark_erasures_host(p2, 2)[0]).tolist() == [3, 9] and np.flatnonzero(code.mark_erasures_host(p2, 1)[0]).tolist() == [9]


def test_mark_erasures_host_deinterleaves_at_depth_5():
    """A Λ whose small values all sit in codeword 3 of frame 1: every erasure lands there, at positions c + I i of that frame."""
    code = make_code("short40", 5)
    rng = np.random.default_rng(10)
    rho = np.full((2 * 5, 40), 7.0, dtype=np.float32)
    small = [0, 1, 13, 38, 39]
    rho[5 + 3, small] = [0.3, 0.2, 0.1, 0.4, 0.2]
    post = _post_from_rho(code, rho, rng)
    out = code.mark_erasures_host(post, 4, 1.0)
    assert out.shape == (2, 200) and not out[0].any()
    assert np.flatnonzero(out[1]).tolist() == [3 + 5 * i for i in (0, 1, 13, 39)]      # (0.4 at index 38 is the fifth)
    by_word = code._split(out, 40)
    assert by_word[8].sum() == 4 and by_word.sum() == 4
    every = code.mark_erasures_host(post, 8)                           # no threshold: f_max per codeword, in every codeword
    assert code._split(every, 40).sum(axis=1).tolist() == [8] * 10


def test_c_refusals_without_a_gpu():
    """WF_ERR_VALUE before the context or device memory is touched (a fake context and a fake code whose t reads as 0)."""
    from waveforms_amd import _hip

    lib = _hip.lib()
    fake = ctypes.create_string_buffer(1 << 16)
    V = _hip.WF_ERR_VALUE
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    dec = lib.wf_rs_decode_erasures
    assert dec(None, fake, p, p, 1, 0, p, None, None, None, None) == V and dec(fake, None, p, p, 1, 0, p, None, None, None, None) == V
    assert dec(fake, fake, None, p, 1, 0, p, None, None, None, None) == V
    assert dec(fake, fake, p, None, 1, 0, p, None, None, None, None) == V                    # NULL d_erase
    assert dec(fake, fake, p, p, 1, 0, None, None, None, None, None) == V
    assert dec(fake, fake, p, p, 0, 0, p, None, None, None, None) == V and dec(fake, fake, p, p, 1, 2, p, None, None, None, None) == V
    assert dec(fake, fake, p, p, 1, 0, p, None, p, None, None) == V                          # a reference without counts
    assert dec(fake, fake, p, p, 1, 0, p, p + 2, None, None, None) == V                      # a misaligned status
    mark = lib.wf_rs_mark_erasures
    assert mark(None, fake, p, 1, 0, 1.0, p, None) == V and mark(fake, None, p, 1, 0, 1.0, p, None) == V
    assert mark(fake, fake, None, 1, 0, 1.0, p, None) == V and mark(fake, fake, p, 1, 0, 1.0, None, None) == V
    assert mark(fake, fake, p, 0, 0, 1.0, p, None) == V
    assert mark(fake, fake, p, 1, -1, 1.0, p, None) == V and mark(fake, fake, p, 1, 1, 1.0, p, None) == V      # f_max outside 0 .. 2t
    for bad in (float("inf"), float("-inf"), float("nan")):
        assert mark(fake, fake, p, 1, 0, bad, p, None) == V
    assert mark(fake, fake, p + 2, 1, 0, 1.0, p, None) == V


def test_entry_points_exported_and_bound():
    from waveforms_amd import _hip
    from waveforms_amd import device
    from waveforms_amd.encoding.rsconv import RSConvSOQPSKLink

    for name in ("wf_rs_decode_erasures", "wf_rs_mark_erasures"):
        assert name in _hip.SIGNATURES and hasattr(_hip.lib(), name)
    assert callable(device.rs_mark_erasures) and callable(RSConvSOQPSKLink.rs_erasure_result)
    assert rs.below_f32(float("inf")) == float(np.finfo(np.float32).max) and rs.below_f32(0.1) == float(np.float32(0.1))


def test_new_kernels_resources():
    """No scratch, no vector or scalar spills in the two new kernels; their VGPR and LDS ceilings are the shipped counts
    (profiles/rs_erasure_kernel_resources.json); the errors-only kernel keeps the figures tests/test_rs.py holds it to."""
    import sys

    sys.path.insert(0, str(ROOT / "tools"))
    import kernel_resources as kr
    from waveforms_amd.csrc.build import build

    so = build(verbose=False)
    tab = kr.kernel_table(so)
    asm = kr.loop_spill_counts(so, "rse_")
    shipped = json.loads((ROOT / "profiles" / "rs_erasure_kernel_resources.json").read_text())["kernels"]
    assert sorted(k for k in tab if k.startswith("rse_")) == sorted(NEW_KERNELS) == sorted(shipped)
    for name in NEW_KERNELS:
        row, a = tab[name], asm[name]
        assert row["vgpr_spill_count"] == 0 and row["sgpr_spill_count"] == 0 and row["private_segment_fixed_size"] == 0, (name, row)
        assert a["scratch_load"] == 0 and a["scratch_store"] == 0 and a["v_writelane"] == 0, (name, a)
        assert row.get("wavefront_size", 64) == 64 and row["max_flat_workgroup_size"] == 512
        assert row["vgpr_count"] + row.get("agpr_count", 0) <= shipped[name]["vgpr_count"], (name, row)
        assert row["group_segment_fixed_size"] <= shipped[name]["group_segment_fixed_size"], (name, row)
        assert kr.waves_per_simd(row["vgpr_count"], row.get("agpr_count", 0)) >= 4, row


# ------------------------------------------------------------------------------------------------ GPU
def _mixed(name, depth, nframes, seed):
    """``nframes`` frames of ``depth`` codewords drawn from the pool -> (code, frames, erasures, expected message frames,
    status, reference message frames)."""
    code = make_code(name, depth)
    P = pool(name)
    idx = np.random.default_rng(seed).integers(0, P["words"].shape[0], nframes * depth)
    return code, code._join(P["words"][idx]), code._join(P["era"][idx]), code._join(P["msg"][idx]), P["status"][idx], code._join(P["ref"][idx])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CODES))
@pytest.mark.parametrize("depth", [1, 5])
def test_gpu_decoder_is_the_host_decoder(name, depth):
    """Message, status and the six counts, both bit forms, 1 / 67 / 3 000 frames; erased positions at the lane-ownership
    edges and over-erased words are in the pool."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    P = pool(name)
    assert {"ok", "edges", "over", "one-too-many", "random", "parity"} <= set(P["kind"].tolist())
    for nframes, bits in itertools.product((1, 67, 3000), (False, True)):
        code, frames, era, want_msg, want_status, ref = _mixed(name, depth, nframes, 1000 * depth + nframes)
        rx, rf = (rs.to_bits(frames), rs.to_bits(ref)) if bits else (frames, ref)
        counts = _hip.to_device(np.array([6, 5, 4, 3, 2, 1], dtype=np.int64))                  # the counts are ADDED
        out = dev.rs_decode(code, _hip.to_device(rx), bits=bits, ref_msg=_hip.to_device(rf), counts=counts, erasures=_hip.to_device(era))
        _hip.device_check()
        tag = (name, depth, nframes, bits)
        got = _hip.to_host(out["msg"])
        assert np.array_equal(_hip.to_host(out["status"]), want_status), tag
        assert np.array_equal(got, rs.to_bits(want_msg) if bits else want_msg), tag
        want_counts = code.counts_host(want_msg, want_status, ref, erasures=era)
        assert len(want_counts) == 6 and (_hip.to_host(counts) - [6, 5, 4, 3, 2, 1]).tolist() == want_counts, tag
        if nframes == 67:
            f = code._split(era, code.n).sum(axis=1)
            assert want_counts[2] > 0 and want_counts[3] > 0 and want_counts[5] > 0 and (f > 2 * code.t).any() and (f == 0).any()
            assert ((want_status >= 0) & (f > 0)).any() and ((want_status < 0) & (f > 0) & (f <= 2 * code.t)).any()
            plain = dev.rs_decode(code, _hip.to_device(rx), bits=bits, want_status=False, erasures=_hip.to_device(era))
            assert plain["status"] is None and plain["counts"] is None and np.array_equal(_hip.to_host(plain["msg"]), got)
    _hip.device_check()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CODES))
def test_gpu_no_erasures_is_wf_rs_decode(name):
    """With an all-zero erasure array the output equals wf_rs_decode byte for byte: message, status and the five counts."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    for depth, bits in itertools.product((1, 5), (False, True)):
        code, frames, _era, _m, _s, ref = _mixed(name, depth, 67, 77 + depth)
        rx, rf = (rs.to_bits(frames), rs.to_bits(ref)) if bits else (frames, ref)
        d_rx, d_rf = _hip.to_device(rx), _hip.to_device(rf)
        old = dev.rs_decode(code, d_rx, bits=bits, ref_msg=d_rf)
        new = dev.rs_decode(code, d_rx, bits=bits, ref_msg=d_rf, erasures=_hip.to_device(np.zeros_like(frames)))
        assert np.array_equal(_hip.to_host(old["msg"]), _hip.to_host(new["msg"])) and np.array_equal(_hip.to_host(old["status"]), _hip.to_host(new["status"]))
        c_old, c_new = _hip.to_host(old["counts"]).tolist(), _hip.to_host(new["counts"]).tolist()
        assert c_new == c_old + [0] and (_hip.to_host(old["status"]) != 0).any()
    _hip.device_check()


@pytest.mark.gpu
def test_gpu_unaligned_bit_buffers_and_the_host_wrapper():
    """A bit-form buffer that is not 8-byte aligned takes the byte path, an aligned one the 8-byte path; RSCode.decode wraps it."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    code, frames, era, want_msg, want_status, ref = _mixed("short40", 2, 9, 5)
    bits = rs.to_bits(frames)
    d_era = _hip.to_device(era)
    buf = _hip.zeros(bits.size + 3, "uint8")
    view = buf[3:]
    view.copy_(_hip.to_device(bits.reshape(-1)))
    assert view.data_ptr() % 8 == 3
    out = dev.rs_decode(code, view, bits=True, erasures=d_era)
    assert np.array_equal(_hip.to_host(out["msg"]), rs.to_bits(want_msg)) and np.array_equal(_hip.to_host(out["status"]), want_status)
    aligned = _hip.to_device(bits)
    assert aligned.data_ptr() % 8 == 0
    out = dev.rs_decode(code, aligned, bits=True, erasures=d_era)
    assert out["msg"].data_ptr() % 8 == 0
    assert np.array_equal(_hip.to_host(out["msg"]), rs.to_bits(want_msg)) and np.array_equal(_hip.to_host(out["status"]), want_status)
    got = code.decode(frames, ref=ref, erasures=era)
    assert np.array_equal(got["msg"], want_msg) and np.array_equal(got["status"], want_status)
    assert got["counts"].tolist() == code.counts_host(want_msg, want_status, ref, erasures=era)
    _hip.device_check()


def _tied_rho(code, nwords, rng):
    """Reliabilities drawn from a handful of values: exact ties across lanes (indices 64 apart and not) and within a lane's four
    symbols (indices i, i + 64, i + 128, i + 192)."""
    rho = rng.choice(np.array([0.0, 0.125, 0.5, 0.5000001, 1.0, 2.0, 1e-40, 3e38], dtype=np.float32), (nwords, code.n)).astype(np.float32)
    rho[0] = 0.5                                                       # every symbol ties
    if nwords > 1:
        rho[1] = 4.0
        rho[1, [i for i in (3, 67, 131, 195, 2, 66) if i < code.n]] = 0.25      # one lane's four symbols and a neighbour's two
    return rho


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ccsds223", "short40", "t1"])
@pytest.mark.parametrize("depth", [1, 5])
def test_gpu_mark_erasures_is_the_host_rule(name, depth):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    code = make_code(name, depth)
    rng = np.random.default_rng(depth + len(name))
    for nframes in (1, 67):
        post = _post_from_rho(code, _tied_rho(code, nframes * depth, rng), rng)
        d_post = _hip.to_device(post)
        for f_max, below in ((0, 1.0), (1, float("inf")), (2 * code.t, float("inf")), (2 * code.t, 0.5), (code.t, 0.75), (2 * code.t, 0.0), (2, 1e-39)):
            got = _hip.to_host(dev.rs_mark_erasures(code, d_post, f_max, below))
            want = code.mark_erasures_host(post, f_max, below)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (name, depth, nframes, f_max, below)
        if nframes == 67:                                              # (the thresholds cut inside the drawn values, the denormal one included)
            assert code.mark_erasures_host(post, 2 * code.t, 0.5).any() and code.mark_erasures_host(post, 2, 1e-39).any()
    _hip.device_check()


@pytest.mark.gpu
def test_gpu_refusals_leave_the_outputs_untouched():
    from waveforms_amd import _hip

    code = make_code("short40", 2)
    lib, ctx, h, V = _hip.lib(), _hip.ctx(), code.handle(), _hip.WF_ERR_VALUE
    rx = _hip.zeros(2 * 80, "uint8")
    era = _hip.zeros(2 * 80, "uint8")
    post = _hip.torch().zeros(2 * 640, dtype=_hip.torch().float32, device="cuda")
    msg = _hip.to_device(np.full(2 * 64, 0xA5, dtype=np.uint8))
    status = _hip.to_device(np.full(4, 77, dtype=np.int32))
    counts = _hip.to_device(np.arange(6, dtype=np.int64) + 10)
    ref = _hip.zeros(2 * 64, "uint8")
    P = _hip.ptr
    args = dict(ctx=ctx, code=h, rx=P(rx), erase=P(era), nframes=2, bits=0, msg=P(msg), status=P(status), ref=P(ref), counts=P(counts))

    def dec(**over):
        a = dict(args, **over)
        return lib.wf_rs_decode_erasures(a["ctx"], a["code"], a["rx"], a["erase"], a["nframes"], a["bits"], a["msg"], a["status"], a["ref"], a["counts"], None)

    for over in (dict(ctx=None), dict(code=None), dict(rx=None), dict(erase=None), dict(msg=None), dict(nframes=0), dict(nframes=-3), dict(bits=2), dict(bits=-1),
                 dict(counts=None), dict(status=P(status) + 2), dict(counts=P(counts) + 4)):
        assert dec(**over) == V, over
    out = _hip.to_device(np.full(2 * 80, 9, dtype=np.uint8))

    def mark(**over):
        a = dict(dict(ctx=ctx, code=h, post=P(post), nframes=2, f_max=2, below=1.0, erase=P(out)), **over)
        return lib.wf_rs_mark_erasures(a["ctx"], a["code"], a["post"], a["nframes"], a["f_max"], a["below"], a["erase"], None)

    for over in (dict(ctx=None), dict(code=None), dict(post=None), dict(erase=None), dict(nframes=0), dict(f_max=-1), dict(f_max=2 * code.t + 1),
                 dict(below=float("inf")), dict(below=float("-inf")), dict(below=float("nan")), dict(post=P(post) + 2)):
        assert mark(**over) == V, over
    _hip.device_check()
    assert (_hip.to_host(msg) == 0xA5).all() and (_hip.to_host(status) == 77).all() and _hip.to_host(counts).tolist() == list(range(10, 16))
    assert (_hip.to_host(out) == 9).all()
    assert dec() == 0 and mark() == 0                                  # (the same arguments, none overridden, are accepted)
    _hip.device_check()
    assert not _hip.to_host(status).any() and not _hip.to_host(msg).any() and _hip.to_host(counts).tolist() == list(range(10, 16))
    assert _hip.to_host(out).reshape(2, 40, 2)[:, :2].all() and _hip.to_host(out).sum() == 2 * 2 * 2      # every ρ is 0: indices 0 and 1
