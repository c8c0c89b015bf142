"""Reed-Solomon codes: wf_rs_code_create / wf_rs_encode / wf_rs_decode (include/wfhip.h) and RSCode
(waveforms_amd/encoding/rs.py).

The decoder's result is defined by its outcome: the codeword within t symbols of the received word if there is one, else the
received message and status -1.  On the CPU the host statements are held to that definition on constructed cases (known
codewords with known error patterns, the shortened code's trap) and, for every successful decode, by re-encoding.  On the GPU the
kernels must equal the host statements BITWISE: message, status and the five counts.

The cases of a code are built once (``pool``) and shared by every test; a GPU call takes its codewords from that pool, mixed
at random, so that clean, correctable and failing codewords sit in neighbouring waves.
"""
import ctypes
import functools
import itertools

import numpy as np
import pytest

from waveforms_amd.encoding import rs

CODES = {"ccsds223": (255, 223), "ccsds239": (255, 239), "short40": (40, 32)}


def make_code(name, depth=1):
    n, k = CODES[name]
    return rs.RSCode(n, k, 0x187, 128 - (n - k) // 2, 11, depth)


def _hit(rng, words, ne, positions=None):
    """``ne`` symbol errors (nonzero differences) per word, at random positions or inside ``positions``."""
    out = words.copy()
    n = words.shape[1]
    for b in range(out.shape[0]):
        pos = rng.choice(n if positions is None else positions, ne, replace=False)
        out[b, pos] ^= rng.integers(1, 256, ne).astype(np.uint8)
    return out


@functools.lru_cache(maxsize=None)
def pool(name):
    """The cases of a code -> dict(words P x n, ref P x k (the message sent; zeros for a random word), kind P (a label), nerr P
    (errors put in, -1 unknown), msg / status: ``decode_words_host`` of the words)."""
    code = make_code(name)
    n, k, t = code.n, code.k, code.t
    rng = np.random.default_rng(sum(map(ord, name)))
    words, ref, kind, nerr = [], [], [], []

    def add(w, m, label, ne):
        words.append(w), ref.append(m), kind.extend([label] * w.shape[0]), nerr.extend([ne] * w.shape[0])

    for ne in (0, 1, t, t + 1):
        m = rng.integers(0, 256, (6, k), dtype=np.uint8)
        add(_hit(rng, code.encode_words_host(m), ne), m, f"cw+{ne}", ne)
    m = rng.integers(0, 256, (4, k), dtype=np.uint8)
    c = code.encode_words_host(m)
    first_last = c.copy()
    first_last[:, 0] ^= 0x5A
    first_last[:, n - 1] ^= 0x01
    add(first_last, m, "ends", 2 if t >= 2 else -1)
    add(_hit(rng, c, t, positions=np.arange(k, n)), m, "parity", t)
    add(rng.integers(0, 256, (6, n), dtype=np.uint8), np.zeros((6, k), dtype=np.uint8), "random", -1)
    add(np.zeros((1, n), dtype=np.uint8), np.zeros((1, k), dtype=np.uint8), "zeros", 0)
    add(np.full((1, n), 0xFF, dtype=np.uint8), np.full((1, k), 0xFF, dtype=np.uint8), "ones", -1)
    if n < 255:                                                       # the shortened code's trap (see the test below)
        for j in range(1, t + 1):
            w, m = _trap(code, rng, j)
            add(w[None, :], m[None, :], "trap", -1)
    words, ref = np.concatenate(words), np.concatenate(ref)
    msg, status = code.decode_words_host(words)
    return dict(words=words, ref=ref, kind=np.array(kind), nerr=np.array(nerr), msg=msg, status=status)


def _trap(code, rng, j):
    """A word of the shortened code that is a FULL-length codeword with j nonzero symbols among the 255 - n leading positions,
    those positions dropped -> (word n, its message part k)."""
    full = rs.RSCode(255, 255 - 2 * code.t, code.prim, code.fcr, code.step)
    lead = 255 - code.n
    m = np.zeros(full.k, dtype=np.uint8)
    m[rng.choice(lead, j, replace=False)] = rng.integers(1, 256, j)
    m[lead:] = rng.integers(0, 256, code.k)
    c = full.encode_words_host(m[None, :])[0]
    return c[lead:], m[lead:]


# ------------------------------------------------------------------------------------------------ CPU
def test_ccsds_generators_are_palindromic_with_the_pinned_coefficients():
    for e, c1 in ((16, 91), (8, 165)):
        code = rs.RSCode.ccsds(e)
        assert (code.n, code.k, code.t, code.prim, code.step, code.fcr) == (255, 255 - 2 * e, e, 0x187, 11, 128 - e)
        assert code.gen.size == 2 * e + 1 and code.gen[-1] == 1
        assert np.array_equal(code.gen, code.gen[::-1]) and code.gen[1] == c1
    conv = rs.RSCode.conventional(255, 223)
    assert (conv.prim, conv.fcr, conv.step) == (0x11d, 0, 1)
    assert sorted(make_code("ccsds223").exp[:255].tolist()) == list(range(1, 256))      # 0x187 is primitive


@pytest.mark.parametrize("name", sorted(CODES))
@pytest.mark.parametrize("depth", [1, 5])
def test_every_encoded_word_has_zero_syndromes(name, depth):
    code = make_code(name, depth)
    rng = np.random.default_rng(depth)
    m = rng.integers(0, 256, (7, code.k * depth), dtype=np.uint8)
    tx = code.encode_host(m)
    assert tx.shape == (7, code.n * depth) and tx.dtype == np.uint8
    words = code._split(tx, code.n)
    assert not code.syndromes_host(words).any()
    # systematic, interleaved: position p of a frame belongs to codeword p mod I at index p div I
    for p in (0, 1, depth, code.k * depth - 1):
        assert np.array_equal(tx[:, p], m[:, p])
    assert np.array_equal(words[::depth, :code.k], m[:, 0::depth])
    # the bit form is the same frames, eight bytes of 0 / 1 per symbol, MSB first
    assert np.array_equal(code.encode_host(rs.to_bits(m), bits=True), rs.to_bits(tx))
    assert rs.to_bits(np.array([[0x80, 0x01]], dtype=np.uint8)).tolist() == [[1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]]
    assert np.array_equal(rs.from_bits(rs.to_bits(tx)), tx)
    # a word off by one symbol is not a codeword
    words[0, 3] ^= 1
    assert code.syndromes_host(words[:1]).all()


@pytest.mark.parametrize("name", sorted(CODES))
def test_decode_host_against_the_definition(name):
    code = make_code(name)
    P = pool(name)
    t = code.t
    mis = 0
    for b in range(P["words"].shape[0]):
        w, st, label, ne = P["words"][b], int(P["status"][b]), P["kind"][b], int(P["nerr"][b])
        if st >= 0:                                                   # the output re-encodes to a word within `status` of the input
            c = code.encode_words_host(P["msg"][b][None, :])[0]
            assert st <= t and int(np.count_nonzero(c != w)) == st, (label, b, st)
        else:
            assert np.array_equal(P["msg"][b], w[:code.k]), (label, b)
        if 0 <= ne <= t:                                              # a codeword within t was put there: it is THE result
            assert st == ne and np.array_equal(P["msg"][b], P["ref"][b]), (label, b, st, ne)
        if label == f"cw+{t + 1}" and st >= 0:
            mis += 1                                                  # (checked above: a codeword within t of the input)
            assert not np.array_equal(P["msg"][b], P["ref"][b])
        if label == "trap":
            assert st == -1, (label, b, st)
        if label == "ones":                                           # (x^255 - 1) / (x - 1) times 0xFF: a codeword when n = 255 and no root of g is 1
            assert st == (0 if code.n == 255 else -1), (label, b, st)
        if label == "zeros":
            assert st == 0
    print(f"{name}: {mis} miscorrections among the {int((P['kind'] == f'cw+{t + 1}').sum())} words with t + 1 errors;",
          "statuses of the random words:", P["status"][P["kind"] == "random"].tolist())


def test_the_shortened_codes_trap():
    """A full-length codeword with j <= t nonzero symbols among the 255 - n leading positions, those positions dropped: a
    shortened codeword within t of it would be a full codeword within j + t <= 2t of another, so the status must be -1."""
    code = make_code("short40")
    rng = np.random.default_rng(40)
    for j in range(1, code.t + 1):
        for _ in range(3):
            w, _m = _trap(code, rng, j)
            msg, status = code.decode_words_host(w[None, :])
            assert status[0] == -1 and np.array_equal(msg[0], w[:code.k]), j
    # (with no nonzero leading symbol the same construction IS a shortened codeword)
    full = rs.RSCode(255, 255 - 2 * code.t, code.prim, code.fcr, code.step)
    m = np.zeros(full.k, dtype=np.uint8)
    m[255 - code.n:] = rng.integers(0, 256, code.k)
    assert np.array_equal(full.encode_words_host(m[None, :])[0, 255 - code.n:], code.encode_words_host(m[None, 255 - code.n:])[0])


def test_frames_and_counts_on_the_host():
    code = make_code("short40", 3)
    P = pool("short40")
    idx = np.arange(6)[None, :].repeat(2, axis=0).reshape(4, 3)       # 4 frames of 3 codewords
    idx[1] = [0, 20, 1]                                                # cw+0, cw+(t+1), cw+0
    frames = code._join(P["words"][idx.reshape(-1)])
    assert np.array_equal(frames[1, 0::3], P["words"][0]) and np.array_equal(frames[1, 1::3], P["words"][20])
    msg, status = code.decode_host(frames)
    assert np.array_equal(status, P["status"][idx.reshape(-1)]) and np.array_equal(msg, code._join(P["msg"][idx.reshape(-1)]))
    ref = code._join(P["ref"][idx.reshape(-1)])
    counts = code.counts_host(msg, status, ref)
    wrong = (P["msg"][idx] != P["ref"][idx]).any(axis=2)
    assert counts[1] == int(wrong.sum()) and counts[4] == int(wrong.any(axis=1).sum()) and counts[2] == int((status < 0).sum())
    mb, sb = code.decode_host(rs.to_bits(frames), bits=True)
    assert np.array_equal(mb, rs.to_bits(msg)) and np.array_equal(sb, status)
    assert code.counts_host(mb, sb, rs.to_bits(ref), bits=True) == counts


def test_c_create_refuses_invalid_codes_without_a_gpu():
    """WF_ERR_VALUE before the context or device memory is touched (a fake context), and the argument checks of the calls."""
    from waveforms_amd import _hip

    lib = _hip.lib()
    fake = ctypes.create_string_buffer(1 << 16)
    V = _hip.WF_ERR_VALUE
    good = dict(prim=0x187, fcr=112, step=11, n=255, k=223, depth=1)

    def create(**over):
        a = dict(good, **over)
        out = ctypes.c_void_p()
        return lib.wf_rs_code_create(fake, a["prim"], a["fcr"], a["step"], a["n"], a["k"], a["depth"], ctypes.byref(out)), out.value

    bad = [dict(prim=0x11b), dict(prim=0x87), dict(prim=0x387), dict(step=3), dict(step=5), dict(step=0), dict(step=255), dict(k=255), dict(k=221),
           dict(k=222), dict(n=256, k=224), dict(n=300, k=268), dict(k=0), dict(n=32, k=0), dict(depth=0), dict(depth=9), dict(fcr=-1), dict(fcr=255)]
    for over in bad:
        rc, h = create(**over)
        assert rc == V and h is None, over
        with pytest.raises(ValueError):
            a = dict(good, **over)
            rs.RSCode(a["n"], a["k"], a["prim"], a["fcr"], a["step"], a["depth"])
    assert lib.wf_rs_code_create(None, 0x187, 112, 11, 255, 223, 1, None) == V
    assert lib.wf_rs_code_free(None) == 0
    geom = (ctypes.c_int64 * 5)()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert lib.wf_rs_decode_geometry(fake, None, 10, geom) == V and lib.wf_rs_decode_geometry(fake, fake, 0, geom) == V
    assert lib.wf_rs_encode(fake, None, p, 1, 0, p, None) == V and lib.wf_rs_encode(fake, fake, None, 1, 0, p, None) == V
    assert lib.wf_rs_encode(fake, fake, p, 0, 0, p, None) == V and lib.wf_rs_encode(fake, fake, p, 1, 2, p, None) == V
    assert lib.wf_rs_encode(fake, fake, p, 1, -1, p, None) == V
    assert lib.wf_rs_decode(fake, None, p, 1, 0, p, None, None, None, None) == V
    assert lib.wf_rs_decode(fake, fake, None, 1, 0, p, None, None, None, None) == V
    assert lib.wf_rs_decode(fake, fake, p, 1, 0, None, None, None, None, None) == V
    assert lib.wf_rs_decode(fake, fake, p, 0, 0, p, None, None, None, None) == V
    assert lib.wf_rs_decode(fake, fake, p, 1, 2, p, None, None, None, None) == V
    assert lib.wf_rs_decode(fake, fake, p, 1, 0, p, None, p, None, None) == V          # a reference without counts


def test_python_validation():
    with pytest.raises(ValueError):
        rs.RSCode.ccsds(4)
    code = make_code("short40", 2)
    with pytest.raises(ValueError):
        code.encode_host(np.zeros((1, 32), dtype=np.uint8))           # a frame is k depth symbols
    with pytest.raises(ValueError):
        code.decode_host(np.zeros((1, 40), dtype=np.uint8))
    assert rs.RSCode.ccsds(8, depth=3, n=100).k == 84 and rs.ccsds(16, 2).depth == 2


def test_rs_entry_points_exported_and_bound():
    from waveforms_amd import _hip
    from waveforms_amd import device

    lib = _hip.lib()
    for name in ("wf_rs_code_create", "wf_rs_code_free", "wf_rs_encode", "wf_rs_decode", "wf_rs_decode_geometry"):
        assert name in _hip.SIGNATURES and hasattr(lib, name)
    assert callable(device.rs_encode) and callable(device.rs_decode) and callable(device.rs_decode_geometry)


def test_rs_kernels_resources():
    """No scratch, no spills; eight waves of a depth-8 frame fit a workgroup."""
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
    import kernel_resources as kr
    from waveforms_amd.csrc.build import build

    so = build(verbose=False)
    tab = {k: v for k, v in kr.kernel_table(so).items() if k.startswith("rs_")}
    assert set(tab) == {"rs_encode_kernel<true>", "rs_decode_kernel<true>"}, sorted(tab)      # (<true>: products by tables in LDS)
    asm = kr.loop_spill_counts(so, "rs_")
    for name, row in tab.items():
        assert row["vgpr_spill_count"] == 0 and row["sgpr_spill_count"] == 0 and row["private_segment_fixed_size"] == 0, (name, row)
        a = asm[name]
        assert a["scratch_load"] == 0 and a["scratch_store"] == 0 and a["v_writelane"] == 0, (name, a)
        assert row.get("wavefront_size", 64) == 64 and row["max_flat_workgroup_size"] == 512
        assert kr.waves_per_simd(row["vgpr_count"], row.get("agpr_count", 0)) >= 4, row
        assert row["group_segment_fixed_size"] <= 776, row


# ------------------------------------------------------------------------------------------------ GPU
def _mixed_frames(name, depth, nframes, seed):
    """``nframes`` frames of ``depth`` codewords drawn from the pool -> (code, frames, expected message frames, status, reference
    message frames)."""
    code = make_code(name, depth)
    P = pool(name)
    idx = np.random.default_rng(seed).integers(0, P["words"].shape[0], nframes * depth)
    return code, code._join(P["words"][idx]), code._join(P["msg"][idx]), P["status"][idx], code._join(P["ref"][idx])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CODES))
@pytest.mark.parametrize("depth", [1, 5])
def test_gpu_decoder_is_the_host_decoder(name, depth):
    """Message, status and the five counts, both bit forms, 1 / 67 / 3 000 frames."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    for nframes, bits in itertools.product((1, 67, 3000), (False, True)):
        code, frames, want_msg, want_status, ref = _mixed_frames(name, depth, nframes, 1000 * depth + nframes)
        geo = dev.rs_decode_geometry(code, nframes)
        assert (geo["waves_per_workgroup"], geo["workgroups"], geo["launches"], geo["threads_per_workgroup"]) == (depth, nframes, 1, 64 * depth)
        rx, rf = (rs.to_bits(frames), rs.to_bits(ref)) if bits else (frames, ref)
        counts = _hip.to_device(np.array([5, 4, 3, 2, 1], dtype=np.int64))                     # the counts are ADDED
        out = dev.rs_decode(code, _hip.to_device(rx), bits=bits, ref_msg=_hip.to_device(rf), counts=counts)
        _hip.device_check()
        tag = (name, depth, nframes, bits)
        got = _hip.to_host(out["msg"])
        assert np.array_equal(got, rs.to_bits(want_msg) if bits else want_msg), tag
        assert np.array_equal(_hip.to_host(out["status"]), want_status), tag
        want_counts = code.counts_host(want_msg, want_status, ref)
        assert (_hip.to_host(counts) - [5, 4, 3, 2, 1]).tolist() == want_counts, tag
        if nframes == 67:
            assert want_counts[2] > 0 and want_counts[3] > 0 and 0 < want_counts[4] <= nframes
            # no reference, no status: the message alone
            plain = dev.rs_decode(code, _hip.to_device(rx), bits=bits, want_status=False)
            assert plain["status"] is None and plain["counts"] is None and np.array_equal(_hip.to_host(plain["msg"]), got)
    _hip.device_check()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CODES))
@pytest.mark.parametrize("depth", [1, 5])
def test_gpu_encoder_is_the_host_encoder(name, depth):
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    code = make_code(name, depth)
    rng = np.random.default_rng(depth)
    for nframes, bits in itertools.product((1, 67, 3000), (False, True)):
        m = rng.integers(0, 256, (nframes, code.k * depth), dtype=np.uint8)
        want = code.encode_host(m)
        got = _hip.to_host(dev.rs_encode(code, _hip.to_device(rs.to_bits(m) if bits else m), bits=bits))
        assert np.array_equal(got, rs.to_bits(want) if bits else want), (name, depth, nframes, bits)
    _hip.device_check()


@pytest.mark.gpu
def test_gpu_unaligned_bit_buffers_and_the_host_wrappers():
    """A bit-form buffer that is not 8-byte aligned takes the byte path; RSCode.encode / decode wrap the device calls."""
    from waveforms_amd import _hip
    from waveforms_amd import device as dev

    code, frames, want_msg, want_status, ref = _mixed_frames("short40", 2, 9, 5)
    bits = rs.to_bits(frames)
    buf = _hip.zeros(bits.size + 3, "uint8")
    view = buf[3:]
    view.copy_(_hip.to_device(bits.reshape(-1)))
    out = dev.rs_decode(code, view, bits=True)
    assert np.array_equal(_hip.to_host(out["msg"]), rs.to_bits(want_msg)) and np.array_equal(_hip.to_host(out["status"]), want_status)
    got = code.decode(frames, ref=ref)
    assert np.array_equal(got["msg"], want_msg) and np.array_equal(got["status"], want_status)
    assert got["counts"].tolist() == code.counts_host(want_msg, want_status, ref)
    m = code._join(pool("short40")["ref"][:8])
    assert np.array_equal(code.encode(m), code.encode_host(m)) and np.array_equal(code.encode(rs.to_bits(m), bits=True), rs.to_bits(code.encode_host(m)))
    conv = rs.RSCode.conventional(255, 223, depth=2)
    m = np.random.default_rng(2).integers(0, 256, (3, conv.k * 2), dtype=np.uint8)
    tx = conv.encode(m)
    assert np.array_equal(tx, conv.encode_host(m))
    tx[:, 7] ^= 0x33
    got = conv.decode(tx, ref=m)
    assert np.array_equal(got["msg"], m) and got["status"].tolist() == [0, 1, 0, 1, 0, 1] and got["counts"].tolist() == [0, 0, 0, 3, 0]
    _hip.device_check()
