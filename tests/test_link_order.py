"""The pipelined SOQPSK link's launch order and the detector's interior-wave path.

wf_link_run with the prologue ahead (WF_OPT_PIPE_RESERVE_CUS other than 0) starts a block's front end behind an event the
back stream records just in front of the previous block's detector launch; viterbi_batch_kernel decodes every wave whose rows
all lie inside the burst with per-wave bookkeeping (vit_step_interior).  Neither may move a decision: the pipelined link gives
the sequential link's counts block for block under the library's default option and under the ordered form, and the detector
gives the sequential oracle's decisions where interior and edge waves sit next to each other.
"""
import ctypes

import numpy as np
import pytest

SPS = 8


# ------------------------------------------------------------------ the default (CPU)
def _stub_link(ctx_buffer, mf_ntaps):
    """A SOQPSKLink with no device behind it: the configuration words and a context handle only."""
    from waveforms_amd import _hip
    from waveforms_amd.link import SOQPSKLink

    link = SOQPSKLink.__new__(SOQPSKLink)
    cfg = _hip.LinkConfig()
    cfg.nsym, cfg.sps, cfg.ntaps, cfg.mf_ntaps, cfg.mf_nfilt, cfg.timing_offset, cfg.fuse = 300_001, SPS, 8 * SPS + 1, mf_ntaps, 3, -1, 47
    link.cfg, link._ctx = cfg, ctypes.cast(ctx_buffer, ctypes.c_void_p)
    assert link.layout()["one_kernel_front_end"] == 1
    return link


def test_default_order_option_and_prologue_ahead_agree():
    """The order of the pipelined link's kernels: _hip's table of the library's defaults says -1 (what wf_ctx_create sets: the GPU test below),
    and SOQPSKLink.prologue_ahead follows wf_link_run's rule for every value — read through wf_ctx_get_option on a zeroed
    context buffer, as tests/test_cascade.py does: -1 the short bank only, N >= 1 every form, 0 none."""
    from waveforms_amd import _hip

    lib = _hip.lib()
    key = _hip.WF_OPT_PIPE_RESERVE_CUS
    assert _hip.LIBRARY_DEFAULT_OPTIONS == {key: -1}
    fake = ctypes.create_string_buffer(1 << 16)                   # (only its option fields are touched on these paths)
    short, long_ = _stub_link(fake, SPS + 1), _stub_link(fake, 9 * SPS + 1)      # the pulse-truncation bank, the 73-tap PAM bank
    v = ctypes.c_int64(5)
    for value, want in ((_hip.LIBRARY_DEFAULT_OPTIONS[key], (True, False)), (0, (False, False)), (8, (True, True)), (-1, (True, False))):
        assert lib.wf_ctx_set_option(fake, key, value) == 0
        assert lib.wf_ctx_get_option(fake, key, ctypes.byref(v)) == 0 and v.value == value
        assert (short.prologue_ahead, long_.prologue_ahead) == want, value
    assert lib.wf_ctx_set_option(fake, key, -2) == _hip.WF_ERR_VALUE          # the range check stays as it is: -1 .. 128
    assert lib.wf_ctx_set_option(fake, key, 129) == _hip.WF_ERR_VALUE
    short.cfg = long_.cfg = None                                  # (nothing for __del__ to join or free)


@pytest.mark.gpu
def test_a_context_starts_with_the_table_of_defaults():
    """wf_ctx_create itself, without the Python layer's table on top."""
    import torch

    from waveforms_amd import _hip

    out = ctypes.c_void_p()
    _hip.check(_hip.lib().wf_ctx_create(torch.cuda.current_device(), ctypes.byref(out)))
    try:
        for key in range(10):
            assert _hip.get_option(out.value, key) == _hip.LIBRARY_DEFAULT_OPTIONS.get(key, 0), key
    finally:
        _hip.free_ctx(out.value)


# ------------------------------------------------------------------ launch order
def _seven_blocks(link):
    """7 blocks with a reset in the middle and alternating Eb/N0: both sets of intermediates, both carry slots and the
    first block of a context all occur.  Counts after every block."""
    got = []
    for k in range(7):
        if k == 3:
            link.reset_counts()
        link.run_block((4.0, 6.0, 10.0)[k % 3], seed=3, stream_id=k, skip_bits=17 * k)
        got.append(link.result())
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("reserve", [-1, 0])
@pytest.mark.parametrize("nsym", [4_000, 65_600, 300_001])       # 125 chunks of 32 calls: under two waves; one modulator tile over 64; several workgroups
def test_pipelined_link_in_the_default_and_the_other_order_equals_the_sequential_link(nsym, reserve):
    """SOQPSKLink(fuse=47) on a private context gives the counts of fuse=15, block for block, from the NULL stream and from a
    stream of the caller's — with the option as the library sets it (-1: the prologue ahead, every front end launched behind
    the previous block's pipe_back_go) and in the other order (0, set on the link's own context)."""
    import torch

    from waveforms_amd import _hip
    from waveforms_amd.link import SOQPSKLink

    key = _hip.WF_OPT_PIPE_RESERVE_CUS
    for own in (False, True):
        with torch.cuda.stream(torch.cuda.Stream() if own else torch.cuda.current_stream()):
            seq = SOQPSKLink(nsym, SPS, fuse=15, private_ctx=True)
            pip = SOQPSKLink(nsym, SPS, fuse=47, private_ctx=True)
            assert _hip.get_option(pip._ctx, key) == _hip.LIBRARY_DEFAULT_OPTIONS[key] == -1      # (no option scope is open: the library's own)
            _hip.set_option(pip._ctx, key, reserve)
            assert pip.prologue_ahead == (reserve == -1) and not seq.prologue_ahead
            want, got = _seven_blocks(seq), _seven_blocks(pip)
            assert got == want, (nsym, own)
            assert want[-1][1] > 0
            torch.cuda.synchronize()
            del seq, pip


@pytest.mark.gpu
def test_links_of_both_orders_take_turns_on_one_context():
    """A PT link (prologue ahead under -1: front end on the context's own stream, carries in slot 0 / 1) and a PAM link (the other
    order: front end on the caller's stream, the one set of carries = slot 0's words), both pipelined, on the SHARED per-device
    context, block by block in turn: each gives the counts of its sequential link.  The two front ends run on streams that do
    not order themselves — from a caller's own (non-blocking) stream nothing but wf_link_run's own wait keeps the PAM block's
    carry kernels from overwriting what the PT front end still reads, and the other way round."""
    import torch

    from waveforms_amd import _hip
    from waveforms_amd.link import SOQPSKLink

    nsym, key = 300_001, _hip.WF_OPT_PIPE_RESERVE_CUS
    for own in (True, False):
        with torch.cuda.stream(torch.cuda.Stream() if own else torch.cuda.current_stream()):
            assert _hip.get_option(_hip.ctx(), key) == -1
            links = {(det, fuse): SOQPSKLink(nsym, SPS, detector=det, fuse=fuse, private_ctx=fuse == 15) for det in ("PT", "PAM") for fuse in (15, 47)}
            assert links["PT", 47]._ctx == links["PAM", 47]._ctx == _hip.ctx()
            assert links["PT", 47].prologue_ahead and not links["PAM", 47].prologue_ahead
            got = {k: [] for k in links}
            for fuse in (15, 47):
                for blk in range(12):
                    for det in (("PT", "PAM") if blk % 4 else ("PAM", "PT")):          # PT PAM PT PAM ..., and PT PT / PAM PAM where the turn flips
                        links[det, fuse].run_block((4.0, 6.0, 10.0)[blk % 3], seed=9, stream_id=blk, skip_bits=31 * blk)
                    if blk % 3 == 2:
                        for det in ("PT", "PAM"):
                            got[det, fuse].append(links[det, fuse].result())
            for det in ("PT", "PAM"):
                assert got[det, 47] == got[det, 15], (det, own)
                assert got[det, 15][-1][1] > 0
            torch.cuda.synchronize()
            del links


@pytest.mark.gpu
def test_the_library_keeps_the_other_order_for_the_long_bank():
    """wf_link_run's own choice under -1, observed through the stage events of one block alone on the chip (SOQPSKLink.prologue_ahead
    is Python's copy of the rule): with the prologue ahead the front-end kernel lies between events 3 and 4 ("phase"), in the
    other order between 2 and 3 ("fir") with nothing between 3 and 4.  The front end of 2e6 symbols takes at least 0.07 ms
    (0.36 ms per 1e7 symbols when alone); two events recorded back to back lie well under 0.01 ms apart."""
    import torch

    from waveforms_amd.link import SOQPSKLink, _Link

    for det, ahead in (("PT", True), ("PAM", False)):
        link = SOQPSKLink(2_000_000, SPS, detector=det, fuse=47, private_ctx=True)
        assert link.prologue_ahead == ahead
        for k in range(3):
            torch.cuda.synchronize()
            link.run_block(10.0, seed=1, stream_id=k, event_slot=0 if k == 2 else -1)
        link.result()
        raw = _Link.stage_ms(link, 0)
        kernel, other = (raw["phase"], raw["fir"]) if ahead else (raw["fir"], raw["phase"])
        assert kernel > 0.05, (det, raw)
        if not ahead:
            assert other < 0.01, (det, raw)
        assert link.stage_ms(0)["fir"] == kernel and link.stage_ms(0)["phase"] == (0.0 if ahead else other)
        del link


# ------------------------------------------------------------------ detector paths
# One wave of 32-call chunks exactly, one call short, one over, one chunk over less a call; three waves and three waves + 5 (the
# middle wave interior, the last one interior when the burst ends with it: the carry is then written by an interior lane); and
# 64 * 160 * 3 + 5 calls (at this size the launch cuts 32-call chunks as well — 160-call chunks need 9.4e6 calls —: 13 interior
# waves between the first and the last two).  The interior path at the benchmark's own chunk length, 160 calls, is run by the
# 1e7-symbol tests of tests/test_gpu_parity.py only (test_link_full_size_equals_oracle_chain_1e7; test_detector_long_burst_ch256
# for 256-call chunks), at the default warm-up, where no repair is forced.
NCALLS = [2047, 2048, 2049, 2048 + 31, 3 * 2048, 3 * 2048 + 5, 64 * 160 * 3 + 5]
HEAD = 77                                                         # an odd piece first: the second piece starts on an odd call index


@pytest.fixture(scope="module")
def burst(oracle):
    """Rows of one noisy burst at 2 dB (a 2-row warm-up misses nearly every chunk there) and the sequential detector's
    decisions over every prefix (the detector is causal: a prefix of the decisions)."""
    n = HEAD + max(NCALLS) + 8
    bits, _ = oracle.glfsr_bits(0x420000, 0x7FFFFF, n)
    noise = oracle.philox_awgn(oracle.sigma_for_ebn0(2.0, SPS), 7, 3, 0, (n + 1) * SPS)
    res = oracle.detection_run(bits, oracle.freq_pulse_soqpsk_tg(SPS), 0.25, SPS, None, noise=noise)
    rows = np.ascontiguousarray(res["mf_rows"])
    seq = {True: (res["det_bits"], res["det_syms"]), False: oracle.viterbi_detect(rows, 2, False)}
    return rows, seq


@pytest.mark.gpu
@pytest.mark.parametrize("differential", [True, False])
@pytest.mark.parametrize("warmup", [2, 0])
def test_detector_interior_and_edge_waves_equal_the_sequential_detector(burst, ctx_options, warmup, differential):
    """wf_viterbi4_detect over a fresh burst (step 0 on an even call) and over the same rows behind a carried state of 77
    calls (step 0 on an odd call: the other instantiation of the body)."""
    from waveforms.viterbi.algorithm import SOQPSKTrellisDetector
    from waveforms_amd import _hip, device as dev

    rows, seq = burst
    want_b, want_s = seq[differential]
    d_rows = _hip.to_device(rows)
    with ctx_options(WF_OPT_DET_FINAL_VERIFY=1):
        for n in NCALLS:
            dev.viterbi_repaired(reset=True)
            b, s = dev.viterbi_detect(d_rows[:n], differential, warmup)
            assert dev.viterbi_unmerged(reset=True) == 0
            if warmup == 2:
                assert dev.viterbi_repaired(reset=True) > 0, n
            assert np.array_equal(_hip.to_host(b), want_b[:n]) and np.array_equal(_hip.to_host(s), want_s[:n]), n
            det = SOQPSKTrellisDetector(2, differantial_encoding=differential)
            parts = [det.detect(rows[:HEAD], warmup=warmup), det.detect(rows[HEAD:HEAD + n], warmup=warmup)]
            if warmup == 2:
                assert dev.viterbi_repaired(reset=True, ctx=det._ctx) > 0, n
            assert np.array_equal(np.concatenate([p[0] for p in parts]), want_b[:HEAD + n]), n
            assert np.array_equal(np.concatenate([p[1] for p in parts]), want_s[:HEAD + n]), n


@pytest.mark.gpu
@pytest.mark.parametrize("differential", [True, False])
@pytest.mark.parametrize("warmup", [2, 0])
def test_detector_on_link_rows_equals_the_sequential_detector(oracle, warmup, differential):
    """wf_viterbi4_detect_packed (the link's detector-packed rows) for the same call counts: the decisions in the link's
    workspace against the sequential oracle chain fed the same bits and the same Philox noise."""
    from waveforms_amd import device as dev
    from waveforms_amd.link import SOQPSKLink

    trellis = "SOQPSKTrellis4x2DiffEncoded" if differential else "SOQPSKTrellis4x2"
    for n in NCALLS:
        nsym = n + 1                                              # (sps 8, timing offset -1: one call fewer than symbols)
        link = SOQPSKLink(nsym, SPS, fuse=15, differential=differential, warmup=warmup, private_ctx=True)
        lay = link.layout()
        assert lay["calls"] == n and lay["row_bytes"] == 32
        link.run_block(2.0, seed=7, stream_id=3)
        se, be, m = link.result()
        if warmup == 2:
            assert dev.viterbi_repaired(reset=True, ctx=link._ctx) > 0, n
        bits, _ = oracle.glfsr_bits(0x420000, 0x7FFFFF, nsym)
        noise = oracle.philox_awgn(oracle.sigma_for_ebn0(2.0, SPS), 7, 3, 0, (nsym + 1) * SPS)
        res = oracle.detection_run(bits, oracle.freq_pulse_soqpsk_tg(SPS), 0.25, SPS, None, noise=noise, trellis=trellis)
        want_b, want_s = (res["det_bits"], res["det_syms"]) if differential else oracle.viterbi_detect(res["mf_rows"], 2, False)
        got_b = link.workspace[lay["off_bits"]:lay["off_bits"] + n].cpu().numpy()
        got_s = link.workspace[lay["off_syms"]:lay["off_syms"] + n].cpu().numpy().view(np.int8)
        assert np.array_equal(got_b, want_b) and np.array_equal(got_s, want_s), n
        if differential:
            assert (se, be, m) == (res["sym_errors"], res["bit_errors"], res["compared"]), n
        del link
