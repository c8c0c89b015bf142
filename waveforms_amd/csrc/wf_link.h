// wf_link.h — the host steps wf_link_run (wf_pipeline.hip), wf_cpm_link_run (wf_cpm_detect.hip) and their stream forms share.
// Host code only: plain inline functions, no kernels.  `fn` is the calling entry point's name, as its messages print it.
#pragma once
#include "wf_common.h"

static inline int64_t round_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

// ---- fuse bit 5: the detector and the error count of a block run on a side stream of the context, beside the front end of the
// NEXT run on the same context; the workspace then holds two sets of intermediates of `set_bytes` each, used alternately.
// Step 1: both sets fit, and the events and the side stream(s) exist (`second`: the CPM links' second side stream; `side` false:
// a block whose back end runs on its own chain stream and needs no side stream — wf_link_run).
static inline int link_pipe_open(wf_ctx *ctx, const char *fn, int64_t set_bytes, int64_t workspace_bytes, bool second, bool side = true)
{
    WF_REQUIRE(2 * set_bytes <= workspace_bytes, "%s: fuse bit 5 needs two sets of intermediates (%lld bytes)", fn, (long long)(2 * set_bytes));
    WF_HIP(hipSetDevice(ctx->device));
    hipStream_t ps;
    if (!ctx->pipe_front) WF_HIP(hipEventCreateWithFlags(&ctx->pipe_front, hipEventDisableTiming));
    for (int k = 0; k < 2; ++k)
        if (!ctx->pipe_done[k]) WF_HIP(hipEventCreateWithFlags(&ctx->pipe_done[k], hipEventDisableTiming));
    if (side && !ctx->pipe_stream) {
        WF_HIP(hipStreamCreateWithFlags(&ps, hipStreamNonBlocking));
        ctx->pipe_stream = ps;
    }
    if (second && !ctx->pipe_stream2) {
        WF_HIP(hipStreamCreateWithFlags(&ps, hipStreamNonBlocking));
        ctx->pipe_stream2 = ps;
    }
    return WF_OK;
}

// Step 2: this block's set; `waiter`, the stream the block starts on, waits for the back end of the block that used it two blocks ago.
// `kind`: where this block's front end goes — 0: the caller's stream, with the one set of carries, which is slot 0's words; 1: the
// context's pipe_main, 2: the chain stream of its set (wf_link_run with the prologue ahead; carries in scratch slot pipe_set).  One
// context may serve all kinds in turn (links of different forms share the per-device context), and their streams do not order
// themselves: where the kind changes, `waiter` also waits for the previous block's front end (pipe_front).
// `carries` (kinds 1 and 2): a word that differs where the carries' size does.  Slot 1 lies behind slot 0 AS THIS BLOCK SIZES IT, so
// the slots of two links of different burst lengths overlap: there too `waiter`, which carries the prologue, waits for the previous
// front end — it may still be reading what this block's carry kernels write.
static inline int link_pipe_select(wf_ctx *ctx, int64_t set_bytes, char *&w, void *waiter, int kind = 0, uint64_t carries = 0)
{
    if ((ctx->pipe_front_kind != kind || ctx->pipe_carries != carries) && ctx->pipe_front_recorded)
        WF_HIP(hipStreamWaitEvent(wf_stream(waiter), ctx->pipe_front, 0));
    ctx->pipe_front_kind = kind;
    ctx->pipe_carries = carries;
    ctx->pipe_front_recorded = true;      // (every pipelined block records it behind its front end, further down the same call)
    w += (int64_t)ctx->pipe_set * set_bytes;
    if (ctx->pipe_done_valid[ctx->pipe_set]) WF_HIP(hipStreamWaitEvent(wf_stream(waiter), ctx->pipe_done[ctx->pipe_set], 0));
    return WF_OK;
}

// Step 2b, in front of the back end on `back`: every back end works in the context's ONE set of detector scratch (proof records and
// repair lists: the fix-up of a block reads what its detector wrote).  Back ends on one side stream follow each other; where the
// previous block's ran on another stream and either of the two is a chain stream, `back` waits for that back end (pipe_done of the
// other set).  In steady state the wait is long satisfied: a back end is a quarter of a front end.
static inline int link_pipe_back_order(wf_ctx *ctx, void *back)
{
    const void *last = ctx->pipe_back_last;
    const bool chains = back == ctx->pipe_chain[0] || back == ctx->pipe_chain[1] || last == ctx->pipe_chain[0] || last == ctx->pipe_chain[1];
    if (last && last != back && chains && ctx->pipe_done_valid[ctx->pipe_set ^ 1])
        WF_HIP(hipStreamWaitEvent(wf_stream(back), ctx->pipe_done[ctx->pipe_set ^ 1], 0));
    return WF_OK;
}

// Step 3: the back end is queued on `back`; the set is busy until it is through, and the next block takes the other set.
static inline int link_pipe_close(wf_ctx *ctx, void *back)
{
    WF_HIP(hipEventRecord(ctx->pipe_done[ctx->pipe_set], wf_stream(back)));
    ctx->pipe_done_valid[ctx->pipe_set] = true;
    ctx->pipe_back_last = back;
    ctx->pipe_set ^= 1;
    return WF_OK;
}

// ---- stage events: ev = the WF_LINK_STAGES + 1 events of `event_slot` (created with the context's first timed run); NULL for slot -1
static inline int link_stage_events(wf_ctx *ctx, const char *fn, int event_slot, hipEvent_t *&ev)
{
    ev = nullptr;
    if (event_slot < 0) return WF_OK;
    WF_REQUIRE(event_slot < WF_LINK_EVENT_SLOTS, "%s: event_slot %d", fn, event_slot);
    if (!ctx->events) {
        ctx->events = new hipEvent_t[WF_LINK_EVENT_SLOTS * (WF_LINK_STAGES + 1)];
        for (int k = 0; k < WF_LINK_EVENT_SLOTS * (WF_LINK_STAGES + 1); ++k) WF_HIP(hipEventCreate(&ctx->events[k]));
    }
    ev = ctx->events + event_slot * (WF_LINK_STAGES + 1);
    return WF_OK;
}

// stage k of a timed run ends, and stage k + 1 begins, here on `stream`
static inline int mark(hipEvent_t *ev, int k, void *stream)
{
    if (ev) WF_HIP(hipEventRecord(ev[k], wf_stream(stream)));
    return WF_OK;
}

// ---- the window of chunk c of a stream: B detector calls out of `ncalls_total`, over N symbols whose modulator runs in
// `ntiles_total` tiles of `spt` symbols.  The chunk detects calls [k_lo, k_lo + ncols), regenerates symbols [ws, ws + nloc)
// (`halo` either side) and modulates tiles [tile_lo, tile_hi) — the tile before the chunk too: its last column is the chunk's
// first; q_out_tile: which of them starts the NEXT chunk's window (where the phase carry is taken), -1: none.
struct link_chunk_window {
    int64_t k_lo, ncols, ws, nloc, tile_lo, tile_hi, ntiles, q_out_tile;
};

static inline link_chunk_window link_chunk_window_of(int64_t B, int64_t c, int64_t halo, int64_t N, int64_t ncalls_total, int64_t spt, int64_t ntiles_total)
{
    link_chunk_window W;
    W.k_lo = c * B;
    const int64_t k_hi = W.k_lo + B < ncalls_total ? W.k_lo + B : ncalls_total;
    W.ncols = k_hi > W.k_lo ? k_hi - W.k_lo : 0;
    W.ws = c * B - halo > 0 ? c * B - halo : 0;
    const int64_t we = (c + 1) * B + halo < N ? (c + 1) * B + halo : N;
    W.nloc = we > W.ws ? we - W.ws : 0;
    W.tile_lo = spt > 0 && c * B / spt - 1 > 0 ? c * B / spt - 1 : 0;
    W.tile_hi = spt > 0 ? (c + 1) * B / spt + 1 : 0;
    if (W.tile_hi > ntiles_total) W.tile_hi = ntiles_total;
    W.ntiles = W.tile_hi > W.tile_lo ? W.tile_hi - W.tile_lo : 0;
    const int64_t next_tile_lo = spt > 0 ? (c + 1) * B / spt - 1 : 0;
    W.q_out_tile = (next_tile_lo >= W.tile_lo && next_tile_lo < W.tile_hi) ? next_tile_lo - W.tile_lo : -1;
    return W;
}

// ---- SOQPSKTrellis4x2 / 4x2DiffEncoded as dense [column][state][input] tables (reference waveforms/cpm/trellis/model.py:205-258)
struct soqpsk_trellis_tables {
    uint8_t next[2][4][2];
    int8_t outp[2][4][2];
};

static inline soqpsk_trellis_tables soqpsk_trellis(int differential)
{
    static const int8_t kOut[2][8] = {{0, 2, 0, -2, -2, 0, 2, 0}, {0, -2, 2, 0, 0, 2, -2, 0}};
    soqpsk_trellis_tables T;
    for (int c = 0; c < 2; ++c)
        for (int b = 0; b < 8; ++b) {
            const int s = b >> 1, flip = differential ? (c == 0 ? (s >> 1) : (s & 1)) : 0, inp = (b & 1) ^ flip;
            T.next[c][s][inp] = (uint8_t)(c == 0 ? (s & 1) + 2 * (b & 1) : (s & 2) + (b & 1));
            T.outp[c][s][inp] = kOut[c][b];
        }
    return T;
}
