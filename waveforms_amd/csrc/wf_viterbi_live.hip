// wf_viterbi_live.hip — the a-priori SOQPSK detector over the LIVE WINDOWS of an iterative detection and decoding loop
// (include/wfhip.h: wf_idd_windows, wf_viterbi4_soft_apriori_windows).  Once most codewords of a burst are frozen a detector
// pass is only needed on the rows of the codewords still open (plus a guard on either side); which those are is known on the
// device only, so everything here is sized on the host for the worst case and decides on the device what it does.
//
//   live_windows_kernel   one workgroup: the decoder's state bytes -> the table of row windows (s, e), merged by the guard rule
//   live_plan_kernel      one workgroup: checks a table and cuts every window into chunks of `ch` rows from its own start;
//                         cum[w] = chunks in front of window w, T = all of them.  A chunk is therefore (window, index in it),
//                         found from its number by a binary search over cum: the live chunks are COMPACT, lane c of the
//                         launches below walks live chunk c, waves stay dense and the lane-interleaved ã scratch coalesced
//                         however the open codewords lie in the burst.  Grids are sized for tmax = every row live plus one
//                         partial chunk per window; lanes c >= T leave after one load.
//   live_bounds_kernel    soft_ap_bounds_kernel per live chunk; the warm-up never crosses its window's edges
//   live_fixup_kernel     the proof and cascading repair of the burst detector, with one change: a window's first chunk
//                         (backward: its last) starts from zero metrics at the window's edge, which is exact by definition
//                         as record 0 of a burst is, so it is neither compared with a predecessor nor handed a repair
//   live_llr_kernel       soft_ap_llr_kernel per live chunk
//
// Rows, priors and outputs are addressed by their index in the BURST: a window starts on an even row, so row k is trellis
// column k % 2 in the burst and in the window alike, and a window's rows go through exactly the operations the burst
// detector applies to the slice (wf_viterbi_soft.h has them: the walks over a soft_chunk whose limits are its window's).  The result is the definition for any chunk length
// and warm-up, as the burst detector's is, because every chunk start that is not exact is proven or repaired.
#include "wf_viterbi_soft.h"

// ---- the window table ---------------------------------------------------------------------------------------------------
struct live_span {
    int64_t s, e;
};

// rows of codeword b widened by the guard; e <= s: no row of the burst
__device__ __forceinline__ live_span live_cw_span(int64_t b, int64_t first, int64_t P, int64_t n_tx, int64_t G, int64_t nrows)
{
    const int64_t a = first + b * P;
    live_span w;
    w.s = (a - G > 0 ? a - G : 0) & ~(int64_t)1;
    w.e = a + n_tx + G < nrows ? a + n_tx + G : nrows;
    return w;
}

#define LIVE_WIN_THREADS 256

// Thread t owns the codewords [t seg, (t + 1) seg).  e_b never decreases with b, so a merged window ends where its last
// member does and "does b start a window" depends only on the open codeword in front of it: three walks over the own
// segment (last open one, windows started, the entries) around two scans over the threads.
__global__ __launch_bounds__(LIVE_WIN_THREADS) void live_windows_kernel(const uint8_t *__restrict__ state, int64_t ncw, int64_t nrows, int64_t n_tx,
                                                                        int64_t P, int64_t row_offset, const int64_t *__restrict__ lock, int64_t L, int64_t G,
                                                                        int64_t *__restrict__ table)
{
    __shared__ long long s_scan[LIVE_WIN_THREADS];
    __shared__ long long s_live, s_open;
    const int t = threadIdx.x;
    const int64_t first = row_offset + (lock ? lock[0] : 0) + L;
    const int64_t seg = (ncw + LIVE_WIN_THREADS - 1) / LIVE_WIN_THREADS;
    const int64_t b0 = t * seg < ncw ? t * seg : ncw, b1 = b0 + seg < ncw ? b0 + seg : ncw;
    if (t == 0) s_live = 0, s_open = 0;

    long long last = -1, opens = 0;
    for (int64_t b = b0; b < b1; ++b) {
        if (state[b] != 0) continue;
        ++opens;
        const live_span w = live_cw_span(b, first, P, n_tx, G, nrows);
        if (w.e > w.s) last = b;
    }
    s_scan[t] = last;
    __syncthreads();
    for (int d = 1; d < LIVE_WIN_THREADS; d <<= 1) {           // inclusive scan, maximum
        const long long v = t >= d ? s_scan[t - d] : -1;
        __syncthreads();
        if (v > s_scan[t]) s_scan[t] = v;
        __syncthreads();
    }
    const long long prev_in = t ? s_scan[t - 1] : -1, glast = s_scan[LIVE_WIN_THREADS - 1];
    __syncthreads();

    long long p = prev_in, starts = 0;
    for (int64_t b = b0; b < b1; ++b) {
        if (state[b] != 0) continue;
        const live_span w = live_cw_span(b, first, P, n_tx, G, nrows);
        if (w.e <= w.s) continue;
        if (p < 0 || w.s - live_cw_span(p, first, P, n_tx, G, nrows).e >= G) ++starts;
        p = b;
    }
    s_scan[t] = starts;
    __syncthreads();
    for (int d = 1; d < LIVE_WIN_THREADS; d <<= 1) {           // inclusive scan, sum
        const long long v = t >= d ? s_scan[t - d] : 0;
        __syncthreads();
        s_scan[t] += v;
        __syncthreads();
    }
    long long wi = s_scan[t] - starts;                         // windows started in front of this segment
    const long long W = s_scan[LIVE_WIN_THREADS - 1];

    long long live = 0;
    p = prev_in;
    for (int64_t b = b0; b < b1; ++b) {
        if (state[b] != 0) continue;
        const live_span w = live_cw_span(b, first, P, n_tx, G, nrows);
        if (w.e <= w.s) continue;
        const int64_t pe = p < 0 ? 0 : live_cw_span(p, first, P, n_tx, G, nrows).e;
        if (p < 0 || w.s - pe >= G) {
            if (p >= 0) {                                      // ... and the window in front of it ends with p
                table[4 + 2 * (wi - 1) + 1] = pe;
                live += pe;
            }
            table[4 + 2 * wi] = w.s;
            live -= w.s;
            ++wi;
        }
        p = b;
    }
    if (t == 0 && glast >= 0) {
        const int64_t e = live_cw_span(glast, first, P, n_tx, G, nrows).e;
        table[4 + 2 * (W - 1) + 1] = e;
        live += e;
    }
    if (live) atomicAdd(reinterpret_cast<unsigned long long *>(&s_live), (unsigned long long)live);
    if (opens) atomicAdd(reinterpret_cast<unsigned long long *>(&s_open), (unsigned long long)opens);
    __syncthreads();
    if (t == 0) {
        table[0] = W;
        table[1] = s_live;
        table[2] = s_open;
        table[3] = 0;
    }
}

extern "C" int wf_idd_windows(wf_ctx *ctx, const uint8_t *d_state, int64_t ncw, int64_t nrows, int32_t n_tx, int64_t P, int64_t row_offset,
                              const void *d_lock, int32_t L, int64_t G, int64_t *d_table, void *stream)
{
    constexpr int64_t kMax = (int64_t)1 << 40;                 // (every product and sum below stays far inside int64)
    WF_REQUIRE(ctx && d_state && d_table, "wf_idd_windows: NULL argument");
    WF_REQUIRE(ncw >= 1 && ncw <= ((int64_t)1 << 31), "wf_idd_windows: ncw = %lld outside 1 .. 2^31", (long long)ncw);
    WF_REQUIRE(nrows >= 1 && nrows <= kMax, "wf_idd_windows: nrows = %lld outside 1 .. 2^40", (long long)nrows);
    WF_REQUIRE(n_tx >= 1 && P >= n_tx && P <= ((int64_t)1 << 31), "wf_idd_windows: n_tx must be at least 1 and the period n_tx .. 2^31");
    WF_REQUIRE(row_offset >= 0 && row_offset <= kMax, "wf_idd_windows: row_offset = %lld outside 0 .. 2^40", (long long)row_offset);
    WF_REQUIRE(L >= 0 && G >= 0 && G <= kMax, "wf_idd_windows: L and G must not be negative (G at most 2^40)");
    WF_REQUIRE((reinterpret_cast<uintptr_t>(d_table) & 7) == 0 && (reinterpret_cast<uintptr_t>(d_lock) & 7) == 0,
               "wf_idd_windows: the table and the lock record must be 8-byte aligned");
    WF_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(live_windows_kernel, dim3(1), dim3(LIVE_WIN_THREADS), 0, wf_stream(stream), d_state, ncw, nrows, (int64_t)n_tx, P, row_offset,
                       static_cast<const int64_t *>(d_lock), (int64_t)L, G, d_table);
    WF_LAUNCH_CHECK();
    return WF_OK;
}

// ---- the plan: windows -> compact chunks ----------------------------------------------------------------------------------
// plan (int64, in the context's scratch): [0] T live chunks, [1] W windows, [2], [3] spare, then cum[0 .. W]
#define LIVE_PLAN_HDR 4

// Also empties both repair lists and their arrival tickets (the launches behind it on the stream read them).  A table that
// is not W <= max_windows increasing, disjoint windows with even starts inside the burst raises the context's fault word
// and plans nothing: no row is touched.
__global__ __launch_bounds__(LIVE_WIN_THREADS) void live_plan_kernel(const int64_t *__restrict__ table, int64_t max_windows, int64_t n, int ch, int64_t tmax,
                                                                     int64_t *__restrict__ plan, unsigned long long *__restrict__ fhdr,
                                                                     unsigned long long *__restrict__ bhdr, unsigned *__restrict__ fault)
{
    __shared__ long long s_scan[LIVE_WIN_THREADS];
    __shared__ long long s_carry;
    __shared__ int s_bad;
    const int t = threadIdx.x;
    if (t < VIT_HDR) fhdr[t] = 0, bhdr[t] = 0;
    if (t == 0) s_carry = 0, s_bad = 0;
    __syncthreads();
    const int64_t W = table[0];
    const bool w_ok = W >= 0 && W <= max_windows;
    int64_t *cum = plan + LIVE_PLAN_HDR;
    for (int64_t w0 = 0; w_ok && w0 < W; w0 += LIVE_WIN_THREADS) {
        const int64_t w = w0 + t;
        long long nch = 0;
        if (w < W) {
            const int64_t s = table[4 + 2 * w], e = table[4 + 2 * w + 1], pe = w ? table[4 + 2 * w - 1] : 0;
            if (s < pe || (s & 1) || e <= s || e > n) s_bad = 1;
            else nch = (e - s + ch - 1) / ch;
        }
        s_scan[t] = nch;
        __syncthreads();
        for (int d = 1; d < LIVE_WIN_THREADS; d <<= 1) {
            const long long v = t >= d ? s_scan[t - d] : 0;
            __syncthreads();
            s_scan[t] += v;
            __syncthreads();
        }
        if (w < W) cum[w + 1] = s_carry + s_scan[t];
        __syncthreads();
        if (t == 0) s_carry += s_scan[LIVE_WIN_THREADS - 1];
        __syncthreads();
    }
    if (t == 0) {
        const bool ok = w_ok && !s_bad && s_carry <= tmax;
        if (!ok) atomicOr(fault, (unsigned)WF_FAULT_LIVE_TABLE);
        cum[0] = 0;
        plan[0] = ok ? s_carry : 0;
        plan[1] = ok ? W : 0;
        plan[2] = plan[3] = 0;
    }
}

struct live_chunk {
    soft_chunk k;           // rows, its window's edges as the limits; records and ã lane by its own number, either direction
    bool first, last;       // of its window
};

__device__ __forceinline__ live_chunk live_find(const int64_t *__restrict__ plan, const int64_t *__restrict__ table, int64_t c, int ch, int64_t tmax)
{
    const int64_t *cum = plan + LIVE_PLAN_HDR;
    int64_t lo = 0, hi = plan[1];                              // cum[lo] <= c < cum[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (cum[mid] <= c) lo = mid;
        else hi = mid;
    }
    const int64_t ws = table[4 + 2 * lo], we = table[4 + 2 * lo + 1], a = ws + (c - cum[lo]) * ch;
    return live_chunk{soft_chunk{a, a + ch < we ? a + ch : we, ws, we, c, c, c, tmax}, c == cum[lo], c + 1 == cum[lo + 1]};
}

struct live_args {
    const double *rows;
    soft_prior pr;
    const int64_t *table, *plan;
    int ch, warmup;
    int64_t tmax;           // lanes the ã scratch is interleaved over
    double *fedge, *bedge;  // records {start[4], end[4]} of chunk c at 8 c, either direction
    double *alpha;
};

template <bool PACKED, int DIFF>
__global__ __launch_bounds__(SOFT_THREADS) void live_bounds_kernel(live_args g)
{
    const int64_t c = (int64_t)blockIdx.x * SOFT_THREADS + threadIdx.x;
    if (c >= g.plan[0]) return;
    soft_bounds_body<PACKED, DIFF, true>(g.rows, g.pr, live_find(g.plan, g.table, c, g.ch, g.tmax).k, g.warmup, g.fedge, g.bedge, g.alpha);
}

// ---- proof and repair -------------------------------------------------------------------------------------------------------
// vit_fixup_verify / vit_fixup_rounds (wf_viterbi4.h) with the records of both directions indexed by the chunk and the
// predecessor of chunk c being c - 1 forward, c + 1 backward — except for a window's first (last) chunk, which has none.
// hdr: [0], [1] entries in list 0 / 1, [2] arrival ticket; the lists (tmax entries each) follow.
template <bool BWD>
__device__ __forceinline__ bool live_fixup_verify(const live_args &g, const double *__restrict__ edge, unsigned long long *__restrict__ hdr,
                                                  unsigned long long *__restrict__ unmerged, int mode)
{
    __shared__ int s_last;
    const int64_t T = g.plan[0];
    if (T == 0) return false;                                  // nothing live: nothing to compare, nobody to elect (every workgroup sees the same T)
    unsigned long long *list0 = hdr + VIT_HDR;
    const unsigned long long *rec = reinterpret_cast<const unsigned long long *>(edge);
    int listed = 0;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < T; c += (int64_t)gridDim.x * blockDim.x) {
        const live_chunk k = live_find(g.plan, g.table, c, g.ch, g.tmax);
        if (BWD ? k.last : k.first) continue;                  // starts at its window's edge: exact
        const unsigned long long *st = rec + 8 * c, *en = rec + 8 * (BWD ? c + 1 : c - 1) + 4;
        if (st[0] != en[0] || st[1] != en[1] || st[2] != en[2] || st[3] != en[3]) {
            if (mode) list0[atomicAdd(&hdr[0], 1ull)] = (unsigned long long)c;
            else atomicAdd(unmerged, 1ull);
            listed = 1;
        }
    }
    if (!mode) return false;
    // arrival: as vit_fixup_verify (only a workgroup that listed something has entries to publish)
    if (__syncthreads_or(listed)) __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) s_last = atomicAdd(&hdr[2], 1ull) + 1 == (unsigned long long)gridDim.x;
    __syncthreads();
    if (!s_last) return false;
    if (__hip_atomic_load(&hdr[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return false;
    __threadfence();
    return true;
}

// Chunk c again from its predecessor's end -> the chunk to list next, -1: its own end changed but it closes its window,
// -2: its end did not change.
template <bool PACKED, bool BWD, int DIFF>
__device__ __forceinline__ int64_t live_rerun(const live_args &g, double *__restrict__ edge, int64_t c)
{
    const live_chunk k = live_find(g.plan, g.table, c, g.ch, g.tmax);
    const bool changed = soft_rerun_body<PACKED, BWD, DIFF, true>(g.rows, g.pr, k.k, edge + 8 * c, edge + 8 * (BWD ? c + 1 : c - 1) + 4, g.alpha);
    if (!changed) return -2;
    if (BWD ? k.first : k.last) return -1;
    return BWD ? c - 1 : c + 1;
}

template <bool PACKED, bool BWD, int DIFF>
__global__ __launch_bounds__(256) void live_fixup_kernel(live_args g, unsigned long long *__restrict__ hdr, unsigned long long *__restrict__ unmerged, int mode)
{
    double *edge = BWD ? g.bedge : g.fedge;
    if (!live_fixup_verify<BWD>(g, edge, hdr, unmerged, mode)) return;
    int lin = 0;
    for (;;) {
        const int64_t n = (int64_t)__hip_atomic_load(&hdr[lin], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n == 0) return;
        unsigned long long *in = hdr + VIT_HDR + (int64_t)lin * g.tmax, *out = hdr + VIT_HDR + (int64_t)(lin ^ 1) * g.tmax;
        for (int64_t idx = threadIdx.x; idx < n; idx += blockDim.x) {
            const int64_t c = (int64_t)__hip_atomic_load(&in[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int64_t next = live_rerun<PACKED, BWD, DIFF>(g, edge, c);
            atomicAdd(unmerged + 1, 1ull);                     // [1]: chunk repairs run, [2]: ... whose end changed
            if (next != -2) atomicAdd(unmerged + 2, 1ull);
            if (next >= 0) out[atomicAdd(&hdr[lin ^ 1], 1ull)] = (unsigned long long)next;
        }
        __threadfence();
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_store(&hdr[lin], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        __syncthreads();
        lin ^= 1;
    }
}

template <bool PACKED, int DIFF>
__global__ __launch_bounds__(SOFT_THREADS) void live_llr_kernel(live_args g, double *__restrict__ ext, uint8_t *__restrict__ bits)
{
    const int64_t c = (int64_t)blockIdx.x * SOFT_THREADS + threadIdx.x;
    if (c >= g.plan[0]) return;
    soft_llr_body<PACKED, DIFF, true>(g.rows, g.pr, live_find(g.plan, g.table, c, g.ch, g.tmax).k, g.bedge, g.alpha, ext, bits);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
// Scratch (doubles), every part a multiple of 4 words so that the 32-byte records stay aligned:
//   plan | forward header + lists | backward header + lists | forward records | backward records | ã per row and lane
struct live_geom {
    int64_t tmax;
    size_t off_fhdr, off_bhdr, off_f, off_b, off_alpha, words;
};

static live_geom live_geometry(const soft_geom &g, int64_t max_windows)
{
    const auto up4 = [](size_t v) { return (v + 3) / 4 * 4; };
    live_geom l;
    l.tmax = g.nch + max_windows;                              // sum over windows of ceil(rows / ch) <= rows / ch + windows
    const size_t hdr = up4(VIT_HDR + 2 * (size_t)l.tmax);
    l.off_fhdr = up4(LIVE_PLAN_HDR + (size_t)max_windows + 1);
    l.off_bhdr = l.off_fhdr + hdr;
    l.off_f = l.off_bhdr + hdr;
    l.off_b = l.off_f + 8 * (size_t)l.tmax;
    l.off_alpha = l.off_b + 8 * (size_t)l.tmax;
    l.words = l.off_alpha + 4 * (size_t)g.ch * (size_t)l.tmax;
    return l;
}

template <bool PACKED, int DIFF>
static int live_run(wf_ctx *ctx, const live_args &a, unsigned long long *fhdr, unsigned long long *bhdr, double *ext, uint8_t *bits, hipStream_t s)
{
    const unsigned grid = (unsigned)((a.tmax + SOFT_THREADS - 1) / SOFT_THREADS);
    hipLaunchKernelGGL((live_bounds_kernel<PACKED, DIFF>), dim3(grid), dim3(SOFT_THREADS), 0, s, a);
    WF_LAUNCH_CHECK();
    const unsigned fgrid = (unsigned)wf_grid_for(a.tmax, 256, 1024);
    const int rc = soft_fixup_passes(ctx, [&](auto bwd, int mode) {
        hipLaunchKernelGGL((live_fixup_kernel<PACKED, decltype(bwd)::value, DIFF>), dim3(fgrid), dim3(256), 0, s, a, bwd ? bhdr : fhdr, ctx->d_vit_unmerged, mode);
    });
    if (rc) return rc;
    hipLaunchKernelGGL((live_llr_kernel<PACKED, DIFF>), dim3(grid), dim3(SOFT_THREADS), 0, s, a, ext, bits);
    WF_LAUNCH_CHECK();
    return WF_OK;
}

extern "C" int wf_viterbi4_soft_apriori_windows(wf_ctx *ctx, const double *d_rows, int64_t ncalls, int row_bytes, int differential, int warmup,
                                                const float *d_apriori, double apriori_scale, const int64_t *d_windows, int64_t max_windows,
                                                double *d_ext, uint8_t *d_bits, void *stream)
{
    static const char who[] = "wf_viterbi4_soft_apriori_windows";
    WF_REQUIRE(d_apriori && d_windows, "%s: NULL argument", who);
    int rc = soft_check_args(who, ctx, d_rows, ncalls, row_bytes, warmup, d_apriori, apriori_scale, d_windows, d_ext, d_bits,
                             "rows must be 16-byte, ext and the window table 8-byte and the prior 4-byte aligned");
    if (rc) return rc;
    WF_REQUIRE(max_windows >= 1 && max_windows <= ((int64_t)1 << 31), "%s: max_windows = %lld outside 1 .. 2^31", who, (long long)max_windows);
    const soft_geom g = soft_geometry(ctx, ncalls, warmup);
    const live_geom l = live_geometry(g, max_windows);
    rc = soft_reserve(who, ctx, l.tmax, l.words);
    if (rc) return rc;
    hipStream_t s = wf_stream(stream);
    double *base = ctx->d_vit_edge;
    int64_t *plan = reinterpret_cast<int64_t *>(base);
    unsigned long long *fhdr = reinterpret_cast<unsigned long long *>(base + l.off_fhdr), *bhdr = reinterpret_cast<unsigned long long *>(base + l.off_bhdr);
    hipLaunchKernelGGL(live_plan_kernel, dim3(1), dim3(LIVE_WIN_THREADS), 0, s, d_windows, max_windows, ncalls, g.ch, l.tmax, plan, fhdr, bhdr,
                       ctx->d_fault);
    WF_LAUNCH_CHECK();
    live_args a;
    a.rows = d_rows;
    a.pr = soft_prior_of(d_apriori, apriori_scale, ncalls);
    a.table = d_windows, a.plan = plan;
    a.ch = g.ch, a.warmup = g.warmup, a.tmax = l.tmax;
    a.fedge = base + l.off_f, a.bedge = base + l.off_b, a.alpha = base + l.off_alpha;
    return soft_dispatch(row_bytes, differential, [&](auto packed, auto diff) {
        return live_run<decltype(packed)::value, decltype(diff)::value>(ctx, a, fhdr, bhdr, d_ext, d_bits, s);
    });
}
