// wf_viterbi_segments.hip — the plain max-log-MAP SOQPSK detector over INDEPENDENT SEGMENTS of one buffer, in one set of
// launches (include/wfhip.h: wf_viterbi4_soft_branch_segments).  A coarse carrier search detects the same burst H times, each
// copy rotated by another hypothesis; as H bursts that is 4 H launches of a few thousand lanes each, as H segments of one
// stacked buffer it is 4 launches of H times the lanes.
//
// Segment s is rows s stride .. s stride + seglen - 1.  Every segment is cut into cps = ceil(seglen / ch) chunks from its own
// start, so chunk c of the launch is (segment c / cps, index c % cps): no table, no search, and a chunk never crosses a
// segment.  Lane c walks chunk c with the bodies of wf_viterbi_soft.h as they stand, its soft_chunk limits being its
// segment's: a warm-up never leaves the segment, as wf_viterbi_live.hip's never leaves its window.
//
//   seg_bounds_kernel   soft_bounds_kernel per chunk
//   seg_fixup_kernel    the proof and cascading repair of the burst detector with wf_viterbi_live.hip's one change: a
//                       segment's first chunk (backward: its last) starts from zero metrics at the segment's edge, which is
//                       exact as record 0 of a burst is, so it is neither compared with a predecessor nor handed a repair.
//                       Records of both directions are indexed by the chunk; the predecessor of c is c - 1 forward, c + 1
//                       backward.
//   seg_llr_kernel      soft_llr_kernel / soft_branch_kernel per chunk; a segment's last chunk also writes the pad outputs
//
// Rows and outputs are addressed by their index in the BUFFER; stride is even, so row k is trellis column k % 2 in the buffer
// and in its segment alike.  Every chunk start that is not exact is proven or repaired, so a segment's result is the
// definition (wf_viterbi_soft.hip) for its rows alone, bitwise, whatever the chunk length and the warm-up.
//
// Launch shape: one lane per chunk, SOFT_THREADS lanes per workgroup, as the burst detector (the walks are latency-bound
// chains of fp64 min / add per lane; what hides them is lanes, and stacking H copies multiplies the lanes by H).  Without
// a prior no branch's input bit enters the recursions, so only the last launch carries DIFF.
#include "wf_viterbi_soft.h"

struct seg_args {
    const double *rows;
    int64_t seglen, stride;
    int64_t cps, T;         // chunks per segment, chunks in all (= lanes the ã scratch is interleaved over)
    int ch, warmup;
    double *fedge, *bedge;  // records {start[4], end[4]} of chunk c at 8 c, either direction
    double *alpha;
};

struct seg_chunk {
    soft_chunk k;           // rows, its segment's edges as the limits; records and ã lane by its own number, either direction
    bool first, last;       // of its segment
};

__device__ __forceinline__ seg_chunk seg_find(const seg_args &g, int64_t c)
{
    const int64_t s = c / g.cps, j = c - s * g.cps;
    const int64_t lo = s * g.stride, hi = lo + g.seglen, a = lo + j * g.ch;
    return seg_chunk{soft_chunk{a, a + g.ch < hi ? a + g.ch : hi, lo, hi, c, c, c, g.T}, j == 0, j + 1 == g.cps};
}

template <bool PACKED>
__global__ __launch_bounds__(SOFT_THREADS) void seg_bounds_kernel(seg_args g, unsigned long long *__restrict__ fhdr, unsigned long long *__restrict__ bhdr)
{
    if (blockIdx.x == 0 && threadIdx.x < VIT_HDR) fhdr[threadIdx.x] = 0, bhdr[threadIdx.x] = 0;      // lists empty, nobody arrived: for the two launches behind
    const int64_t c = (int64_t)blockIdx.x * SOFT_THREADS + threadIdx.x;
    if (c >= g.T) return;
    soft_bounds_body<PACKED, 0, false>(g.rows, soft_no_prior{}, seg_find(g, c).k, g.warmup, g.fedge, g.bedge, g.alpha);
}

// ---- proof and repair: wf_viterbi_live.hip's, with seg_find in place of the plan ------------------------------------------
// hdr: [0], [1] entries in list 0 / 1, [2] arrival ticket; the lists (T entries each) follow.
template <bool BWD>
__device__ __forceinline__ bool seg_fixup_verify(const seg_args &g, const double *__restrict__ edge, unsigned long long *__restrict__ hdr,
                                                 unsigned long long *__restrict__ unmerged, int mode)
{
    __shared__ int s_last;
    unsigned long long *list0 = hdr + VIT_HDR;
    const unsigned long long *rec = reinterpret_cast<const unsigned long long *>(edge);
    int listed = 0;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < g.T; c += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = c % g.cps;
        if (BWD ? j + 1 == g.cps : j == 0) continue;           // starts at its segment's edge: exact
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

// Chunk c again from its predecessor's end -> the chunk to list next, -1: its own end changed but it closes its segment,
// -2: its end did not change.
template <bool PACKED, bool BWD>
__device__ __forceinline__ int64_t seg_rerun(const seg_args &g, double *__restrict__ edge, int64_t c)
{
    const seg_chunk k = seg_find(g, c);
    const bool changed = soft_rerun_body<PACKED, BWD, 0, false>(g.rows, soft_no_prior{}, k.k, edge + 8 * c, edge + 8 * (BWD ? c + 1 : c - 1) + 4, g.alpha);
    if (!changed) return -2;
    if (BWD ? k.first : k.last) return -1;
    return BWD ? c - 1 : c + 1;
}

template <bool PACKED, bool BWD>
__global__ __launch_bounds__(256) void seg_fixup_kernel(seg_args g, unsigned long long *__restrict__ hdr, unsigned long long *__restrict__ unmerged, int mode)
{
    double *edge = BWD ? g.bedge : g.fedge;
    if (!seg_fixup_verify<BWD>(g, edge, hdr, unmerged, mode)) return;
    int lin = 0;
    for (;;) {
        const int64_t n = (int64_t)__hip_atomic_load(&hdr[lin], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n == 0) return;
        unsigned long long *in = hdr + VIT_HDR + (int64_t)lin * g.T, *out = hdr + VIT_HDR + (int64_t)(lin ^ 1) * g.T;
        for (int64_t idx = threadIdx.x; idx < n; idx += blockDim.x) {
            const int64_t c = (int64_t)__hip_atomic_load(&in[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int64_t next = seg_rerun<PACKED, BWD>(g, edge, c);
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

// BRANCH: soft_branch_body (48-byte rows), otherwise soft_llr_body.  The lane of a segment's last chunk writes the pad outputs.
template <bool PACKED, int DIFF, bool BRANCH>
__global__ __launch_bounds__(SOFT_THREADS) void seg_llr_kernel(seg_args g, double *__restrict__ llr, uint8_t *__restrict__ bits, uint8_t *__restrict__ branch)
{
    const int64_t c = (int64_t)blockIdx.x * SOFT_THREADS + threadIdx.x;
    if (c >= g.T) return;
    const seg_chunk k = seg_find(g, c);
    if constexpr (BRANCH) soft_branch_body<PACKED, DIFF, false>(g.rows, soft_no_prior{}, k.k, g.bedge, g.alpha, llr, bits, branch);
    else soft_llr_body<PACKED, DIFF, false>(g.rows, soft_no_prior{}, k.k, g.bedge, g.alpha, llr, bits);
    if (k.last)
        for (int64_t r = k.k.hi; r < k.k.lo + g.stride; ++r) {
            llr[r] = 0.0;
            bits[r] = 0;
            if constexpr (BRANCH) branch[r] = 0;
        }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
// Scratch (doubles), every part a multiple of 4 words so that the 32-byte records stay aligned:
//   forward header + lists | backward header + lists | forward records | backward records | ã per row and lane
struct seg_geom {
    size_t off_bhdr, off_f, off_b, off_alpha, words;
};

static seg_geom seg_geometry(int64_t T, int ch)
{
    const auto up4 = [](size_t v) { return (v + 3) / 4 * 4; };
    seg_geom l;
    const size_t hdr = up4(VIT_HDR + 2 * (size_t)T);
    l.off_bhdr = hdr;
    l.off_f = 2 * hdr;
    l.off_b = l.off_f + 8 * (size_t)T;
    l.off_alpha = l.off_b + 8 * (size_t)T;
    l.words = l.off_alpha + 4 * (size_t)ch * (size_t)T;
    return l;
}

template <bool PACKED, int DIFF>
static int seg_run(wf_ctx *ctx, const seg_args &a, unsigned long long *fhdr, unsigned long long *bhdr, double *llr, uint8_t *bits, uint8_t *branch, hipStream_t s)
{
    const unsigned grid = (unsigned)((a.T + SOFT_THREADS - 1) / SOFT_THREADS);
    hipLaunchKernelGGL((seg_bounds_kernel<PACKED>), dim3(grid), dim3(SOFT_THREADS), 0, s, a, fhdr, bhdr);
    WF_LAUNCH_CHECK();
    if (a.cps > 1) {
        const unsigned fgrid = (unsigned)wf_grid_for(a.T, 256, 1024);
        const int rc = soft_fixup_passes(ctx, [&](auto bwd, int mode) {
            hipLaunchKernelGGL((seg_fixup_kernel<PACKED, decltype(bwd)::value>), dim3(fgrid), dim3(256), 0, s, a, bwd ? bhdr : fhdr, ctx->d_vit_unmerged, mode);
        });
        if (rc) return rc;
    }
    if constexpr (!PACKED) {
        if (branch) {
            hipLaunchKernelGGL((seg_llr_kernel<false, DIFF, true>), dim3(grid), dim3(SOFT_THREADS), 0, s, a, llr, bits, branch);
            WF_LAUNCH_CHECK();
            return WF_OK;
        }
    }
    hipLaunchKernelGGL((seg_llr_kernel<PACKED, DIFF, false>), dim3(grid), dim3(SOFT_THREADS), 0, s, a, llr, bits, branch);
    WF_LAUNCH_CHECK();
    return WF_OK;
}

extern "C" int wf_viterbi4_soft_branch_segments(wf_ctx *ctx, const double *d_rows, int64_t nseg, int64_t seglen, int64_t stride, int row_bytes,
                                                int differential, int warmup, double *d_llr, uint8_t *d_bits, uint8_t *d_branch, void *stream)
{
    static const char who[] = "wf_viterbi4_soft_branch_segments";
    constexpr int64_t kMax = (int64_t)1 << 40;
    WF_REQUIRE(nseg >= 1 && nseg <= ((int64_t)1 << 20), "%s: nseg = %lld outside 1 .. 2^20", who, (long long)nseg);
    WF_REQUIRE(seglen >= 1 && seglen <= kMax, "%s: seglen = %lld outside 1 .. 2^40", who, (long long)seglen);
    WF_REQUIRE(stride >= seglen && stride % 2 == 0 && stride <= kMax / nseg, "%s: stride must be even, at least seglen, and nseg stride at most 2^40", who);
    int rc = soft_check_args(who, ctx, d_rows, nseg * seglen, row_bytes, warmup, nullptr, 0.0, nullptr, d_llr, d_bits,
                             "rows must be 16-byte and llr 8-byte aligned");
    if (rc) return rc;
    WF_REQUIRE(!(d_branch && row_bytes == 32), "%s: the branches need 48-byte rows", who);
    const soft_geom sg = soft_geometry(ctx, nseg * seglen, warmup);
    seg_args a;
    a.rows = d_rows;
    a.seglen = seglen, a.stride = stride;
    a.ch = (int)(sg.ch < seglen ? sg.ch : seglen);
    a.warmup = sg.warmup;
    a.cps = (seglen + a.ch - 1) / a.ch;
    a.T = nseg * a.cps;
    const seg_geom l = seg_geometry(a.T, a.ch);
    rc = soft_reserve(who, ctx, a.T, l.words);
    if (rc) return rc;
    double *base = ctx->d_vit_edge;
    unsigned long long *fhdr = reinterpret_cast<unsigned long long *>(base), *bhdr = reinterpret_cast<unsigned long long *>(base + l.off_bhdr);
    a.fedge = base + l.off_f, a.bedge = base + l.off_b, a.alpha = base + l.off_alpha;
    hipStream_t s = wf_stream(stream);
    return soft_dispatch(row_bytes, differential, [&](auto packed, auto diff) {
        return seg_run<decltype(packed)::value, decltype(diff)::value>(ctx, a, fhdr, bhdr, d_llr, d_bits, d_branch, s);
    });
}
