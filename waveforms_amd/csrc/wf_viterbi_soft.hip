// wf_viterbi_soft.hip — max-log-MAP soft-output detector over the SOQPSK 4-state, 2-column trellis.
//
// Build-defined (the reference's detector, waveforms/viterbi/algorithm.py:18-101, is hard-decision only); it keeps the
// reference's conventions: branch increments Re(state_exp_term[start] * z[idx(out)]) (:57-63), the trellis and the
// column schedule (row k is section k with column k % 2, :69-87), metrics MINIMISED.  For a burst of N rows, free
// start and free end, in float64 and in exactly this order of operations:
//   ã_0 = 0,        a'_{k+1}(s') = min_{end b = s'} (ã_k(start b) + inc_k(b)),        ã_{k+1} = a'_{k+1} - min a'_{k+1}
//   b̃_N = 0,        b'_k(s)      = min_{start b = s} (inc_k(b) + b̃_{k+1}(end b)),      b̃_k     = b'_k - min b'_k
//   λ_k = min_{inp b = 1} ((ã_k(start b) + inc_k(b)) + b̃_{k+1}(end b)) - min_{inp b = 0} (the same)
// bits_k = λ_k < 0.  Every metric is >= +0 and no sum is ever -0, so fmin and the subtractions are exact restatements.
//
// Chunk-parallel, a thread (lane) per chunk of `ch` consecutive rows, in four launches:
//   soft_bounds_kernel   forward: ã at the chunk start from zeros `warmup` rows earlier (exact for the chunks that
//                        reach row 0), then over the chunk's own rows, storing ã_k per row in the context's scratch
//                        (lane-interleaved: consecutive lanes write consecutive 32 B); backward, the mirror: b̃ at
//                        the chunk end from zeros `warmup` rows later (exact for the chunks that reach row N), then
//                        back over the chunk's rows.  Each direction records {start, end} per chunk.
//   soft_fixup_kernel    x2: the proof and cascading repair of the hard detectors (wf_viterbi4.h), once per
//                        direction.  The backward records are kept in MIRRORED chunk order (chunk c at nch - 1 - c),
//                        so "a chunk's start is bitwise its predecessor's end" is the same check and the repairs
//                        cascade toward the start of the burst.  A forward repair rewrites the chunk's stored ã.
//   soft_llr_kernel      from the proven b̃ at the chunk end, back over the chunk: λ_k from the stored ã_k, then b̃_k.
// The result is bitwise the definition whatever `warmup` and the chunking; the warm-up only sets how often the
// repairs run.
#include "wf_viterbi_soft.h"

template <bool PACKED>
__global__ __launch_bounds__(SOFT_THREADS) void soft_bounds_kernel(const double *__restrict__ rows, int64_t n, int ch, int warmup, int64_t nch,
                                                                 double *__restrict__ fedge, double *__restrict__ bedge, double *__restrict__ alpha)
{
    if (blockIdx.x == 0 && threadIdx.x < VIT_HDR) {        // lists empty, nobody arrived (both directions)
        reinterpret_cast<uint64_t *>(fedge + 8 * nch)[threadIdx.x] = 0;
        reinterpret_cast<uint64_t *>(bedge + 8 * nch)[threadIdx.x] = 0;
    }
    const int64_t c = (int64_t)blockIdx.x * SOFT_THREADS + threadIdx.x;
    if (c >= nch) return;
    const int64_t a = c * ch, e = a + ch < n ? a + ch : n;
    double m[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t k = a - warmup > 0 ? a - warmup : 0; k < a; ++k) soft_fwd_row<PACKED>(m, rows, k);
    soft_put4(fedge + 8 * c, m);
    soft_fwd_chunk<PACKED>(rows, a, e, c, nch, alpha, m);
    soft_put4(fedge + 8 * c + 4, m);

    double b[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t k = (e + warmup < n ? e + warmup : n) - 1; k >= e; --k) soft_bwd_row<PACKED>(b, rows, k);
    const int64_t cm = nch - 1 - c;                        // mirrored record index
    soft_put4(bedge + 8 * cm, b);
    for (int64_t k = e - 1; k >= a; --k) soft_bwd_row<PACKED>(b, rows, k);
    soft_put4(bedge + 8 * cm + 4, b);
}

// Repair of record r (forward: chunk r; backward: chunk nch - 1 - r) by one thread: start from the predecessor
// record's end as it is now, run the chunk, rewrite the end; true when the end changed.
template <bool PACKED, bool BWD>
__device__ __forceinline__ bool soft_rerun(const double *__restrict__ rows, int64_t n, int ch, int64_t nch, double *__restrict__ edge,
                                           double *__restrict__ alpha, int64_t r)
{
    double *rec = edge + 8 * r;
    double m[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        m[q] = __hip_atomic_load(rec - 4 + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (r >= 1: record 0 is exact)
        rec[q] = m[q];
    }
    const int64_t c = BWD ? nch - 1 - r : r;
    const int64_t a = c * ch, e = a + ch < n ? a + ch : n;
    if (BWD)
        for (int64_t k = e - 1; k >= a; --k) soft_bwd_row<PACKED>(m, rows, k);
    else
        soft_fwd_chunk<PACKED>(rows, a, e, c, nch, alpha, m);
    bool changed = false;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        changed |= __double_as_longlong(rec[4 + q]) != __double_as_longlong(m[q]);
        rec[4 + q] = m[q];
    }
    return changed;
}

template <bool PACKED, bool BWD>
__global__ __launch_bounds__(256) void soft_fixup_kernel(const double *__restrict__ rows, int64_t n, int ch, double *__restrict__ edge, int64_t nch,
                                                         double *__restrict__ alpha, unsigned long long *__restrict__ unmerged, int mode)
{
    if (!vit_fixup_verify(edge, nch, unmerged, mode)) return;
    vit_fixup_rounds(edge, nch, unmerged, [&](int64_t r) { return soft_rerun<PACKED, BWD>(rows, n, ch, nch, edge, alpha, r); });
}

template <bool PACKED, int DIFF>
__global__ __launch_bounds__(SOFT_THREADS) void soft_llr_kernel(const double *__restrict__ rows, int64_t n, int ch, int64_t nch,
                                                              const double *__restrict__ bedge, const double *__restrict__ alpha,
                                                              double *__restrict__ llr, uint8_t *__restrict__ bits)
{
    const int64_t c = (int64_t)blockIdx.x * SOFT_THREADS + threadIdx.x;
    if (c >= nch) return;
    const int64_t a = c * ch, e = a + ch < n ? a + ch : n;
    double b[4], m[4];
    soft_get4(bedge + 8 * (nch - 1 - c), b);               // b̃_e, proven
    for (int64_t k = e - 1; k >= a; --k) {
        soft_get4(alpha + 4 * ((k - a) * nch + c), m);     // ã_k
        const double2 *z = soft_row<PACKED>(rows, k);
        double lam;
        if (k & 1) {
            const vit_comp q = vit_components<1, PACKED>(z);
            lam = soft_llr<1, DIFF>(m, b, q);
            soft_bwd<1>(b, q);
        } else {
            const vit_comp q = vit_components<0, PACKED>(z);
            lam = soft_llr<0, DIFF>(m, b, q);
            soft_bwd<0>(b, q);
        }
        llr[k] = lam;
        bits[k] = lam < 0.0 ? 1 : 0;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------

extern "C" int wf_viterbi4_soft_geometry(wf_ctx *ctx, int64_t ncalls, int warmup, int64_t *h_geom)
{
    WF_REQUIRE(ctx && h_geom && ncalls >= 1 && warmup >= 0, "wf_viterbi4_soft_geometry: bad argument");
    const soft_geom g = soft_geometry(ctx, ncalls, warmup);
    h_geom[0] = g.ch;
    h_geom[1] = g.nch;
    h_geom[2] = g.warmup;
    h_geom[3] = (int64_t)(g.words * sizeof(double));
    return WF_OK;
}

template <bool PACKED>
static void soft_launch_llr(int diff, unsigned grid, hipStream_t s, const double *rows, int64_t n, const soft_geom &g, const double *bedge,
                            const double *alpha, double *llr, uint8_t *bits)
{
    if (diff)
        hipLaunchKernelGGL((soft_llr_kernel<PACKED, 1>), dim3(grid), dim3(SOFT_THREADS), 0, s, rows, n, g.ch, g.nch, bedge, alpha, llr, bits);
    else
        hipLaunchKernelGGL((soft_llr_kernel<PACKED, 0>), dim3(grid), dim3(SOFT_THREADS), 0, s, rows, n, g.ch, g.nch, bedge, alpha, llr, bits);
}

template <bool PACKED>
static int soft_run(wf_ctx *ctx, const double *rows, int64_t n, int diff, const soft_geom &g, double *llr, uint8_t *bits, hipStream_t s)
{
    double *fedge = ctx->d_vit_edge, *bedge = fedge + g.off_b, *alpha = fedge + g.off_alpha;
    const unsigned grid = (unsigned)((g.nch + SOFT_THREADS - 1) / SOFT_THREADS);
    hipLaunchKernelGGL((soft_bounds_kernel<PACKED>), dim3(grid), dim3(SOFT_THREADS), 0, s, rows, n, g.ch, g.warmup, g.nch, fedge, bedge, alpha);
    WF_LAUNCH_CHECK();
    if (g.nch > 1) {
        // as the hard detectors (wf_viterbi.hip: viterbi_launch): repair, or only count under WF_OPT_DET_REPAIR = 1;
        // WF_OPT_DET_FINAL_VERIFY adds a counting pass behind the repairs
        const unsigned fgrid = (unsigned)wf_grid_for(g.nch - 1, 256, 1024);
        const int passes = ctx->opt[WF_OPT_DET_REPAIR] == 0 && ctx->opt[WF_OPT_DET_FINAL_VERIFY] ? 2 : 1;
        for (int pass = 0; pass < passes; ++pass) {
            const int mode = pass == 0 && ctx->opt[WF_OPT_DET_REPAIR] == 0 ? 1 : 0;
            hipLaunchKernelGGL((soft_fixup_kernel<PACKED, false>), dim3(fgrid), dim3(256), 0, s, rows, n, g.ch, fedge, g.nch, alpha,
                               ctx->d_vit_unmerged, mode);
            WF_LAUNCH_CHECK();
            hipLaunchKernelGGL((soft_fixup_kernel<PACKED, true>), dim3(fgrid), dim3(256), 0, s, rows, n, g.ch, bedge, g.nch, alpha,
                               ctx->d_vit_unmerged, mode);
            WF_LAUNCH_CHECK();
        }
    }
    soft_launch_llr<PACKED>(diff, grid, s, rows, n, g, bedge, alpha, llr, bits);
    WF_LAUNCH_CHECK();
    return WF_OK;
}

extern "C" int wf_viterbi4_soft(wf_ctx *ctx, const double *d_rows, int64_t ncalls, int row_bytes, int differential, int warmup,
                                double *d_llr, uint8_t *d_bits, void *stream)
{
    WF_REQUIRE(ctx && d_rows && d_llr && d_bits, "wf_viterbi4_soft: NULL argument");
    WF_REQUIRE(ncalls >= 1 && warmup >= 0, "wf_viterbi4_soft: bad argument");
    WF_REQUIRE(row_bytes == 32 || row_bytes == 48, "wf_viterbi4_soft: row_bytes must be 32 (packed) or 48 (3 complex128)");
    WF_REQUIRE((reinterpret_cast<uintptr_t>(d_rows) & 15) == 0 && (reinterpret_cast<uintptr_t>(d_llr) & 7) == 0,
               "wf_viterbi4_soft: rows must be 16-byte and llr 8-byte aligned");
    const soft_geom g = soft_geometry(ctx, ncalls, warmup);
    WF_REQUIRE((g.nch + SOFT_THREADS - 1) / SOFT_THREADS < (1ll << 31), "wf_viterbi4_soft: burst too long for one launch");
    WF_HIP(hipSetDevice(ctx->device));
    const int rc = wf_ctx_reserve_vit(ctx, g.words);
    if (rc) return rc;
    hipStream_t s = wf_stream(stream);
    return row_bytes == 32 ? soft_run<true>(ctx, d_rows, ncalls, differential ? 1 : 0, g, d_llr, d_bits, s)
                           : soft_run<false>(ctx, d_rows, ncalls, differential ? 1 : 0, g, d_llr, d_bits, s);
}
