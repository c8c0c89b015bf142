// wf_viterbi_soft_apriori.hip — the max-log-MAP SOQPSK detector of wf_viterbi_soft.hip with a per-row prior on the input bit
// and EXTRINSIC output (include/wfhip.h, wf_viterbi4_soft_apriori, states the definition): the inner half of iterative
// detection and decoding.
//
//   π_k = scale * (double)prior[k];   inc'_k(b) = inc_k(b) + π_k for the branches whose input bit is 1 (one float64 addition)
//   ã, b̃: the recursions of the plain detector over inc';   λᵉ_k from (ã_k + inc_k) + b̃_{k+1}: the CHANNEL increment.
//
// Signed zeros: a prior can make an increment negative or -0, but a normalised metric is o - min(o) >= +0 and is never -0
// (x - x = +0 in round-to-nearest), and a sum with one operand that is not -0 is not -0 either.  So no value that reaches
// an fmin is -0, equal values are bitwise equal, and fmin restates the definition's strict compare whatever the order of
// its operands.  Rows and priors are finite, so there is no NaN.
//
// The four-launch structure, the scratch layout and the chunk proof are those of wf_viterbi_soft.hip (wf_viterbi_soft.h
// holds what the two files share).  Every kernel here also needs the input bit of a branch, so all of them carry the
// DIFF template argument.  The prior is read the way the rows are, by each lane along its own chunk, but 32 B at a time
// into a register window (soft_prior_win): 4 B per row beside the row's 32 / 48 B.
#include "wf_viterbi_soft_apriori.h"

#include <cmath>

template <bool PACKED, int DIFF>
__global__ __launch_bounds__(SOFT_THREADS) void soft_ap_bounds_kernel(const double *__restrict__ rows, soft_prior pr, int64_t n, int ch, int warmup,
                                                                    int64_t nch, double *__restrict__ fedge, double *__restrict__ bedge,
                                                                    double *__restrict__ alpha)
{
    if (blockIdx.x == 0 && threadIdx.x < VIT_HDR) {        // lists empty, nobody arrived (both directions)
        reinterpret_cast<uint64_t *>(fedge + 8 * nch)[threadIdx.x] = 0;
        reinterpret_cast<uint64_t *>(bedge + 8 * nch)[threadIdx.x] = 0;
    }
    const int64_t c = (int64_t)blockIdx.x * SOFT_THREADS + threadIdx.x;
    if (c >= nch) return;
    const int64_t a = c * ch, e = a + ch < n ? a + ch : n;
    soft_prior_win w;
    double m[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t k = a - warmup > 0 ? a - warmup : 0; k < a; ++k) soft_ap_fwd_row<PACKED, DIFF>(m, rows, pr, w, k);
    soft_put4(fedge + 8 * c, m);
    soft_ap_fwd_chunk<PACKED, DIFF>(rows, pr, w, a, e, c, nch, alpha, m);
    soft_put4(fedge + 8 * c + 4, m);

    double b[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t k = (e + warmup < n ? e + warmup : n) - 1; k >= e; --k) soft_ap_bwd_row<PACKED, DIFF>(b, rows, pr, w, k);
    const int64_t cm = nch - 1 - c;                        // mirrored record index
    soft_put4(bedge + 8 * cm, b);
    for (int64_t k = e - 1; k >= a; --k) soft_ap_bwd_row<PACKED, DIFF>(b, rows, pr, w, k);
    soft_put4(bedge + 8 * cm + 4, b);
}

// soft_rerun of wf_viterbi_soft.hip over inc'
template <bool PACKED, bool BWD, int DIFF>
__device__ __forceinline__ bool soft_ap_rerun(const double *__restrict__ rows, const soft_prior &pr, int64_t n, int ch, int64_t nch,
                                              double *__restrict__ edge, double *__restrict__ alpha, int64_t r)
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
    soft_prior_win w;
    if (BWD)
        for (int64_t k = e - 1; k >= a; --k) soft_ap_bwd_row<PACKED, DIFF>(m, rows, pr, w, k);
    else
        soft_ap_fwd_chunk<PACKED, DIFF>(rows, pr, w, a, e, c, nch, alpha, m);
    bool changed = false;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        changed |= __double_as_longlong(rec[4 + q]) != __double_as_longlong(m[q]);
        rec[4 + q] = m[q];
    }
    return changed;
}

template <bool PACKED, bool BWD, int DIFF>
__global__ __launch_bounds__(256) void soft_ap_fixup_kernel(const double *__restrict__ rows, soft_prior pr, int64_t n, int ch, double *__restrict__ edge,
                                                            int64_t nch, double *__restrict__ alpha, unsigned long long *__restrict__ unmerged, int mode)
{
    if (!vit_fixup_verify(edge, nch, unmerged, mode)) return;
    vit_fixup_rounds(edge, nch, unmerged, [&](int64_t r) { return soft_ap_rerun<PACKED, BWD, DIFF>(rows, pr, n, ch, nch, edge, alpha, r); });
}

template <bool PACKED, int DIFF>
__global__ __launch_bounds__(SOFT_THREADS) void soft_ap_llr_kernel(const double *__restrict__ rows, soft_prior pr, int64_t n, int ch, int64_t nch,
                                                                 const double *__restrict__ bedge, const double *__restrict__ alpha,
                                                                 double *__restrict__ ext, uint8_t *__restrict__ bits)
{
    const int64_t c = (int64_t)blockIdx.x * SOFT_THREADS + threadIdx.x;
    if (c >= nch) return;
    const int64_t a = c * ch, e = a + ch < n ? a + ch : n;
    double b[4], m[4];
    soft_prior_win w;
    soft_get4(bedge + 8 * (nch - 1 - c), b);               // b̃_e, proven
    for (int64_t k = e - 1; k >= a; --k) {
        soft_get4(alpha + 4 * ((k - a) * nch + c), m);     // ã_k (of inc')
        const double2 *z = soft_row<PACKED>(rows, k);
        const double pi = soft_prior_at(pr, w, k);
        double lam;
        if (k & 1) {
            const vit_comp q = vit_components<1, PACKED>(z);
            lam = soft_llr<1, DIFF>(m, b, q);              // the channel's inc in section k
            soft_ap_bwd<1, DIFF>(b, q, pi);
        } else {
            const vit_comp q = vit_components<0, PACKED>(z);
            lam = soft_llr<0, DIFF>(m, b, q);
            soft_ap_bwd<0, DIFF>(b, q, pi);
        }
        ext[k] = lam;
        bits[k] = lam + pi < 0.0 ? 1 : 0;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
template <bool PACKED, int DIFF>
static int soft_ap_run(wf_ctx *ctx, const double *rows, const soft_prior &pr, int64_t n, const soft_geom &g, double *ext, uint8_t *bits, hipStream_t s)
{
    double *fedge = ctx->d_vit_edge, *bedge = fedge + g.off_b, *alpha = fedge + g.off_alpha;
    const unsigned grid = (unsigned)((g.nch + SOFT_THREADS - 1) / SOFT_THREADS);
    hipLaunchKernelGGL((soft_ap_bounds_kernel<PACKED, DIFF>), dim3(grid), dim3(SOFT_THREADS), 0, s, rows, pr, n, g.ch, g.warmup, g.nch, fedge, bedge,
                       alpha);
    WF_LAUNCH_CHECK();
    if (g.nch > 1) {
        // repair, count only, or repair and count behind it: as wf_viterbi_soft.hip (soft_run)
        const unsigned fgrid = (unsigned)wf_grid_for(g.nch - 1, 256, 1024);
        const int passes = ctx->opt[WF_OPT_DET_REPAIR] == 0 && ctx->opt[WF_OPT_DET_FINAL_VERIFY] ? 2 : 1;
        for (int pass = 0; pass < passes; ++pass) {
            const int mode = pass == 0 && ctx->opt[WF_OPT_DET_REPAIR] == 0 ? 1 : 0;
            hipLaunchKernelGGL((soft_ap_fixup_kernel<PACKED, false, DIFF>), dim3(fgrid), dim3(256), 0, s, rows, pr, n, g.ch, fedge, g.nch, alpha,
                               ctx->d_vit_unmerged, mode);
            WF_LAUNCH_CHECK();
            hipLaunchKernelGGL((soft_ap_fixup_kernel<PACKED, true, DIFF>), dim3(fgrid), dim3(256), 0, s, rows, pr, n, g.ch, bedge, g.nch, alpha,
                               ctx->d_vit_unmerged, mode);
            WF_LAUNCH_CHECK();
        }
    }
    hipLaunchKernelGGL((soft_ap_llr_kernel<PACKED, DIFF>), dim3(grid), dim3(SOFT_THREADS), 0, s, rows, pr, n, g.ch, g.nch, bedge, alpha, ext, bits);
    WF_LAUNCH_CHECK();
    return WF_OK;
}

extern "C" int wf_viterbi4_soft_apriori(wf_ctx *ctx, const double *d_rows, int64_t ncalls, int row_bytes, int differential, int warmup,
                                        const float *d_apriori, double apriori_scale, double *d_ext, uint8_t *d_bits, void *stream)
{
    WF_REQUIRE(ctx && d_rows && d_ext && d_bits, "wf_viterbi4_soft_apriori: NULL argument");
    WF_REQUIRE(ncalls >= 1 && warmup >= 0, "wf_viterbi4_soft_apriori: bad argument");
    WF_REQUIRE(row_bytes == 32 || row_bytes == 48, "wf_viterbi4_soft_apriori: row_bytes must be 32 (packed) or 48 (3 complex128)");
    WF_REQUIRE(std::isfinite(apriori_scale), "wf_viterbi4_soft_apriori: apriori_scale must be finite");
    WF_REQUIRE((reinterpret_cast<uintptr_t>(d_rows) & 15) == 0 && (reinterpret_cast<uintptr_t>(d_ext) & 7) == 0 &&
                   (reinterpret_cast<uintptr_t>(d_apriori) & 3) == 0,
               "wf_viterbi4_soft_apriori: rows must be 16-byte, ext 8-byte and the prior 4-byte aligned");
    if (!d_apriori)            // π = 0: the plain detector (bitwise: ã + (inc + 0) = ã + inc, since ã is never -0)
        return wf_viterbi4_soft(ctx, d_rows, ncalls, row_bytes, differential, warmup, d_ext, d_bits, stream);
    const soft_geom g = soft_geometry(ctx, ncalls, warmup);
    WF_REQUIRE((g.nch + SOFT_THREADS - 1) / SOFT_THREADS < (1ll << 31), "wf_viterbi4_soft_apriori: burst too long for one launch");
    WF_HIP(hipSetDevice(ctx->device));
    const int rc = wf_ctx_reserve_vit(ctx, g.words);
    if (rc) return rc;
    hipStream_t s = wf_stream(stream);
    const soft_prior pr{d_apriori, apriori_scale, ncalls, (reinterpret_cast<uintptr_t>(d_apriori) & 15) == 0 ? 1 : 0};
    if (row_bytes == 32)
        return differential ? soft_ap_run<true, 1>(ctx, d_rows, pr, ncalls, g, d_ext, d_bits, s) : soft_ap_run<true, 0>(ctx, d_rows, pr, ncalls, g, d_ext, d_bits, s);
    return differential ? soft_ap_run<false, 1>(ctx, d_rows, pr, ncalls, g, d_ext, d_bits, s) : soft_ap_run<false, 0>(ctx, d_rows, pr, ncalls, g, d_ext, d_bits, s);
}
