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
// its operands.  Rows and priors are finite, so there is no NaN.  This is why the one statement of the steps in
// wf_viterbi_soft.h is bitwise the definition in all three of its uses: the plain detector is the case without the
// additions of π, the live windows apply the same operations to a slice of the burst.
//
// The four launches, the scratch layout and the chunk proof are those of wf_viterbi_soft.hip, and the walks are the ones it
// uses (wf_viterbi_soft.h, AP = true); this file owns the prior's arithmetic above, the kernels below and its entry point.
// Every kernel here also needs the input bit of a branch, so all of them carry the DIFF template argument.  The prior is
// read the way the rows are, by each lane along its own chunk, but 32 B at a time into a register window
// (soft_prior_win): 4 B per row beside the row's 32 / 48 B.
#include "wf_viterbi_soft.h"

template <bool PACKED, int DIFF>
__global__ __launch_bounds__(SOFT_THREADS) void soft_ap_bounds_kernel(const double *__restrict__ rows, soft_prior pr, int64_t n, int ch, int warmup,
                                                                    int64_t nch, double *__restrict__ fedge, double *__restrict__ bedge,
                                                                    double *__restrict__ alpha)
{
    soft_burst_clear_lists(fedge, bedge, nch);
    const int64_t c = (int64_t)blockIdx.x * SOFT_THREADS + threadIdx.x;
    if (c >= nch) return;
    soft_bounds_body<PACKED, DIFF, true>(rows, pr, soft_burst_chunk(c, ch, n, nch), warmup, fedge, bedge, alpha);
}

template <bool PACKED, bool BWD, int DIFF>
__global__ __launch_bounds__(256) void soft_ap_fixup_kernel(const double *__restrict__ rows, soft_prior pr, int64_t n, int ch, double *__restrict__ edge,
                                                            int64_t nch, double *__restrict__ alpha, unsigned long long *__restrict__ unmerged, int mode)
{
    if (!vit_fixup_verify(edge, nch, unmerged, mode)) return;
    vit_fixup_rounds(edge, nch, unmerged, [&](int64_t r) { return soft_burst_rerun<PACKED, BWD, DIFF, true>(rows, pr, n, ch, nch, edge, alpha, r); });
}

template <bool PACKED, int DIFF>
__global__ __launch_bounds__(SOFT_THREADS) void soft_ap_llr_kernel(const double *__restrict__ rows, soft_prior pr, int64_t n, int ch, int64_t nch,
                                                                 const double *__restrict__ bedge, const double *__restrict__ alpha,
                                                                 double *__restrict__ ext, uint8_t *__restrict__ bits)
{
    const int64_t c = (int64_t)blockIdx.x * SOFT_THREADS + threadIdx.x;
    if (c >= nch) return;
    soft_llr_body<PACKED, DIFF, true>(rows, pr, soft_burst_chunk(c, ch, n, nch), bedge, alpha, ext, bits);
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
        const unsigned fgrid = (unsigned)wf_grid_for(g.nch - 1, 256, 1024);
        const int rc = soft_fixup_passes(ctx, [&](auto bwd, int mode) {
            hipLaunchKernelGGL((soft_ap_fixup_kernel<PACKED, decltype(bwd)::value, DIFF>), dim3(fgrid), dim3(256), 0, s, rows, pr, n, g.ch, bwd ? bedge : fedge,
                               g.nch, alpha, ctx->d_vit_unmerged, mode);
        });
        if (rc) return rc;
    }
    hipLaunchKernelGGL((soft_ap_llr_kernel<PACKED, DIFF>), dim3(grid), dim3(SOFT_THREADS), 0, s, rows, pr, n, g.ch, g.nch, bedge, alpha, ext, bits);
    WF_LAUNCH_CHECK();
    return WF_OK;
}

extern "C" int wf_viterbi4_soft_apriori(wf_ctx *ctx, const double *d_rows, int64_t ncalls, int row_bytes, int differential, int warmup,
                                        const float *d_apriori, double apriori_scale, double *d_ext, uint8_t *d_bits, void *stream)
{
    static const char who[] = "wf_viterbi4_soft_apriori";
    int rc = soft_check_args(who, ctx, d_rows, ncalls, row_bytes, warmup, d_apriori, apriori_scale, nullptr, d_ext, d_bits,
                             "rows must be 16-byte, ext 8-byte and the prior 4-byte aligned");
    if (rc) return rc;
    if (!d_apriori)            // π = 0: the plain detector (bitwise: ã + (inc + 0) = ã + inc, since ã is never -0)
        return wf_viterbi4_soft(ctx, d_rows, ncalls, row_bytes, differential, warmup, d_ext, d_bits, stream);
    const soft_geom g = soft_geometry(ctx, ncalls, warmup);
    rc = soft_reserve(who, ctx, g.nch, g.words);
    if (rc) return rc;
    hipStream_t s = wf_stream(stream);
    const soft_prior pr = soft_prior_of(d_apriori, apriori_scale, ncalls);
    return soft_dispatch(row_bytes, differential, [&](auto packed, auto diff) {
        return soft_ap_run<decltype(packed)::value, decltype(diff)::value>(ctx, d_rows, pr, ncalls, g, d_ext, d_bits, s);
    });
}
