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
//
// This file owns the definition above, the plain kernels and the entry points wf_viterbi4_soft, wf_viterbi4_soft_geometry
// and wf_viterbi4_soft_branch (the same launches with soft_branch_kernel as the last one: the decided branch per row).  The trellis steps and the walks of the three launches live in wf_viterbi_soft.h, shared with
// wf_viterbi_soft_apriori.hip and wf_viterbi_live.hip; the kernels here are its AP = false form.  Without a prior no
// branch's input bit enters the recursions, so only the last launch carries DIFF.
#include "wf_viterbi_soft.h"

template <bool PACKED>
__global__ __launch_bounds__(SOFT_THREADS) void soft_bounds_kernel(const double *__restrict__ rows, int64_t n, int ch, int warmup, int64_t nch,
                                                                 double *__restrict__ fedge, double *__restrict__ bedge, double *__restrict__ alpha)
{
    soft_burst_clear_lists(fedge, bedge, nch);
    const int64_t c = (int64_t)blockIdx.x * SOFT_THREADS + threadIdx.x;
    if (c >= nch) return;
    soft_bounds_body<PACKED, 0, false>(rows, soft_no_prior{}, soft_burst_chunk(c, ch, n, nch), warmup, fedge, bedge, alpha);
}

template <bool PACKED, bool BWD>
__global__ __launch_bounds__(256) void soft_fixup_kernel(const double *__restrict__ rows, int64_t n, int ch, double *__restrict__ edge, int64_t nch,
                                                         double *__restrict__ alpha, unsigned long long *__restrict__ unmerged, int mode)
{
    if (!vit_fixup_verify(edge, nch, unmerged, mode)) return;
    vit_fixup_rounds(edge, nch, unmerged, [&](int64_t r) { return soft_burst_rerun<PACKED, BWD, 0, false>(rows, soft_no_prior{}, n, ch, nch, edge, alpha, r); });
}

template <bool PACKED, int DIFF>
__global__ __launch_bounds__(SOFT_THREADS) void soft_llr_kernel(const double *__restrict__ rows, int64_t n, int ch, int64_t nch,
                                                              const double *__restrict__ bedge, const double *__restrict__ alpha,
                                                              double *__restrict__ llr, uint8_t *__restrict__ bits)
{
    const int64_t c = (int64_t)blockIdx.x * SOFT_THREADS + threadIdx.x;
    if (c >= nch) return;
    soft_llr_body<PACKED, DIFF, false>(rows, soft_no_prior{}, soft_burst_chunk(c, ch, n, nch), bedge, alpha, llr, bits);
}

// the last launch of wf_viterbi4_soft_branch (48-byte rows only: the packed rows drop the quadrature components its user reads)
template <int DIFF>
__global__ __launch_bounds__(SOFT_THREADS) void soft_branch_kernel(const double *__restrict__ rows, int64_t n, int ch, int64_t nch,
                                                                 const double *__restrict__ bedge, const double *__restrict__ alpha,
                                                                 double *__restrict__ llr, uint8_t *__restrict__ bits, uint8_t *__restrict__ branch)
{
    const int64_t c = (int64_t)blockIdx.x * SOFT_THREADS + threadIdx.x;
    if (c >= nch) return;
    soft_branch_body<false, DIFF, false>(rows, soft_no_prior{}, soft_burst_chunk(c, ch, n, nch), bedge, alpha, llr, bits, branch);
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

template <bool PACKED, int DIFF>
static int soft_run(wf_ctx *ctx, const double *rows, int64_t n, const soft_geom &g, double *llr, uint8_t *bits, hipStream_t s, uint8_t *branch = nullptr)
{
    double *fedge = ctx->d_vit_edge, *bedge = fedge + g.off_b, *alpha = fedge + g.off_alpha;
    const unsigned grid = (unsigned)((g.nch + SOFT_THREADS - 1) / SOFT_THREADS);
    hipLaunchKernelGGL((soft_bounds_kernel<PACKED>), dim3(grid), dim3(SOFT_THREADS), 0, s, rows, n, g.ch, g.warmup, g.nch, fedge, bedge, alpha);
    WF_LAUNCH_CHECK();
    if (g.nch > 1) {
        const unsigned fgrid = (unsigned)wf_grid_for(g.nch - 1, 256, 1024);
        const int rc = soft_fixup_passes(ctx, [&](auto bwd, int mode) {
            hipLaunchKernelGGL((soft_fixup_kernel<PACKED, decltype(bwd)::value>), dim3(fgrid), dim3(256), 0, s, rows, n, g.ch, bwd ? bedge : fedge, g.nch, alpha,
                               ctx->d_vit_unmerged, mode);
        });
        if (rc) return rc;
    }
    if constexpr (!PACKED) {
        if (branch) {
            hipLaunchKernelGGL((soft_branch_kernel<DIFF>), dim3(grid), dim3(SOFT_THREADS), 0, s, rows, n, g.ch, g.nch, bedge, alpha, llr, bits, branch);
            WF_LAUNCH_CHECK();
            return WF_OK;
        }
    }
    hipLaunchKernelGGL((soft_llr_kernel<PACKED, DIFF>), dim3(grid), dim3(SOFT_THREADS), 0, s, rows, n, g.ch, g.nch, bedge, alpha, llr, bits);
    WF_LAUNCH_CHECK();
    return WF_OK;
}

extern "C" int wf_viterbi4_soft(wf_ctx *ctx, const double *d_rows, int64_t ncalls, int row_bytes, int differential, int warmup,
                                double *d_llr, uint8_t *d_bits, void *stream)
{
    static const char who[] = "wf_viterbi4_soft";
    int rc = soft_check_args(who, ctx, d_rows, ncalls, row_bytes, warmup, nullptr, 0.0, nullptr, d_llr, d_bits,
                             "rows must be 16-byte and llr 8-byte aligned");
    if (rc) return rc;
    const soft_geom g = soft_geometry(ctx, ncalls, warmup);
    rc = soft_reserve(who, ctx, g.nch, g.words);
    if (rc) return rc;
    hipStream_t s = wf_stream(stream);
    return soft_dispatch(row_bytes, differential, [&](auto packed, auto diff) {
        return soft_run<decltype(packed)::value, decltype(diff)::value>(ctx, d_rows, ncalls, g, d_llr, d_bits, s);
    });
}

// wf_viterbi4_soft on 48-byte rows with the arg-min branch of every row (include/wfhip.h): the same first launch, proof and
// repairs; only the last launch differs (soft_branch_body).
extern "C" int wf_viterbi4_soft_branch(wf_ctx *ctx, const double *d_rows, int64_t ncalls, int differential, int warmup, double *d_llr, uint8_t *d_bits,
                                       uint8_t *d_branch, void *stream)
{
    static const char who[] = "wf_viterbi4_soft_branch";
    int rc = soft_check_args(who, ctx, d_rows, ncalls, 48, warmup, nullptr, 0.0, nullptr, d_llr, d_bits, "rows must be 16-byte and llr 8-byte aligned");
    if (rc) return rc;
    WF_REQUIRE(d_branch, "%s: NULL argument", who);
    const soft_geom g = soft_geometry(ctx, ncalls, warmup);
    rc = soft_reserve(who, ctx, g.nch, g.words);
    if (rc) return rc;
    hipStream_t s = wf_stream(stream);
    if (differential) return soft_run<false, 1>(ctx, d_rows, ncalls, g, d_llr, d_bits, s, d_branch);
    return soft_run<false, 0>(ctx, d_rows, ncalls, g, d_llr, d_bits, s, d_branch);
}
