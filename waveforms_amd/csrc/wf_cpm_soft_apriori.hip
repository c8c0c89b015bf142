// wf_cpm_soft_apriori.hip — the max-log-MAP CPM detector of wf_cpm_soft.hip (ARTM multi-h, PCM/FM) with a per-bit prior and
// EXTRINSIC per-bit output (include/wfhip.h, wf_cpm_soft_apriori, states the definition): the inner half of iterative
// detection and decoding for the generic CPM trellis.
//
//   π_{k,i} = scale * (double)prior[lgM k + i];   inc'_k(s,u) = inc_k(s,u) + Π_k(u) for u != 0 (one float64 addition)
//   ã, b̃: the recursions of the plain detector over inc';   λᵉ_{k,i} from (ã_k + x_{k,i}) + b̃_{k+1}, x the CHANNEL increment
//   plus the prior of the other bit of the same symbol (M = 4) — never bit i's own.
//
// Signed zeros: a prior can make an increment negative or -0, but a normalised metric is x - min x >= +0 and never -0
// (x - x = +0 in round-to-nearest), +inf in the lanes that hold no state, and a sum with an operand that is not -0 is not
// -0 either.  Every operand of a v_min_f64 here is such a sum (ã + inc', inc' + b̃, (ã + x) + b̃), so none is -0, equal
// operands are bitwise equal and the minima do not depend on the order they are taken in.  Rows and priors are finite, the
// lanes without a state carry +inf into sums with finite increments only, so there is no NaN.
//
// The four steps, the scratch layout, the chunk proof and the cascading repair are those of wf_cpm_soft.hip; the device
// code is wf_cpm_soft.h's with AP = true: the priors of a staged batch of calls ride in next to its rows (lgM values per
// call, one 256-byte LDS slot per wave, read as a broadcast), and the repair kernels run the same inc', so proof and repair
// stay bitwise the sequential definition at any warm-up and chunking — a strong prior changes how fast paths merge, hence
// how often the repair runs, never the result.
#include "wf_cpm_soft.h"

#include <cmath>

template <int M, int LP>
__global__ __launch_bounds__(CS_THREADS) void cpm_soft_ap_bounds_kernel(const double2 *__restrict__ rows, const double2 *__restrict__ rot_cs,
                                                                        cpm_soft_prior prior, uint64_t *__restrict__ fedge,
                                                                        uint64_t *__restrict__ bedge, double *__restrict__ ckpt, cpm_soft_params P)
{
    __shared__ __attribute__((aligned(16))) char smem[CS_WAVES * CS_WAVE_BYTES_AP];
    __shared__ double rot[2 * CPM_ROT_SIN];
    cs_bounds_body<M, LP, true>(smem, rot, rows, rot_cs, fedge, bedge, ckpt, P, prior);
}

__global__ void cpm_soft_ap_verify_kernel(uint64_t *__restrict__ edge, int64_t nch, int S, unsigned long long *__restrict__ unmerged, int repair)
{
    cs_verify_body(edge, nch, S, unmerged, repair);
}

template <int M, int LP, bool BWD>
__global__ __launch_bounds__(CS_THREADS) void cpm_soft_ap_repair_kernel(const double2 *__restrict__ rows, const double2 *__restrict__ rot_cs,
                                                                        cpm_soft_prior prior, uint64_t *__restrict__ edge,
                                                                        double *__restrict__ ckpt, unsigned long long *__restrict__ unmerged,
                                                                        cpm_soft_params P, int lin, int lout, int finisher)
{
    __shared__ __attribute__((aligned(16))) char smem[CS_WAVES * CS_WAVE_BYTES_AP];
    __shared__ double rot[2 * CPM_ROT_SIN];
    cs_repair_body<M, LP, BWD, true>(smem, rot, rows, rot_cs, edge, ckpt, unmerged, P, prior, lin, lout, finisher);
}

template <int M, int LP>
__global__ __launch_bounds__(CS_THREADS) void cpm_soft_ap_llr_kernel(const double2 *__restrict__ rows, const double2 *__restrict__ rot_cs,
                                                                     cpm_soft_prior prior, const uint64_t *__restrict__ bedge,
                                                                     const double *__restrict__ ckpt, double *__restrict__ ext,
                                                                     uint8_t *__restrict__ bits, cpm_soft_params P)
{
    __shared__ __attribute__((aligned(16))) char smem[CS_WAVES * CS_WAVE_BYTES_AP];
    __shared__ double ring_all[CS_WAVES * CS_SUB * 64];       // ã (of inc') of the sub-block, lane-private columns
    __shared__ double rot[2 * CPM_ROT_SIN];
    cs_llr_body<M, LP, true>(smem, ring_all, rot, rows, rot_cs, bedge, ckpt, ext, bits, P, prior);
}

// ---- host side ------------------------------------------------------------------------------------------------------
template <int M, int LP>
static int cs_ap_run(wf_ctx *ctx, const cpm_soft_params &P, const cs_geom &g, const double2 *rows, const double2 *rot, const cpm_soft_prior &pr,
                     double *ext, uint8_t *bits, hipStream_t s)
{
    uint64_t *fedge = reinterpret_cast<uint64_t *>(ctx->d_vit_edge), *bedge = fedge + g.off_b;
    double *ckpt = ctx->d_vit_edge + g.off_ck;
    const unsigned grid = (unsigned)((g.nch + CS_WAVES - 1) / CS_WAVES);
    hipLaunchKernelGGL((cpm_soft_ap_bounds_kernel<M, LP>), dim3(grid), dim3(CS_THREADS), 0, s, rows, rot, pr, fedge, bedge, ckpt, P);
    WF_LAUNCH_CHECK();
    if (g.nch > 1) {
        // verify and list, two parallel repair rounds and the finisher, or count only: as wf_cpm_soft.hip (cs_run)
        const int repair = ctx->opt[WF_OPT_DET_REPAIR] == 0 ? 1 : 0;
        const dim3 vgrid((unsigned)(((g.nch - 1) * 64 + 255) / 256));
        for (int dir = 0; dir < 2; ++dir) {
            uint64_t *edge = dir ? bedge : fedge;
            hipLaunchKernelGGL(cpm_soft_ap_verify_kernel, vgrid, dim3(256), 0, s, edge, g.nch, P.S, ctx->d_vit_unmerged, repair);
            WF_LAUNCH_CHECK();
            if (!repair) continue;
            for (int round = 0; round < 3; ++round) {
                const dim3 rgrid(round < 2 ? CPM_REPAIR_BLOCKS : 1);
                if (dir)
                    hipLaunchKernelGGL((cpm_soft_ap_repair_kernel<M, LP, true>), rgrid, dim3(CS_THREADS), 0, s, rows, rot, pr, edge, ckpt,
                                       ctx->d_vit_unmerged, P, round, round + 1, round == 2 ? 1 : 0);
                else
                    hipLaunchKernelGGL((cpm_soft_ap_repair_kernel<M, LP, false>), rgrid, dim3(CS_THREADS), 0, s, rows, rot, pr, edge, ckpt,
                                       ctx->d_vit_unmerged, P, round, round + 1, round == 2 ? 1 : 0);
                WF_LAUNCH_CHECK();
            }
            if (ctx->opt[WF_OPT_DET_FINAL_VERIFY]) {
                hipLaunchKernelGGL(cpm_soft_ap_verify_kernel, vgrid, dim3(256), 0, s, edge, g.nch, P.S, ctx->d_vit_unmerged, 0);
                WF_LAUNCH_CHECK();
            }
        }
    }
    hipLaunchKernelGGL((cpm_soft_ap_llr_kernel<M, LP>), dim3(grid), dim3(CS_THREADS), 0, s, rows, rot, pr, bedge, ckpt, ext, bits, P);
    WF_LAUNCH_CHECK();
    return WF_OK;
}

extern "C" int wf_cpm_soft_apriori(wf_ctx *ctx, const wf_cpm_detector_config *det, const double *d_rot_cs, const double *d_rows_ri,
                                   int64_t ncalls, int64_t first_call, int warmup, const float *d_apriori, double apriori_scale,
                                   double *d_ext, uint8_t *d_bits, void *stream)
{
    WF_REQUIRE(ctx && det && d_rot_cs && d_rows_ri && d_ext && d_bits, "wf_cpm_soft_apriori: NULL argument");
    WF_REQUIRE(ncalls >= 1 && first_call >= 0 && warmup >= 0, "wf_cpm_soft_apriori: bad argument (ncalls %lld, first_call %lld, warmup %d)",
               (long long)ncalls, (long long)first_call, warmup);
    WF_REQUIRE(std::isfinite(apriori_scale), "wf_cpm_soft_apriori: apriori_scale must be finite");
    int rc = cs_check(det, "wf_cpm_soft_apriori");
    if (rc) return rc;
    WF_REQUIRE((reinterpret_cast<uintptr_t>(d_rows_ri) & 15) == 0 && (reinterpret_cast<uintptr_t>(d_rot_cs) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(d_ext) & 7) == 0 && (reinterpret_cast<uintptr_t>(d_apriori) & 3) == 0,
               "wf_cpm_soft_apriori: rows and rotation table must be 16-byte, ext 8-byte and the prior 4-byte aligned");
    if (!d_apriori)            // π = 0: the plain detector (bitwise: ã + (inc + 0) = ã + inc, since ã is never -0)
        return wf_cpm_soft(ctx, det, d_rot_cs, d_rows_ri, ncalls, first_call, warmup, d_ext, d_bits, stream);
    const cs_geom g = cs_geometry(ctx, cs_states(det), ncalls, warmup);
    WF_REQUIRE((g.nch + CS_WAVES - 1) / CS_WAVES < (1ll << 31), "wf_cpm_soft_apriori: burst too long for one launch");
    cpm_soft_params P{};
    cs_fill_params(det, g, ncalls, first_call, P);
    WF_HIP(hipSetDevice(ctx->device));
    rc = wf_ctx_reserve_vit(ctx, g.words);
    if (rc) return rc;
    hipStream_t s = wf_stream(stream);
    const double2 *rows = reinterpret_cast<const double2 *>(d_rows_ri), *rot = reinterpret_cast<const double2 *>(d_rot_cs);
    const cpm_soft_prior pr{d_apriori, apriori_scale};
    if (P.M == 4)
        return P.Lp == 1 ? cs_ap_run<4, 1>(ctx, P, g, rows, rot, pr, d_ext, d_bits, s)
                         : (P.Lp == 2 ? cs_ap_run<4, 2>(ctx, P, g, rows, rot, pr, d_ext, d_bits, s)
                                      : cs_ap_run<4, 3>(ctx, P, g, rows, rot, pr, d_ext, d_bits, s));
    return P.Lp == 1 ? cs_ap_run<2, 1>(ctx, P, g, rows, rot, pr, d_ext, d_bits, s)
                     : (P.Lp == 2 ? cs_ap_run<2, 2>(ctx, P, g, rows, rot, pr, d_ext, d_bits, s)
                                  : cs_ap_run<2, 3>(ctx, P, g, rows, rot, pr, d_ext, d_bits, s));
}
