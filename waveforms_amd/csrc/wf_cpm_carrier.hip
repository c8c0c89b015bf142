// wf_cpm_carrier.hip — wf_cpm_soft_branch: wf_cpm_soft with the decided branch and its phase term per call, the detector
// pass of the carrier recovery for ARTM and PCM/FM (waveforms_amd/sync/carrier_cpm.py).  Definition: include/wfhip.h.
//
// The bounds, proof and repair launches are wf_cpm_soft's own (cpm_soft_front, wf_cpm_soft.hip); only the last launch is
// this file's: cs_llr_body with BR, which adds to each call's λ step the argmin over the 64 lanes (wf_cpm_soft.h, cs_llr) and,
// from the one lane that holds it, a 1-byte and a 16-byte store.  A coarse hypothesis needs no kernel of its own: it is
// this entry point with a rotated table d_rot_cs.  The other stages of the recovery (wf_carrier_stat_terms,
// wf_carrier_track_mod, wf_rows_derotate_n) live with their SOQPSK forms in wf_carrier.hip.
#include "wf_cpm_soft.h"

template <int M, int LP>
__global__ __launch_bounds__(CS_THREADS) void cpm_soft_branch_llr_kernel(const double2 *__restrict__ rows, const double2 *__restrict__ rot_cs,
                                                                         const uint64_t *__restrict__ bedge, const double *__restrict__ ckpt,
                                                                         double *__restrict__ llr, uint8_t *__restrict__ bits,
                                                                         uint8_t *__restrict__ branch, double2 *__restrict__ term, cpm_soft_params P)
{
    __shared__ __attribute__((aligned(16))) char smem[CS_WAVES * CS_WAVE_BYTES];
    __shared__ double ring_all[CS_WAVES * CS_SUB * 64];       // ã of the sub-block, lane-private columns
    __shared__ double rot[2 * CPM_ROT_SIN];
    cs_llr_body<M, LP, false, true>(smem, ring_all, rot, rows, rot_cs, bedge, ckpt, llr, bits, P, cpm_soft_prior{nullptr, 0.0}, branch, term);
}

template <int M, int LP>
static int csb_last(wf_ctx *ctx, const cpm_soft_params &P, const cs_geom &g, const double2 *rows, const double2 *rot, double *llr, uint8_t *bits,
                    uint8_t *branch, double2 *term, hipStream_t s)
{
    hipLaunchKernelGGL((cpm_soft_branch_llr_kernel<M, LP>), dim3((unsigned)((g.nch + CS_WAVES - 1) / CS_WAVES)), dim3(CS_THREADS), 0, s, rows, rot,
                       reinterpret_cast<const uint64_t *>(ctx->d_vit_edge) + g.off_b, ctx->d_vit_edge + g.off_ck, llr, bits, branch, term, P);
    WF_LAUNCH_CHECK();
    return WF_OK;
}

extern "C" int wf_cpm_soft_branch(wf_ctx *ctx, const wf_cpm_detector_config *det, const double *d_rot_cs, const double *d_rows_ri, int64_t ncalls,
                                  int64_t first_call, int warmup, double *d_llr, uint8_t *d_bits, uint8_t *d_branch, double *d_term, void *stream)
{
    static const char who[] = "wf_cpm_soft_branch";
    WF_REQUIRE(ctx && det && d_rot_cs && d_rows_ri && d_llr && d_bits && d_branch, "%s: NULL argument", who);
    WF_REQUIRE(ncalls >= 1 && first_call >= 0 && warmup >= 0, "%s: bad argument (ncalls %lld, first_call %lld, warmup %d)", who, (long long)ncalls,
               (long long)first_call, warmup);
    int rc = cs_check(det, who);
    if (rc) return rc;
    WF_REQUIRE((reinterpret_cast<uintptr_t>(d_rows_ri) & 15) == 0 && (reinterpret_cast<uintptr_t>(d_rot_cs) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(d_llr) & 7) == 0 && (reinterpret_cast<uintptr_t>(d_term) & 15) == 0,
               "%s: rows, rotation table and terms must be 16-byte, llr 8-byte aligned", who);
    const cs_geom g = cs_geometry(ctx, cs_states(det), ncalls, warmup);
    WF_REQUIRE((g.nch + CS_WAVES - 1) / CS_WAVES < (1ll << 31), "%s: burst too long for one launch", who);
    cpm_soft_params P{};
    cs_fill_params(det, g, ncalls, first_call, P);
    WF_HIP(hipSetDevice(ctx->device));
    rc = wf_ctx_reserve_vit(ctx, g.words);
    if (rc) return rc;
    hipStream_t s = wf_stream(stream);
    const double2 *rows = reinterpret_cast<const double2 *>(d_rows_ri), *rot = reinterpret_cast<const double2 *>(d_rot_cs);
    double2 *term = reinterpret_cast<double2 *>(d_term);
    rc = cpm_soft_front(ctx, P, g, rows, rot, s);
    if (rc) return rc;
    if (P.M == 4)
        return P.Lp == 1 ? csb_last<4, 1>(ctx, P, g, rows, rot, d_llr, d_bits, d_branch, term, s)
                         : (P.Lp == 2 ? csb_last<4, 2>(ctx, P, g, rows, rot, d_llr, d_bits, d_branch, term, s)
                                      : csb_last<4, 3>(ctx, P, g, rows, rot, d_llr, d_bits, d_branch, term, s));
    return P.Lp == 1 ? csb_last<2, 1>(ctx, P, g, rows, rot, d_llr, d_bits, d_branch, term, s)
                     : (P.Lp == 2 ? csb_last<2, 2>(ctx, P, g, rows, rot, d_llr, d_bits, d_branch, term, s)
                                  : csb_last<2, 3>(ctx, P, g, rows, rot, d_llr, d_bits, d_branch, term, s));
}
