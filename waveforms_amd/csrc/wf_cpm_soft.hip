// wf_cpm_soft.hip — max-log-MAP soft output of the generic CPM trellis (ARTM multi-h, PCM/FM), per-bit LLRs.
//
// Definition: include/wfhip.h (wf_cpm_soft).  The trellis is cpm_oracle.c's with every phase state in it (NC = p): state
// s = v + p c, v the phase index, c the Lp - 1 previous symbols.  The shipped reduced designs (ARTM_16: NC 4 of p 16,
// PCMFM_10: NC 5 of p 10) carry the phase index per SURVIVOR, which a backward recursion has no survivor to carry; on the
// full-phase trellis every branch's increment and end state follow from the state alone, so forward and backward are plain
// min-sum recursions over the same matched filters (ARTM: the 64 states of ARTM_64, PCM/FM: 20 states).
//
// Lane = state, one wave = one chunk of `ch` consecutive calls (the layout of the hard wide form, wf_cpm_wide.hip), in
// three steps:
//   cpm_soft_bounds_kernel   forward: ã at the chunk start from zeros `warmup` calls earlier (exact for the chunks that
//                            reach call 0), then over the chunk's own calls, keeping ã every CS_SUB calls (checkpoints,
//                            in the context's scratch); backward, the mirror: b̃ at the chunk end from zeros `warmup`
//                            calls later (exact for the chunks that reach the burst's end), then back over the chunk.  Each
//                            direction records {start, end} per chunk; the backward records in MIRRORED chunk order
//                            (record r = chunk nch - 1 - r), so "a record's start is bitwise its predecessor's end" is the
//                            same check in both directions.
//   cpm_soft_verify_kernel + cpm_soft_repair_kernel, once per direction: the proof and cascading repair of the hard
//                            detectors (lists and rounds of wf_cpm_detect.h: two parallel rounds, then one workgroup that
//                            follows a chain to its end).  A forward repair rewrites the chunk's checkpoints too.
//   cpm_soft_llr_kernel      per sub-block of CS_SUB calls, the last first: ã again from its checkpoint into a wave-private
//                            LDS ring, then back over the sub-block from the proven b̃: λ from ã_k and b̃_{k+1}, then b̃_k.
// ã never goes through HBM: a 64-state ã is 512 B per call (5.1 GB written and read per 1e7 calls); the checkpoints are
// 1/CS_SUB of that, for one more forward recursion per call (DESIGN.md §4 has the measurement).
// Every metric is >= +0 and no sum is ever -0, so v_min_f64 and the normalisations are exact restatements of the definition
// in any order; the result is bitwise the definition whatever `warmup` and the chunking.
#include "wf_cpm_soft.h"

// The device code lives in wf_cpm_soft.h (shared with wf_cpm_soft_apriori.hip); these are its AP = false kernels.
template <int M, int LP>
__global__ __launch_bounds__(CS_THREADS) void cpm_soft_bounds_kernel(const double2 *__restrict__ rows, const double2 *__restrict__ rot_cs,
                                                                     uint64_t *__restrict__ fedge, uint64_t *__restrict__ bedge,
                                                                     double *__restrict__ ckpt, cpm_soft_params P)
{
    __shared__ __attribute__((aligned(16))) char smem[CS_WAVES * CS_WAVE_BYTES];
    __shared__ double rot[2 * CPM_ROT_SIN];
    cs_bounds_body<M, LP, false>(smem, rot, rows, rot_cs, fedge, bedge, ckpt, P, cpm_soft_prior{nullptr, 0.0});
}

__global__ void cpm_soft_verify_kernel(uint64_t *__restrict__ edge, int64_t nch, int S, unsigned long long *__restrict__ unmerged, int repair)
{
    cs_verify_body(edge, nch, S, unmerged, repair);
}

template <int M, int LP, bool BWD>
__global__ __launch_bounds__(CS_THREADS) void cpm_soft_repair_kernel(const double2 *__restrict__ rows, const double2 *__restrict__ rot_cs,
                                                                     uint64_t *__restrict__ edge, double *__restrict__ ckpt,
                                                                     unsigned long long *__restrict__ unmerged, cpm_soft_params P, int lin,
                                                                     int lout, int finisher)
{
    __shared__ __attribute__((aligned(16))) char smem[CS_WAVES * CS_WAVE_BYTES];
    __shared__ double rot[2 * CPM_ROT_SIN];
    cs_repair_body<M, LP, BWD, false>(smem, rot, rows, rot_cs, edge, ckpt, unmerged, P, cpm_soft_prior{nullptr, 0.0}, lin, lout, finisher);
}

template <int M, int LP>
__global__ __launch_bounds__(CS_THREADS) void cpm_soft_llr_kernel(const double2 *__restrict__ rows, const double2 *__restrict__ rot_cs,
                                                                  const uint64_t *__restrict__ bedge, const double *__restrict__ ckpt,
                                                                  double *__restrict__ llr, uint8_t *__restrict__ bits, cpm_soft_params P)
{
    __shared__ __attribute__((aligned(16))) char smem[CS_WAVES * CS_WAVE_BYTES];
    __shared__ double ring_all[CS_WAVES * CS_SUB * 64];       // ã of the sub-block, lane-private columns
    __shared__ double rot[2 * CPM_ROT_SIN];
    cs_llr_body<M, LP, false>(smem, ring_all, rot, rows, rot_cs, bedge, ckpt, llr, bits, P, cpm_soft_prior{nullptr, 0.0});
}

// ---- host side (geometry, checks and tables: wf_cpm_soft.h) -----------------------------------------------------------
extern "C" int wf_cpm_soft_geometry(wf_ctx *ctx, const wf_cpm_detector_config *det, int64_t ncalls, int warmup, int64_t *h_geom)
{
    WF_REQUIRE(ctx && det && h_geom, "wf_cpm_soft_geometry: NULL argument");
    WF_REQUIRE(ncalls >= 1 && warmup >= 0, "wf_cpm_soft_geometry: bad argument");
    const int rc = cs_check(det, "wf_cpm_soft_geometry");
    if (rc) return rc;
    const cs_geom g = cs_geometry(ctx, cs_states(det), ncalls, warmup);
    h_geom[0] = g.ch;
    h_geom[1] = g.nch;
    h_geom[2] = g.W;
    h_geom[3] = (int64_t)(g.words * sizeof(double));
    return WF_OK;
}

// every launch but the last: bounds, then proof and repairs in both directions
template <int M, int LP>
static int cs_front(wf_ctx *ctx, const cpm_soft_params &P, const cs_geom &g, const double2 *rows, const double2 *rot, hipStream_t s)
{
    uint64_t *fedge = reinterpret_cast<uint64_t *>(ctx->d_vit_edge), *bedge = fedge + g.off_b;
    double *ckpt = ctx->d_vit_edge + g.off_ck;
    const unsigned grid = (unsigned)((g.nch + CS_WAVES - 1) / CS_WAVES);
    hipLaunchKernelGGL((cpm_soft_bounds_kernel<M, LP>), dim3(grid), dim3(CS_THREADS), 0, s, rows, rot, fedge, bedge, ckpt, P);
    WF_LAUNCH_CHECK();
    if (g.nch > 1) {
        const dim3 vgrid((unsigned)(((g.nch - 1) * 64 + 255) / 256));
        return cs_proof_passes(
            ctx,
            [&](int dir, int repair) {
                hipLaunchKernelGGL(cpm_soft_verify_kernel, vgrid, dim3(256), 0, s, dir ? bedge : fedge, g.nch, P.S, ctx->d_vit_unmerged, repair);
            },
            [&](int dir, int round, unsigned blocks, int finisher) {
                if (dir)
                    hipLaunchKernelGGL((cpm_soft_repair_kernel<M, LP, true>), dim3(blocks), dim3(CS_THREADS), 0, s, rows, rot, bedge, ckpt,
                                       ctx->d_vit_unmerged, P, round, round + 1, finisher);
                else
                    hipLaunchKernelGGL((cpm_soft_repair_kernel<M, LP, false>), dim3(blocks), dim3(CS_THREADS), 0, s, rows, rot, fedge, ckpt,
                                       ctx->d_vit_unmerged, P, round, round + 1, finisher);
            });
    }
    return WF_OK;
}

// ... for the detectors whose last launch lives in another file (wf_cpm_carrier.hip: wf_cpm_soft_branch)
int cpm_soft_front(wf_ctx *ctx, const cpm_soft_params &P, const cs_geom &g, const double2 *rows, const double2 *rot, hipStream_t s)
{
    if (P.M == 4) return P.Lp == 1 ? cs_front<4, 1>(ctx, P, g, rows, rot, s) : (P.Lp == 2 ? cs_front<4, 2>(ctx, P, g, rows, rot, s) : cs_front<4, 3>(ctx, P, g, rows, rot, s));
    return P.Lp == 1 ? cs_front<2, 1>(ctx, P, g, rows, rot, s) : (P.Lp == 2 ? cs_front<2, 2>(ctx, P, g, rows, rot, s) : cs_front<2, 3>(ctx, P, g, rows, rot, s));
}

template <int M, int LP>
static int cs_run(wf_ctx *ctx, const cpm_soft_params &P, const cs_geom &g, const double2 *rows, const double2 *rot, double *llr, uint8_t *bits,
                  hipStream_t s)
{
    const int rc = cs_front<M, LP>(ctx, P, g, rows, rot, s);
    if (rc) return rc;
    hipLaunchKernelGGL((cpm_soft_llr_kernel<M, LP>), dim3((unsigned)((g.nch + CS_WAVES - 1) / CS_WAVES)), dim3(CS_THREADS), 0, s, rows, rot,
                       reinterpret_cast<const uint64_t *>(ctx->d_vit_edge) + g.off_b, ctx->d_vit_edge + g.off_ck, llr, bits, P);
    WF_LAUNCH_CHECK();
    return WF_OK;
}

extern "C" int wf_cpm_soft(wf_ctx *ctx, const wf_cpm_detector_config *det, const double *d_rot_cs, const double *d_rows_ri, int64_t ncalls,
                           int64_t first_call, int warmup, double *d_llr, uint8_t *d_bits, void *stream)
{
    WF_REQUIRE(ctx && det && d_rot_cs && d_rows_ri && d_llr && d_bits, "wf_cpm_soft: NULL argument");
    WF_REQUIRE(ncalls >= 1 && first_call >= 0 && warmup >= 0, "wf_cpm_soft: bad argument (ncalls %lld, first_call %lld, warmup %d)",
               (long long)ncalls, (long long)first_call, warmup);
    int rc = cs_check(det, "wf_cpm_soft");
    if (rc) return rc;
    WF_REQUIRE((reinterpret_cast<uintptr_t>(d_rows_ri) & 15) == 0 && (reinterpret_cast<uintptr_t>(d_rot_cs) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(d_llr) & 7) == 0,
               "wf_cpm_soft: rows and rotation table must be 16-byte, llr 8-byte aligned");
    const cs_geom g = cs_geometry(ctx, cs_states(det), ncalls, warmup);
    WF_REQUIRE((g.nch + CS_WAVES - 1) / CS_WAVES < (1ll << 31), "wf_cpm_soft: burst too long for one launch");
    cpm_soft_params P{};
    cs_fill_params(det, g, ncalls, first_call, P);
    WF_HIP(hipSetDevice(ctx->device));
    rc = wf_ctx_reserve_vit(ctx, g.words);
    if (rc) return rc;
    hipStream_t s = wf_stream(stream);
    const double2 *rows = reinterpret_cast<const double2 *>(d_rows_ri), *rot = reinterpret_cast<const double2 *>(d_rot_cs);
    if (P.M == 4)
        return P.Lp == 1 ? cs_run<4, 1>(ctx, P, g, rows, rot, d_llr, d_bits, s)
                         : (P.Lp == 2 ? cs_run<4, 2>(ctx, P, g, rows, rot, d_llr, d_bits, s) : cs_run<4, 3>(ctx, P, g, rows, rot, d_llr, d_bits, s));
    return P.Lp == 1 ? cs_run<2, 1>(ctx, P, g, rows, rot, d_llr, d_bits, s)
                     : (P.Lp == 2 ? cs_run<2, 2>(ctx, P, g, rows, rot, d_llr, d_bits, s) : cs_run<2, 3>(ctx, P, g, rows, rot, d_llr, d_bits, s));
}
