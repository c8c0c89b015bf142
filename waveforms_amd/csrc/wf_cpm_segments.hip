// wf_cpm_segments.hip — the plain max-log-MAP CPM detector with branches (wf_cpm_soft_branch) over INDEPENDENT SEGMENTS in one
// set of launches (include/wfhip.h: wf_cpm_soft_branch_segments).  A joint carrier and timing search detects one set of rows
// under Hc rotation tables, and three sets of rows under one; as bursts that is up to ten launches of a few dozen waves each
// per detection, as segments of one launch set it is the same ten launches of nseg times the waves.
//
// The device bodies are wf_cpm_soft.h's with SEG: every segment is cut into cps = ceil(seglen / ch) chunks from its own start,
// chunk c of the launch is (segment c / cps, index c % cps) (cs_find), and a wave counts its calls from its segment's start
// with the segment's length as the burst's - so no chunk crosses a segment, no warm-up leaves one, and a segment's first and
// last chunk start from zero metrics exactly as a burst's do.  The proof chain of either direction skips the records
// r % cps == 0 (the chunks at their segment's edge; the backward records are mirrored over the whole launch, and the launch
// holds nseg cps chunks), so it never compares or repairs across two segments; every other chunk start is proven or repaired.
// A segment's result is therefore the definition (wf_cpm_soft.hip) for its rows, its table and first_call alone, bitwise,
// whatever the chunk length and the warm-up.
//
// The rotation table: the waves of a workgroup may belong to different segments, so each wave stages its own segment's table
// into its own 2 KB of LDS (cs_stage_rot_wave), and a repair wave stages the table of each record it takes.
#include "wf_cpm_soft.h"

template <int M, int LP>
__global__ __launch_bounds__(CS_THREADS) void cpm_seg_bounds_kernel(const double2 *__restrict__ rows, const double2 *__restrict__ rot_cs,
                                                                    uint64_t *__restrict__ fedge, uint64_t *__restrict__ bedge,
                                                                    double *__restrict__ ckpt, cpm_soft_params P)
{
    __shared__ __attribute__((aligned(16))) char smem[CS_WAVES * CS_WAVE_BYTES];
    __shared__ double rot[CS_WAVES * 2 * CPM_ROT_SIN];
    cs_bounds_body<M, LP, false, true>(smem, rot, rows, rot_cs, fedge, bedge, ckpt, P, cpm_soft_prior{nullptr, 0.0});
}

__global__ void cpm_seg_verify_kernel(uint64_t *__restrict__ edge, int64_t nch, int S, unsigned long long *__restrict__ unmerged, int repair, int cps)
{
    cs_verify_body(edge, nch, S, unmerged, repair, cps);
}

template <int M, int LP, bool BWD>
__global__ __launch_bounds__(CS_THREADS) void cpm_seg_repair_kernel(const double2 *__restrict__ rows, const double2 *__restrict__ rot_cs,
                                                                    uint64_t *__restrict__ edge, double *__restrict__ ckpt,
                                                                    unsigned long long *__restrict__ unmerged, cpm_soft_params P, int lin,
                                                                    int lout, int finisher)
{
    __shared__ __attribute__((aligned(16))) char smem[CS_WAVES * CS_WAVE_BYTES];
    __shared__ double rot[CS_WAVES * 2 * CPM_ROT_SIN];
    cs_repair_body<M, LP, BWD, false, true>(smem, rot, rows, rot_cs, edge, ckpt, unmerged, P, cpm_soft_prior{nullptr, 0.0}, lin, lout, finisher);
}

template <int M, int LP>
__global__ __launch_bounds__(CS_THREADS) void cpm_seg_llr_kernel(const double2 *__restrict__ rows, const double2 *__restrict__ rot_cs,
                                                                 const uint64_t *__restrict__ bedge, const double *__restrict__ ckpt,
                                                                 double *__restrict__ llr, uint8_t *__restrict__ bits,
                                                                 uint8_t *__restrict__ branch, double2 *__restrict__ term, cpm_soft_params P)
{
    __shared__ __attribute__((aligned(16))) char smem[CS_WAVES * CS_WAVE_BYTES];
    __shared__ double ring_all[CS_WAVES * CS_SUB * 64];       // ã of the sub-block, lane-private columns
    __shared__ double rot[CS_WAVES * 2 * CPM_ROT_SIN];
    cs_llr_body<M, LP, false, true, true>(smem, ring_all, rot, rows, rot_cs, bedge, ckpt, llr, bits, P, cpm_soft_prior{nullptr, 0.0}, branch, term);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
struct cseg_out {
    double *llr;
    uint8_t *bits, *branch;
    double2 *term;
};

template <int M, int LP>
static int cseg_run(wf_ctx *ctx, const cpm_soft_params &P, const cs_geom &g, const double2 *rows, const double2 *rot, const cseg_out &o, hipStream_t s)
{
    uint64_t *fedge = reinterpret_cast<uint64_t *>(ctx->d_vit_edge), *bedge = fedge + g.off_b;
    double *ckpt = ctx->d_vit_edge + g.off_ck;
    const unsigned grid = (unsigned)((g.nch + CS_WAVES - 1) / CS_WAVES);
    hipLaunchKernelGGL((cpm_seg_bounds_kernel<M, LP>), dim3(grid), dim3(CS_THREADS), 0, s, rows, rot, fedge, bedge, ckpt, P);
    WF_LAUNCH_CHECK();
    if (P.cps > 1) {
        const dim3 vgrid((unsigned)(((g.nch - 1) * 64 + 255) / 256));
        const int rc = cs_proof_passes(
            ctx,
            [&](int dir, int repair) {
                hipLaunchKernelGGL(cpm_seg_verify_kernel, vgrid, dim3(256), 0, s, dir ? bedge : fedge, g.nch, P.S, ctx->d_vit_unmerged, repair, P.cps);
            },
            [&](int dir, int round, unsigned blocks, int finisher) {
                if (dir)
                    hipLaunchKernelGGL((cpm_seg_repair_kernel<M, LP, true>), dim3(blocks), dim3(CS_THREADS), 0, s, rows, rot, bedge, ckpt,
                                       ctx->d_vit_unmerged, P, round, round + 1, finisher);
                else
                    hipLaunchKernelGGL((cpm_seg_repair_kernel<M, LP, false>), dim3(blocks), dim3(CS_THREADS), 0, s, rows, rot, fedge, ckpt,
                                       ctx->d_vit_unmerged, P, round, round + 1, finisher);
            });
        if (rc) return rc;
    }
    hipLaunchKernelGGL((cpm_seg_llr_kernel<M, LP>), dim3(grid), dim3(CS_THREADS), 0, s, rows, rot, bedge, ckpt, o.llr, o.bits, o.branch, o.term, P);
    WF_LAUNCH_CHECK();
    return WF_OK;
}

// the chunk length of a burst of nseg seglen calls, cps chunks per segment, and the scratch of the nseg cps chunks
static cs_geom cseg_geometry(const wf_ctx *ctx, int S, int64_t nseg, int64_t seglen, int warmup, int64_t *cps)
{
    cs_geom g = cs_geometry(ctx, S, nseg * seglen, warmup);
    *cps = (seglen + g.ch - 1) / g.ch;
    g.nch = nseg * *cps;
    cs_layout(g, S);
    return g;
}

static int cseg_check_shape(const char *who, int64_t nseg, int64_t seglen, int warmup)
{
    WF_REQUIRE(nseg >= 1 && nseg <= ((int64_t)1 << 20), "%s: nseg = %lld outside 1 .. 2^20", who, (long long)nseg);
    WF_REQUIRE(seglen >= 1 && seglen <= ((int64_t)1 << 40) / nseg, "%s: seglen = %lld outside 1 .. 2^40 / nseg", who, (long long)seglen);
    WF_REQUIRE(warmup >= 0, "%s: warmup = %d", who, warmup);
    return WF_OK;
}

extern "C" int wf_cpm_soft_segments_geometry(wf_ctx *ctx, const wf_cpm_detector_config *det, int64_t nseg, int64_t seglen, int warmup, int64_t *h_geom)
{
    static const char who[] = "wf_cpm_soft_segments_geometry";
    WF_REQUIRE(ctx && det && h_geom, "%s: NULL argument", who);
    int rc = cseg_check_shape(who, nseg, seglen, warmup);
    if (rc) return rc;
    rc = cs_check(det, who);
    if (rc) return rc;
    int64_t cps;
    const cs_geom g = cseg_geometry(ctx, cs_states(det), nseg, seglen, warmup, &cps);
    h_geom[0] = g.ch;
    h_geom[1] = g.nch;
    h_geom[2] = g.W;
    h_geom[3] = (int64_t)(g.words * sizeof(double));
    h_geom[4] = cps;
    return WF_OK;
}

extern "C" int wf_cpm_soft_branch_segments(wf_ctx *ctx, const wf_cpm_detector_config *det, const double *d_rot_cs, int64_t rot_stride,
                                           const double *d_rows_ri, int64_t nseg, int64_t seglen, int64_t row_stride, int64_t out_stride,
                                           int64_t first_call, int warmup, double *d_llr, uint8_t *d_bits, uint8_t *d_branch, double *d_term,
                                           void *stream)
{
    static const char who[] = "wf_cpm_soft_branch_segments";
    WF_REQUIRE(ctx && det && d_rot_cs && d_rows_ri && d_llr && d_bits && d_branch, "%s: NULL argument", who);
    int rc = cseg_check_shape(who, nseg, seglen, warmup);
    if (rc) return rc;
    WF_REQUIRE(first_call >= 0, "%s: first_call = %lld", who, (long long)first_call);
    WF_REQUIRE(row_stride == 0 || (row_stride >= seglen && row_stride <= ((int64_t)1 << 40) / nseg), "%s: row_stride = %lld: 0, or seglen .. 2^40 / nseg",
               who, (long long)row_stride);
    WF_REQUIRE(rot_stride == 0 || rot_stride == 1, "%s: rot_stride = %lld (0 or 1)", who, (long long)rot_stride);
    WF_REQUIRE(out_stride >= seglen && out_stride % 64 == 0 && out_stride <= ((int64_t)1 << 40) / nseg,
               "%s: out_stride must be a multiple of 64, at least seglen, and nseg out_stride at most 2^40", who);
    rc = cs_check(det, who);
    if (rc) return rc;
    WF_REQUIRE((reinterpret_cast<uintptr_t>(d_rows_ri) & 15) == 0 && (reinterpret_cast<uintptr_t>(d_rot_cs) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(d_llr) & 7) == 0 && (reinterpret_cast<uintptr_t>(d_term) & 15) == 0,
               "%s: rows, rotation tables and terms must be 16-byte, llr 8-byte aligned", who);
    int64_t cps;
    const cs_geom g = cseg_geometry(ctx, cs_states(det), nseg, seglen, warmup, &cps);
    WF_REQUIRE(g.nch < (1ll << 31), "%s: too many chunks for one launch", who);
    cpm_soft_params P{};
    cs_fill_params(det, g, seglen, first_call, P);
    int nf = 1;
    for (int i = 0; i < det->Lp; ++i) nf *= det->M;
    P.cps = (int)cps;
    P.row_stride = row_stride * nf;             // in double2: a row is M^Lp of them
    P.rot_stride = (int)rot_stride * 2 * det->p;
    P.out_stride = out_stride;
    WF_HIP(hipSetDevice(ctx->device));
    rc = wf_ctx_reserve_vit(ctx, g.words);
    if (rc) return rc;
    hipStream_t s = wf_stream(stream);
    const double2 *rows = reinterpret_cast<const double2 *>(d_rows_ri), *rot = reinterpret_cast<const double2 *>(d_rot_cs);
    const cseg_out o{d_llr, d_bits, d_branch, reinterpret_cast<double2 *>(d_term)};
    if (P.M == 4)
        return P.Lp == 1 ? cseg_run<4, 1>(ctx, P, g, rows, rot, o, s) : (P.Lp == 2 ? cseg_run<4, 2>(ctx, P, g, rows, rot, o, s) : cseg_run<4, 3>(ctx, P, g, rows, rot, o, s));
    return P.Lp == 1 ? cseg_run<2, 1>(ctx, P, g, rows, rot, o, s) : (P.Lp == 2 ? cseg_run<2, 2>(ctx, P, g, rows, rot, o, s) : cseg_run<2, 3>(ctx, P, g, rows, rot, o, s));
}
