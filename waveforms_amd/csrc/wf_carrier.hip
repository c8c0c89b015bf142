// wf_carrier.hip — carrier phase and frequency: the impairment (wf_carrier_offset_c128) and the stages of the
// decision-directed recovery over windows of detector rows (wf_carrier_stat, wf_carrier_track, wf_rows_derotate, and their
// forms for the CPM detectors: wf_carrier_stat_terms, wf_carrier_track_mod, wf_rows_derotate_n — the same kernels).
// include/wfhip.h states every definition; waveforms_amd/sync/carrier.py restates them in numpy.  The reference has no
// synchroniser: these are the build's own.  The branch decisions come from wf_viterbi4_soft_branch (wf_viterbi_soft.hip).
//
//   carrier_offset_kernel   elementwise, 16 B in / 16 B out per sample; the turn count nu (first_index + k) is reduced to
//                           its fraction in float64 before the multiply by 2π, one fp64 sincos per sample.
//   carrier_stat_kernel     one WAVE per window of W rows: lane l adds the rows wW + 64 i + l (i increasing), so a wave's
//                           loads are one row apart across lanes; the 64 partials are folded by a shuffle-down butterfly
//                           (d = 32 .. 1, wf_sync.h) in the order the header states.  ONE body for both statistics: the
//                           row's term comes from a fetch.  q = state_exp_term[start] z[idx] is a signed pick of z's
//                           components (no product, nothing rounded but the sums), or the term wf_cpm_soft_branch wrote.
//   carrier_track_kernel    ONE workgroup: per window the best hypothesis and its phase (threads in parallel), the
//                           unwrapping modulo the period (π, or 2π/p for CPM) as a blocked scan (a segment of windows per thread, the 1024 segment sums
//                           added in order: the definition's running sum to rounding), the centred mean (threads in
//                           parallel).  The unwrapped phases pass through the context's detector scratch.  The argmin, the
//                           scan and the mean are wf_sync.h's, shared with timing_track_kernel.
//   rows_derotate_kernel    a thread per row of nvals values (3: the 48-byte rows; 4 / 16: PCM/FM / ARTM): one fp64 sincos a row;
//                           the row's phase is wf_sync.h's trajectory value, the rotation its sync_rotate.
//
// The phase arithmetic is written one operation per statement where the host statement must see the same roundings
// (-ffp-contract=on fuses within an expression only).
#include "wf_sync.h"
#include "wf_viterbi4.h"

#include <cmath>

#define CARRIER_THREADS 256
#define CARRIER_WAVES (CARRIER_THREADS / WF_WAVE)
#define TRACK_THREADS 1024          // carrier_track_kernel: ONE workgroup, as wide as a workgroup gets (its loops are latency-bound)
static constexpr double kCarrierTwoPi = kSyncTwoPi;
static constexpr double kCarrierPi = 3.14159265358979323846;

__global__ __launch_bounds__(CARRIER_THREADS) void carrier_offset_kernel(const double2 *in, int64_t n, double theta0, double nu, int64_t first_index,
                                                                         double2 *out)
{
    for (int64_t k = (int64_t)blockIdx.x * CARRIER_THREADS + threadIdx.x; k < n; k += (int64_t)gridDim.x * CARRIER_THREADS) {
        out[k] = sync_carrier_turn(in[k], theta0, nu, first_index + k);
    }
}

// (x, y) of q = state_exp_term[start] * z, state_exp_term = [+j, -1, +1, -j]
__device__ __forceinline__ double2 carrier_q(int start, double2 z)
{
    return start == 0 ? make_double2(-z.y, z.x) : start == 1 ? make_double2(-z.x, -z.y) : start == 2 ? z : make_double2(z.y, -z.x);
}

// a row's term q_k = (x, y) formed from the row and its decided branch
struct carrier_term_of_rows {
    const double *__restrict__ rows;
    const uint8_t *__restrict__ branch;
    __device__ __forceinline__ double2 operator()(int64_t k) const
    {
        const int b = branch[k] & 7;
        const double2 z = reinterpret_cast<const double2 *>(rows)[3 * k + br_out_idx((int)(k & 1), b)];
        return carrier_q(b >> 1, z);
    }
};

// the same term as wf_cpm_soft_branch wrote it: q_k = (x_k, y_k) is read, not formed
struct carrier_term_read {
    const double2 *__restrict__ term;
    __device__ __forceinline__ double2 operator()(int64_t k) const { return term[k]; }
};

template <class FETCH>
__global__ __launch_bounds__(CARRIER_THREADS) void carrier_stat_kernel(const FETCH fetch, int64_t n, int W, int64_t nwin, double *__restrict__ stat)
{
    const int64_t w = (int64_t)blockIdx.x * CARRIER_WAVES + threadIdx.x / WF_WAVE;      // wave-uniform
    if (w >= nwin) return;
    const int lane = wf_lane();
    double px = 0.0, py = 0.0;
    for (int i = 0; i < W / WF_WAVE; ++i) {
        const int64_t k = w * W + (int64_t)i * WF_WAVE + lane;
        if (k < n) {
            const double2 q = fetch(k);
            px += q.x;
            py += q.y;
        }
    }
    px = sync_wave_fold(px);
    py = sync_wave_fold(py);
    if (lane == 0) {
        stat[2 * w] = px;
        stat[2 * w + 1] = py;
    }
}

__device__ __forceinline__ double carrier_psi(const double *stat, int H, int64_t nwin, double period, int64_t w, uint8_t *choice)
{
    double bx;
    const int best = sync_argmin(stat, H, nwin, w, &bx);
    if (choice) choice[w] = (uint8_t)best;
    const double by = stat[2 * ((int64_t)best * nwin + w) + 1];
    const double base = (double)best * period;
    const double off = base / (double)H;
    const double at = atan2(-by, -bx);
    return off + at;
}

__global__ __launch_bounds__(TRACK_THREADS) void carrier_track_kernel(const double *__restrict__ stat, int H, int64_t nwin, int span, double period, double *tmp,
                                                                        double *__restrict__ phase, uint8_t *__restrict__ choice)
{
    __shared__ double s_seg[TRACK_THREADS];
    for (int64_t w = threadIdx.x; w < nwin; w += TRACK_THREADS) tmp[w] = carrier_psi(stat, H, nwin, period, w, choice);      // ψ_w, once per window
    __syncthreads();
    sync_unwrap_scan<TRACK_THREADS>(tmp, nwin, period, s_seg);
    sync_centred_mean<TRACK_THREADS>(tmp, nwin, span, phase);
}

// The anchored track (wf_sync.h): the drift search over (segments, candidates), then the one workgroup behind it
struct carrier_psi_of {
    const double *stat;
    int H;
    int64_t nwin;
    double period;
    uint8_t *choice;
    __device__ __forceinline__ double operator()(int64_t w, bool keep) const { return carrier_psi(stat, H, nwin, period, w, keep ? choice : nullptr); }
};

__global__ __launch_bounds__(ANCHOR_THREADS) void carrier_anchor_score_kernel(carrier_psi_of psi_of, int K, int n, double *psi, double2 *z, double *score)
{
    __shared__ double2 s_z[ANCHOR_MAX_K];
    sync_anchor_score<ANCHOR_THREADS>(psi_of, psi_of.nwin, psi_of.period, K, n, psi, z, score, s_z);
}

__global__ __launch_bounds__(TRACK_THREADS) void carrier_anchor_tail_kernel(int64_t nwin, int span, double period, double reject, int K, int n, int64_t nseg,
                                                                            double *psi, double2 *z, double *alpha, const double *score,
                                                                            double *__restrict__ phase, double *__restrict__ drift, uint8_t *__restrict__ marks)
{
    __shared__ double s_seg[TRACK_THREADS];
    __shared__ int s_idx[TRACK_THREADS];
    sync_anchor_tail<TRACK_THREADS>(nwin, span, period, reject, K, n, nseg, psi, z, alpha, score, phase, drift, marks, s_seg, s_idx);
}

__global__ __launch_bounds__(CARRIER_THREADS) void rows_derotate_kernel(const double2 *rows, int64_t n, int nvals, int W, const double *__restrict__ phase,
                                                                        int64_t nwin, double phase0, double2 *out)
{
    for (int64_t k = (int64_t)blockIdx.x * CARRIER_THREADS + threadIdx.x; k < n; k += (int64_t)gridDim.x * CARRIER_THREADS) {
        const double phi = phase ? sync_traj_at(phase, nwin, W, k) : 0.0;
        const double tot = phase0 + phi;
        double sn, cs;
        sincos(-tot, &sn, &cs);
        for (int j = 0; j < nvals; ++j) out[(int64_t)nvals * k + j] = sync_rotate(rows[(int64_t)nvals * k + j], cs, sn);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
extern "C" int wf_carrier_offset_c128(wf_ctx *ctx, const double *d_in_ri, int64_t n, double theta0, double nu, int64_t first_index, double *d_out_ri,
                                      void *stream)
{
    WF_REQUIRE(ctx && d_in_ri && d_out_ri, "wf_carrier_offset_c128: NULL argument");
    WF_REQUIRE(n >= 1 && first_index >= 0 && n <= ((int64_t)1 << 53) - first_index, "wf_carrier_offset_c128: n must be at least 1 and first_index + n at most 2^53");
    WF_REQUIRE(std::isfinite(theta0) && std::isfinite(nu), "wf_carrier_offset_c128: theta0 and nu must be finite");
    WF_REQUIRE(!sync_mis(d_in_ri, 15) && !sync_mis(d_out_ri, 15), "wf_carrier_offset_c128: samples must be 16-byte aligned");
    WF_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(carrier_offset_kernel, dim3(wf_grid_for(n, CARRIER_THREADS, 1 << 16)), dim3(CARRIER_THREADS), 0, wf_stream(stream),
                       reinterpret_cast<const double2 *>(d_in_ri), n, theta0, nu, first_index, reinterpret_cast<double2 *>(d_out_ri));
    WF_LAUNCH_CHECK();
    return WF_OK;
}

extern "C" int wf_carrier_stat(wf_ctx *ctx, const double *d_rows, const uint8_t *d_branch, int64_t ncalls, int W, double *d_stat, void *stream)
{
    WF_REQUIRE(ctx && d_rows && d_branch && d_stat, "wf_carrier_stat: NULL argument");
    WF_REQUIRE(ncalls >= 1, "wf_carrier_stat: ncalls must be at least 1");
    WF_REQUIRE(sync_window_ok(W), "wf_carrier_stat: W must be a multiple of 64 from 64 to 8192");
    WF_REQUIRE(!sync_mis(d_rows, 15) && !sync_mis(d_stat, 7), "wf_carrier_stat: rows must be 16-byte and stat 8-byte aligned");
    const int64_t nwin = (ncalls + W - 1) / W;
    WF_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(carrier_stat_kernel<carrier_term_of_rows>, dim3((unsigned)((nwin + CARRIER_WAVES - 1) / CARRIER_WAVES)), dim3(CARRIER_THREADS), 0,
                       wf_stream(stream), carrier_term_of_rows{d_rows, d_branch}, ncalls, W, nwin, d_stat);
    WF_LAUNCH_CHECK();
    return WF_OK;
}

extern "C" int wf_carrier_stat_terms(wf_ctx *ctx, const double *d_term, int64_t ncalls, int W, double *d_stat, void *stream)
{
    WF_REQUIRE(ctx && d_term && d_stat, "wf_carrier_stat_terms: NULL argument");
    WF_REQUIRE(ncalls >= 1, "wf_carrier_stat_terms: ncalls must be at least 1");
    WF_REQUIRE(sync_window_ok(W), "wf_carrier_stat_terms: W must be a multiple of 64 from 64 to 8192");
    WF_REQUIRE(!sync_mis(d_term, 15) && !sync_mis(d_stat, 7), "wf_carrier_stat_terms: terms must be 16-byte and stat 8-byte aligned");
    const int64_t nwin = (ncalls + W - 1) / W;
    WF_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(carrier_stat_kernel<carrier_term_read>, dim3((unsigned)((nwin + CARRIER_WAVES - 1) / CARRIER_WAVES)), dim3(CARRIER_THREADS), 0,
                       wf_stream(stream), carrier_term_read{reinterpret_cast<const double2 *>(d_term)}, ncalls, W, nwin, d_stat);
    WF_LAUNCH_CHECK();
    return WF_OK;
}

static int carrier_track_run(const char *who, wf_ctx *ctx, const double *d_stat_h, int H, int64_t nwin, int span, double period, double *d_phase,
                             uint8_t *d_choice, void *stream)
{
    WF_REQUIRE(ctx && d_stat_h && d_phase && d_choice, "%s: NULL argument", who);
    WF_REQUIRE(H >= 1 && H <= 256, "%s: H must be 1 .. 256", who);
    WF_REQUIRE(nwin >= 1 && nwin <= ((int64_t)1 << 40), "%s: nwin must be at least 1", who);
    WF_REQUIRE(span >= 1 && span % 2 == 1, "%s: span must be odd and at least 1", who);
    WF_REQUIRE(std::isfinite(period) && period > 0.0 && period <= kCarrierTwoPi, "%s: period must be in (0, 2 pi]", who);
    WF_REQUIRE(!sync_mis(d_stat_h, 7) && !sync_mis(d_phase, 7), "%s: stat and phase must be 8-byte aligned", who);
    WF_HIP(hipSetDevice(ctx->device));
    const int rc = wf_ctx_reserve_vit(ctx, (size_t)nwin);
    if (rc) return rc;
    hipLaunchKernelGGL(carrier_track_kernel, dim3(1), dim3(TRACK_THREADS), 0, wf_stream(stream), d_stat_h, H, nwin, span, period, ctx->d_vit_edge, d_phase,
                       d_choice);
    WF_LAUNCH_CHECK();
    return WF_OK;
}

extern "C" int wf_carrier_track(wf_ctx *ctx, const double *d_stat_h, int H, int64_t nwin, int span, double *d_phase, uint8_t *d_choice, void *stream)
{
    return carrier_track_run("wf_carrier_track", ctx, d_stat_h, H, nwin, span, kCarrierPi, d_phase, d_choice, stream);
}

extern "C" int wf_carrier_track_mod(wf_ctx *ctx, const double *d_stat_h, int H, int64_t nwin, int span, double period, double *d_phase, uint8_t *d_choice,
                                    void *stream)
{
    return carrier_track_run("wf_carrier_track_mod", ctx, d_stat_h, H, nwin, span, period, d_phase, d_choice, stream);
}

extern "C" int wf_carrier_track_anchored(wf_ctx *ctx, const double *d_stat_h, int H, int64_t nwin, int span, double period, int anchor, double max_drift,
                                         double reject, double *d_phase, uint8_t *d_choice, double *d_drift, uint8_t *d_marks, void *stream)
{
    const char *who = "wf_carrier_track_anchored";
    WF_REQUIRE(ctx && d_stat_h && d_phase && d_choice && d_drift && d_marks, "%s: NULL argument", who);
    WF_REQUIRE(H >= 1 && H <= 256, "%s: H must be 1 .. 256", who);
    WF_REQUIRE(nwin >= 1, "%s: nwin must be at least 1", who);
    WF_REQUIRE(span >= 1 && span % 2 == 1, "%s: span must be odd and at least 1", who);
    WF_REQUIRE(std::isfinite(period) && period > 0.0 && period <= kCarrierTwoPi, "%s: period must be in (0, 2 pi]", who);
    WF_REQUIRE(!sync_mis(d_stat_h, 7) && !sync_mis(d_phase, 7) && !sync_mis(d_drift, 7), "%s: stat, phase and drift must be 8-byte aligned", who);
    return sync_anchor_run(who, ctx, carrier_anchor_score_kernel, carrier_anchor_tail_kernel, TRACK_THREADS, carrier_psi_of{d_stat_h, H, nwin, period, d_choice}, nwin, span, period,
                           anchor, max_drift, reject, d_phase, d_drift, d_marks, stream);
}

static int rows_derotate_run(const char *who, wf_ctx *ctx, const double *d_rows, int64_t ncalls, int nvals, int W, const double *d_phase, int64_t nwin,
                             double phase0, double *d_out, void *stream)
{
    WF_REQUIRE(ctx && d_rows && d_out, "%s: NULL argument", who);
    WF_REQUIRE(ncalls >= 1, "%s: ncalls must be at least 1", who);
    WF_REQUIRE(nvals >= 1 && nvals <= 64, "%s: nvals must be 1 .. 64", who);
    WF_REQUIRE(std::isfinite(phase0), "%s: phase0 must be finite", who);
    WF_REQUIRE(!d_phase || (sync_window_ok(W) && nwin >= 1), "%s: W must be a multiple of 64 from 64 to 8192 and nwin at least 1", who);
    WF_REQUIRE(!sync_mis(d_rows, 15) && !sync_mis(d_out, 15) && !sync_mis(d_phase, 7), "%s: rows must be 16-byte and phase 8-byte aligned", who);
    WF_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(rows_derotate_kernel, dim3(wf_grid_for(ncalls, CARRIER_THREADS, 1 << 16)), dim3(CARRIER_THREADS), 0, wf_stream(stream),
                       reinterpret_cast<const double2 *>(d_rows), ncalls, nvals, d_phase ? W : 64, d_phase, nwin, phase0, reinterpret_cast<double2 *>(d_out));
    WF_LAUNCH_CHECK();
    return WF_OK;
}

extern "C" int wf_rows_derotate(wf_ctx *ctx, const double *d_rows, int64_t ncalls, int W, const double *d_phase, int64_t nwin, double phase0, double *d_out,
                                void *stream)
{
    return rows_derotate_run("wf_rows_derotate", ctx, d_rows, ncalls, 3, W, d_phase, nwin, phase0, d_out, stream);
}

extern "C" int wf_rows_derotate_n(wf_ctx *ctx, const double *d_rows, int64_t ncalls, int nvals, int W, const double *d_phase, int64_t nwin, double phase0,
                                  double *d_out, void *stream)
{
    return rows_derotate_run("wf_rows_derotate_n", ctx, d_rows, ncalls, nvals, W, d_phase, nwin, phase0, d_out, stream);
}
