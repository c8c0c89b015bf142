// wf_timing.hip — symbol timing: the impairment (wf_timing_offset_c128), the resampling matched-filter bank
// (wf_mf_bank_resample_c128) and the trajectory stages of the feed-forward recovery (wf_timing_track, wf_timing_track_anchored,
// wf_timing_refine).
// include/wfhip.h states every definition; waveforms_amd/sync/timing.py restates them in numpy.  The reference has no
// synchroniser: these are the build's own.  The statistic the trajectory stages read is wf_carrier_stat's X (wf_carrier.hip).
//
//   timing_offset_kernel    elementwise, out of place: four neighbours of one input sample, cubic Lagrange weights of the
//                           fraction of tau0 + eps (first_index + n).
//   mf_resample_kernel      a thread per output row, a workgroup per tile of rows.  Every thread forms its row's instant (the
//                           interpolated trajectory, wf_sync.h's sync_traj_at), the workgroup takes the smallest
//                           and the largest integer instant of the tile and stages that span of samples ONCE in LDS (coalesced
//                           16 B loads, one pad slot per `step` samples for an even step so that the rows' ds_read_b128 walk
//                           distinct banks: the layout of wf_mfbank.hip), zeros outside the burst.  A row then walks its
//                           ntaps + 3 samples: each of the ntaps positions is interpolated once (4 real-by-complex multiply-
//                           adds, the row's own weights) and feeds the three filters, whose taps are broadcast reads of a copy
//                           behind the window.  Nothing at full rate exists anywhere.  A tile whose span is wider than the
//                           staged region (a trajectory that jumps by more than RS_EXTRA samples inside a tile) reads its
//                           samples from global memory instead, bounds-checked, with the same arithmetic: nothing is read
//                           from LDS that was not staged.
//   timing_track_kernel     ONE workgroup: per window a value (threads in parallel) — the argmin over the hypotheses and its
//                           guarded parabola vertex, or the vertex of a refinement's three points —, for the track the
//                           unwrapping modulo the period as a blocked scan, then the centred mean: the argmin, the scan and the
//                           mean are wf_sync.h's, shared with carrier_track_kernel.
//   timing_anchor_score_kernel / timing_anchor_tail_kernel   the track with wf_sync.h's anchored unwrapping: a grid over the
//                           drift search's segments (a thread per candidate), then ONE workgroup for the rest.
//
// The instants' arithmetic is written one operation per statement where the host statement must see the same roundings
// (-ffp-contract=on fuses within an expression only).
#include "wf_sync.h"

#include <climits>

#define TIMING_THREADS 256
#define RS_THREADS 256
#define RS_LDS_SLOTS 3072     // 48 KiB of complex128: window (with its pad slots) + the tap copy
#define RS_MAXI 12            // staged samples per thread: RS_LDS_SLOTS / RS_THREADS
#define RS_EXTRA 64           // samples of room for the trajectory to move inside one tile before the tile leaves LDS
#define RS_MAX_TAPS 255
#define TTRACK_THREADS 1024   // timing_track_kernel: ONE workgroup (its loops are latency-bound)

__global__ __launch_bounds__(TIMING_THREADS) void timing_offset_kernel(const double2 *__restrict__ in, int64_t n, double tau0, double eps, int64_t first_index,
                                                                       double2 *__restrict__ out)
{
    for (int64_t k = (int64_t)blockIdx.x * TIMING_THREADS + threadIdx.x; k < n; k += (int64_t)gridDim.x * TIMING_THREADS) {
        const double pr = eps * (double)(first_index + k);
        const double t = tau0 + pr;
        double2 acc = make_double2(0.0, 0.0);
        if (fabs(t) < kTimingHuge) {
            const double fl = floor(t);
            const double mu = t - fl;                           // exact
            const int64_t b = k + (int64_t)fl;
            double c[4];
            timing_lagrange(mu, c);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t s = b + (i - 1);
                if (s >= 0 && s < n) {
                    const double2 x = in[s];
                    acc.x = i == 0 ? c[0] * x.x : fma(c[i], x.x, acc.x);
                    acc.y = i == 0 ? c[0] * x.y : fma(c[i], x.y, acc.y);
                }
            }
        }
        out[k] = acc;
    }
}

struct rs_params {
    int64_t nsamp, first, ncols, nwin, nblk;
    int step, ntaps, c, W;
    int ob;          // rows per workgroup iteration (<= RS_THREADS)
    int region;      // samples the window holds
    int pad;         // 1: one pad slot every `step` samples
    int taps_slot;   // LDS slot of the tap copy [3][ntaps]
    double tau0;
    const double *tau;
};

// One row: x[m] = sample B - 1 - c + m, m < ntaps + 3; y_j = Σ_i w_i x[j + i] pairs with tap ntaps - 1 - j of every filter.
// LDS: `src` is the window and p the row's first offset in it; otherwise `src` is the burst and g0 the row's first sample index.
template <bool LDS>
__device__ __forceinline__ void rs_row(const double2 *__restrict__ src, int p, int64_t g0, int64_t nsamp, int step, int pad, const double2 *__restrict__ s_taps,
                                       int ntaps, const double w[4], double2 o[3])
{
    int idx = 0, rem = 0;
    int64_t g = g0;
    if (LDS) {
        const int q = p / step;
        rem = p - q * step;
        idx = p + (pad ? q : 0);
    }
    auto next = [&]() {
        double2 v;
        if (LDS) {
            v = src[idx];
            ++idx;
            if (++rem == step) {
                rem = 0;
                idx += pad;
            }
        } else {
            v = (g >= 0 && g < nsamp) ? src[g] : make_double2(0.0, 0.0);
            ++g;
        }
        return v;
    };
    double2 xa = next(), xb = next(), xc = next();
    double A[3], B[3], C[3], D[3];
#pragma unroll
    for (int f = 0; f < 3; ++f) A[f] = B[f] = C[f] = D[f] = 0.0;
    for (int j = 0; j < ntaps; ++j) {
        const double2 xd = next();
        const double yx = fma(w[3], xd.x, fma(w[2], xc.x, fma(w[1], xb.x, w[0] * xa.x)));
        const double yy = fma(w[3], xd.y, fma(w[2], xc.y, fma(w[1], xb.y, w[0] * xa.y)));
        const double2 *tp = s_taps + (ntaps - 1 - j);
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            const double2 tap = tp[f * ntaps];
            A[f] = fma(yx, tap.x, A[f]);
            B[f] = fma(yy, tap.y, B[f]);
            C[f] = fma(yx, tap.y, C[f]);
            D[f] = fma(yy, tap.x, D[f]);
        }
        xa = xb;
        xb = xc;
        xc = xd;
    }
#pragma unroll
    for (int f = 0; f < 3; ++f) o[f] = make_double2(A[f] - B[f], C[f] + D[f]);
}

__global__ __launch_bounds__(RS_THREADS) void mf_resample_kernel(const double2 *__restrict__ r, const double2 *__restrict__ taps, double2 *__restrict__ out,
                                                                 rs_params P)
{
    extern __shared__ double2 s_rs[];
    __shared__ long long s_lo[RS_THREADS / WF_WAVE], s_hi[RS_THREADS / WF_WAVE];
    const int t = threadIdx.x;
    const int step = P.step, pad = P.pad, ntaps = P.ntaps;
    double2 *s_taps = s_rs + P.taps_slot;
    for (int k = t; k < 3 * ntaps; k += RS_THREADS) s_taps[k] = taps[k];      // (first read behind the loop's barriers)
    for (int64_t blk = blockIdx.x; blk < P.nblk; blk += gridDim.x) {
        const int64_t k = blk * P.ob + t;
        const bool row = t < P.ob && k < P.ncols;
        // the row's instant: tau0 + τ_k, τ interpolated between the window centres
        double tk = P.tau0;
        if (row && P.tau) {
            const double phi = sync_traj_at(P.tau, P.nwin, P.W, k);
            tk = P.tau0 + phi;
        }
        bool live = row && fabs(tk) < kTimingHuge;             // (false for a NaN)
        int64_t B = 0;
        double mu = 0.0;
        if (live) {
            const double fl = floor(tk);
            mu = tk - fl;                                       // exact
            B = P.first + k * step + (int64_t)fl;
            live = B + 2 >= 0 && B - 1 < P.nsamp;               // otherwise all four full-rate values lie outside the burst: a zero row
        }
        // the tile's span of integer instants
        long long mn = live ? (long long)B : LLONG_MAX, mx = live ? (long long)B : LLONG_MIN;
#pragma unroll
        for (int d = WF_WAVE / 2; d >= 1; d >>= 1) {
            const long long a = __shfl_xor(mn, d, WF_WAVE), b = __shfl_xor(mx, d, WF_WAVE);
            mn = a < mn ? a : mn;
            mx = b > mx ? b : mx;
        }
        __syncthreads();                                        // the previous tile's reads of the window and of s_lo / s_hi are done
        if (wf_lane() == 0) {
            s_lo[t / WF_WAVE] = mn;
            s_hi[t / WF_WAVE] = mx;
        }
        __syncthreads();
#pragma unroll
        for (int v = 0; v < RS_THREADS / WF_WAVE; ++v) {
            mn = s_lo[v] < mn ? s_lo[v] : mn;
            mx = s_hi[v] > mx ? s_hi[v] : mx;
        }
        const bool any = mn <= mx;                              // block-uniform from here
        const int64_t lo = any ? (int64_t)mn - 1 - P.c : 0;     // first sample any row of the tile reads
        const int64_t need = any ? ((int64_t)mx + 2 + P.c) - lo + 1 : 0;
        const bool fits = any && need <= P.region;
        if (fits) {
            // all of this thread's loads are issued before the first one is consumed, then the LDS writes
            double2 v[RS_MAXI];
#pragma unroll
            for (int u = 0; u < RS_MAXI; ++u) {
                const int i = t + u * RS_THREADS;
                const int64_t s = lo + i;
                v[u] = make_double2(0.0, 0.0);
                if (i < need && s >= 0 && s < P.nsamp) v[u] = r[s];
            }
            int q = t / step, rem = t - q * step;
            const int dq = RS_THREADS / step, dr = RS_THREADS - dq * step;
#pragma unroll
            for (int u = 0; u < RS_MAXI; ++u) {
                const int i = t + u * RS_THREADS;
                if (i < need) s_rs[i + (pad ? q : 0)] = v[u];
                q += dq;
                rem += dr;
                if (rem >= step) {
                    rem -= step;
                    ++q;
                }
            }
        }
        __syncthreads();
        if (!row) continue;
        double2 o[3] = {make_double2(0.0, 0.0), make_double2(0.0, 0.0), make_double2(0.0, 0.0)};
        if (live) {
            double w[4];
            timing_lagrange(mu, w);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (B + (i - 1) < 0 || B + (i - 1) >= P.nsamp) w[i] = 0.0;      // v_f is zero outside the burst
            const int64_t g0 = B - 1 - P.c;
            if (fits) rs_row<true>(s_rs, (int)(g0 - lo), 0, P.nsamp, step, pad, s_taps, ntaps, w, o);
            else rs_row<false>(r, 0, g0, P.nsamp, step, pad, s_taps, ntaps, w, o);
        }
        out[3 * k] = o[0];
        out[3 * k + 1] = o[1];
        out[3 * k + 2] = o[2];
    }
}

// V of the parabola through (-1, a), (0, b), (1, c), guarded: 0 unless the three points are strictly convex; clamped to ±lim
__device__ __forceinline__ double timing_vertex(double a, double b, double c, double lim)
{
    const double ab = a - b;
    const double cb = c - b;
    const double den = ab + cb;
    if (!(den > 0.0)) return 0.0;
    const double ac = a - c;
    const double half = 0.5 * ac;
    const double v = half / den;
    return v > lim ? lim : (v < -lim ? -lim : v);
}

// ψ_w of H hypotheses a period / H apart: the best one's instant moved by its guarded vertex; choice (or null): the best one
__device__ __forceinline__ double timing_psi(const double *__restrict__ stat, int H, int64_t nwin, double period, int64_t w, uint8_t *__restrict__ choice)
{
    double bx;
    const int best = sync_argmin(stat, H, nwin, w, &bx);
    if (choice) choice[w] = (uint8_t)best;
    const double a = stat[2 * ((int64_t)(best == 0 ? H - 1 : best - 1) * nwin + w)];
    const double c = stat[2 * ((int64_t)(best == H - 1 ? 0 : best + 1) * nwin + w)];
    const double v = timing_vertex(a, bx, c, 0.5);
    const double dh = period / (double)H;
    const double ih = (double)best * dh;
    const double hp = 0.5 * period;
    const double s = ih - hp;
    const double sv = dh * v;
    return s + sv;
}

// TRACK: ψ_w of H hypotheses, unwrapped modulo the period; otherwise scale * V of the three points of a refinement.  Then the mean.
template <bool TRACK>
__global__ __launch_bounds__(TTRACK_THREADS) void timing_track_kernel(const double *__restrict__ stat, int H, int64_t nwin, int span, double scale, double *tmp,
                                                                      double *__restrict__ tau, uint8_t *__restrict__ choice)
{
    __shared__ double s_seg[TTRACK_THREADS];
    for (int64_t w = threadIdx.x; w < nwin; w += TTRACK_THREADS) {
        if (TRACK) {
            tmp[w] = timing_psi(stat, H, nwin, scale, w, choice);      // scale: the period
        } else {
            const double v = timing_vertex(stat[2 * w], stat[2 * (nwin + w)], stat[2 * (2 * nwin + w)], 1.0);
            tmp[w] = scale * v;                                 // scale: δ
        }
    }
    __syncthreads();
    if (TRACK) sync_unwrap_scan<TTRACK_THREADS>(tmp, nwin, scale, s_seg);
    sync_centred_mean<TTRACK_THREADS>(tmp, nwin, span, tau);
}

// The anchored track (wf_sync.h): the drift search over (segments, candidates), then the one workgroup behind it
struct timing_psi_of {
    const double *stat;
    int H;
    int64_t nwin;
    double period;
    uint8_t *choice;
    __device__ __forceinline__ double operator()(int64_t w, bool keep) const { return timing_psi(stat, H, nwin, period, w, keep ? choice : nullptr); }
};

__global__ __launch_bounds__(ANCHOR_THREADS) void timing_anchor_score_kernel(timing_psi_of psi_of, int K, int n, double *psi, double2 *z, double *score)
{
    __shared__ double2 s_z[ANCHOR_MAX_K];
    sync_anchor_score<ANCHOR_THREADS>(psi_of, psi_of.nwin, psi_of.period, K, n, psi, z, score, s_z);
}

__global__ __launch_bounds__(TTRACK_THREADS) void timing_anchor_tail_kernel(int64_t nwin, int span, double period, double reject, int K, int n, int64_t nseg,
                                                                            double *psi, double2 *z, double *alpha, const double *score,
                                                                            double *__restrict__ tau, double *__restrict__ drift, uint8_t *__restrict__ marks)
{
    __shared__ double s_seg[TTRACK_THREADS];
    __shared__ int s_idx[TTRACK_THREADS];
    sync_anchor_tail<TTRACK_THREADS>(nwin, span, period, reject, K, n, nseg, psi, z, alpha, score, tau, drift, marks, s_seg, s_idx);
}

// ---- host side ------------------------------------------------------------------------------------------------------

extern "C" int wf_timing_offset_c128(wf_ctx *ctx, const double *d_in_ri, int64_t n, double tau0, double eps, int64_t first_index, double *d_out_ri,
                                     void *stream)
{
    WF_REQUIRE(ctx && d_in_ri && d_out_ri, "wf_timing_offset_c128: NULL argument");
    WF_REQUIRE(n >= 1 && first_index >= 0 && n <= ((int64_t)1 << 53) - first_index, "wf_timing_offset_c128: n must be at least 1 and first_index + n at most 2^53");
    WF_REQUIRE(std::isfinite(tau0) && std::isfinite(eps), "wf_timing_offset_c128: tau0 and eps must be finite");
    WF_REQUIRE(!sync_mis(d_in_ri, 15) && !sync_mis(d_out_ri, 15), "wf_timing_offset_c128: samples must be 16-byte aligned");
    {
        const uintptr_t a = reinterpret_cast<uintptr_t>(d_in_ri), b = reinterpret_cast<uintptr_t>(d_out_ri), bytes = (uintptr_t)n * 16;
        WF_REQUIRE(a + bytes <= b || b + bytes <= a, "wf_timing_offset_c128: out of place only (the output overlaps the input)");
    }
    WF_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(timing_offset_kernel, dim3(wf_grid_for(n, TIMING_THREADS, 1 << 16)), dim3(TIMING_THREADS), 0, wf_stream(stream),
                       reinterpret_cast<const double2 *>(d_in_ri), n, tau0, eps, first_index, reinterpret_cast<double2 *>(d_out_ri));
    WF_LAUNCH_CHECK();
    return WF_OK;
}

extern "C" int wf_mf_bank_resample_c128(wf_ctx *ctx, const double *d_r_ri, int64_t nsamp, const double *d_taps_ri, int nfilt, int ntaps, int64_t first, int step,
                                        int64_t ncols, int W, const double *d_tau, int64_t nwin, double tau0, double *d_out_ri, void *stream)
{
    const char *who = "wf_mf_bank_resample_c128";
    WF_REQUIRE(ctx && d_r_ri && d_taps_ri && d_out_ri, "%s: NULL argument", who);
    WF_REQUIRE(nfilt == 3, "%s: nfilt must be 3 (the 48-byte detector rows), not %d", who, nfilt);
    WF_REQUIRE(ntaps >= 1 && ntaps <= RS_MAX_TAPS && ntaps % 2 == 1, "%s: ntaps must be odd, 1 .. %d, not %d", who, RS_MAX_TAPS, ntaps);
    WF_REQUIRE(step >= 1 && step <= 64, "%s: step must be 1 .. 64, not %d", who, step);
    WF_REQUIRE(nsamp >= 1 && nsamp <= kTimingMaxN && ncols >= 1 && ncols <= kTimingMaxN && first >= -kTimingMaxN && first <= kTimingMaxN,
               "%s: nsamp and ncols must be 1 .. 2^40 and |first| at most 2^40", who);
    WF_REQUIRE(std::isfinite(tau0), "%s: tau0 must be finite", who);
    WF_REQUIRE(!d_tau || (sync_window_ok(W) && nwin >= 1 && nwin <= kTimingMaxN), "%s: W must be a multiple of 64 from 64 to 8192 and nwin at least 1", who);
    WF_REQUIRE(!sync_mis(d_r_ri, 15) && !sync_mis(d_taps_ri, 15) && !sync_mis(d_out_ri, 15) && !sync_mis(d_tau, 7),
               "%s: samples, taps and rows must be 16-byte and tau 8-byte aligned", who);
    WF_HIP(hipSetDevice(ctx->device));
    rs_params P;
    P.nsamp = nsamp;
    P.first = first;
    P.ncols = ncols;
    P.nwin = d_tau ? nwin : 0;
    P.step = step;
    P.ntaps = ntaps;
    P.c = (ntaps - 1) / 2;
    P.W = d_tau ? W : 64;
    P.pad = (step % 2 == 0) ? 1 : 0;
    P.tau0 = tau0;
    P.tau = d_tau;
    // window slots(ob) = region + pad * (region / step + 1), region = (ob - 1) step + ntaps + 3 + RS_EXTRA, and 3 ntaps slots of taps
    int ob = RS_THREADS;
    for (;;) {
        const int region = (ob - 1) * step + ntaps + 3 + RS_EXTRA;
        const int slots = region + (P.pad ? region / step + 1 : 0);
        if (slots + 3 * ntaps <= RS_LDS_SLOTS) {
            P.ob = ob;
            P.region = region;
            P.taps_slot = slots;
            break;
        }
        WF_REQUIRE(ob > 1, "%s: a bank of %d taps does not fit the window", who, ntaps);
        ob = ob > 16 ? ob - 16 : ob - 1;
    }
    P.nblk = (ncols + P.ob - 1) / P.ob;
    const int grid = (int)(P.nblk < 4096 ? P.nblk : 4096);
    const size_t lds = (size_t)(P.taps_slot + 3 * ntaps) * sizeof(double2);
    hipLaunchKernelGGL(mf_resample_kernel, dim3(grid), dim3(RS_THREADS), lds, wf_stream(stream), reinterpret_cast<const double2 *>(d_r_ri),
                       reinterpret_cast<const double2 *>(d_taps_ri), reinterpret_cast<double2 *>(d_out_ri), P);
    WF_LAUNCH_CHECK();
    return WF_OK;
}

extern "C" int wf_timing_track(wf_ctx *ctx, const double *d_stat_h, int H, int64_t nwin, int span, double period, double *d_tau, uint8_t *d_choice,
                               void *stream)
{
    WF_REQUIRE(ctx && d_stat_h && d_tau && d_choice, "wf_timing_track: NULL argument");
    WF_REQUIRE(H >= 3 && H <= 64, "wf_timing_track: H must be 3 .. 64");
    WF_REQUIRE(nwin >= 1 && nwin <= kTimingMaxN, "wf_timing_track: nwin must be at least 1");
    WF_REQUIRE(span >= 1 && span % 2 == 1, "wf_timing_track: span must be odd and at least 1");
    WF_REQUIRE(std::isfinite(period) && period > 0.0, "wf_timing_track: period must be finite and positive");
    WF_REQUIRE(!sync_mis(d_stat_h, 7) && !sync_mis(d_tau, 7), "wf_timing_track: stat and tau must be 8-byte aligned");
    WF_HIP(hipSetDevice(ctx->device));
    const int rc = wf_ctx_reserve_vit(ctx, (size_t)nwin);
    if (rc) return rc;
    hipLaunchKernelGGL(timing_track_kernel<true>, dim3(1), dim3(TTRACK_THREADS), 0, wf_stream(stream), d_stat_h, H, nwin, span, period, ctx->d_vit_edge, d_tau,
                       d_choice);
    WF_LAUNCH_CHECK();
    return WF_OK;
}

extern "C" int wf_timing_track_anchored(wf_ctx *ctx, const double *d_stat_h, int H, int64_t nwin, int span, double period, int anchor, double max_drift,
                                        double reject, double *d_tau, uint8_t *d_choice, double *d_drift, uint8_t *d_marks, void *stream)
{
    const char *who = "wf_timing_track_anchored";
    WF_REQUIRE(ctx && d_stat_h && d_tau && d_choice && d_drift && d_marks, "%s: NULL argument", who);
    WF_REQUIRE(H >= 3 && H <= 64, "%s: H must be 3 .. 64", who);
    WF_REQUIRE(nwin >= 1, "%s: nwin must be at least 1", who);
    WF_REQUIRE(span >= 1 && span % 2 == 1, "%s: span must be odd and at least 1", who);
    WF_REQUIRE(std::isfinite(period) && period > 0.0, "%s: period must be finite and positive", who);
    WF_REQUIRE(!sync_mis(d_stat_h, 7) && !sync_mis(d_tau, 7) && !sync_mis(d_drift, 7), "%s: stat, tau and drift must be 8-byte aligned", who);
    return sync_anchor_run(who, ctx, timing_anchor_score_kernel, timing_anchor_tail_kernel, TTRACK_THREADS, timing_psi_of{d_stat_h, H, nwin, period, d_choice}, nwin, span, period,
                           anchor, max_drift, reject, d_tau, d_drift, d_marks, stream);
}

extern "C" int wf_timing_refine(wf_ctx *ctx, const double *d_stat3, int64_t nwin, int span, double delta, double *d_more, void *stream)
{
    WF_REQUIRE(ctx && d_stat3 && d_more, "wf_timing_refine: NULL argument");
    WF_REQUIRE(nwin >= 1 && nwin <= kTimingMaxN, "wf_timing_refine: nwin must be at least 1");
    WF_REQUIRE(span >= 1 && span % 2 == 1, "wf_timing_refine: span must be odd and at least 1");
    WF_REQUIRE(std::isfinite(delta) && delta > 0.0, "wf_timing_refine: delta must be finite and positive");
    WF_REQUIRE(!sync_mis(d_stat3, 7) && !sync_mis(d_more, 7), "wf_timing_refine: stat and more must be 8-byte aligned");
    WF_HIP(hipSetDevice(ctx->device));
    const int rc = wf_ctx_reserve_vit(ctx, (size_t)nwin);
    if (rc) return rc;
    hipLaunchKernelGGL(timing_track_kernel<false>, dim3(1), dim3(TTRACK_THREADS), 0, wf_stream(stream), d_stat3, 3, nwin, span, delta, ctx->d_vit_edge, d_more,
                       (uint8_t *)nullptr);
    WF_LAUNCH_CHECK();
    return WF_OK;
}
