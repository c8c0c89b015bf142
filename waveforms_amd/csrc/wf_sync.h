// wf_sync.h — what the synchronisers' device stages share (wf_carrier.hip, wf_timing.hip, wf_cpm_timing.hip, wf_rows_hyp.hip):
// the cubic Lagrange weights, the wrap modulo a period, a row's interpolated trajectory value, the argmin over the hypotheses,
// the trackers' blocked unwrap scan and centred mean, the anchored unwrapping (phasors, drift search, anchor, re-wrap), the
// statistics' wave fold, the rotation of a value and the argument checks.
// include/wfhip.h states every definition.  One operation per statement where a host statement must see the same roundings
// (-ffp-contract=on fuses within an expression only).
#pragma once
#include "wf_common.h"

#include <cmath>

static constexpr double kTimingHuge = 4611686018427387904.0;   // 2^62: an instant at or beyond it has no sample near it
static constexpr int64_t kTimingMaxN = (int64_t)1 << 40;

// cubic Lagrange weights of the nodes -1, 0, 1, 2 at the fraction mu (products and one division each: nothing to contract)
__device__ __forceinline__ void timing_lagrange(double mu, double c[4])
{
    const double p1 = mu + 1.0, m1 = mu - 1.0, m2 = mu - 2.0;
    c[0] = -(mu * m1 * m2) / 6.0;
    c[1] = (p1 * m1 * m2) / 2.0;
    c[2] = -(p1 * mu * m2) / 2.0;
    c[3] = (p1 * mu * m1) / 6.0;
}

// x - P ceil(x / P - 1/2): into (-P/2, P/2], P the period (π for SOQPSK-TG's phase, 2π/p for CPM's, the samples of the timing's alias)
__device__ __forceinline__ double sync_wrap(double x, double period)
{
    const double r = x / period;
    const double c = ceil(r - 0.5);
    const double m = period * c;
    return x - m;
}

// The carrier impairment of one sample (wf_carrier_offset_c128 and wf_carrier_offset_dev_c128: ONE text, so the two are bitwise
// each other): z exp(j (theta0 + 2π frac(nu idx))), the turn count reduced to its fraction before the product with 2π
static constexpr double kSyncTwoPi = 6.28318530717958647692;
__device__ __forceinline__ double2 sync_carrier_turn(double2 z, double theta0, double nu, int64_t idx)
{
    const double t = nu * (double)idx;                   // turns
    const double fr = t - floor(t);                      // exact
    const double w = kSyncTwoPi * fr;
    const double a = theta0 + w;
    double sn, cs;
    sincos(a, &sn, &cs);
    return make_double2(z.x * cs - z.y * sn, z.x * sn + z.y * cs);
}

// The trajectory's value at row k: traj[nwin] (a phase or an instant per window) interpolated between the centres
// w W + (W - 1) / 2 of the windows of W rows, flat outside the first and the last (one division: W need not be a power of two)
__device__ __forceinline__ double sync_traj_at(const double *__restrict__ traj, int64_t nwin, int W, int64_t k)
{
    const double c0 = 0.5 * (double)(W - 1);
    const double tt = ((double)k - c0) / (double)W;
    if (tt <= 0.0) return traj[0];
    if (tt >= (double)(nwin - 1)) return traj[nwin - 1];
    const double fl = floor(tt);
    const int64_t w = (int64_t)fl;
    const double f = tt - fl;
    const double p0 = traj[w];
    const double d = traj[w + 1] - p0;
    const double fd = f * d;
    return p0 + fd;
}

// The hypothesis with the smallest X of window w in stat[H][nwin][2], the first of equal minima; *bx: that X (kept in a local and
// written once: a running minimum behind the pointer, which may alias stat, cost carrier_track_kernel six registers and an occupancy step)
__device__ __forceinline__ int sync_argmin(const double *stat, int H, int64_t nwin, int64_t w, double *bx)
{
    int best = 0;
    double m = stat[2 * w];
    for (int h = 1; h < H; ++h) {
        const double x = stat[2 * ((int64_t)h * nwin + w)];
        if (x < m) {
            m = x;
            best = h;
        }
    }
    *bx = m;
    return best;
}

// tmp[w] = ψ_w on entry (every thread's writes behind a barrier), u_w = ψ_0 + Σ_{j <= w} wrap(ψ_j - ψ_{j-1}) on return (behind a
// barrier), as a blocked scan by ONE workgroup of THREADS threads: thread t owns the windows [a, e) and adds its own steps,
// thread 0 adds the THREADS segment sums in order, and every thread rewrites its ψ_w as offset + its running sum (ψ_{a-1}, the
// one value it needs of its neighbour's, is read before anybody writes): the definition's running sum to rounding
template <int THREADS>
__device__ __forceinline__ void sync_unwrap_scan(double *tmp, int64_t nwin, double period, double *s_seg)
{
    const int64_t seg = (nwin + THREADS - 1) / THREADS;
    const int64_t a = threadIdx.x * seg < nwin ? threadIdx.x * seg : nwin, e = a + seg < nwin ? a + seg : nwin;
    const double before = a > 0 && a < nwin ? tmp[a - 1] : 0.0;
    double sum = 0.0, prev = before;
    for (int64_t w = a; w < e; ++w) {
        const double psi = tmp[w];
        sum += w == 0 ? psi : sync_wrap(psi - prev, period);
        prev = psi;
    }
    s_seg[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double off = 0.0;
        for (int t = 0; t < THREADS; ++t) {
            const double v = s_seg[t];
            s_seg[t] = off;
            off += v;
        }
    }
    __syncthreads();
    const double off = s_seg[threadIdx.x];
    sum = 0.0;
    prev = before;
    for (int64_t w = a; w < e; ++w) {
        const double psi = tmp[w];
        sum += w == 0 ? psi : sync_wrap(psi - prev, period);
        prev = psi;
        tmp[w] = off + sum;
    }
    __syncthreads();
}

// out[w] = the mean of tmp over the windows within span / 2 of w, clipped to the burst, added in increasing order (threads in parallel)
template <int THREADS>
__device__ __forceinline__ void sync_centred_mean(const double *tmp, int64_t nwin, int span, double *__restrict__ out)
{
    const int64_t r = span / 2;
    for (int64_t w = threadIdx.x; w < nwin; w += THREADS) {
        const int64_t lo = w - r > 0 ? w - r : 0, hi = w + r < nwin - 1 ? w + r : nwin - 1;
        double s = 0.0;
        for (int64_t j = lo; j <= hi; ++j) s += tmp[j];
        out[w] = s / (double)(hi - lo + 1);
    }
}

// the 64 lane partials of a window folded by a shuffle-down butterfly, d = 32 .. 1: p_l + p_{l+d} is what lanes l < d keep (the
// others' sums are never read); lane 0 returns the window's sum
__device__ __forceinline__ double sync_wave_fold(double p)
{
#pragma unroll
    for (int d = WF_WAVE / 2; d >= 1; d >>= 1) p += __shfl_down(p, d, WF_WAVE);
    return p;
}

// z (cs + j sn): the two products and the sum of a component in ONE expression, so that every user contracts alike
__device__ __forceinline__ double2 sync_rotate(double2 z, double cs, double sn)
{
    return make_double2(z.x * cs - z.y * sn, z.x * sn + z.y * cs);
}

// ---- the anchored unwrapping (include/wfhip.h states it; waveforms_amd/sync/_stages.py's anchored_unwrap is the host statement) ----
// Two launches: a grid over the segments of the drift search, a thread per candidate (sync_anchor_score), which also leaves
// ψ_w and z_w of every window in the scratch, then ONE workgroup (sync_anchor_tail) that adds the segments' scores in segment
// order, takes the first largest, and does the anchor, the re-wrap and the mean.
#define ANCHOR_THREADS 256      // sync_anchor_score: candidates per workgroup
#define ANCHOR_MAX_K 1023       // the segment's phasors in LDS: 16 KiB

// What both entry points check and lay out: |i| <= n candidates, nseg segments, and the scratch in doubles:
// z[nwin] (complex) | psi[nwin] | alpha[nwin] | score[nseg][2n + 1]
struct sync_anchor_plan {
    int K, n, ncand;
    int64_t nseg;
    size_t words;
    double reject;
};

static inline int sync_anchor_check(const char *who, int64_t nwin, double period, int anchor, double max_drift, double reject, sync_anchor_plan *p)
{
    WF_REQUIRE(nwin <= ((int64_t)1 << 31), "%s: nwin must be at most 2^31", who);
    WF_REQUIRE(anchor >= 3 && anchor <= ANCHOR_MAX_K && anchor % 2 == 1, "%s: anchor must be odd, 3 .. %d, not %d", who, ANCHOR_MAX_K, anchor);
    WF_REQUIRE(std::isfinite(max_drift) && max_drift >= 0.0 && max_drift < 0.5 * period, "%s: max_drift must be in [0, period / 2)", who);
    WF_REQUIRE(std::isfinite(reject) && reject > 0.0 && reject <= 0.5 * period, "%s: reject must be in (0, period / 2]", who);
    const double span = (double)(4 * anchor) * max_drift;
    p->K = anchor;
    p->n = (int)std::ceil(span / period);                    // <= 2K
    p->ncand = 2 * p->n + 1;
    p->nseg = (nwin + 2 * (int64_t)anchor - 1) / (2 * (int64_t)anchor);
    p->words = 4 * (size_t)nwin + (size_t)p->nseg * (size_t)p->ncand;
    p->reject = reject;
    return WF_OK;
}

// z_w = exp(j 2π frac(ψ_w / P)); a ψ_w that is not finite: 0
__device__ __forceinline__ double2 sync_anchor_phasor(double psi, double period)
{
    if (!(fabs(psi) < INFINITY)) return make_double2(0.0, 0.0);
    const double t = psi / period;
    const double fr = t - floor(t);
    const double a = kSyncTwoPi * fr;
    double sn, cs;
    sincos(a, &sn, &cs);
    return make_double2(cs, sn);
}

// v exp(-j 2π m / q), m = (i j) mod q in [0, q): the angle is reduced as an integer, so it never grows with the burst
__device__ __forceinline__ double2 sync_anchor_turn(double2 v, int64_t i, int64_t j, int q)
{
    int64_t m = (i * j) % q;
    if (m < 0) m += q;
    const double fr = (double)m / (double)q;
    const double a = kSyncTwoPi * fr;
    double sn, cs;
    sincos(a, &sn, &cs);
    return sync_rotate(v, cs, -sn);
}

// Workgroup (b, c) of the drift search: segment b = the windows [2K b, 2K b + K), candidates c THREADS + thread.  Every
// workgroup forms ψ and z of the windows [2K b, 2K (b + 1)) - psi_of(w, keep) is the tracker's own ψ_w, keep: write its choice -
// and the workgroups c = 0 leave them in psi[] and z[]; score[b][candidate] = |Σ_j z_{2K b + j} exp(-j 2π frac(i j / 4K))|², j increasing.
template <int THREADS, class PSI>
__device__ __forceinline__ void sync_anchor_score(PSI psi_of, int64_t nwin, double period, int K, int n, double *psi, double2 *z, double *score,
                                                  double2 *s_z)
{
    const int64_t s = (int64_t)blockIdx.x * 2 * K;
    const int64_t e = s + 2 * K < nwin ? s + 2 * K : nwin;
    const int len = (int)(s + K < nwin ? K : nwin - s);
    const bool keep = blockIdx.y == 0;
    for (int64_t w = s + threadIdx.x; w < e; w += THREADS) {
        const double p = psi_of(w, keep);
        const double2 v = sync_anchor_phasor(p, period);
        if (w - s < K) s_z[w - s] = v;
        if (keep) {
            psi[w] = p;
            z[w] = v;
        }
    }
    __syncthreads();
    const int ncand = 2 * n + 1;
    const int c = blockIdx.y * THREADS + threadIdx.x;
    if (c >= ncand) return;
    double ax = 0.0, ay = 0.0;
    for (int j = 0; j < len; ++j) {
        const double2 r = sync_anchor_turn(s_z[j], c - n, j, 4 * K);
        ax += r.x;
        ay += r.y;
    }
    const double xx = ax * ax;
    const double yy = ay * ay;
    score[(int64_t)blockIdx.x * ncand + c] = xx + yy;
}

// ONE workgroup of THREADS threads behind sync_anchor_score: the scores added over the segments in order and the first
// candidate of the largest total (a fold that prefers the smaller index among equals), y_w in place of z_w, the anchor's angle,
// its running unwrap modulo 2π (sync_unwrap_scan), the reference, the re-wrapped and rejected ψ' in place of ψ, the centred mean.
template <int THREADS>
__device__ __forceinline__ void sync_anchor_tail(int64_t nwin, int span, double period, double reject, int K, int n, int64_t nseg, double *psi, double2 *z,
                                                 double *alpha, const double *score, double *__restrict__ out, double *__restrict__ drift,
                                                 uint8_t *__restrict__ marks, double *s_seg, int *s_idx)
{
    const int t = threadIdx.x, ncand = 2 * n + 1, q = 4 * K;
    if (nwin == 1) {                                            // nothing to anchor: ψ_0 itself
        if (t == 0) {
            const double p = psi[0];
            const bool fin = fabs(p) < INFINITY;
            out[0] = fin ? p : 0.0;
            marks[0] = fin ? 0 : 1;
            drift[0] = 0.0;
        }
        return;
    }
    double bv = -1.0;                                           // (every total is >= 0)
    int bi = ncand;
    for (int c = t; c < ncand; c += THREADS) {
        double tot = 0.0;
        for (int64_t g = 0; g < nseg; ++g) tot += score[g * ncand + c];
        if (tot > bv) {
            bv = tot;
            bi = c;
        }
    }
    s_seg[t] = bv;
    s_idx[t] = bi;
    __syncthreads();
    for (int d = THREADS / 2; d >= 1; d >>= 1) {
        if (t < d) {
            const double ov = s_seg[t + d];
            const int oi = s_idx[t + d];
            if (ov > s_seg[t] || (ov == s_seg[t] && oi < s_idx[t])) {
                s_seg[t] = ov;
                s_idx[t] = oi;
            }
        }
        __syncthreads();
    }
    const int64_t ib = (int64_t)s_idx[0] - n;
    __syncthreads();                                            // s_seg is the scan's from here
    for (int64_t w = t; w < nwin; w += THREADS) z[w] = sync_anchor_turn(z[w], ib, w, q);
    __syncthreads();
    const int64_t r = K / 2;
    for (int64_t w = t; w < nwin; w += THREADS) {
        const int64_t lo = w - r > 0 ? w - r : 0, hi = w + r < nwin - 1 ? w + r : nwin - 1;
        double ax = 0.0, ay = 0.0;
        for (int64_t j = lo; j <= hi; ++j) {
            const double2 y = z[j];
            ax += y.x;
            ay += y.y;
        }
        alpha[w] = atan2(ay, ax);
    }
    __syncthreads();
    sync_unwrap_scan<THREADS>(alpha, nwin, kSyncTwoPi, s_seg);
    const double fhat = (double)ib / (double)q;
    const double c0 = period / kSyncTwoPi;
    const double pf = period * fhat;
    if (t == 0) drift[0] = pf;
    for (int64_t w = t; w < nwin; w += THREADS) {
        const double cu = c0 * alpha[w];
        const double lin = pf * (double)w;
        const double ref = cu + lin;
        const double p = psi[w];
        const bool fin = fabs(p) < INFINITY;
        const double df = (fin ? p : 0.0) - ref;
        const double d = sync_wrap(df, period);
        const bool rej = !fin || fabs(d) > reject;
        marks[w] = rej ? 1 : 0;
        psi[w] = rej ? ref : ref + d;
    }
    __syncthreads();
    sync_centred_mean<THREADS>(psi, nwin, span, out);
}

static inline bool sync_mis(const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }
static inline bool sync_window_ok(int W) { return W >= 64 && W <= 8192 && W % 64 == 0; }

// Both anchored entry points behind their own checks of H, nwin, span and the period: the anchor's checks, the scratch and the
// two launches.  score_kernel(psi_of, K, n, psi, z, score) and tail_kernel(nwin, span, period, reject, K, n, nseg, psi, z, alpha,
// score, out, drift, marks) are the tracker's instantiations of sync_anchor_score and sync_anchor_tail (tail_threads: the latter's THREADS).
template <class PSI, class SCORE, class TAIL>
static int sync_anchor_run(const char *who, wf_ctx *ctx, SCORE score_kernel, TAIL tail_kernel, int tail_threads, PSI psi_of, int64_t nwin, int span,
                           double period, int anchor, double max_drift, double reject, double *d_out, double *d_drift, uint8_t *d_marks, void *stream)
{
    sync_anchor_plan P;
    int rc = sync_anchor_check(who, nwin, period, anchor, max_drift, reject, &P);
    if (rc) return rc;
    WF_HIP(hipSetDevice(ctx->device));
    rc = wf_ctx_reserve_vit(ctx, P.words);
    if (rc) return rc;
    double2 *z = reinterpret_cast<double2 *>(ctx->d_vit_edge);
    double *psi = ctx->d_vit_edge + 2 * nwin, *alpha = psi + nwin, *score = alpha + nwin;
    hipLaunchKernelGGL(score_kernel, dim3((unsigned)P.nseg, (unsigned)((P.ncand + ANCHOR_THREADS - 1) / ANCHOR_THREADS)), dim3(ANCHOR_THREADS), 0,
                       wf_stream(stream), psi_of, P.K, P.n, psi, z, score);
    WF_LAUNCH_CHECK();
    hipLaunchKernelGGL(tail_kernel, dim3(1), dim3(tail_threads), 0, wf_stream(stream), nwin, span, period, P.reject, P.K, P.n, P.nseg, psi, z, alpha,
                       (const double *)score, d_out, d_drift, d_marks);
    WF_LAUNCH_CHECK();
    return WF_OK;
}
