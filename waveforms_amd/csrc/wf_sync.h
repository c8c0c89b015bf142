// wf_sync.h — what the synchronisers' device stages share (wf_carrier.hip, wf_timing.hip, wf_cpm_timing.hip, wf_rows_hyp.hip):
// the cubic Lagrange weights, the wrap modulo a period, a row's interpolated trajectory value, the argmin over the hypotheses,
// the trackers' blocked unwrap scan and centred mean, the statistics' wave fold, the rotation of a value and the argument checks.
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

static inline bool sync_mis(const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }
static inline bool sync_window_ok(int W) { return W >= 64 && W <= 8192 && W % 64 == 0; }
