// wf_timing.h — what the resampling front ends share (wf_timing.hip: wf_mf_bank_resample_c128; wf_cpm_timing.hip:
// wf_cpm_mf_rows_resample_c128): the cubic Lagrange weights, a row's interpolated trajectory value and the argument checks.
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

// τ_k: tau[nwin] interpolated between the centres of the windows of W rows as rows_derotate_kernel interpolates its phase
__device__ __forceinline__ double timing_tau_at(const double *__restrict__ tau, int64_t nwin, int W, int64_t k)
{
    const double c0 = 0.5 * (double)(W - 1);
    const double tt = ((double)k - c0) / (double)W;
    if (tt <= 0.0) return tau[0];
    if (tt >= (double)(nwin - 1)) return tau[nwin - 1];
    const double fl = floor(tt);
    const int64_t w = (int64_t)fl;
    const double f = tt - fl;
    const double p0 = tau[w];
    const double d = tau[w + 1] - p0;
    const double fd = f * d;
    return p0 + fd;
}

static inline bool timing_mis(const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }
static inline bool timing_window_ok(int W) { return W >= 64 && W <= 8192 && W % 64 == 0; }
