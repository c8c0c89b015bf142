// wf_viterbi_soft_apriori.h — device code shared by the a-priori SOQPSK detectors: wf_viterbi_soft_apriori.hip
// (wf_viterbi4_soft_apriori, the whole burst) and wf_viterbi_live.hip (wf_viterbi4_soft_apriori_windows, the live windows of an
// iterative loop): the prior's register window and the recursions over inc' = inc + π.  wf_viterbi_soft_apriori.hip states the
// arithmetic and why fmin restates the definition's compare.
#pragma once

#include "wf_viterbi_soft.h"

struct soft_prior {
    const float *p;
    double scale;
    int64_t n;          // rows of the burst = values at p
    int vec;            // p is 16-byte aligned: windows are filled by two float4 loads
};

// A lane's window on the prior: the 8 consecutive values of the 32-byte group its row lies in, refilled when the row
// leaves the group (either direction).  A lane walks its own chunk, so a scalar load per row would touch the lane's
// line of the prior on EVERY row beside the row's own lines; the window touches it once per 8 rows.
struct soft_prior_win {
    float v[8];
    int64_t base = -8;
};

__device__ __forceinline__ double soft_prior_at(const soft_prior &pr, soft_prior_win &w, int64_t k)
{
    const int64_t g = k & ~(int64_t)7;
    if (g != w.base) {
        w.base = g;
        if (pr.vec && g + 8 <= pr.n) {
            const float4 a = *reinterpret_cast<const float4 *>(pr.p + g), b = *reinterpret_cast<const float4 *>(pr.p + g + 4);
            w.v[0] = a.x; w.v[1] = a.y; w.v[2] = a.z; w.v[3] = a.w;
            w.v[4] = b.x; w.v[5] = b.y; w.v[6] = b.z; w.v[7] = b.w;
        } else {        // the burst's last group, or an unaligned prior: value by value, never past row n - 1
#pragma unroll
            for (int j = 0; j < 8; ++j) w.v[j] = g + j < pr.n ? pr.p[g + j] : 0.0f;
        }
    }
    const int j = (int)(k & 7);
    float x = w.v[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) x = j == i ? w.v[i] : x;
    return pr.scale * (double)x;
}

// inc' of the branch that enters end state e as the first (ia) / second (ib) listed one; start states as in soft_sums
template <int COL, int DIFF>
__device__ __forceinline__ void soft_ap_incs(const vit_comp &q, double pi, double ia[4], double ib[4])
{
    if (COL == 0) {
        ia[0] = -q.i1; ia[1] = -q.r1; ia[2] = -q.b; ia[3] = -q.a;
        ib[0] = q.a;   ib[1] = q.b;   ib[2] = q.r1; ib[3] = q.i1;
    } else {
        ia[0] = -q.i1; ia[1] = -q.a;  ia[2] = q.r1; ia[3] = q.b;
        ib[0] = -q.b;  ib[1] = -q.r1; ib[2] = q.a;  ib[3] = q.i1;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (soft_inp<COL, DIFF>(e, 0)) ia[e] += pi;
        if (soft_inp<COL, DIFF>(e, 1)) ib[e] += pi;
    }
}

// ã_k -> ã_{k+1} over inc'
template <int COL, int DIFF>
__device__ __forceinline__ void soft_ap_fwd(double m[4], const vit_comp &q, double pi)
{
    double ia[4], ib[4], o[4];
    soft_ap_incs<COL, DIFF>(q, pi, ia, ib);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int sa = COL == 0 ? (e & 1) : (e & 2), sb = COL == 0 ? (e & 1) + 2 : (e & 2) + 1;
        o[e] = fmin(m[sa] + ia[e], m[sb] + ib[e]);
    }
    soft_normalise(o, m);
}

// b̃_{k+1} -> b̃_k over inc': start state s leaves to e0 / e1 as the sec-th listed branch into each
template <int COL, int DIFF>
__device__ __forceinline__ void soft_ap_bwd(double b[4], const vit_comp &q, double pi)
{
    double ia[4], ib[4], o[4];
    soft_ap_incs<COL, DIFF>(q, pi, ia, ib);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int sec = COL == 0 ? s >> 1 : s & 1;
        const int e0 = COL == 0 ? (s & 1) : (s & 2), e1 = COL == 0 ? (s & 1) + 2 : (s & 2) + 1;
        o[s] = fmin((sec ? ib[e0] : ia[e0]) + b[e0], (sec ? ib[e1] : ia[e1]) + b[e1]);
    }
    soft_normalise(o, b);
}

template <bool PACKED, int DIFF>
__device__ __forceinline__ void soft_ap_fwd_row(double m[4], const double *rows, const soft_prior &pr, soft_prior_win &w, int64_t k)
{
    const double pi = soft_prior_at(pr, w, k);
    if (k & 1) soft_ap_fwd<1, DIFF>(m, vit_components<1, PACKED>(soft_row<PACKED>(rows, k)), pi);
    else soft_ap_fwd<0, DIFF>(m, vit_components<0, PACKED>(soft_row<PACKED>(rows, k)), pi);
}

template <bool PACKED, int DIFF>
__device__ __forceinline__ void soft_ap_bwd_row(double b[4], const double *rows, const soft_prior &pr, soft_prior_win &w, int64_t k)
{
    const double pi = soft_prior_at(pr, w, k);
    if (k & 1) soft_ap_bwd<1, DIFF>(b, vit_components<1, PACKED>(soft_row<PACKED>(rows, k)), pi);
    else soft_ap_bwd<0, DIFF>(b, vit_components<0, PACKED>(soft_row<PACKED>(rows, k)), pi);
}

// The chunk's own rows forward from m = ã_a: ã_k of every row stored (lane-interleaved), m left at ã_e.
template <bool PACKED, int DIFF>
__device__ __forceinline__ void soft_ap_fwd_chunk(const double *rows, const soft_prior &pr, soft_prior_win &w, int64_t a, int64_t e, int64_t c, int64_t nch,
                                                  double *alpha, double m[4])
{
    for (int64_t k = a; k < e; ++k) {
        soft_put4(alpha + 4 * ((k - a) * nch + c), m);
        soft_ap_fwd_row<PACKED, DIFF>(m, rows, pr, w, k);
    }
}
