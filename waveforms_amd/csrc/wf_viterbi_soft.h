// wf_viterbi_soft.h — device code and launch geometry shared by the soft-output SOQPSK detectors: wf_viterbi_soft.hip
// (wf_viterbi4_soft) and wf_viterbi_soft_apriori.hip (wf_viterbi4_soft_apriori).  Both cut a burst into the same chunks and
// lay the context's scratch out the same way, so one geometry call describes either.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "wf_viterbi4.h"

#define SOFT_THREADS 256
static constexpr int kSoftDefaultWarmup = 32;          // rows; the hard detector's 31 + its priming row
static constexpr int64_t kSoftLanes = (int64_t)1 << 18; // lanes the burst is cut for by default (~4 waves per SIMD)
static constexpr int kSoftMaxChunk = 8192;             // = the WF_OPT_SOFT_CHUNK_CALLS range

// ã + inc for the two branches that enter end state s (list order: fa first), section COL; the signed components of
// vit_components as in the hard detector's ACS (wf_viterbi.hip: vit_acs).
template <int COL>
__device__ __forceinline__ void soft_sums(const double m[4], const vit_comp &q, double fa[4], double fb[4])
{
    if (COL == 0) {
        fa[0] = m[0] - q.i1; fb[0] = m[2] + q.a;
        fa[1] = m[1] - q.r1; fb[1] = m[3] + q.b;
        fa[2] = m[0] - q.b;  fb[2] = m[2] + q.r1;
        fa[3] = m[1] - q.a;  fb[3] = m[3] + q.i1;
    } else {
        fa[0] = m[0] - q.i1; fb[0] = m[1] - q.b;
        fa[1] = m[0] - q.a;  fb[1] = m[1] - q.r1;
        fa[2] = m[2] + q.r1; fb[2] = m[3] + q.a;
        fa[3] = m[2] + q.b;  fb[3] = m[3] + q.i1;
    }
}

__device__ __forceinline__ void soft_normalise(const double o[4], double m[4])
{
    const double mn = fmin(fmin(o[0], o[1]), fmin(o[2], o[3]));
#pragma unroll
    for (int s = 0; s < 4; ++s) m[s] = o[s] - mn;
}

// ã_k -> ã_{k+1}
template <int COL>
__device__ __forceinline__ void soft_fwd(double m[4], const vit_comp &q)
{
    double fa[4], fb[4], o[4];
    soft_sums<COL>(m, q, fa, fb);
#pragma unroll
    for (int s = 0; s < 4; ++s) o[s] = fmin(fa[s], fb[s]);
    soft_normalise(o, m);
}

// b̃_{k+1} -> b̃_k: the two branches that LEAVE start state s, inc + b̃(end).  Column 0: s -> (s & 1), (s & 1) + 2;
// column 1: s -> (s & 2), (s & 2) + 1; increments from the same table as soft_sums.
template <int COL>
__device__ __forceinline__ void soft_bwd(double b[4], const vit_comp &q)
{
    double o[4];
    if (COL == 0) {
        o[0] = fmin(b[0] - q.i1, b[2] - q.b);
        o[1] = fmin(b[1] - q.r1, b[3] - q.a);
        o[2] = fmin(b[0] + q.a, b[2] + q.r1);
        o[3] = fmin(b[1] + q.b, b[3] + q.i1);
    } else {
        o[0] = fmin(b[0] - q.i1, b[1] - q.a);
        o[1] = fmin(b[0] - q.b, b[1] - q.r1);
        o[2] = fmin(b[2] + q.r1, b[3] + q.b);
        o[3] = fmin(b[2] + q.a, b[3] + q.i1);
    }
    soft_normalise(o, b);
}

// input bit of the branch that enters end state e as the first (sec 0) or second (sec 1) listed one
template <int COL, int DIFF>
__device__ __forceinline__ constexpr int soft_inp(int e, int sec)
{
    const int start = COL == 0 ? (e & 1) + 2 * sec : (e & 2) + sec;
    const int lsb = COL == 0 ? e >> 1 : e & 1;                       // b & 1 of branch b = 2 * start + lsb
    const int flip = DIFF ? (COL == 0 ? (start >> 1) : (start & 1)) : 0;
    return lsb ^ flip;                                               // = br_inp(COL, 2 * start + lsb, DIFF)
}

template <int COL, int DIFF>
__device__ __forceinline__ double soft_llr(const double a[4], const double b[4], const vit_comp &q)
{
    double fa[4], fb[4];
    soft_sums<COL>(a, q, fa, fb);
    double m0 = __builtin_inf(), m1 = __builtin_inf();
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const double ta = fa[e] + b[e], tb = fb[e] + b[e];
        if (soft_inp<COL, DIFF>(e, 0)) m1 = fmin(m1, ta); else m0 = fmin(m0, ta);
        if (soft_inp<COL, DIFF>(e, 1)) m1 = fmin(m1, tb); else m0 = fmin(m0, tb);
    }
    return m1 - m0;
}

template <bool PACKED>
__device__ __forceinline__ const double2 *soft_row(const double *rows, int64_t k)
{
    return reinterpret_cast<const double2 *>(rows) + (PACKED ? 2 : 3) * k;
}

template <bool PACKED>
__device__ __forceinline__ void soft_fwd_row(double m[4], const double *rows, int64_t k)
{
    if (k & 1) soft_fwd<1>(m, vit_components<1, PACKED>(soft_row<PACKED>(rows, k)));
    else soft_fwd<0>(m, vit_components<0, PACKED>(soft_row<PACKED>(rows, k)));
}

template <bool PACKED>
__device__ __forceinline__ void soft_bwd_row(double b[4], const double *rows, int64_t k)
{
    if (k & 1) soft_bwd<1>(b, vit_components<1, PACKED>(soft_row<PACKED>(rows, k)));
    else soft_bwd<0>(b, vit_components<0, PACKED>(soft_row<PACKED>(rows, k)));
}

__device__ __forceinline__ void soft_put4(double *p, const double m[4]) { *reinterpret_cast<double4 *>(p) = make_double4(m[0], m[1], m[2], m[3]); }

__device__ __forceinline__ void soft_get4(const double *p, double m[4])
{
    const double4 v = *reinterpret_cast<const double4 *>(p);
    m[0] = v.x; m[1] = v.y; m[2] = v.z; m[3] = v.w;
}

// The chunk's own rows forward from m = ã_a: ã_k of every row stored (lane-interleaved), m left at ã_e.
template <bool PACKED>
__device__ __forceinline__ void soft_fwd_chunk(const double *rows, int64_t a, int64_t e, int64_t c, int64_t nch, double *alpha, double m[4])
{
    for (int64_t k = a; k < e; ++k) {
        soft_put4(alpha + 4 * ((k - a) * nch + c), m);
        soft_fwd_row<PACKED>(m, rows, k);
    }
}

// ---- launch geometry (host) ------------------------------------------------------------------------------------------
struct soft_geom {
    int ch, warmup;
    int64_t nch;
    size_t off_b, off_alpha, words;   // scratch layout (doubles): forward records, backward records, ã per row
};

static soft_geom soft_geometry(const wf_ctx *ctx, int64_t n, int warmup)
{
    soft_geom g;
    g.warmup = warmup == 0 ? kSoftDefaultWarmup : (warmup > 4096 ? 4096 : warmup);
    int64_t ch = ctx->opt[WF_OPT_SOFT_CHUNK_CALLS];
    if (ch == 0) {
        ch = (n + kSoftLanes - 1) / kSoftLanes;
        ch = (ch + 1) / 2 * 2;
        if (ch < 32) ch = 32;
        if (ch > kSoftMaxChunk) ch = kSoftMaxChunk;
    }
    g.ch = (int)ch;
    g.nch = (n + ch - 1) / ch;
    g.off_b = (vit_edge_words(g.nch) + 3) / 4 * 4;         // 32 B records stay aligned
    g.off_alpha = 2 * g.off_b;
    g.words = g.off_alpha + 4 * (size_t)ch * (size_t)g.nch;
    return g;
}
