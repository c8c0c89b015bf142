// wf_viterbi_soft.h — what the three soft-output SOQPSK detectors share: wf_viterbi_soft.hip (wf_viterbi4_soft),
// wf_viterbi_soft_apriori.hip (wf_viterbi4_soft_apriori) and wf_viterbi_live.hip (wf_viterbi4_soft_apriori_windows).  ONE
// statement of the trellis steps, of the walk of a chunk in each of the three launches and of the host's checks, repair
// passes and dispatch, plus the geometry of a burst; each .hip file wraps the bodies in kernels of its own name.
//
// Everything on the device carries the template argument AP: true runs over inc' = inc + π (wf_viterbi_soft_apriori.hip
// states the arithmetic), false is the plain detector — no prior anywhere: π is the constant +0.0, nothing is loaded and
// the additions are compiled out, so the code is that of wf_viterbi_soft.hip's definition.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <type_traits>

#include "wf_viterbi4.h"

#define SOFT_THREADS 256
static constexpr int kSoftDefaultWarmup = 32;          // rows; the hard detector's 31 + its priming row
static constexpr int64_t kSoftLanes = (int64_t)1 << 18; // lanes the burst is cut for by default (~4 waves per SIMD)
static constexpr int kSoftMaxChunk = 8192;             // = the WF_OPT_SOFT_CHUNK_CALLS range

// ---- the prior ----------------------------------------------------------------------------------------------------------
struct soft_prior {
    const float *p;
    double scale;
    int64_t n;          // rows of the burst = values at p
    int vec;            // p is 16-byte aligned: windows are filled by two float4 loads
};

static soft_prior soft_prior_of(const float *p, double scale, int64_t n) { return soft_prior{p, scale, n, (reinterpret_cast<uintptr_t>(p) & 15) == 0 ? 1 : 0}; }

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

// AP = false: the empty form.  (bits = λ + π < 0 stays λ < 0: x + 0.0 < 0.0 is x < 0.0 for every double.)
struct soft_no_prior {};
struct soft_no_win {};
__device__ __forceinline__ double soft_prior_at(const soft_no_prior &, soft_no_win &, int64_t) { return 0.0; }

template <bool AP> using soft_prior_t = std::conditional_t<AP, soft_prior, soft_no_prior>;
template <bool AP> using soft_win_t = std::conditional_t<AP, soft_prior_win, soft_no_win>;

// ---- the trellis steps ----------------------------------------------------------------------------------------------------
// input bit of the branch that enters end state e as the first (sec 0) or second (sec 1) listed one
template <int COL, int DIFF>
__device__ __forceinline__ constexpr int soft_inp(int e, int sec)
{
    const int start = COL == 0 ? (e & 1) + 2 * sec : (e & 2) + sec;
    const int lsb = COL == 0 ? e >> 1 : e & 1;                       // b & 1 of branch b = 2 * start + lsb
    const int flip = DIFF ? (COL == 0 ? (start >> 1) : (start & 1)) : 0;
    return lsb ^ flip;                                               // = br_inp(COL, 2 * start + lsb, DIFF)
}

// The increment table: inc (AP: inc' = inc + π where the input bit is 1) of the branch that enters end state e as the
// first (ia) / second (ib) listed one, section COL; the signed components of vit_components as in the hard detector's
// ACS (wf_viterbi.hip: vit_acs).  Start states: column 0: e & 1, (e & 1) + 2; column 1: e & 2, (e & 2) + 1.
template <int COL, int DIFF, bool AP>
__device__ __forceinline__ void soft_incs(const vit_comp &q, double pi, double ia[4], double ib[4])
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
        if (AP && soft_inp<COL, DIFF>(e, 0)) ia[e] += pi;
        if (AP && soft_inp<COL, DIFF>(e, 1)) ib[e] += pi;
    }
}

__device__ __forceinline__ void soft_normalise(const double o[4], double m[4])
{
    const double mn = fmin(fmin(o[0], o[1]), fmin(o[2], o[3]));
#pragma unroll
    for (int s = 0; s < 4; ++s) m[s] = o[s] - mn;
}

// ã_k -> ã_{k+1}
template <int COL, int DIFF, bool AP>
__device__ __forceinline__ void soft_fwd(double m[4], const vit_comp &q, double pi)
{
    double ia[4], ib[4], o[4];
    soft_incs<COL, DIFF, AP>(q, pi, ia, ib);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int sa = COL == 0 ? (e & 1) : (e & 2), sb = COL == 0 ? (e & 1) + 2 : (e & 2) + 1;
        o[e] = fmin(m[sa] + ia[e], m[sb] + ib[e]);
    }
    soft_normalise(o, m);
}

// b̃_{k+1} -> b̃_k: start state s leaves to e0 / e1 as the sec-th listed branch into each, inc + b̃(end)
template <int COL, int DIFF, bool AP>
__device__ __forceinline__ void soft_bwd(double b[4], const vit_comp &q, double pi)
{
    double ia[4], ib[4], o[4];
    soft_incs<COL, DIFF, AP>(q, pi, ia, ib);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int sec = COL == 0 ? s >> 1 : s & 1;
        const int e0 = COL == 0 ? (s & 1) : (s & 2), e1 = COL == 0 ? (s & 1) + 2 : (s & 2) + 1;
        o[s] = fmin((sec ? ib[e0] : ia[e0]) + b[e0], (sec ? ib[e1] : ia[e1]) + b[e1]);
    }
    soft_normalise(o, b);
}

// λ_k from a = ã_k, b = b̃_{k+1} and the CHANNEL increment (so under a prior it is extrinsic), then b -> b̃_k
template <int COL, int DIFF, bool AP>
__device__ __forceinline__ double soft_llr(const double a[4], double b[4], const vit_comp &q, double pi)
{
    double ia[4], ib[4];
    soft_incs<COL, DIFF, false>(q, 0.0, ia, ib);
    double m0 = __builtin_inf(), m1 = __builtin_inf();
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int sa = COL == 0 ? (e & 1) : (e & 2), sb = COL == 0 ? (e & 1) + 2 : (e & 2) + 1;
        const double ta = (a[sa] + ia[e]) + b[e], tb = (a[sb] + ib[e]) + b[e];
        if (soft_inp<COL, DIFF>(e, 0)) m1 = fmin(m1, ta); else m0 = fmin(m0, ta);
        if (soft_inp<COL, DIFF>(e, 1)) m1 = fmin(m1, tb); else m0 = fmin(m0, tb);
    }
    soft_bwd<COL, DIFF, AP>(b, q, pi);
    return m1 - m0;
}

// soft_llr, and *branch = the branch b* (list order, b = 2 start + lsb) with the smallest of the eight sums
// T(b) = (a(start b) + inc(b)) + b(end b) it forms, ties to the smallest b
template <int COL, int DIFF, bool AP>
__device__ __forceinline__ double soft_llr_branch(const double a[4], double b[4], const vit_comp &q, double pi, int *branch)
{
    double ia[4], ib[4], t[8];
    soft_incs<COL, DIFF, false>(q, 0.0, ia, ib);
    double m0 = __builtin_inf(), m1 = __builtin_inf();
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int sa = COL == 0 ? (e & 1) : (e & 2), sb = COL == 0 ? (e & 1) + 2 : (e & 2) + 1;
        const int lsb = COL == 0 ? e >> 1 : e & 1;
        const double ta = (a[sa] + ia[e]) + b[e], tb = (a[sb] + ib[e]) + b[e];
        if (soft_inp<COL, DIFF>(e, 0)) m1 = fmin(m1, ta); else m0 = fmin(m0, ta);
        if (soft_inp<COL, DIFF>(e, 1)) m1 = fmin(m1, tb); else m0 = fmin(m0, tb);
        t[2 * sa + lsb] = ta;
        t[2 * sb + lsb] = tb;
    }
    int best = 0;
    double tv = t[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) {
        const bool lt = t[i] < tv;
        best = lt ? i : best;
        tv = lt ? t[i] : tv;
    }
    *branch = best;
    soft_bwd<COL, DIFF, AP>(b, q, pi);
    return m1 - m0;
}

// ---- a lane's chunk and its walks --------------------------------------------------------------------------------------------
template <bool PACKED>
__device__ __forceinline__ const double2 *soft_row(const double *rows, int64_t k)
{
    return reinterpret_cast<const double2 *>(rows) + (PACKED ? 2 : 3) * k;
}

__device__ __forceinline__ void soft_put4(double *p, const double m[4]) { *reinterpret_cast<double4 *>(p) = make_double4(m[0], m[1], m[2], m[3]); }

__device__ __forceinline__ void soft_get4(const double *p, double m[4])
{
    const double4 v = *reinterpret_cast<const double4 *>(p);
    m[0] = v.x; m[1] = v.y; m[2] = v.z; m[3] = v.w;
}

// What a lane works on.  Rows, priors and outputs are addressed by their index in the burst.
struct soft_chunk {
    int64_t a, e;           // its rows
    int64_t lo, hi;         // the rows a warm-up may not cross: the burst's, or its window's
    int64_t frec, brec;     // its forward / backward record {start[4], end[4]}, at 8 x these
    int64_t lane, lanes;    // ã_k of its row k lies at 4 ((k - a) lanes + lane): consecutive lanes write consecutive 32 B
};

// Chunk c of a burst of n rows cut into nch chunks of ch.  The backward records are kept in MIRRORED order, so that in
// both directions a record's predecessor is the one in front of it.
__device__ __forceinline__ soft_chunk soft_burst_chunk(int64_t c, int ch, int64_t n, int64_t nch)
{
    const int64_t a = c * ch;
    return soft_chunk{a, a + ch < n ? a + ch : n, 0, n, c, nch - 1 - c, c, nch};
}

template <bool PACKED, int DIFF, bool AP>
__device__ __forceinline__ void soft_fwd_row(double m[4], const double *rows, const soft_prior_t<AP> &pr, soft_win_t<AP> &w, int64_t k)
{
    const double pi = soft_prior_at(pr, w, k);
    if (k & 1) soft_fwd<1, DIFF, AP>(m, vit_components<1, PACKED>(soft_row<PACKED>(rows, k)), pi);
    else soft_fwd<0, DIFF, AP>(m, vit_components<0, PACKED>(soft_row<PACKED>(rows, k)), pi);
}

template <bool PACKED, int DIFF, bool AP>
__device__ __forceinline__ void soft_bwd_row(double b[4], const double *rows, const soft_prior_t<AP> &pr, soft_win_t<AP> &w, int64_t k)
{
    const double pi = soft_prior_at(pr, w, k);
    if (k & 1) soft_bwd<1, DIFF, AP>(b, vit_components<1, PACKED>(soft_row<PACKED>(rows, k)), pi);
    else soft_bwd<0, DIFF, AP>(b, vit_components<0, PACKED>(soft_row<PACKED>(rows, k)), pi);
}

// The chunk's own rows forward from m = ã_a: ã_k of every row stored, m left at ã_e.
template <bool PACKED, int DIFF, bool AP>
__device__ __forceinline__ void soft_fwd_own(const double *rows, const soft_prior_t<AP> &pr, soft_win_t<AP> &w, const soft_chunk &k, double *alpha, double m[4])
{
    for (int64_t r = k.a; r < k.e; ++r) {
        soft_put4(alpha + 4 * ((r - k.a) * k.lanes + k.lane), m);
        soft_fwd_row<PACKED, DIFF, AP>(m, rows, pr, w, r);
    }
}

// First launch.  Forward: ã at the chunk's start from zeros `warmup` rows earlier (exact where that reaches lo), then over
// its own rows; backward, the mirror: b̃ at its end from zeros `warmup` rows later (exact where that reaches hi), then
// back over its rows.  Each direction records {start, end}.
template <bool PACKED, int DIFF, bool AP>
__device__ __forceinline__ void soft_bounds_body(const double *rows, const soft_prior_t<AP> &pr, const soft_chunk &k, int warmup, double *fedge, double *bedge,
                                                 double *alpha)
{
    soft_win_t<AP> w;
    double m[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t r = k.a - warmup > k.lo ? k.a - warmup : k.lo; r < k.a; ++r) soft_fwd_row<PACKED, DIFF, AP>(m, rows, pr, w, r);
    soft_put4(fedge + 8 * k.frec, m);
    soft_fwd_own<PACKED, DIFF, AP>(rows, pr, w, k, alpha, m);
    soft_put4(fedge + 8 * k.frec + 4, m);

    double b[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t r = (k.e + warmup < k.hi ? k.e + warmup : k.hi) - 1; r >= k.e; --r) soft_bwd_row<PACKED, DIFF, AP>(b, rows, pr, w, r);
    soft_put4(bedge + 8 * k.brec, b);
    for (int64_t r = k.e - 1; r >= k.a; --r) soft_bwd_row<PACKED, DIFF, AP>(b, rows, pr, w, r);
    soft_put4(bedge + 8 * k.brec + 4, b);
}

// Repair of a chunk's record `rec` by one thread: start from the predecessor record's end `pred` as it is now, run the
// chunk (forward: rewriting its stored ã), rewrite the end; true when the end changed.
template <bool PACKED, bool BWD, int DIFF, bool AP>
__device__ __forceinline__ bool soft_rerun_body(const double *rows, const soft_prior_t<AP> &pr, const soft_chunk &k, double *rec, const double *pred, double *alpha)
{
    double m[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        m[q] = __hip_atomic_load(pred + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        rec[q] = m[q];
    }
    soft_win_t<AP> w;
    if (BWD)
        for (int64_t r = k.e - 1; r >= k.a; --r) soft_bwd_row<PACKED, DIFF, AP>(m, rows, pr, w, r);
    else
        soft_fwd_own<PACKED, DIFF, AP>(rows, pr, w, k, alpha, m);
    bool changed = false;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        changed |= __double_as_longlong(rec[4 + q]) != __double_as_longlong(m[q]);
        rec[4 + q] = m[q];
    }
    return changed;
}

// ... of record r >= 1 of a burst (record 0 is exact); forward: chunk r, backward: chunk nch - 1 - r
template <bool PACKED, bool BWD, int DIFF, bool AP>
__device__ __forceinline__ bool soft_burst_rerun(const double *rows, const soft_prior_t<AP> &pr, int64_t n, int ch, int64_t nch, double *edge, double *alpha, int64_t r)
{
    return soft_rerun_body<PACKED, BWD, DIFF, AP>(rows, pr, soft_burst_chunk(BWD ? nch - 1 - r : r, ch, n, nch), edge + 8 * r, edge + 8 * r - 4, alpha);
}

// Last launch: from the proven b̃ at the chunk's end back over the chunk, λ_k from the stored ã_k, then b̃_k.
template <bool PACKED, int DIFF, bool AP>
__device__ __forceinline__ void soft_llr_body(const double *rows, const soft_prior_t<AP> &pr, const soft_chunk &k, const double *bedge, const double *alpha,
                                              double *out, uint8_t *bits)
{
    double b[4], m[4];
    soft_win_t<AP> w;
    soft_get4(bedge + 8 * k.brec, b);
    for (int64_t r = k.e - 1; r >= k.a; --r) {
        soft_get4(alpha + 4 * ((r - k.a) * k.lanes + k.lane), m);
        const double2 *z = soft_row<PACKED>(rows, r);
        const double pi = soft_prior_at(pr, w, r);
        const double lam = r & 1 ? soft_llr<1, DIFF, AP>(m, b, vit_components<1, PACKED>(z), pi) : soft_llr<0, DIFF, AP>(m, b, vit_components<0, PACKED>(z), pi);
        out[r] = lam;
        bits[r] = lam + pi < 0.0 ? 1 : 0;
    }
}

// The last launch of wf_viterbi4_soft_branch: soft_llr_body, and the arg-min branch of every row beside its λ.
template <bool PACKED, int DIFF, bool AP>
__device__ __forceinline__ void soft_branch_body(const double *rows, const soft_prior_t<AP> &pr, const soft_chunk &k, const double *bedge, const double *alpha,
                                                 double *out, uint8_t *bits, uint8_t *branch)
{
    double b[4], m[4];
    soft_win_t<AP> w;
    soft_get4(bedge + 8 * k.brec, b);
    for (int64_t r = k.e - 1; r >= k.a; --r) {
        soft_get4(alpha + 4 * ((r - k.a) * k.lanes + k.lane), m);
        const double2 *z = soft_row<PACKED>(rows, r);
        const double pi = soft_prior_at(pr, w, r);
        int br;
        const double lam = r & 1 ? soft_llr_branch<1, DIFF, AP>(m, b, vit_components<1, PACKED>(z), pi, &br)
                                 : soft_llr_branch<0, DIFF, AP>(m, b, vit_components<0, PACKED>(z), pi, &br);
        out[r] = lam;
        bits[r] = lam + pi < 0.0 ? 1 : 0;
        branch[r] = (uint8_t)br;
    }
}

// a burst's repair lists empty, nobody arrived (both directions): by the first launch, for the two behind it
__device__ __forceinline__ void soft_burst_clear_lists(double *fedge, double *bedge, int64_t nch)
{
    if (blockIdx.x == 0 && threadIdx.x < VIT_HDR) {
        reinterpret_cast<uint64_t *>(fedge + 8 * nch)[threadIdx.x] = 0;
        reinterpret_cast<uint64_t *>(bedge + 8 * nch)[threadIdx.x] = 0;
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

// ---- what the entry points share (host) ---------------------------------------------------------------------------------
// The argument checks, in the name `who` of the entry point that was called.  prior, windows: NULL where the entry point
// has no such argument (whether it allows NULL is its own business); `aligned` is its sentence on the alignments, which
// names what it takes.
static int soft_check_args(const char *who, const wf_ctx *ctx, const double *rows, int64_t ncalls, int row_bytes, int warmup, const float *prior, double scale,
                           const int64_t *windows, const double *out, const uint8_t *bits, const char *aligned)
{
    const auto mis = [](const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; };
    WF_REQUIRE(ctx && rows && out && bits, "%s: NULL argument", who);
    WF_REQUIRE(ncalls >= 1 && warmup >= 0, "%s: bad argument", who);
    WF_REQUIRE(row_bytes == 32 || row_bytes == 48, "%s: row_bytes must be 32 (packed) or 48 (3 complex128)", who);
    WF_REQUIRE(std::isfinite(scale), "%s: apriori_scale must be finite", who);
    WF_REQUIRE(!mis(rows, 15) && !mis(out, 7) && !mis(prior, 3) && !mis(windows, 7), "%s: %s", who, aligned);
    return WF_OK;
}

// ... and, once the geometry is known: one launch must hold a lane per chunk; the context's scratch, `words` doubles
static int soft_reserve(const char *who, wf_ctx *ctx, int64_t lanes, size_t words)
{
    WF_REQUIRE((lanes + SOFT_THREADS - 1) / SOFT_THREADS < (1ll << 31), "%s: burst too long for one launch", who);
    WF_HIP(hipSetDevice(ctx->device));
    return wf_ctx_reserve_vit(ctx, words);
}

// The two fix-up launches between the first and the last one, as the hard detectors (wf_viterbi.hip: viterbi_launch):
// repair, or only count under WF_OPT_DET_REPAIR = 1; WF_OPT_DET_FINAL_VERIFY adds a counting pass behind the repairs.
// launch(bwd, mode): the caller's fix-up kernel of direction decltype(bwd)::value.
template <class F>
static int soft_fixup_passes(const wf_ctx *ctx, F &&launch)
{
    const int passes = ctx->opt[WF_OPT_DET_REPAIR] == 0 && ctx->opt[WF_OPT_DET_FINAL_VERIFY] ? 2 : 1;
    for (int pass = 0; pass < passes; ++pass) {
        const int mode = pass == 0 && ctx->opt[WF_OPT_DET_REPAIR] == 0 ? 1 : 0;
        launch(std::false_type{}, mode);
        WF_LAUNCH_CHECK();
        launch(std::true_type{}, mode);
        WF_LAUNCH_CHECK();
    }
    return WF_OK;
}

// run(packed, diff) with the row form and `differential` as compile-time constants (decltype(packed)::value, ...)
template <class F>
static int soft_dispatch(int row_bytes, int differential, F &&run)
{
    using d0 = std::integral_constant<int, 0>;
    using d1 = std::integral_constant<int, 1>;
    if (row_bytes == 32) return differential ? run(std::true_type{}, d1{}) : run(std::true_type{}, d0{});
    return differential ? run(std::false_type{}, d1{}) : run(std::false_type{}, d0{});
}
