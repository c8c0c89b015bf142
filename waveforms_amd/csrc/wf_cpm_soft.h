// wf_cpm_soft.h — device code, launch geometry and trellis tables shared by the soft-output CPM detectors: wf_cpm_soft.hip
// (wf_cpm_soft) and wf_cpm_soft_apriori.hip (wf_cpm_soft_apriori).  Both cut a burst into the same chunks and lay the
// context's scratch out the same way, so one geometry call describes either.
//
// Everything here carries the template argument AP: false is the plain detector (no prior anywhere: the code it had when it
// lived in wf_cpm_soft.hip), true adds the per-bit prior of include/wfhip.h (wf_cpm_soft_apriori):
//   * the lgM TB float32 priors of a staged batch of TB calls come in next to its rows, one per lane, and go as
//     π = scale * (double)prior into one 256-byte LDS slot per wave (every lane of the wave needs the same lgM values per
//     call: a broadcast LDS read, no per-lane global load in the inner loop);
//   * inc'(s, u) = inc(s, u) + Π(u) for u != 0, one addition on the branch, before the exchange
//     (forward) and before the minimum (backward);
//   * the λ step leaves the own bit's prior out and keeps the other bit's (M = 4).
// The last launch also carries BR (plain only): true adds the decided branch and its term per call (wf_cpm_soft_branch,
// wf_cpm_carrier.hip); false compiles to the code without it.
// The kernels themselves are thin wrappers around the cs_*_body functions, so each file names its own.
#pragma once
#include <stddef.h>
#include <string.h>

#include "wf_cpm_detect.h"
#include "wf_cpm_wide.h"

#define CS_WAVES 4                      // chunks (waves) per workgroup
#define CS_THREADS (64 * CS_WAVES)
#define CS_XS 68                        // forward exchange: candidate j of end lane e at word j * CS_XS + e
#define CS_SUB 16                       // calls per λ sub-block = checkpoint spacing
#define CS_REC 128                      // proof record words per chunk: metrics at the start [64], at the end [64]
#define CS_WAVE_BYTES (64 * 16 + 4 * CS_XS * 8)    // staged rows (one 16-B piece per lane) + exchange
#define CS_PRIOR_BYTES 256              // AP: π of the staged batch's calls, lgM TB <= 32 float64
#define CS_WAVE_BYTES_AP (CS_WAVE_BYTES + CS_PRIOR_BYTES)

static constexpr int kCsDefaultWarmup = 64;      // calls (the hard wide form's)
static constexpr int64_t kCsChunks = 8192;       // chunks a burst is cut into by default: 8 waves per SIMD of 256 CUs
static constexpr int kCsMinChunk = 64;
static constexpr int kCsMaxChunk = 8192;         // = the WF_OPT_CPM_SOFT_CHUNK_CALLS range

struct cpm_soft_params {
    int M, p, nh, K0, K1, Lp, S;
    int dt[3];                  // tilt(n + 1) - tilt(n) mod 2p by the variant of call n's leaving symbol: (M - 1) K; 0 pre-start
    int ch, W;
    int64_t n, n0, nch, nsub;   // calls, global index of call 0, chunks, checkpoints per chunk
    // SEG only (wf_cpm_segments.hip; a burst's kernels never read them): n is then a SEGMENT's calls and nch the launch's chunks,
    // cps of them per segment; per segment the rows and the rotation table advance by row_stride / rot_stride double2, the
    // outputs by out_stride calls
    int64_t row_stride, out_stride;
    int cps, rot_stride;
    // dest[kv][s][u] = 4 * end state + slot of branch (s, u); kv 0 / 1: the leaving symbol uses K[0] / K[1], 2: pre-start
    uint8_t dest[3][64][4];
};

struct cpm_soft_prior {         // AP: lgM n float32 (bit i of call k at [lgM k + i]) and the scale π is formed with
    const float *p;
    double scale;
};

template <int M, int LP, bool AP = false>
struct cs_lane {
    static constexpr int NF = LP == 1 ? M : (LP == 2 ? M * M : M * M * M);
    static constexpr int TB = 64 / NF;      // calls per staged batch: one 16-B piece of a row per lane
    static constexpr int LGM = M == 4 ? 2 : 1;
    static constexpr int WAVE_BYTES = AP ? CS_WAVE_BYTES_AP : CS_WAVE_BYTES;
    static_assert(LGM * TB * 8 <= CS_PRIOR_BYTES, "a staged batch's priors fit the wave's slot");
    const double2 *rows;
    double2 *rowbuf;
    double *xch;
    const double *rot;
    int lane, v2, zoff;
    bool active;
    uint32_t dsel[3];
    // AP only.  Held per lane (vector registers) on purpose: the forward repair kernel has no scalar registers to spare.
    const float *pp;            // prior.p + lane: staging lane `lane` fetches the batch's value `lane`
    double scale;               // prior.scale in the staging lanes (the first LGM TB), 0 elsewhere
    double *pri;                // AP only: the wave's slot, π of bit i of the call staged in slot t at [LGM t + i]
};

template <int M, int LP, bool AP>
__device__ __forceinline__ cs_lane<M, LP, AP> cs_setup(const double2 *rows, const cpm_soft_params &P, char *wbase, const double *rot,
                                                       const cpm_soft_prior &prior = cpm_soft_prior{nullptr, 0.0})
{
    cs_lane<M, LP, AP> L;
    L.rows = rows;
    L.rowbuf = reinterpret_cast<double2 *>(wbase);
    L.xch = reinterpret_cast<double *>(wbase + 64 * 16);
    L.rot = rot;
    L.lane = threadIdx.x & 63;
    L.active = L.lane < P.S;
    const int s = L.active ? L.lane : 0;            // (lanes that hold no state compute on state 0 and never publish it)
    L.v2 = 2 * (s % P.p);
    L.zoff = M * (s / P.p);
#pragma unroll
    for (int kv = 0; kv < 3; ++kv) L.dsel[kv] = *reinterpret_cast<const uint32_t *>(&P.dest[kv][s][0]);
    L.pp = prior.p + L.lane;
    L.scale = L.lane < cs_lane<M, LP, AP>::LGM * cs_lane<M, LP, AP>::TB ? prior.scale : 0.0;
    L.pri = reinterpret_cast<double *>(wbase + CS_WAVE_BYTES);
    return L;
}

__device__ __forceinline__ void cs_stage_rot(const double2 *__restrict__ rot_cs, const cpm_soft_params &P, double *rot)   // the caller synchronises
{
    for (int k = threadIdx.x; k < 2 * P.p; k += blockDim.x) {
        const double2 e = rot_cs[k];
        rot[k] = e.x;
        rot[CPM_ROT_SIN + k] = e.y;
    }
}

// SEG: the table of ONE wave's segment, staged by that wave into its own copy (waves of a workgroup may belong to different segments)
__device__ __forceinline__ void cs_stage_rot_wave(const double2 *__restrict__ rot_cs, const cpm_soft_params &P, double *rot)
{
    wide_wave_sync();                                // (a repair's previous record has been read to its end)
    for (int k = threadIdx.x & 63; k < 2 * P.p; k += 64) {
        const double2 e = rot_cs[k];
        rot[k] = e.x;
        rot[CPM_ROT_SIN + k] = e.y;
    }
    wide_wave_sync();
}

// Chunk c of the launch: calls a .. e - 1 of segment seg.  A burst is segment 0 and c counts its chunks; with SEG every segment
// is cut into cps chunks from its own start, so chunk c is (segment c / cps, index c % cps): no table, no search, and a chunk
// never crosses a segment.  The calls are counted from the segment's start, and P.n is its length: the clamps of cs_sweep and
// the warm-ups' limits are then the segment's, as they are the burst's.
struct cs_chunk {
    int64_t a, e;
    uint32_t seg;
};

// cps: P.cps, wherever the caller holds it (seg comes back in the same kind of register; a and e are scalar)
template <bool SEG>
__device__ __forceinline__ cs_chunk cs_find(const cpm_soft_params &P, int64_t c, uint32_t cps)
{
    uint32_t seg = 0;
    int64_t j = c;
    if constexpr (SEG) {                             // (a launch of segments holds fewer than 2^31 chunks)
        seg = (uint32_t)c / cps;
        j = __builtin_amdgcn_readfirstlane((uint32_t)c - seg * cps);
    }
    const int64_t a = j * P.ch;
    return cs_chunk{a, a + P.ch < P.n ? a + P.ch : P.n, seg};
}

// Wave-uniform values held in VECTOR registers from here on: the segments' per-wave offsets are added to per-lane indices
// anyway, and the repair kernels have no scalar registers to spare.
__device__ __forceinline__ int64_t cs_in_vgpr(int64_t v)
{
    asm("" : "+v"(v));
    return v;
}

__device__ __forceinline__ uint32_t cs_in_vgpr(uint32_t v)
{
    asm("" : "+v"(v));
    return v;
}

__device__ __forceinline__ const double2 *cs_in_vgpr(const double2 *global_ptr)       // (stays a pointer to global memory)
{
    uintptr_t v = reinterpret_cast<uintptr_t>(global_ptr);
    asm("" : "+v"(v));
    return (const double2 *)(const __attribute__((address_space(1))) double2 *)v;
}

__device__ __forceinline__ int cs_kv(const cpm_soft_params &P, int64_t n)
{
    const int64_t m_old = n - P.Lp + 1;             // the symbol that leaves the window at call n
    return m_old < 0 ? 2 : (P.nh == 2 ? (int)(m_old & 1) : 0);
}

__device__ __forceinline__ uint32_t cs_pick(const uint32_t d[3], int kv) { return kv == 0 ? d[0] : (kv == 1 ? d[1] : d[2]); }

// the M increments of the branches that leave this lane's state at the call staged in slot t
template <int M, int LP, bool AP>
__device__ __forceinline__ void cs_incs(const cs_lane<M, LP, AP> &L, const cpm_soft_params &P, int t, int tilt, double inc[M])
{
    int r = L.v2 - tilt;
    r += r < 0 ? 2 * P.p : 0;
    const double cr = L.rot[r], sr = L.rot[CPM_ROT_SIN + r];
    const double2 *z = L.rowbuf + t * cs_lane<M, LP, AP>::NF + L.zoff;
#pragma unroll
    for (int u = 0; u < M; ++u) {
        const double2 q = z[u];
        inc[u] = -fma(cr, q.x, sr * q.y);            // -Re(e^{-j theta} Z), cpm_oracle.c:151
    }
}

// AP: π_{k,i} of the call staged in slot t (the same in every lane)
template <int M, int LP, bool AP>
__device__ __forceinline__ void cs_pi(const cs_lane<M, LP, AP> &L, int t, double pi[cs_lane<M, LP, AP>::LGM])
{
#pragma unroll
    for (int i = 0; i < cs_lane<M, LP, AP>::LGM; ++i) pi[i] = L.pri[cs_lane<M, LP, AP>::LGM * t + i];
}

// AP: inc -> inc' = inc + Π(u), u != 0 (bit 0 = MSB of u)
template <int M>
__device__ __forceinline__ void cs_add_prior(double inc[M], const double *pi)
{
    if constexpr (M == 2) {
        inc[1] += pi[0];
    } else {
        inc[1] += pi[1];
        inc[2] += pi[0];
        inc[3] += pi[0] + pi[1];
    }
}

// the increments the recursions run over: inc (plain), inc' (AP)
template <int M, int LP, bool AP>
__device__ __forceinline__ void cs_rec_incs(const cs_lane<M, LP, AP> &L, const cpm_soft_params &P, int t, int tilt, double inc[M])
{
    cs_incs(L, P, t, tilt, inc);
    if constexpr (AP) {
        double pi[cs_lane<M, LP, AP>::LGM];
        cs_pi(L, t, pi);
        cs_add_prior<M>(inc, pi);
    }
}

// ã_k -> ã_{k+1}: candidates into the end states' exchange slots, each end lane takes the minimum of its M, then the
// wave-wide normalisation.  m = +inf in lanes that hold no state (their candidates park in their own column).
template <int M, int LP, bool AP>
__device__ __forceinline__ void cs_fwd(const cs_lane<M, LP, AP> &L, const cpm_soft_params &P, int t, int tilt, int kv, double &m)
{
    double inc[M];
    cs_rec_incs(L, P, t, tilt, inc);
    const uint32_t d = cs_pick(L.dsel, kv);
#pragma unroll
    for (int u = 0; u < M; ++u) {
        const int dst = (int)((d >> (8 * u)) & 0xFFu);
        L.xch[L.active ? (dst & 3) * CS_XS + (dst >> 2) : u * CS_XS + L.lane] = m + inc[u];
    }
    wide_wave_sync();
    double best = L.xch[L.lane];
#pragma unroll
    for (int j = 1; j < M; ++j) best = wide_min_raw(best, L.xch[j * CS_XS + L.lane]);
    wide_wave_sync();                                // read before the next call's candidates land
    m = best - wide_wave_min(best);
}

// b̃_{k+1} of the M end states of this lane's branches (ds_bpermute from the end lanes)
template <int M, int LP, bool AP>
__device__ __forceinline__ void cs_gather(const cs_lane<M, LP, AP> &L, int kv, double b, double g[M])
{
    const uint32_t d = cs_pick(L.dsel, kv);
#pragma unroll
    for (int u = 0; u < M; ++u) {
        const int e = L.active ? (int)((d >> (8 * u + 2)) & 63u) : L.lane;
        g[u] = __longlong_as_double((long long)wide_bperm_u64(e << 2, (uint64_t)__double_as_longlong(b)));
    }
}

// b̃_{k+1} -> b̃_k, from increments and gathered b̃_{k+1}
template <int M, int LP, bool AP>
__device__ __forceinline__ void cs_bwd_from(const cs_lane<M, LP, AP> &L, const double inc[M], const double g[M], double &b)
{
    double best = inc[0] + g[0];
#pragma unroll
    for (int u = 1; u < M; ++u) best = wide_min_raw(best, inc[u] + g[u]);
    best = L.active ? best : __builtin_inf();
    b = best - wide_wave_min(best);
}

template <int M, int LP, bool AP>
__device__ __forceinline__ void cs_bwd(const cs_lane<M, LP, AP> &L, const cpm_soft_params &P, int t, int tilt, int kv, double &b)
{
    double inc[M], g[M];
    cs_rec_incs(L, P, t, tilt, inc);
    cs_gather(L, kv, b, g);
    cs_bwd_from(L, inc, g, b);
}

// λ_{k,i} (into lam, uniform across the wave) from a = ã_k(s) and b = b̃_{k+1}, then b -> b̃_k.  AP: λᵉ — bit i's minima
// run over inc plus the prior of the OTHER bit of u where that bit is 1 (M = 2: over inc alone) — and π_{k,i} into pi.
// BR (plain only): the branch b* = M s* + u* with the smallest T = tt over the wave, ties to the smallest b, and its term q = (x, y)
// (include/wfhip.h, wf_cpm_soft_branch).  The argmin lives in the lanes: per-lane minimum over u, the wave-wide minimum (the
// smaller of the two minima bit 0's λ has just taken: every (s, u) is in one of them), a ballot of the lanes that hold it —
// the lowest is s* — and the smallest u of that lane that attains it.  bsel = b* in lane s*, -1 in every other lane; q is
// formed in lane s* alone.  Every T is >= +0 and never -0: equal operands are bitwise equal.
template <int M, int LP, bool AP, bool BR = false>
__device__ __forceinline__ void cs_llr(const cs_lane<M, LP, AP> &L, const cpm_soft_params &P, int t, int tilt, int kv, double a, double &b,
                                       double lam[cs_lane<M, LP, AP>::LGM], double pi[cs_lane<M, LP, AP>::LGM], int &bsel, double2 &q)
{
    static_assert(!(AP && BR), "the branch output is the plain detector's");
    double inc[M], g[M], tt[M];
    cs_incs(L, P, t, tilt, inc);
    cs_gather(L, kv, b, g);
    const double av = L.active ? a : __builtin_inf();
    if constexpr (!AP) {
#pragma unroll
        for (int u = 0; u < M; ++u) tt[u] = (av + inc[u]) + g[u];
        double w1, w0;                               // bit 0's two minima over the wave: the smaller is the minimum of all T
        if constexpr (M == 2) {
            w1 = wide_wave_min(tt[1]);
            w0 = wide_wave_min(tt[0]);
            lam[0] = w1 - w0;
        } else {                                     // bit 0 = MSB of U: 1 for U in {2, 3}; bit 1 = LSB: 1 for U in {1, 3}
            w1 = wide_wave_min(wide_min_raw(tt[2], tt[3]));
            w0 = wide_wave_min(wide_min_raw(tt[0], tt[1]));
            lam[0] = w1 - w0;
            lam[1] = wide_wave_min(wide_min_raw(tt[1], tt[3])) - wide_wave_min(wide_min_raw(tt[0], tt[2]));
        }
        if constexpr (BR) {
            double lm = tt[0];
#pragma unroll
            for (int u = 1; u < M; ++u) lm = wide_min_raw(lm, tt[u]);
            const double wm = wide_min_raw(w1, w0);  // = wide_wave_min(lm): no further pass over the wave
            const unsigned long long held = __builtin_amdgcn_ballot_w64(lm == wm);       // (lanes that hold no state carry +inf)
            const int sstar = held ? __builtin_ctzll(held) : 0;                          // (held = 0: rows that are not finite)
            bsel = -1;
            if (L.lane == sstar) {
                int us = M - 1;
                double x = inc[M - 1];
#pragma unroll
                for (int u = M - 2; u >= 0; --u) {
                    const bool hit = tt[u] == wm;
                    us = hit ? u : us;
                    x = hit ? inc[u] : x;
                }
                int r = L.v2 - tilt;
                r += r < 0 ? 2 * P.p : 0;
                const double cr = L.rot[r], sr = L.rot[CPM_ROT_SIN + r];
                const double2 z = L.rowbuf[t * cs_lane<M, LP, AP>::NF + L.zoff + us];
                bsel = M * sstar + us;
                q = make_double2(x, -fma(cr, z.y, -(sr * z.x)));
            }
        }
    } else {
        cs_pi(L, t, pi);
        if constexpr (M == 2) {
#pragma unroll
            for (int u = 0; u < M; ++u) tt[u] = (av + inc[u]) + g[u];
            lam[0] = wide_wave_min(tt[1]) - wide_wave_min(tt[0]);
            inc[1] += pi[0];
        } else {
            const double i1 = inc[1] + pi[1], i2 = inc[2] + pi[0];                  // = inc'(u = 1), inc'(u = 2)
            const double t0 = (av + inc[0]) + g[0];
            // bit 0 (MSB): the LSB's prior π_1 on u = 1, 3
            const double m1 = wide_min_raw((av + inc[2]) + g[2], (av + (inc[3] + pi[1])) + g[3]);
            const double m0 = wide_min_raw(t0, (av + i1) + g[1]);
            lam[0] = wide_wave_min(m1) - wide_wave_min(m0);
            // bit 1 (LSB): the MSB's prior π_0 on u = 2, 3
            const double n1 = wide_min_raw((av + inc[1]) + g[1], (av + (inc[3] + pi[0])) + g[3]);
            const double n0 = wide_min_raw(t0, (av + i2) + g[2]);
            lam[1] = wide_wave_min(n1) - wide_wave_min(n0);
            inc[1] = i1;
            inc[2] = i2;
            inc[3] += pi[0] + pi[1];
        }
    }
    cs_bwd_from(L, inc, g, b);
}

// Calls lo .. hi - 1 (FWD: ascending, else descending), rows staged through the wave's LDS in batches of TB calls (the next
// batch in flight while this one runs; AP: and the batch's LGM TB priors, one per lane of the first LGM TB lanes, 0 where
// the batch reaches outside the burst).  body(k, t, tilt, kv): call k, in slot t of the staged batch, with its tilt and
// variant (tilt tracked call by call: tilt(n + 1) = tilt(n) + dt[kv(n)] mod 2p).
template <int M, int LP, bool FWD, bool AP, class F>
__device__ __forceinline__ void cs_sweep(const cs_lane<M, LP, AP> &L, const cpm_soft_params &P, int64_t lo, int64_t hi, F &&body)
{
    constexpr int NF = cs_lane<M, LP, AP>::NF, TB = cs_lane<M, LP, AP>::TB, LGM = cs_lane<M, LP, AP>::LGM;
    if (lo >= hi) return;
    const int64_t nb = (hi - lo + TB - 1) / TB;
    const int p2 = 2 * P.p;
    auto fetch = [&](int64_t b) __attribute__((always_inline)) {
        int64_t row = (FWD ? lo + b * TB : hi - (b + 1) * TB) + L.lane / NF;
        row = row < 0 ? 0 : (row >= P.n ? P.n - 1 : row);          // (never used when clamped)
        return L.rows[row * NF + L.lane % NF];
    };
    auto fetch_prior = [&](int64_t b) __attribute__((always_inline)) {
        const int64_t rb = FWD ? lo + b * TB : hi - (b + 1) * TB, call = rb + L.lane / LGM;
        return L.lane < LGM * TB && call >= 0 && call < P.n ? L.pp[LGM * rb] : 0.0f;
    };
    int tilt = cpm_tilt(P.M, P.p, P.nh, P.K0, P.K1, P.Lp, P.n0 + (FWD ? lo : hi));
    double2 pend = fetch(0);
    float ppend = 0.0f;
    if constexpr (AP) ppend = fetch_prior(0);
    for (int64_t b = 0; b < nb; ++b) {
        L.rowbuf[L.lane] = pend;
        if constexpr (AP) {
            if (L.lane < LGM * TB) L.pri[L.lane] = L.scale * (double)ppend;     // π, formed once per staged value
        }
        if (b + 1 < nb) {
            pend = fetch(b + 1);
            if constexpr (AP) ppend = fetch_prior(b + 1);
        }
        wide_wave_sync();
        if constexpr (FWD) {
            const int64_t kb = lo + b * TB;
#pragma unroll 1
            for (int t = 0; t < TB; ++t) {
                const int64_t k = kb + t;
                if (k >= hi) break;
                const int kv = cs_kv(P, P.n0 + k);
                body(k, t, tilt, kv);
                tilt += P.dt[kv];
                tilt -= tilt >= p2 ? p2 : 0;
            }
        } else {
            const int64_t kb = hi - (b + 1) * TB;
#pragma unroll 1
            for (int t = TB - 1; t >= 0; --t) {
                const int64_t k = kb + t;
                if (k < lo) break;
                const int kv = cs_kv(P, P.n0 + k);
                tilt -= P.dt[kv];
                tilt += tilt < 0 ? p2 : 0;
                body(k, t, tilt, kv);
            }
        }
        wide_wave_sync();                            // batch consumed before the next stash
    }
}

// forward over the chunk's calls a .. e - 1 from m = ã_a, checkpoint j = ã_{a + j CS_SUB} stored (S doubles each)
template <int M, int LP, bool AP>
__device__ __forceinline__ void cs_fwd_chunk(const cs_lane<M, LP, AP> &L, const cpm_soft_params &P, int64_t a, int64_t e, double *__restrict__ ck, double &m)
{
    cs_sweep<M, LP, true>(L, P, a, e, [&](int64_t k, int t, int tilt, int kv) __attribute__((always_inline)) {
        const int off = (int)(k - a);
        if ((off & (CS_SUB - 1)) == 0 && L.active) ck[(off / CS_SUB) * P.S + L.lane] = m;
        cs_fwd(L, P, t, tilt, kv, m);
    });
}

// ---- the four steps (wf_cpm_soft.hip describes them); smem: CS_WAVES * WAVE_BYTES, rot: 2 * CPM_ROT_SIN doubles -------------
// SEG (plain only; wf_cpm_segments.hip): the launch's chunks are those of P.nch / P.cps independent segments (cs_find); rot then
// holds CS_WAVES tables, one per wave.  Records and checkpoints are indexed by the launch's chunk in either case, the backward
// records mirrored over the LAUNCH (record r = chunk nch - 1 - r): nch is a multiple of cps, so in both directions the records
// r with r % cps == 0 are those of the chunks that start at their segment's edge - exact, as record 0 of a burst is: never
// compared with a predecessor and never handed a repair.
template <int M, int LP, bool AP, bool SEG = false>
__device__ __forceinline__ void cs_bounds_body(char *smem, double *rot, const double2 *__restrict__ rows, const double2 *__restrict__ rot_cs,
                                               uint64_t *__restrict__ fedge, uint64_t *__restrict__ bedge, double *__restrict__ ckpt,
                                               const cpm_soft_params &P, const cpm_soft_prior &prior)
{
    static_assert(!(AP && SEG), "the segments are the plain detector's");
    if constexpr (!SEG) cs_stage_rot(rot_cs, P, rot);
    if (blockIdx.x == 0 && threadIdx.x < CPM_NLIST) {          // the repair lists of both directions: empty
        cpm_list_counts(fedge, P.nch, CS_REC)[threadIdx.x] = 0;
        cpm_list_counts(bedge, P.nch, CS_REC)[threadIdx.x] = 0;
    }
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t c = (int64_t)blockIdx.x * CS_WAVES + wave;
    if (c >= P.nch) return;
    const cs_chunk k = cs_find<SEG>(P, c, (uint32_t)P.cps);
    if constexpr (SEG) {
        rot += cs_in_vgpr((int64_t)wave * 2 * CPM_ROT_SIN);
        rows += cs_in_vgpr((int64_t)k.seg * P.row_stride);
        cs_stage_rot_wave(rot_cs + (int64_t)k.seg * P.rot_stride, P, rot);
    }
    const cs_lane<M, LP, AP> L = cs_setup<M, LP, AP>(rows, P, smem + wave * cs_lane<M, LP, AP>::WAVE_BYTES, rot, prior);
    const int64_t a = k.a, e = k.e;

    double m = L.active ? 0.0 : __builtin_inf();
    cs_sweep<M, LP, true>(L, P, a - P.W > 0 ? a - P.W : 0, a, [&](int64_t, int t, int tilt, int kv) __attribute__((always_inline)) { cs_fwd(L, P, t, tilt, kv, m); });
    uint64_t *fr = fedge + c * CS_REC;
    if (L.active) fr[L.lane] = (uint64_t)__double_as_longlong(m);
    cs_fwd_chunk(L, P, a, e, ckpt + (size_t)c * P.nsub * P.S, m);
    if (L.active) fr[64 + L.lane] = (uint64_t)__double_as_longlong(m);

    double b = L.active ? 0.0 : __builtin_inf();
    cs_sweep<M, LP, false>(L, P, e, e + P.W < P.n ? e + P.W : P.n, [&](int64_t, int t, int tilt, int kv) __attribute__((always_inline)) { cs_bwd(L, P, t, tilt, kv, b); });
    uint64_t *br = bedge + (P.nch - 1 - c) * CS_REC;
    if (L.active) br[L.lane] = (uint64_t)__double_as_longlong(b);
    cs_sweep<M, LP, false>(L, P, a, e, [&](int64_t, int t, int tilt, int kv) __attribute__((always_inline)) { cs_bwd(L, P, t, tilt, kv, b); });
    if (L.active) br[64 + L.lane] = (uint64_t)__double_as_longlong(b);
}

// Every record against its predecessor: a wave per record r >= 1, lane = state.  Failed records are LISTED (list 0) for
// the repair launches, or (repair = 0) counted as unproven.  cps != 0 (segments): the records r % cps == 0 are exact, not compared.
__device__ __forceinline__ void cs_verify_body(uint64_t *__restrict__ edge, int64_t nch, int S, unsigned long long *__restrict__ unmerged, int repair,
                                               int cps = 0)
{
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = idx / 64 + 1;
    const int s = (int)(idx & 63);
    bool bad = false;
    if (r < nch && s < S && (cps == 0 || r % cps != 0)) bad = edge[r * CS_REC + s] != edge[(r - 1) * CS_REC + 64 + s];
    const unsigned long long m = __builtin_amdgcn_ballot_w64(bad);
    if (s == 0 && m) {
        if (repair) {
            unsigned long long *counts = reinterpret_cast<unsigned long long *>(cpm_list_counts(edge, nch, CS_REC));
            cpm_list(edge, nch, CS_REC, 0)[atomicAdd(counts, 1ull)] = (uint64_t)r;
        } else {
            atomicAdd(unmerged, 1ull);
        }
    }
}

// One repair round (lists and invariant: wf_cpm_detect.h): a wave per listed record — start from the predecessor's end as
// it is now (it becomes the record's start), run the chunk's calls again in the record's direction, rewrite its end (and,
// forward, its checkpoints), and list the next record when the end changed.  finisher != 0: one workgroup that goes on,
// round after round, until a round hands nothing on.
template <int M, int LP, bool BWD, bool AP, bool SEG = false>
__device__ __forceinline__ void cs_repair_body(char *smem, double *rot, const double2 *__restrict__ rows, const double2 *__restrict__ rot_cs,
                                               uint64_t *__restrict__ edge, double *__restrict__ ckpt, unsigned long long *__restrict__ unmerged,
                                               const cpm_soft_params &P, const cpm_soft_prior &prior, int lin, int lout, int finisher)
{
    uint64_t *const counts = cpm_list_counts(edge, P.nch, CS_REC);
    int64_t cnt = (int64_t)__hip_atomic_load(&counts[lin], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cnt == 0) return;                                      // (the whole grid)
    static_assert(!(AP && SEG), "the segments are the plain detector's");
    if constexpr (!SEG) cs_stage_rot(rot_cs, P, rot);
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t cps = 0, rot_stride = 0;
    int64_t row_stride = 0;
    if constexpr (SEG) {
        rot += cs_in_vgpr((int64_t)wave * 2 * CPM_ROT_SIN);
        rows = cs_in_vgpr(rows);
        rot_cs = cs_in_vgpr(rot_cs);
        cps = cs_in_vgpr((uint32_t)P.cps);
        rot_stride = cs_in_vgpr((uint32_t)P.rot_stride);
        row_stride = cs_in_vgpr(P.row_stride);
    }
    cs_lane<M, LP, AP> L = cs_setup<M, LP, AP>(rows, P, smem + wave * cs_lane<M, LP, AP>::WAVE_BYTES, rot, prior);
    const int64_t stride = (int64_t)gridDim.x * CS_WAVES;
    for (;;) {
        const uint64_t *list = cpm_list(edge, P.nch, CS_REC, lin);
        for (int64_t idx = (int64_t)blockIdx.x * CS_WAVES + wave; idx < cnt; idx += stride) {
            const uint64_t rw = __hip_atomic_load(&list[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int64_t r = (int64_t)(((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(rw >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)rw));
            uint64_t *rec = edge + r * CS_REC;
            const uint64_t w = L.active ? __hip_atomic_load(&rec[64 + L.lane - CS_REC], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
            const uint64_t old_end = L.active ? __hip_atomic_load(&rec[64 + L.lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
            if (L.active) rec[L.lane] = w;
            double m = L.active ? __longlong_as_double((long long)w) : __builtin_inf();
            const int64_t c = BWD ? P.nch - 1 - r : r;
            const cs_chunk k = cs_find<SEG>(P, c, cps);
            if constexpr (SEG) {                               // this record's segment: its rows and its table
                L.rows = rows + (int64_t)k.seg * row_stride;
                cs_stage_rot_wave(rot_cs + k.seg * rot_stride, P, rot);
            }
            const int64_t a = k.a, e = k.e;
            if constexpr (BWD)
                cs_sweep<M, LP, false>(L, P, a, e, [&](int64_t, int t, int tilt, int kv) __attribute__((always_inline)) { cs_bwd(L, P, t, tilt, kv, m); });
            else
                cs_fwd_chunk(L, P, a, e, ckpt + (size_t)c * P.nsub * P.S, m);
            const uint64_t nw = (uint64_t)__double_as_longlong(m);
            const bool changed = __builtin_amdgcn_ballot_w64(L.active && nw != old_end) != 0ull;
            if (L.active) rec[64 + L.lane] = nw;
            if (L.lane == 0) {
                atomicAdd(unmerged + 1, 1ull);                 // [1]: chunk repairs run, [2]: ... that handed on
                if (changed) {
                    atomicAdd(unmerged + 2, 1ull);
                    if (r + 1 < P.nch && (!SEG || (uint32_t)(r + 1) % cps != 0))     // (SEG: the next record opens another segment)
                        cpm_list(edge, P.nch, CS_REC, lout)[atomicAdd(reinterpret_cast<unsigned long long *>(&counts[lout]), 1ull)] = (uint64_t)(r + 1);
                }
            }
        }
        if (!finisher) return;
        __threadfence();
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_store(&counts[lin], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // consumed: the next round's output
        cnt = (int64_t)__hip_atomic_load(&counts[lout], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        __syncthreads();
        if (cnt == 0) return;
        const int t = lin;
        lin = lout;
        lout = t;
    }
}

// ring_all: CS_WAVES * CS_SUB * 64 doubles — ã of the sub-block, lane-private columns.  AP: out = λᵉ, bits = (λᵉ + π) < 0.
// BR: lane s* of call k writes branch[k] and, where term is not NULL, term[k] (1 + 16 bytes a call).
// SEG: call k of segment seg goes to output call seg * out_stride + k, and the wave of a segment's last chunk writes its pad.
template <int M, int LP, bool AP, bool BR = false, bool SEG = false>
__device__ __forceinline__ void cs_llr_body(char *smem, double *ring_all, double *rot, const double2 *__restrict__ rows,
                                            const double2 *__restrict__ rot_cs, const uint64_t *__restrict__ bedge, const double *__restrict__ ckpt,
                                            double *__restrict__ llr, uint8_t *__restrict__ bits, const cpm_soft_params &P,
                                            const cpm_soft_prior &prior, uint8_t *__restrict__ branch = nullptr, double2 *__restrict__ term = nullptr)
{
    constexpr int LGM = cs_lane<M, LP, AP>::LGM;
    static_assert(!(AP && SEG), "the segments are the plain detector's");
    if constexpr (!SEG) cs_stage_rot(rot_cs, P, rot);
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t c = (int64_t)blockIdx.x * CS_WAVES + wave;
    if (c >= P.nch) return;
    const cs_chunk kc = cs_find<SEG>(P, c, (uint32_t)P.cps);
    if constexpr (SEG) {
        rot += cs_in_vgpr((int64_t)wave * 2 * CPM_ROT_SIN);
        rows += cs_in_vgpr((int64_t)kc.seg * P.row_stride);
        cs_stage_rot_wave(rot_cs + (int64_t)kc.seg * P.rot_stride, P, rot);
        const int64_t o = cs_in_vgpr((int64_t)kc.seg * P.out_stride);
        llr += LGM * o;
        bits += LGM * o;
        if constexpr (BR) {
            branch += o;
            if (term) term += o;
        }
    }
    const cs_lane<M, LP, AP> L = cs_setup<M, LP, AP>(rows, P, smem + wave * cs_lane<M, LP, AP>::WAVE_BYTES, rot, prior);
    double *ring = ring_all + wave * CS_SUB * 64 + L.lane;
    const int64_t a = kc.a, e = kc.e;
    double b = L.active ? __longlong_as_double((long long)bedge[(P.nch - 1 - c) * CS_REC + L.lane]) : __builtin_inf();   // b̃_e, proven
    const double *ck = ckpt + (size_t)c * P.nsub * P.S;
    for (int j = (int)((e - a - 1) / CS_SUB); j >= 0; --j) {
        const int64_t k0 = a + (int64_t)j * CS_SUB, k1 = k0 + CS_SUB < e ? k0 + CS_SUB : e;
        double m = L.active ? ck[j * P.S + L.lane] : __builtin_inf();
        ring[0] = m;                                            // ã_{k0}
        cs_sweep<M, LP, true>(L, P, k0, k1 - 1, [&](int64_t k, int t, int tilt, int kv) __attribute__((always_inline)) {
            cs_fwd(L, P, t, tilt, kv, m);
            ring[(int)(k + 1 - k0) * 64] = m;                   // ã_{k+1}
        });
        cs_sweep<M, LP, false>(L, P, k0, k1, [&](int64_t k, int t, int tilt, int kv) __attribute__((always_inline)) {
            double lam[LGM], pi[LGM];
            int bsel = -1;
            double2 q = make_double2(0.0, 0.0);
            cs_llr<M, LP, AP, BR>(L, P, t, tilt, kv, ring[(int)(k - k0) * 64], b, lam, pi, bsel, q);
            if constexpr (BR) {
                if (bsel >= 0) {
                    branch[k] = (uint8_t)bsel;
                    if (term) term[k] = q;
                }
            }
            if (L.lane < LGM) {
                const double v = LGM == 1 || L.lane == 0 ? lam[0] : lam[LGM - 1];
                llr[LGM * k + L.lane] = v;
                if constexpr (AP) {
                    const double q = LGM == 1 || L.lane == 0 ? pi[0] : pi[LGM - 1];
                    bits[LGM * k + L.lane] = v + q < 0.0 ? 1 : 0;
                } else {
                    bits[LGM * k + L.lane] = v < 0.0 ? 1 : 0;
                }
            }
        });
    }
    if constexpr (SEG) {
        if (e == P.n)                                          // the segment's last chunk: the pad outputs, +0 / 0
            for (int64_t r = P.n + L.lane; r < P.out_stride; r += 64) {
#pragma unroll
                for (int i = 0; i < LGM; ++i) {
                    llr[LGM * r + i] = 0.0;
                    bits[LGM * r + i] = 0;
                }
                if constexpr (BR) {
                    branch[r] = 0;
                    if (term) term[r] = make_double2(0.0, 0.0);
                }
            }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
struct cs_geom {
    int ch, W;
    int64_t nch, nsub;
    size_t off_b, off_ck, words;   // scratch layout (8-B words): forward records + lists, backward records + lists, checkpoints
};

static int cs_states(const wf_cpm_detector_config *d)
{
    int S = d->p;
    for (int i = 1; i < d->Lp; ++i) S *= d->M;
    return S;
}

static int cs_check(const wf_cpm_detector_config *d, const char *who)
{
    WF_REQUIRE(d->M == 2 || d->M == 4, "%s: M = %d (2 or 4)", who, d->M);
    WF_REQUIRE(d->nh == 1 || d->nh == 2, "%s: nh = %d (1 or 2)", who, d->nh);
    WF_REQUIRE(d->Lp >= 1 && d->Lp <= 3, "%s: Lp = %d (1 .. 3)", who, d->Lp);
    WF_REQUIRE(d->p >= 1 && d->p <= 64, "%s: p = %d (1 .. 64)", who, d->p);
    WF_REQUIRE(d->NC == d->p, "%s: NC = %d: the soft output is defined on the full-phase trellis, NC = p = %d", who, d->NC, d->p);
    for (int i = 0; i < d->nh; ++i) WF_REQUIRE(d->K[i] >= 0 && d->K[i] < d->p, "%s: K[%d] = %d outside [0, p)", who, i, d->K[i]);
    WF_REQUIRE(cs_states(d) <= 64, "%s: %d states (at most 64)", who, cs_states(d));
    return WF_OK;
}

// The scratch of a launch of nch chunks of ch calls (a burst: its own; segments: nseg times the chunks of one)
static void cs_layout(cs_geom &g, int S)
{
    g.nsub = (g.ch + CS_SUB - 1) / CS_SUB;
    const size_t rec = (cpm_edge_total_words(g.nch, CS_REC) + 1) / 2 * 2;
    g.off_b = rec;
    g.off_ck = 2 * rec;
    g.words = g.off_ck + (size_t)g.nch * (size_t)g.nsub * (size_t)S;
}

static cs_geom cs_geometry(const wf_ctx *ctx, int S, int64_t n, int warmup)
{
    cs_geom g;
    g.W = warmup == 0 ? kCsDefaultWarmup : (warmup > 4096 ? 4096 : warmup);
    int64_t ch = ctx->opt[WF_OPT_CPM_SOFT_CHUNK_CALLS];
    if (ch == 0) {
        ch = (n + kCsChunks - 1) / kCsChunks;
        ch = (ch + CS_SUB - 1) / CS_SUB * CS_SUB;
        if (ch < kCsMinChunk) ch = kCsMinChunk;
        if (ch > kCsMaxChunk) ch = kCsMaxChunk;
    }
    g.ch = (int)ch;
    g.nch = (n + ch - 1) / ch;
    cs_layout(g, S);
    return g;
}

// The proof and repair launches behind the bounds launch, per direction (0 forward, 1 backward), as the hard detectors
// (wf_cpm_wide.hip): verify and list, two parallel repair rounds and the finisher - or, under WF_OPT_DET_REPAIR = 1, only count;
// WF_OPT_DET_FINAL_VERIFY adds a counting pass behind the repairs.  verify(dir, repair) and repair(dir, round, blocks, finisher)
// launch the caller's own kernels.
template <class V, class R>
static int cs_proof_passes(wf_ctx *ctx, V &&verify, R &&repair)
{
    const int rep = ctx->opt[WF_OPT_DET_REPAIR] == 0 ? 1 : 0;
    for (int dir = 0; dir < 2; ++dir) {
        verify(dir, rep);
        WF_LAUNCH_CHECK();
        if (!rep) continue;
        for (int round = 0; round < 3; ++round) {
            repair(dir, round, round < 2 ? CPM_REPAIR_BLOCKS : 1, round == 2 ? 1 : 0);
            WF_LAUNCH_CHECK();
        }
        if (ctx->opt[WF_OPT_DET_FINAL_VERIFY]) {
            verify(dir, 0);
            WF_LAUNCH_CHECK();
        }
    }
    return WF_OK;
}

// The full-phase trellis, enumerated as cpm_oracle.c does (state s = v + p c, branch (s, u)).
static void cs_build_tables(const wf_cpm_detector_config *d, cpm_soft_params &P)
{
    const int M = d->M, Lp = d->Lp, p = d->p;
    int msub = 1;
    for (int i = 2; i < Lp; ++i) msub *= M;
    P.M = M; P.p = p; P.nh = d->nh; P.K0 = d->K[0]; P.K1 = d->nh == 2 ? d->K[1] : d->K[0];
    P.Lp = Lp; P.S = cs_states(d);
    memset(P.dest, 0xFF, sizeof P.dest);
    for (int kv = 0; kv < 3; ++kv) {
        const int K_old = kv == 2 ? 0 : (kv == 1 ? P.K1 : P.K0);
        P.dt[kv] = ((M - 1) * K_old) % (2 * p);
        int fill[64] = {0};
        for (int s = 0; s < P.S; ++s) {
            const int v = s % p, corr = s / p;
            for (int u = 0; u < M; ++u) {
                const int u_old = Lp == 1 ? u : corr / msub;
                const int corr2 = Lp == 1 ? 0 : u + M * (corr % msub);
                const int e = (v + K_old * u_old) % p + p * corr2;
                P.dest[kv][s][u] = (uint8_t)(4 * e + fill[e]++);
            }
        }
    }
}

// wf_cpm_soft's launches but the last — bounds, proof and repairs of both directions — into the context's scratch (wf_cpm_soft.hip)
int cpm_soft_front(wf_ctx *ctx, const cpm_soft_params &P, const cs_geom &g, const double2 *rows, const double2 *rot, hipStream_t s);

// the launch parameters of one burst (tables, geometry) — after the arguments have been checked
static void cs_fill_params(const wf_cpm_detector_config *det, const cs_geom &g, int64_t ncalls, int64_t first_call, cpm_soft_params &P)
{
    cs_build_tables(det, P);
    P.ch = g.ch;
    P.W = g.W;
    P.n = ncalls;
    P.n0 = first_call;
    P.nch = g.nch;
    P.nsub = g.nsub;
}
