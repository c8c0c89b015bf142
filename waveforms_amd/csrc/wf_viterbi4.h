// wf_viterbi4.h — the SOQPSK 4-state trellis and the chunk-proof machinery shared by the hard
// detectors (wf_viterbi.hip) and the soft-output detector (wf_viterbi_soft.hip).
#pragma once

#include "wf_common.h"

// Branch b of column c: start = b >> 1; ends / output-symbol index (0: -2, 1: 0, 2: +2):
//   column 0 (even / I): end = (start & 1) + 2*(b & 1)
//   column 1 (odd  / Q): end = (start & 2) + (b & 1)
// (model.py:205-230; the diff-encoded trellis :233-258 only relabels the inputs).
// {{1, 2, 1, 0, 0, 1, 2, 1}, {1, 0, 2, 1, 1, 2, 0, 1}} as 2-bit fields of one literal: a table in constant memory
// is a dependent ~0.5 us load each time the per-symbol server (one wave on an idle chip) looks an entry up
__device__ __forceinline__ int br_out_idx(int col, int b) { return (int)((0x49616419u >> (2 * (8 * col + b))) & 3u); }

__device__ __forceinline__ int br_end(int col, int b)
{
    const int s = b >> 1;
    return col == 0 ? (s & 1) + 2 * (b & 1) : (s & 2) + (b & 1);
}

__device__ __forceinline__ int br_inp(int col, int b, int diff)
{
    const int s = b >> 1;
    const int flip = diff ? (col == 0 ? (s >> 1) : (s & 1)) : 0;
    return (b & 1) ^ flip;
}

// Re(state_exp_term[start] * z), state_exp_term = [+1j, -1, +1, -1j] (algorithm.py:30)
__device__ __forceinline__ double br_inc(int start, double re, double im)
{
    return start == 0 ? -im : start == 1 ? -re : start == 2 ? re : im;
}

// ---- lean detector step for the batch kernel --------------------------------------------
// Per trellis section only 4 of the 6 components of a matched-filter row are ever used:
// Re/Im of z[1] (alpha = 0) in both sections, plus (Re z[0], Im z[2]) in the even (I) section
// and (Im z[0], Re z[2]) in the odd (Q) one.  Incoming branches per end state, first in
// LIST order (ties keep the first: strict '<', algorithm.py:79-83), with their increment
// Re(state_exp_term[start] * z[idx(out)]) written as a signed component:
//   even: st0: (0: -i1 | 2: +a)   st1: (1: -r1 | 3: +b)   st2: (0: -b | 2: +r1)   st3: (1: -a | 3: +i1)
//   odd : st0: (0: -i1 | 1: -b)   st1: (0: -a | 1: -r1)   st2: (2: +r1 | 3: +a)   st3: (2: +b | 3: +i1)
// with r1 = Re z[1], i1 = Im z[1], (a, b) = (Re z[0], Im z[2]) even / (Im z[0], Re z[2]) odd.
// m + (-x) and m - x are the same IEEE operation, so every compare is bit-identical to the
// reference's.
struct vit_comp {
    double r1, i1, a, b;
};

template <int COL, bool PACKED>
__device__ __forceinline__ vit_comp vit_components(const double2 *__restrict__ z)
{
    vit_comp c;
    if (PACKED) {   // row = {r1, i1, a, b}: the bank already picked the section's components
        c.r1 = z[0].x;
        c.i1 = z[0].y;
        c.a = z[1].x;
        c.b = z[1].y;
        return c;
    }
    c.r1 = z[1].x;
    c.i1 = z[1].y;
    c.a = COL == 0 ? z[0].x : z[0].y;
    c.b = COL == 0 ? z[2].y : z[2].x;
    return c;
}

// Proof records and repair lists of the 4-state detectors (batch and window form alike), in the context's scratch:
//   rec[nchunks][8]   doubles: {the C / metrics a chunk's own calls started from [4], what they ended with [4]}
//   hdr[VIT_HDR]      u64: [0], [1] entries in list 0 / 1, [2] the fix-up launch's arrival ticket
//   list[2][nchunks]  u64 chunk indices
// viterbi_fixup_kernel / vwin_fixup_kernel, ONE launch behind the detector: every workgroup compares its share of the
// chunk boundaries and lists the chunks whose start is not bitwise their predecessor's end; the workgroup that arrives
// last then repairs: a thread per listed chunk runs the chunk's calls AGAIN from the predecessor's end (which becomes the
// chunk's recorded start), rewrites its decisions and its end, and lists the next chunk when that end changed — round
// after round (lists 0 <-> 1) until a round lists nothing.  Every round's smallest chunk is run from the true state, so
// the consistent prefix grows each round: at worst the rounds are the sequential detector (algorithm.py:44-101), and
// the warm-up only decides how often any of this runs (at the default, at any Eb/N0 measured: never).
#define VIT_HDR 8
__host__ __device__ inline size_t vit_edge_words(int64_t nchunks) { return (size_t)nchunks * 8 + VIT_HDR + 2 * (size_t)nchunks; }

// The part of the fix-up launch both forms share: compare, list (or, mode 0, count), and elect the last workgroup.
// Returns true in every thread of the workgroup that arrived last (all others are done).  mode: 1 = list for repair,
// 0 = count as unproven (WF_OPT_DET_REPAIR off; the closing check of WF_OPT_DET_FINAL_VERIFY).
__device__ __forceinline__ bool vit_fixup_verify(double *__restrict__ edge, int64_t nchunks, unsigned long long *__restrict__ unmerged, int mode)
{
    __shared__ int s_last;
    unsigned long long *hdr = reinterpret_cast<unsigned long long *>(edge + 8 * nchunks);
    unsigned long long *list0 = hdr + VIT_HDR;
    const unsigned long long *rec = reinterpret_cast<const unsigned long long *>(edge);
    int listed = 0;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x + 1; c < nchunks; c += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long *st = rec + 8 * c, *en = rec + 8 * (c - 1) + 4;
        if (st[0] != en[0] || st[1] != en[1] || st[2] != en[2] || st[3] != en[3]) {
            if (mode) list0[atomicAdd(&hdr[0], 1ull)] = (unsigned long long)c;
            else atomicAdd(unmerged, 1ull);
            listed = 1;
        }
    }
    if (!mode) return false;
    // Arrival.  A workgroup that listed something publishes its entries (agent-scope release) before it arrives; the
    // others have nothing to publish and only arrive — in the usual launch nobody lists anything, and a release fence
    // writes back the XCD's whole L2 under the front end that is streaming rows through it on the other stream.  The
    // list COUNT needs no fence: it and the ticket are device-scope atomics, and every thread's count increment has
    // returned (the barrier waits for it) before thread 0 takes the ticket.
    if (__syncthreads_or(listed)) __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) s_last = atomicAdd(&hdr[2], 1ull) + 1 == (unsigned long long)gridDim.x;
    __syncthreads();
    if (!s_last) return false;
    if (__hip_atomic_load(&hdr[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return false;   // nothing to repair: the usual case
    __threadfence();                                       // ... everybody's entries before the repairs read them
    return true;
}

// The round loop of the last workgroup: `repair(c)` runs chunk c again and returns true when its end changed.
template <class F>
__device__ __forceinline__ void vit_fixup_rounds(double *__restrict__ edge, int64_t nchunks, unsigned long long *__restrict__ unmerged, F &&repair)
{
    unsigned long long *hdr = reinterpret_cast<unsigned long long *>(edge + 8 * nchunks);
    int lin = 0;
    for (;;) {
        const int64_t n = (int64_t)__hip_atomic_load(&hdr[lin], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n == 0) return;
        unsigned long long *in = hdr + VIT_HDR + (int64_t)lin * nchunks, *out = hdr + VIT_HDR + (int64_t)(lin ^ 1) * nchunks;
        for (int64_t idx = threadIdx.x; idx < n; idx += blockDim.x) {
            const int64_t c = (int64_t)__hip_atomic_load(&in[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const bool changed = repair(c);
            atomicAdd(unmerged + 1, 1ull);                 // [1]: chunk repairs run, [2]: ... whose end changed (handed on)
            if (changed) {
                atomicAdd(unmerged + 2, 1ull);
                if (c + 1 < nchunks) out[atomicAdd(&hdr[lin ^ 1], 1ull)] = (unsigned long long)(c + 1);
            }
        }
        __threadfence();
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_store(&hdr[lin], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // consumed: the round after next fills it
        __threadfence();
        __syncthreads();
        lin ^= 1;
    }
}
