// wf_frame.hip — framed coded links (include/wfhip.h states the definitions): wf_frame_build puts an attached sync marker
// in front of every randomised codeword, wf_frame_search finds the frame offset and the polarity of a burst from the soft
// detector's λ, wf_frame_gather / wf_frame_scatter move a located burst's codeword λ into the decoder's ncw x n_tx input
// and the decoder's extrinsic output back into the detector's prior buffer.
//
// Search, one pass over λ: a workgroup of FRAME_TILE threads takes FRAME_TILE consecutive residues p and one slice of
// FRAME_SLICE frames.  Per frame it stages the tile's λ plus the L - 1 values behind it in LDS (consecutive threads load
// consecutive doubles, one frame ahead, through registers); every lane then walks its own L values, lane j reading word j + i at step i, so the lanes of a wave
// read consecutive doubles at every step: no bank conflict.  s_i λ is a sign flip (xor of the marker bit into the sign), the
// marker word is wave-uniform (a kernel argument).  The slice's partial G± stay in registers and are written once.
// frame_fold_kernel adds the slice sums in slice order (independent loads, dependent adds), one thread per value;
// frame_pick_kernel, one workgroup, takes the maximum of the 2P values with the tie rule and writes the lock record.
#include "wf_common.h"

#include <algorithm>
#include <cmath>

#define FRAME_TILE 256
#define FRAME_SLICE 32              // frames per slice: part of the definition of G± (include/wfhip.h)
#define FRAME_MAX_L 64

struct frame_lock {                 // wf_frame_search's record, 32 bytes
    int64_t p, sigma;
    double best, other;
};

__device__ __forceinline__ double frame_flip(double x, uint64_t neg)      // neg = 1: -x (sign bit only)
{
    return __longlong_as_double(__double_as_longlong(x) ^ (long long)(neg << 63));
}

__global__ __launch_bounds__(FRAME_TILE) void frame_build_kernel(const uint8_t *__restrict__ tx, const uint8_t *__restrict__ pn, int64_t ncw,
                                                                 int32_t n_tx, uint64_t marker, int32_t L, uint8_t *__restrict__ out)
{
    const int64_t P = (int64_t)L + n_tx, total = ncw * P;
    for (int64_t g = (int64_t)blockIdx.x * FRAME_TILE + threadIdx.x; g < total; g += (int64_t)gridDim.x * FRAME_TILE) {
        const int64_t b = g / P;
        const int32_t j = (int32_t)(g - b * P);
        uint8_t v;
        if (j < L) {
            v = (uint8_t)((marker >> (L - 1 - j)) & 1u);
        } else {
            const int32_t t = j - L;
            v = (uint8_t)((tx[b * n_tx + t] ^ (pn ? pn[t] : 0)) & 1u);
        }
        out[g] = v;
    }
}

// part[(slice * 2 + pol) * P + p] = the slice's sum of M±(p + f P), f = slice FRAME_SLICE .. min(F, (slice + 1) FRAME_SLICE) - 1
__global__ __launch_bounds__(FRAME_TILE) void frame_search_kernel(const double *__restrict__ llr, uint64_t marker, int32_t L, int64_t P, int64_t F,
                                                                  double *__restrict__ part)
{
    __shared__ double s_l[FRAME_TILE + FRAME_MAX_L];
    const int tid = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.y * FRAME_TILE, p = p0 + tid, slice = blockIdx.x;
    const int64_t f0 = slice * FRAME_SLICE, f1 = f0 + FRAME_SLICE < F ? f0 + FRAME_SLICE : F;
    // values of this tile that a residue below P reads: p0 .. min(p0 + FRAME_TILE, P) - 1 + L - 1 (all below nllr for f < F)
    const int64_t live = (p0 + FRAME_TILE < P ? FRAME_TILE : P - p0) + L - 1;
    double gp = 0.0, gm = 0.0;
    // a thread stages at most two values per frame (live <= FRAME_TILE + FRAME_MAX_L - 1); the next frame's are loaded into
    // registers before this frame's sums, so the global latency is paid beside the arithmetic, not between two barriers
    const bool two = tid + FRAME_TILE < live;
    const double *src = llr + f0 * P + p0;
    double r0 = tid < live ? src[tid] : 0.0, r1 = two ? src[tid + FRAME_TILE] : 0.0;
    for (int64_t f = f0; f < f1; ++f) {
        __syncthreads();
        s_l[tid] = r0;
        if (two) s_l[tid + FRAME_TILE] = r1;
        __syncthreads();
        if (f + 1 < f1) {
            src += P;
            if (tid < live) r0 = src[tid];
            if (two) r1 = src[tid + FRAME_TILE];
        }
        if (p < P) {
            double c = 0.0, a = 0.0;
            for (int i = 0; i < L; ++i) {
                const double v = s_l[tid + i];
                c += frame_flip(v, (marker >> (L - 1 - i)) & 1u);
                a += fabs(v);
            }
            gp += c - a;
            gm += -c - a;
        }
    }
    if (p < P) {
        part[(slice * 2 + 0) * P + p] = gp;
        part[(slice * 2 + 1) * P + p] = gm;
    }
}

// folded[q] (q = pol P + p) = the slice sums added in slice order from +0
__global__ __launch_bounds__(FRAME_TILE) void frame_fold_kernel(const double *__restrict__ part, int64_t P, int64_t nslices, double *__restrict__ folded)
{
    const int64_t q = (int64_t)blockIdx.x * FRAME_TILE + threadIdx.x;
    if (q >= 2 * P) return;
    double g = 0.0;
    int64_t s = 0;
    for (; s + 8 <= nslices; s += 8) {          // eight loads in flight, the additions in slice order
        double v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = part[(s + j) * 2 * P + q];
#pragma unroll
        for (int j = 0; j < 8; ++j) g += v[j];
    }
    for (; s < nslices; ++s) g += part[s * 2 * P + q];
    folded[q] = g;
}

struct frame_cand {
    double best, other;
    int64_t q;
};
// a then b, where every q of a that matters for a tie is compared by value: the larger value wins, equal values the smaller q
__device__ __forceinline__ frame_cand frame_merge(const frame_cand &a, const frame_cand &b)
{
    frame_cand r;
    if (b.best > a.best || (b.best == a.best && b.q < a.q)) {
        r.best = b.best, r.q = b.q;
        r.other = fmax(a.best, fmax(a.other, b.other));
    } else {
        r.best = a.best, r.q = a.q;
        r.other = fmax(b.best, fmax(a.other, b.other));
    }
    return r;
}

__global__ __launch_bounds__(FRAME_TILE) void frame_pick_kernel(const double *__restrict__ folded, int64_t P, frame_lock *__restrict__ lock)
{
    __shared__ frame_cand s_c[FRAME_TILE];
    const int tid = threadIdx.x;
    frame_cand c;
    c.best = -INFINITY, c.other = -INFINITY, c.q = INT64_MAX;
    for (int64_t q = tid; q < 2 * P; q += FRAME_TILE) {
        frame_cand n;
        n.best = folded[q], n.other = -INFINITY, n.q = q;
        c = frame_merge(c, n);
    }
    s_c[tid] = c;
    __syncthreads();
    for (int h = FRAME_TILE / 2; h > 0; h /= 2) {
        if (tid < h) s_c[tid] = frame_merge(s_c[tid], s_c[tid + h]);
        __syncthreads();
    }
    if (tid == 0) {
        const frame_cand w = s_c[0];
        frame_lock r;
        r.sigma = w.q < P ? 1 : -1;
        r.p = w.q < P ? w.q : w.q - P;
        r.best = w.best, r.other = w.other;
        *lock = r;
    }
}

__global__ __launch_bounds__(FRAME_TILE) void frame_gather_kernel(const double *__restrict__ llr, int64_t nllr, const frame_lock *__restrict__ lock,
                                                                  int32_t L, int32_t n_tx, const uint8_t *__restrict__ pn, int64_t ncw,
                                                                  double *__restrict__ out)
{
    const int64_t P = (int64_t)L + n_tx, total = ncw * n_tx, ph = lock->p;
    const uint64_t inv = lock->sigma < 0 ? 1u : 0u;
    for (int64_t g = (int64_t)blockIdx.x * FRAME_TILE + threadIdx.x; g < total; g += (int64_t)gridDim.x * FRAME_TILE) {
        const int64_t b = g / n_tx;
        const int32_t t = (int32_t)(g - b * n_tx);
        const int64_t pos = ph + b * P + L + t;
        double v = 0.0;
        if (pos >= 0 && pos < nllr) v = frame_flip(llr[pos], inv ^ (pn ? (uint64_t)(pn[t] & 1u) : 0u));
        out[g] = v;
    }
}

__device__ __forceinline__ float frame_flipf(float x, uint32_t neg)
{
    return __uint_as_float(__float_as_uint(x) ^ (neg << 31));
}

__global__ __launch_bounds__(FRAME_TILE) void frame_scatter_kernel(const float *__restrict__ ext, int64_t ext_stride, const frame_lock *__restrict__ lock,
                                                                   uint64_t marker, int32_t L, int32_t n_tx, const uint8_t *__restrict__ pn,
                                                                   int64_t ncw, float marker_prior, float *__restrict__ prior, int64_t nprior)
{
    const int64_t P = (int64_t)L + n_tx, total = ncw * P, ph = lock->p;
    const uint32_t inv = lock->sigma < 0 ? 1u : 0u;
    for (int64_t g = (int64_t)blockIdx.x * FRAME_TILE + threadIdx.x; g < total; g += (int64_t)gridDim.x * FRAME_TILE) {
        const int64_t b = g / P;
        const int32_t j = (int32_t)(g - b * P);
        const int64_t pos = ph + g;
        if (pos < 0 || pos >= nprior) continue;
        if (j < L) {
            if (marker_prior != 0.0f) prior[pos] = frame_flipf(marker_prior, inv ^ (uint32_t)((marker >> (L - 1 - j)) & 1u));
        } else {
            const int32_t t = j - L;
            prior[pos] = frame_flipf(ext[b * ext_stride + t], inv ^ (pn ? (uint32_t)(pn[t] & 1u) : 0u));
        }
    }
}

static unsigned frame_grid(const wf_ctx *ctx, int64_t total)
{
    const int64_t want = (total + FRAME_TILE - 1) / FRAME_TILE;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)std::max(ctx->cus, 1) * 32));
}

extern "C" int wf_frame_build(wf_ctx *ctx, const uint8_t *d_tx, int64_t ncw, int32_t n_tx, uint64_t marker, int32_t L, const uint8_t *d_pn,
                              uint8_t *d_out, void *stream)
{
    WF_REQUIRE(ctx && d_tx && d_out, "wf_frame_build: NULL argument");
    WF_REQUIRE(L >= 1 && L <= FRAME_MAX_L, "wf_frame_build: L = %d outside 1 .. %d", L, FRAME_MAX_L);
    WF_REQUIRE(ncw >= 1 && n_tx >= 1, "wf_frame_build: ncw and n_tx must be at least 1");
    WF_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(frame_build_kernel, dim3(frame_grid(ctx, ncw * ((int64_t)L + n_tx))), dim3(FRAME_TILE), 0, wf_stream(stream), d_tx, d_pn, ncw,
                       n_tx, marker, L, d_out);
    WF_LAUNCH_CHECK();
    return WF_OK;
}

extern "C" int wf_frame_search(wf_ctx *ctx, const double *d_llr, int64_t nllr, uint64_t marker, int32_t L, int64_t P, void *d_lock,
                               double *d_folded, void *stream)
{
    WF_REQUIRE(ctx && d_llr && d_lock, "wf_frame_search: NULL argument");
    WF_REQUIRE(L >= 1 && L <= FRAME_MAX_L, "wf_frame_search: L = %d outside 1 .. %d", L, FRAME_MAX_L);
    WF_REQUIRE(P > L && P <= (int64_t)1 << 23, "wf_frame_search: P = %lld must be above L = %d (and at most 2^23)", (long long)P, L);
    WF_REQUIRE(nllr >= L + P, "wf_frame_search: %lld values hold no whole frame of period %lld behind a marker of %d", (long long)nllr,
               (long long)P, L);
    WF_REQUIRE((reinterpret_cast<uintptr_t>(d_llr) & 7) == 0 && (reinterpret_cast<uintptr_t>(d_lock) & 7) == 0 &&
                   (reinterpret_cast<uintptr_t>(d_folded) & 7) == 0,
               "wf_frame_search: llr, lock and folded must be 8-byte aligned");
    const int64_t F = (nllr - L) / P, nslices = (F + FRAME_SLICE - 1) / FRAME_SLICE, tiles = (P + FRAME_TILE - 1) / FRAME_TILE;
    // slice sums, then the folded values when the caller does not take them
    const int rc = wf_ctx_reserve_vit(ctx, (size_t)((nslices + 1) * 2 * P));
    if (rc) return rc;
    WF_HIP(hipSetDevice(ctx->device));
    double *part = ctx->d_vit_edge, *folded = d_folded ? d_folded : part + nslices * 2 * P;
    hipLaunchKernelGGL(frame_search_kernel, dim3((unsigned)nslices, (unsigned)tiles), dim3(FRAME_TILE), 0, wf_stream(stream), d_llr, marker, L, P,
                       F, part);
    WF_LAUNCH_CHECK();
    hipLaunchKernelGGL(frame_fold_kernel, dim3((unsigned)((2 * P + FRAME_TILE - 1) / FRAME_TILE)), dim3(FRAME_TILE), 0, wf_stream(stream), part, P,
                       nslices, folded);
    WF_LAUNCH_CHECK();
    hipLaunchKernelGGL(frame_pick_kernel, dim3(1), dim3(FRAME_TILE), 0, wf_stream(stream), folded, P, static_cast<frame_lock *>(d_lock));
    WF_LAUNCH_CHECK();
    return WF_OK;
}

extern "C" int wf_frame_gather(wf_ctx *ctx, const double *d_llr, int64_t nllr, const void *d_lock, int32_t L, int32_t n_tx, const uint8_t *d_pn,
                               int64_t ncw, double *d_out, void *stream)
{
    WF_REQUIRE(ctx && d_llr && d_lock && d_out, "wf_frame_gather: NULL argument");
    WF_REQUIRE(L >= 1 && L <= FRAME_MAX_L, "wf_frame_gather: L = %d outside 1 .. %d", L, FRAME_MAX_L);
    WF_REQUIRE(ncw >= 1 && n_tx >= 1 && nllr >= 1, "wf_frame_gather: ncw, n_tx and nllr must be at least 1");
    WF_REQUIRE((reinterpret_cast<uintptr_t>(d_llr) & 7) == 0 && (reinterpret_cast<uintptr_t>(d_lock) & 7) == 0 &&
                   (reinterpret_cast<uintptr_t>(d_out) & 7) == 0,
               "wf_frame_gather: llr, lock and out must be 8-byte aligned");
    WF_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(frame_gather_kernel, dim3(frame_grid(ctx, ncw * n_tx)), dim3(FRAME_TILE), 0, wf_stream(stream), d_llr, nllr,
                       static_cast<const frame_lock *>(d_lock), L, n_tx, d_pn, ncw, d_out);
    WF_LAUNCH_CHECK();
    return WF_OK;
}

extern "C" int wf_frame_scatter(wf_ctx *ctx, const float *d_ext, int64_t ext_stride, const void *d_lock, uint64_t marker, int32_t L, int32_t n_tx,
                                const uint8_t *d_pn, int64_t ncw, float marker_prior, float *d_prior, int64_t nprior, void *stream)
{
    WF_REQUIRE(ctx && d_ext && d_lock && d_prior, "wf_frame_scatter: NULL argument");
    WF_REQUIRE(L >= 1 && L <= FRAME_MAX_L, "wf_frame_scatter: L = %d outside 1 .. %d", L, FRAME_MAX_L);
    WF_REQUIRE(ncw >= 1 && n_tx >= 1 && nprior >= 1, "wf_frame_scatter: ncw, n_tx and nprior must be at least 1");
    WF_REQUIRE(ext_stride >= n_tx, "wf_frame_scatter: ext_stride = %lld is below n_tx = %d", (long long)ext_stride, n_tx);
    WF_REQUIRE(std::isfinite(marker_prior), "wf_frame_scatter: marker_prior must be finite");
    WF_REQUIRE((reinterpret_cast<uintptr_t>(d_ext) & 3) == 0 && (reinterpret_cast<uintptr_t>(d_lock) & 7) == 0 &&
                   (reinterpret_cast<uintptr_t>(d_prior) & 3) == 0,
               "wf_frame_scatter: ext and prior must be 4-byte, lock 8-byte aligned");
    WF_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(frame_scatter_kernel, dim3(frame_grid(ctx, ncw * ((int64_t)L + n_tx))), dim3(FRAME_TILE), 0, wf_stream(stream), d_ext,
                       ext_stride, static_cast<const frame_lock *>(d_lock), marker, L, n_tx, d_pn, ncw, marker_prior, d_prior, nprior);
    WF_LAUNCH_CHECK();
    return WF_OK;
}
