// wf_coarse.hip — coarse carrier frequency acquisition for the SOQPSK-TG receiver: the two spectral lines of the squared signal
// (wf_coarse_lines_c128), the estimate from their periodograms (wf_coarse_estimate) and the correction by a frequency that
// stays in device memory (wf_carrier_offset_dev_c128).  include/wfhip.h states every definition;
// waveforms_amd/sync/coarse.py restates them in numpy.  The reference has no synchroniser: these are the build's own.
//
//   coarse_lines_kernel     one workgroup per segment of nfft bits (grid-strided), a lane per bit, both lines from one pass.
//                           Samples: STAGED (whenever the tile fits beside the FFT, COARSE_MAX_LDS) the workgroup copies a tile of
//                           256 bits' samples and the S - 1 behind them into LDS with coalesced 16-byte loads, COARSE_BATCH in
//                           flight per lane, so every sample is read from memory once; one slot of padding after every sps samples
//                           puts the lanes' reads, one bit apart, into different banks for an even sps.  Otherwise each lane
//                           reads its bit's samples from memory itself, sps * 16 bytes apart across lanes.  Both forms add in the
//                           same order (coarse_dump) and give the same bits.
//                           Dump: boxcar sums, square, the 2 sps rotations from a table, one sample per bit and line.
//                           FFTs: the σ = -1 line goes to LDS bit-reversed, the σ = +1 line waits in registers (16 values a lane at
//                           nfft 4096), and the two FFTs (wf_fft.h) run one after the other in the 64 KB + 32 KB of LDS that
//                           welch_kernel uses - two buffers at once would fill the CU's 160 KiB.
//                           Sums: |X|² per bin in registers across the workgroup's segments, per-workgroup partials, reduced in
//                           a fixed order by coarse_reduce_kernel (no floating-point atomics: nothing depends on scheduling).
//   coarse_estimate_kernel  ONE workgroup: the first maximum of the summed periodogram (per-thread strided scan, a tree that
//                           breaks ties towards the smaller bin), its mean (fixed tree), then one thread: each line's first
//                           maximum within the search range and the guarded log-parabola vertex.
//   carrier_offset_dev_kernel  carrier_offset_kernel with nu = gain * d_nu[0]: the same sync_carrier_turn per sample.
#include "wf_fft.h"
#include "wf_sync.h"

#include <cmath>

#define COARSE_THREADS 256
#define COARSE_Q ((1 << FFT_MAX_LOG2) / COARSE_THREADS)      // bins (and bits) per lane at the largest nfft
#define COARSE_MAX_BLOCKS 256
#define COARSE_MAX_SPS 64
#define COARSE_MAX_SMOOTH 1024
#define COARSE_MIN_LOG2 6
#define COARSE_BATCH 8                                       // staged loads in flight per lane: a tile at sps 8 is one batch and a halo
#define COARSE_MAX_LDS (160 * 1024)                          // a workgroup's share of the CU's LDS on gfx950

// One bit's two line samples from its sps samples and the S - 1 behind them, p[0] the bit's first.  PADDED: sample a of the tile
// lives at slot a + a / sps and p is the slot of a sample whose index is a multiple of sps
template <bool PADDED>
__device__ __forceinline__ void coarse_dump(const double2 *p, int sps, int S, const double2 *rot, double2 &um, double2 &ul)
{
    um = ul = make_double2(0.0, 0.0);
    int s0 = 0;
    for (int j = 0; j < sps; ++j) {
        int s = s0, rm = j;
        double2 y = p[s];
        for (int k = 1; k < S; ++k) {
            ++s;
            if (PADDED && ++rm == sps) {
                rm = 0;
                ++s;
            }
            const double2 v = p[s];
            y.x += v.x;
            y.y += v.y;
        }
        const double2 z = make_double2(y.x * y.x - y.y * y.y, 2.0 * (y.x * y.y));
        const double2 e = rot[j];
        um.x += z.x * e.x + z.y * e.y;                        // z conj(e): σ = -1
        um.y += z.y * e.x - z.x * e.y;
        ul.x += z.x * e.x - z.y * e.y;                        // z e: σ = +1
        ul.y += z.y * e.x + z.x * e.y;
        ++s0;
    }
}

template <bool STAGED>
__global__ __launch_bounds__(COARSE_THREADS) void coarse_lines_kernel(const double2 *__restrict__ r, int64_t nseg, int nfft, int m, int sps, int S,
                                                                       const double *__restrict__ window, double *__restrict__ partial)
{
    extern __shared__ __attribute__((aligned(16))) double2 s_buf[];
    double2 *s_tw = s_buf + nfft;
    double2 *s_rot = s_tw + nfft / 2;                         // exp(jπ q / sps), q < 2 sps
    double2 *s_stage = s_rot + 2 * sps;                       // STAGED: a tile's samples, padded (coarse_stage_slots)
    const int t = threadIdx.x;
    fft_twiddles<COARSE_THREADS>(s_tw, nfft, t);
    for (int q = t; q < 2 * sps; q += COARSE_THREADS) {
        double sn, cs;
        sincospi((double)q / (double)sps, &sn, &cs);
        s_rot[q] = make_double2(cs, sn);
    }
    double acc[2][COARSE_Q];
#pragma unroll
    for (int q = 0; q < COARSE_Q; ++q) acc[0][q] = acc[1][q] = 0.0;
    for (int64_t seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
        __syncthreads();                                      // the tables are written; the segment before has been read
        double2 up[COARSE_Q];
#pragma unroll
        for (int qq = 0; qq < COARSE_Q; ++qq) up[qq] = make_double2(0.0, 0.0);
        // ONE copy of the dump's loops (unrolled sixteen times they took 59 scalar registers into spill lanes): q is a run-time
        // count and the value finds its register through sixteen selects
#pragma unroll 1
        for (int q = 0; q * COARSE_THREADS < nfft; ++q) {
            const int i = t + q * COARSE_THREADS;
            if (STAGED) {                                     // (q and nfft are uniform: every thread meets the barriers)
                const int tile = nfft - q * COARSE_THREADS < COARSE_THREADS ? nfft - q * COARSE_THREADS : COARSE_THREADS;
                const int count = tile * sps + S - 1;         // the last sample read is (nseg nfft) sps + S - 2 <= n - 1
                const double2 *src = r + (seg * nfft + q * COARSE_THREADS) * sps;
                if (q) __syncthreads();                       // the tile before has been read
                // COARSE_BATCH loads in flight per lane before the first is waited for (one at a time, a tile took eight memory
                // latencies: with four waves on the CU nothing else hides them)
                for (int k0 = t; k0 < count; k0 += COARSE_BATCH * COARSE_THREADS) {
                    double2 v[COARSE_BATCH];
#pragma unroll
                    for (int u = 0; u < COARSE_BATCH; ++u) {
                        const int k = k0 + u * COARSE_THREADS;
                        v[u] = k < count ? src[k] : make_double2(0.0, 0.0);
                    }
#pragma unroll
                    for (int u = 0; u < COARSE_BATCH; ++u) {
                        const int k = k0 + u * COARSE_THREADS;
                        if (k < count) s_stage[k + k / sps] = v[u];
                    }
                }
                __syncthreads();
            }
            if (i < nfft) {
                const int64_t bit = seg * nfft + i;
                const double2 *rot = s_rot + (int)(bit & 1) * sps;   // (bit sps + j) mod 2 sps = (bit mod 2) sps + j
                double2 um, ul;
                if (STAGED)
                    coarse_dump<true>(s_stage + t * (sps + 1), sps, S, rot, um, ul);
                else
                    coarse_dump<false>(r + bit * sps, sps, S, rot, um, ul);   // the last sample read is (nseg nfft) sps + S - 2 <= n - 1
                const double w = window[i];
                s_buf[fft_brev(i, m)] = make_double2(um.x * w, um.y * w);
                const double2 keep = make_double2(ul.x * w, ul.y * w);
#pragma unroll
                for (int qq = 0; qq < COARSE_Q; ++qq)
                    if (qq == q) up[qq] = keep;
            }
        }
#pragma unroll
        for (int line = 0; line < 2; ++line) {
            if (line == 1) {
                __syncthreads();                              // the first line's bins have been read
#pragma unroll
                for (int q = 0; q < COARSE_Q; ++q) {
                    const int i = t + q * COARSE_THREADS;
                    if (i < nfft) s_buf[fft_brev(i, m)] = up[q];
                }
            }
            fft_stages<COARSE_THREADS>(s_buf, s_tw, nfft, m, t);
            __syncthreads();
#pragma unroll
            for (int q = 0; q < COARSE_Q; ++q) {
                const int i = t + q * COARSE_THREADS;
                if (i < nfft) acc[line][q] += fma(s_buf[i].x, s_buf[i].x, s_buf[i].y * s_buf[i].y);
            }
        }
    }
#pragma unroll
    for (int line = 0; line < 2; ++line)
#pragma unroll
        for (int q = 0; q < COARSE_Q; ++q) {
            const int i = t + q * COARSE_THREADS;
            if (i < nfft) partial[((size_t)blockIdx.x * 2 + line) * nfft + ((i + nfft / 2) & (nfft - 1))] = acc[line][q];   // fftshift
        }
}

// spectra[line][k] = Σ_b partial[b][line][k], b increasing
__global__ void coarse_reduce_kernel(const double *__restrict__ partial, int nblocks, int nfft, double *__restrict__ spectra)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= 2 * nfft) return;
    double s = 0.0;
    for (int b = 0; b < nblocks; ++b) s += partial[(size_t)b * 2 * nfft + k];
    spectra[k] = s;
}

// the first of the largest p[lo .. hi]; a NaN never wins
__device__ __forceinline__ int coarse_first_max(const double *p, int lo, int hi)
{
    int best = lo;
    double m = p[lo] == p[lo] ? p[lo] : -INFINITY;
    for (int i = lo + 1; i <= hi; ++i) {
        const double v = p[i];
        if (v > m) {
            m = v;
            best = i;
        }
    }
    return best;
}

// The guarded vertex of the parabola through the natural logs of p[i - 1], p[i], p[i + 1]: 0 where a bin is <= 0 or not finite, or
// where the denominator is not negative and finite
__device__ __forceinline__ double coarse_vertex(const double *p, int i)
{
    const double pa = p[i - 1], pb = p[i], pc = p[i + 1];
    const bool ok = pa > 0.0 && pb > 0.0 && pc > 0.0 && pa < INFINITY && pb < INFINITY && pc < INFINITY;
    if (!ok) return 0.0;
    const double a = log(pa), b = log(pb), c = log(pc);
    const double l = a - b, h = c - b;
    const double den = l + h;
    if (!(den < 0.0 && den > -INFINITY)) return 0.0;
    const double num = 0.5 * (a - c);
    return num / den;
}

__global__ __launch_bounds__(COARSE_THREADS) void coarse_estimate_kernel(const double *__restrict__ P, int L, int sps, int R, double *__restrict__ found)
{
    __shared__ double s_v[COARSE_THREADS], s_sum[COARSE_THREADS];
    __shared__ int s_i[COARSE_THREADS];
    const int t = threadIdx.x;
    double best = -INFINITY, sum = 0.0;
    int bi = 0x7fffffff;
    for (int b = t; b < L; b += COARSE_THREADS) {
        const double T = P[b] + P[L + b];
        sum += T;
        if (b >= R + 1 && b <= L - R - 2) {
            const double v = T == T ? T : -INFINITY;
            if (v > best || bi == 0x7fffffff) {
                best = v;
                bi = b;
            }
        }
    }
    s_v[t] = best;
    s_i[t] = bi;
    s_sum[t] = sum;
    for (int d = COARSE_THREADS / 2; d >= 1; d >>= 1) {
        __syncthreads();
        if (t < d) {
            s_sum[t] += s_sum[t + d];
            const double v = s_v[t + d];
            const int i = s_i[t + d];
            if (v > s_v[t] || (v == s_v[t] && i < s_i[t])) {
                s_v[t] = v;
                s_i[t] = i;
            }
        }
    }
    if (t == 0) {
        const int star = s_i[0];                              // R + 1 <= star <= L - R - 2: every bin read below exists
        const int im = coarse_first_max(P, star - R, star + R), ip = coarse_first_max(P + L, star - R, star + R);
        const double fm = (double)im + coarse_vertex(P, im);
        const double fp = (double)ip + coarse_vertex(P + L, ip);
        const double mid = 0.5 * (fm + fp);
        const double off = mid - 0.5 * (double)L;
        const double scale = 2.0 * (double)L * (double)sps;
        found[0] = off / scale;
        found[1] = (fm - fp) / (double)L;
        found[2] = P[star] + P[L + star];
        found[3] = s_sum[0] / (double)L;
    }
}

__global__ __launch_bounds__(COARSE_THREADS) void carrier_offset_dev_kernel(const double2 *in, int64_t n, const double *__restrict__ d_nu, double gain,
                                                                             int64_t first_index, double2 *out)
{
    const double nu = gain * d_nu[0];
    for (int64_t k = (int64_t)blockIdx.x * COARSE_THREADS + threadIdx.x; k < n; k += (int64_t)gridDim.x * COARSE_THREADS)
        out[k] = sync_carrier_turn(in[k], 0.0, nu, first_index + k);
}

// ---- host side ------------------------------------------------------------------------------------------------------
static inline bool coarse_overlap(const void *a, size_t abytes, const void *b, size_t bbytes)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + bbytes && y < x + abytes;
}

// STAGED: the slots of a tile of up to COARSE_THREADS bits, their halo and one slot of padding per sps samples
static inline size_t coarse_stage_slots(int nfft, int sps, int smooth)
{
    const size_t tile = nfft < COARSE_THREADS ? nfft : COARSE_THREADS, count = tile * sps + smooth - 1;
    return count + count / sps + 1;
}

// log2 of nfft where it is a power of two from 64 to 4096, otherwise -1
static inline int coarse_log2(int nfft)
{
    for (int m = COARSE_MIN_LOG2; m <= FFT_MAX_LOG2; ++m)
        if ((1 << m) == nfft) return m;
    return -1;
}

// the whole segments of a burst of n samples, or -1 where an argument is out of range
static int64_t coarse_segments(int64_t n, int sps, int nfft, int smooth)
{
    if (n < 1 || n > kTimingMaxN || sps < 2 || sps > COARSE_MAX_SPS || smooth < 1 || smooth > COARSE_MAX_SMOOTH || coarse_log2(nfft) < 0) return -1;
    if (n < smooth) return 0;
    return ((n - smooth + 1) / sps) / nfft;
}

extern "C" int64_t wf_coarse_scratch_doubles(int64_t n, int sps, int nfft, int smooth)
{
    const int64_t nseg = coarse_segments(n, sps, nfft, smooth);
    if (nseg < 1) return -1;
    return (nseg < COARSE_MAX_BLOCKS ? nseg : COARSE_MAX_BLOCKS) * 2 * (int64_t)nfft;
}

extern "C" int wf_coarse_lines_c128(wf_ctx *ctx, const double *d_r_ri, int64_t n, int sps, int smooth, int nfft, const double *d_window, double *d_scratch,
                                    double *d_spectra, void *stream)
{
    const char *who = "wf_coarse_lines_c128";
    WF_REQUIRE(ctx && d_r_ri && d_window && d_scratch && d_spectra, "%s: NULL argument", who);
    const int64_t nseg = coarse_segments(n, sps, nfft, smooth);
    WF_REQUIRE(nseg >= 0, "%s: n must be 1 .. 2^40, sps 2 .. %d, smooth 1 .. %d and nfft a power of two from 64 to 4096", who, COARSE_MAX_SPS,
               COARSE_MAX_SMOOTH);
    WF_REQUIRE(nseg >= 1, "%s: %lld samples do not fill one segment of %d bits", who, (long long)n, nfft);
    WF_REQUIRE(!sync_mis(d_r_ri, 15) && !sync_mis(d_window, 7) && !sync_mis(d_scratch, 7) && !sync_mis(d_spectra, 7),
               "%s: samples must be 16-byte, window, scratch and spectra 8-byte aligned", who);
    const int grid = (int)(nseg < COARSE_MAX_BLOCKS ? nseg : COARSE_MAX_BLOCKS);
    const size_t in_bytes = (size_t)n * 16, win_bytes = (size_t)nfft * 8, scr_bytes = (size_t)grid * 2 * nfft * 8, out_bytes = (size_t)2 * nfft * 8;
    WF_REQUIRE(!coarse_overlap(d_spectra, out_bytes, d_r_ri, in_bytes) && !coarse_overlap(d_spectra, out_bytes, d_window, win_bytes) &&
                   !coarse_overlap(d_spectra, out_bytes, d_scratch, scr_bytes) && !coarse_overlap(d_scratch, scr_bytes, d_r_ri, in_bytes) &&
                   !coarse_overlap(d_scratch, scr_bytes, d_window, win_bytes),
               "%s: the scratch and the spectra overlap each other or an input", who);
    WF_HIP(hipSetDevice(ctx->device));
    const int m = coarse_log2(nfft);
    size_t lds = (size_t)(nfft + nfft / 2 + 2 * sps) * sizeof(double2);
    const size_t staged_lds = lds + coarse_stage_slots(nfft, sps, smooth) * sizeof(double2);
    const bool staged = staged_lds <= COARSE_MAX_LDS;
    auto kernel = staged ? coarse_lines_kernel<true> : coarse_lines_kernel<false>;
    if (staged) lds = staged_lds;
    if (lds > 48 * 1024) WF_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipStream_t s = wf_stream(stream);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(COARSE_THREADS), lds, s, reinterpret_cast<const double2 *>(d_r_ri), nseg, nfft, m, sps, smooth, d_window,
                       d_scratch);
    WF_LAUNCH_CHECK();
    hipLaunchKernelGGL(coarse_reduce_kernel, dim3((2 * nfft + 255) / 256), dim3(256), 0, s, (const double *)d_scratch, grid, nfft, d_spectra);
    WF_LAUNCH_CHECK();
    return WF_OK;
}

extern "C" int wf_coarse_estimate(wf_ctx *ctx, const double *d_spectra, int nfft, int sps, int search, double *d_found, void *stream)
{
    const char *who = "wf_coarse_estimate";
    WF_REQUIRE(ctx && d_spectra && d_found, "%s: NULL argument", who);
    WF_REQUIRE(coarse_log2(nfft) >= 0, "%s: nfft %d must be a power of two from 64 to 4096", who, nfft);
    WF_REQUIRE(sps >= 2 && sps <= COARSE_MAX_SPS, "%s: sps must be 2 .. %d, not %d", who, COARSE_MAX_SPS, sps);
    WF_REQUIRE(search >= 1 && search < nfft / 2 - 1, "%s: search must be 1 .. nfft / 2 - 2, not %d", who, search);
    WF_REQUIRE(!sync_mis(d_spectra, 7) && !sync_mis(d_found, 7), "%s: spectra and found must be 8-byte aligned", who);
    WF_REQUIRE(!coarse_overlap(d_found, 32, d_spectra, (size_t)2 * nfft * 8), "%s: found overlaps the spectra", who);
    WF_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(coarse_estimate_kernel, dim3(1), dim3(COARSE_THREADS), 0, wf_stream(stream), d_spectra, nfft, sps, search, d_found);
    WF_LAUNCH_CHECK();
    return WF_OK;
}

extern "C" int wf_carrier_offset_dev_c128(wf_ctx *ctx, const double *d_in_ri, int64_t n, const double *d_nu, double gain, int64_t first_index,
                                          double *d_out_ri, void *stream)
{
    const char *who = "wf_carrier_offset_dev_c128";
    WF_REQUIRE(ctx && d_in_ri && d_nu && d_out_ri, "%s: NULL argument", who);
    WF_REQUIRE(n >= 1 && first_index >= 0 && n <= ((int64_t)1 << 53) - first_index, "%s: n must be at least 1 and first_index + n at most 2^53", who);
    WF_REQUIRE(std::isfinite(gain), "%s: gain must be finite", who);
    WF_REQUIRE(!sync_mis(d_in_ri, 15) && !sync_mis(d_out_ri, 15) && !sync_mis(d_nu, 7), "%s: samples must be 16-byte and nu 8-byte aligned", who);
    WF_REQUIRE(d_in_ri == d_out_ri || !coarse_overlap(d_in_ri, (size_t)n * 16, d_out_ri, (size_t)n * 16),
               "%s: in place or out of place (the output overlaps the input in part)", who);
    WF_REQUIRE(!coarse_overlap(d_nu, 8, d_out_ri, (size_t)n * 16), "%s: nu lies inside the output", who);
    WF_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(carrier_offset_dev_kernel, dim3(wf_grid_for(n, COARSE_THREADS, 1 << 16)), dim3(COARSE_THREADS), 0, wf_stream(stream),
                       reinterpret_cast<const double2 *>(d_in_ri), n, d_nu, gain, first_index, reinterpret_cast<double2 *>(d_out_ri));
    WF_LAUNCH_CHECK();
    return WF_OK;
}
