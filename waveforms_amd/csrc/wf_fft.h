// wf_fft.h — the radix-2 decimation-in-time FFT of one workgroup in LDS, shared by welch_kernel (wf_viz.hip) and
// coarse_lines_kernel (wf_coarse.hip): the twiddle table and the butterfly stages.  The caller writes its nfft = 2^m inputs at
// the bit-reversed positions (fft_brev) of s_buf and reads the bins in natural order behind a barrier of its own.
#pragma once
#include "wf_common.h"

#define FFT_MAX_LOG2 12          // segments of up to 4096 samples live in LDS (64 KB), their twiddles beside them (32 KB)

__device__ __forceinline__ int fft_brev(int i, int m) { return (int)(__brev((unsigned)i) >> (32 - m)); }

// s_tw[j] = exp(-2πj i / nfft), j < nfft / 2 (visible behind the caller's next barrier)
template <int THREADS>
__device__ __forceinline__ void fft_twiddles(double2 *s_tw, int nfft, int t)
{
    for (int j = t; j < nfft / 2; j += THREADS) {
        double sn, cs;
        sincospi(-2.0 * (double)j / (double)nfft, &sn, &cs);
        s_tw[j] = make_double2(cs, sn);
    }
}

// the m stages, each behind a barrier; the last stage's writes are NOT behind one
template <int THREADS>
__device__ __forceinline__ void fft_stages(double2 *s_buf, const double2 *s_tw, int nfft, int m, int t)
{
    for (int s = 1; s <= m; ++s) {
        __syncthreads();
        const int half = 1 << (s - 1), tstep = nfft >> s;
        for (int b = t; b < nfft / 2; b += THREADS) {
            const int pos = b & (half - 1);
            const int i0 = ((b >> (s - 1)) << s) + pos, i1 = i0 + half;
            const double2 w = s_tw[pos * tstep], a = s_buf[i0], c = s_buf[i1];
            const double2 cw = make_double2(fma(c.x, w.x, -c.y * w.y), fma(c.x, w.y, c.y * w.x));
            s_buf[i0] = make_double2(a.x + cw.x, a.y + cw.y);
            s_buf[i1] = make_double2(a.x - cw.x, a.y - cw.y);
        }
    }
}
