// wf_rows_hyp.hip — the H rotated copies of a burst of 48-byte rows that a coarse carrier search detects, written by ONE pass
// over the rows (include/wfhip.h: wf_rows_derotate_hyp): out[h][k] = rows[k] exp(-j h π / H), h < H, k < ncalls, and zero rows
// up to `stride` in every copy.  H launches of wf_rows_derotate read the burst H times and evaluate the same sincos ncalls
// times each; here a workgroup evaluates the H rotations once into LDS (thread h the h-th: one fp64 sincos), every thread
// reads its row once (three 16-byte loads) and writes its H rotated copies.
//
// The values are bitwise wf_rows_derotate's at phase0 = ((double)h * π) / H: the same quotient, the same sum with the absent
// trajectory's +0.0, the same device sincos of the same argument, and the same rotation: wf_sync.h's sync_rotate, one text for
// both files (-ffp-contract=on fuses within an expression only, so both contract alike).
//
// Launch shape: memory-bound (48 B in, 48 H B out per row), a thread per row and a grid-stride loop as wf_rows_derotate;
// across a wave the stores of one copy are 48 bytes apart, which the three 16-byte stores of neighbouring lanes fill without
// gaps.  LDS: H <= 256 rotations of 16 bytes = 4 KiB.
#include "wf_sync.h"

#include <cmath>

#define HYP_THREADS 256
#define HYP_MAX_H 256
static constexpr double kHypPi = 3.14159265358979323846;

__global__ __launch_bounds__(HYP_THREADS) void rows_derotate_hyp_kernel(const double2 *__restrict__ rows, int64_t n, int H, int64_t stride, double2 *__restrict__ out)
{
    __shared__ double2 s_cs[HYP_MAX_H];
    for (int h = threadIdx.x; h < H; h += HYP_THREADS) {
        const double base = (double)h * kHypPi;
        const double phase0 = base / (double)H;
        const double tot = phase0 + 0.0;                     // (wf_rows_derotate's phase0 + φ with no trajectory)
        double sn, cs;
        sincos(-tot, &sn, &cs);
        s_cs[h] = make_double2(cs, sn);
    }
    __syncthreads();
    for (int64_t k = (int64_t)blockIdx.x * HYP_THREADS + threadIdx.x; k < stride; k += (int64_t)gridDim.x * HYP_THREADS) {
        if (k < n) {
            const double2 z0 = rows[3 * k], z1 = rows[3 * k + 1], z2 = rows[3 * k + 2];
            for (int h = 0; h < H; ++h) {
                const double cs = s_cs[h].x, sn = s_cs[h].y;
                double2 *o = out + 3 * ((int64_t)h * stride + k);
                o[0] = sync_rotate(z0, cs, sn);
                o[1] = sync_rotate(z1, cs, sn);
                o[2] = sync_rotate(z2, cs, sn);
            }
        } else {
            for (int h = 0; h < H; ++h) {
                double2 *o = out + 3 * ((int64_t)h * stride + k);
                o[0] = o[1] = o[2] = make_double2(0.0, 0.0);
            }
        }
    }
}

extern "C" int wf_rows_derotate_hyp(wf_ctx *ctx, const double *d_rows, int64_t ncalls, int H, int64_t stride, double *d_out, void *stream)
{
    static const char who[] = "wf_rows_derotate_hyp";
    WF_REQUIRE(ctx && d_rows && d_out, "%s: NULL argument", who);
    WF_REQUIRE(H >= 1 && H <= HYP_MAX_H, "%s: H must be 1 .. 256", who);
    WF_REQUIRE(ncalls >= 1, "%s: ncalls must be at least 1", who);
    WF_REQUIRE(stride >= ncalls && stride % 64 == 0 && stride <= ((int64_t)1 << 40) / H, "%s: stride must be a multiple of 64, at least ncalls, and H stride at most 2^40",
               who);
    const uintptr_t in = reinterpret_cast<uintptr_t>(d_rows), out = reinterpret_cast<uintptr_t>(d_out);
    WF_REQUIRE((in & 15) == 0 && (out & 15) == 0, "%s: rows must be 16-byte aligned", who);
    WF_REQUIRE(in + 48 * (uintptr_t)ncalls <= out || out + 48 * (uintptr_t)H * (uintptr_t)stride <= in, "%s: out of place only: the output overlaps the input", who);
    WF_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(rows_derotate_hyp_kernel, dim3(wf_grid_for(stride, HYP_THREADS, 1 << 16)), dim3(HYP_THREADS), 0, wf_stream(stream),
                       reinterpret_cast<const double2 *>(d_rows), ncalls, H, stride, reinterpret_cast<double2 *>(d_out));
    WF_LAUNCH_CHECK();
    return WF_OK;
}
