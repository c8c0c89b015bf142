// wf_cpm_timing.hip — symbol timing for the generic CPM chains (ARTM multi-h, PCM/FM): the resampling front end
// (wf_cpm_mf_rows_resample_c128) and the statistic of the feed-forward recovery (wf_llr_stat).  include/wfhip.h states every
// definition; waveforms_amd/sync/timing_cpm.py restates them in numpy.  The trajectory stages are wf_timing.hip's.
//
//   cpm_mf_rows_resample_kernel   cpm_mf_rows_kernel's tile (a run of symbols staged once in LDS, thread = (filter, sub-row), the
//                                 9-tap templates in registers) at mf_resample_kernel's instants, in three phases per tile:
//                                 A  a thread per row forms the row's instant, its integer part B and its four weights; the
//                                    workgroup takes the smallest and the largest B and stages that span of samples ONCE in LDS
//                                    (zeros outside the burst);
//                                 B  the tile's syms x ntm interpolated samples x_n[k], one per work item, into LDS: a row's ntm
//                                    samples are interpolated once, not once per filter;
//                                 C  cpm_mf_rows_kernel's correlation on them, k ascending, the same fma chain.
//                                 A tile whose span is wider than the staged region (a trajectory that jumps by more than
//                                 CRS_EXTRA samples inside a tile) reads its samples from global memory in phase B instead,
//                                 bounds-checked, with the same arithmetic: nothing is read from LDS that was not staged.
//                                 __launch_bounds__(256, 4) and three taps' loads in flight in phase C: 128 VGPRs, no spill, four
//                                 waves a SIMD; at 130 VGPRs and three waves the kernel took 1.2 times as long on 1e7 calls
//                                 (profiles/timing_recovery_cpm.json).
//   llr_stat_kernel               one WAVE per window: carrier_stat_kernel's order of additions on |λ| (the fold is wf_sync.h's).
#include "wf_sync.h"

#include <climits>

#define CRS_THREADS 256
#define CRS_EXTRA 64                // samples of room for the trajectory to move inside one tile before the tile leaves LDS
#define CRS_GRID_CAP 2048
#define CRS_TARGET_SLOTS 2560       // 40 KiB of complex128: four workgroups a CU
#define CRS_MAX_SLOTS 9984          // 156 KiB: what a tile may take when 32 rows do not fit the target
#define CRS_MIN_SYMS 32
#define LSTAT_THREADS 256
#define LSTAT_WAVES (LSTAT_THREADS / WF_WAVE)

struct crs_params {
    int64_t nsamp, start0, ncalls, nwin, nblk;
    int sps, ntm, nh, W;
    int syms;                       // rows per tile (<= CRS_THREADS)
    int region;                     // samples the window holds
    int x_slot, w_slot, b_slot, t_slot;   // LDS slots (16 B) of x[syms][ntm], the weights [syms][4], B[syms], the template copy
    double tau0;
    const double *tau;
};

template <int NF, int NTM>
__global__ __launch_bounds__(CRS_THREADS, 4) void cpm_mf_rows_resample_kernel(const double2 *__restrict__ r, const double2 *__restrict__ templ,
                                                                           double2 *__restrict__ out, crs_params P)
{
    extern __shared__ __attribute__((aligned(16))) char crs_smem[];
    double2 *s_r = reinterpret_cast<double2 *>(crs_smem);
    double2 *s_x = s_r + P.x_slot;
    double *s_w = reinterpret_cast<double *>(s_r + P.w_slot);
    long long *s_B = reinterpret_cast<long long *>(s_r + P.b_slot);
    double2 *s_t = s_r + P.t_slot;                                    // generic path: nh x NF x ntm templates
    __shared__ long long s_lo[CRS_THREADS / WF_WAVE], s_hi[CRS_THREADS / WF_WAVE];
    const int ntm = NTM ? NTM : P.ntm;
    const int t = threadIdx.x;
    const int f = t % NF, sub = t / NF;
    constexpr int SUBS = CRS_THREADS / NF;
    double2 tap[2][NTM ? NTM : 1];
    if (NTM) {
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int k = 0; k < NTM; ++k) tap[c][k] = templ[((c < P.nh ? c : 0) * NF + f) * NTM + k];
    } else {
        for (int k = t; k < P.nh * NF * ntm; k += CRS_THREADS) s_t[k] = templ[k];       // (first read behind the loop's barriers)
    }
    for (int64_t blk = blockIdx.x; blk < P.nblk; blk += gridDim.x) {
        const int64_t nb = blk * P.syms;
        // ---- A: the row's instant tau0 + τ_n, its integer part and its weights
        const int64_t n = nb + t;
        const bool row = t < P.syms && n < P.ncalls;
        double tk = P.tau0;
        if (row && P.tau) {
            const double phi = sync_traj_at(P.tau, P.nwin, P.W, n);
            tk = P.tau0 + phi;
        }
        bool live = row && fabs(tk) < kTimingHuge;             // (false for a NaN)
        int64_t B = 0;
        double w[4] = {0.0, 0.0, 0.0, 0.0};
        if (live) {
            const double fl = floor(tk);
            const double mu = tk - fl;                          // exact
            B = P.start0 + n * P.sps + (int64_t)fl;             // the sample that pairs with template tap 0 at weight c_0
            live = B + ntm + 1 >= 0 && B - 1 < P.nsamp;         // otherwise every sample the row reads lies outside the burst: a zero row
            if (live) timing_lagrange(mu, w);
        }
        long long mn = live ? (long long)B : LLONG_MAX, mx = live ? (long long)B : LLONG_MIN;
#pragma unroll
        for (int d = WF_WAVE / 2; d >= 1; d >>= 1) {
            const long long a = __shfl_xor(mn, d, WF_WAVE), b = __shfl_xor(mx, d, WF_WAVE);
            mn = a < mn ? a : mn;
            mx = b > mx ? b : mx;
        }
        __syncthreads();                                        // the previous tile's reads of LDS are done
        if (wf_lane() == 0) {
            s_lo[t / WF_WAVE] = mn;
            s_hi[t / WF_WAVE] = mx;
        }
        if (t < P.syms) {
            s_B[t] = live ? (long long)B : LLONG_MIN;
#pragma unroll
            for (int i = 0; i < 4; ++i) s_w[4 * t + i] = w[i];
        }
        __syncthreads();
#pragma unroll
        for (int v = 0; v < CRS_THREADS / WF_WAVE; ++v) {
            mn = s_lo[v] < mn ? s_lo[v] : mn;
            mx = s_hi[v] > mx ? s_hi[v] : mx;
        }
        const bool any = mn <= mx;                              // block-uniform from here
        const int64_t lo = any ? (int64_t)mn - 1 : 0;           // first sample any row of the tile reads
        const int64_t need = any ? ((int64_t)mx + ntm + 1) - lo + 1 : 0;
        const bool fits = any && need <= P.region;
        if (fits) {
            for (int i = t; i < (int)need; i += CRS_THREADS) {
                const int64_t s = lo + i;
                s_r[i] = (s >= 0 && s < P.nsamp) ? wf_load16_nt(r + s) : make_double2(0.0, 0.0);
            }
        }
        __syncthreads();
        // ---- B: x_n[k] = Σ_i c_i r[B_n + k + i], i = -1 .. 2, once per (row, k)
        if (any) {
            const int items = P.syms * ntm;
            for (int i = t; i < items; i += CRS_THREADS) {
                const int rw = i / ntm, k = i - rw * ntm;
                const long long Bn = s_B[rw];
                double2 x = make_double2(0.0, 0.0);
                if (Bn != LLONG_MIN) {
                    const double *c = s_w + 4 * rw;
                    double2 xa, xb, xc, xd;
                    if (fits) {
                        const double2 *p = s_r + ((int)(Bn - 1 - lo) + k);
                        xa = p[0];
                        xb = p[1];
                        xc = p[2];
                        xd = p[3];
                    } else {
                        const int64_t g = (int64_t)Bn - 1 + k;
                        const double2 z = make_double2(0.0, 0.0);
                        xa = (g >= 0 && g < P.nsamp) ? r[g] : z;
                        xb = (g + 1 >= 0 && g + 1 < P.nsamp) ? r[g + 1] : z;
                        xc = (g + 2 >= 0 && g + 2 < P.nsamp) ? r[g + 2] : z;
                        xd = (g + 3 >= 0 && g + 3 < P.nsamp) ? r[g + 3] : z;
                    }
                    x.x = fma(c[3], xd.x, fma(c[2], xc.x, fma(c[1], xb.x, c[0] * xa.x)));
                    x.y = fma(c[3], xd.y, fma(c[2], xc.y, fma(c[1], xb.y, c[0] * xa.y)));
                }
                s_x[i] = x;
            }
        }
        __syncthreads();
        // ---- C: rows[n][f] = Σ_k x_n[k] conj(T[n % nh][f][k]) in cpm_mf_rows_kernel's chain
        for (int sym = sub; sym < P.syms; sym += SUBS) {
            const int64_t m = nb + sym;
            if (m >= P.ncalls) break;
            double zr = 0.0, zi = 0.0;
            if (any && s_B[sym] != LLONG_MIN) {
                const int c = (int)(m % P.nh);
                const double2 *x = s_x + sym * ntm;
                if (NTM) {
#pragma unroll
                    for (int k = 0; k < NTM; ++k) {
                        const double2 xv = x[k];
                        const double2 tp = c ? tap[1][k] : tap[0][k];
                        zr = fma(xv.x, tp.x, fma(xv.y, tp.y, zr));
                        zi = fma(-xv.x, tp.y, fma(xv.y, tp.x, zi));
                        if (k % 3 == 2) __builtin_amdgcn_sched_barrier(0);      // three taps' loads in flight, not nine: 128 VGPRs without a spill
                    }
                } else {
                    const double2 *tp = s_t + (c * NF + f) * ntm;
                    for (int k = 0; k < ntm; ++k) {
                        const double2 xv = x[k];
                        zr = fma(xv.x, tp[k].x, fma(xv.y, tp[k].y, zr));
                        zi = fma(-xv.x, tp[k].y, fma(xv.y, tp[k].x, zi));
                    }
                }
            }
            out[m * NF + f] = make_double2(zr, zi);
        }
    }
}

// d_stat[2w] = -Σ |λ| over the window's values in carrier_stat_kernel's order (64 lane partials from +0, index increasing, then
// sync_wave_fold's butterfly d = 32 .. 1); d_stat[2w + 1] = +0
__global__ __launch_bounds__(LSTAT_THREADS) void llr_stat_kernel(const double *__restrict__ llr, int64_t nvals, int64_t per, int64_t nwin,
                                                                 double *__restrict__ stat)
{
    const int lane = wf_lane();
    for (int64_t w = (int64_t)blockIdx.x * LSTAT_WAVES + threadIdx.x / WF_WAVE; w < nwin; w += (int64_t)gridDim.x * LSTAT_WAVES) {   // wave-uniform
        const int64_t base = w * per;
        const int64_t end = base + per < nvals ? base + per : nvals;
        double p = 0.0;
        for (int64_t i = base + lane; i < end; i += WF_WAVE) p += fabs(llr[i]);
        p = sync_wave_fold(p);
        if (lane == 0) {
            stat[2 * w] = -p;
            stat[2 * w + 1] = 0.0;
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
// The tile: the most rows (<= 256) whose window, interpolated samples, weights and instants fit CRS_TARGET_SLOTS; where fewer
// than CRS_MIN_SYMS do, CRS_MIN_SYMS rows (or as many as fit) in up to CRS_MAX_SLOTS.  false: one row does not fit.
static bool crs_geometry(int nh, int nfilt, int ntm, int sps, crs_params *P, size_t *lds)
{
    const int tmpl = ntm == 9 ? 0 : nh * nfilt * ntm;
    auto total = [&](int S) { return (S - 1) * sps + ntm + 3 + CRS_EXTRA + S * ntm + 2 * S + (S + 1) / 2 + tmpl; };
    int S = CRS_THREADS;
    while (S > 1 && total(S) > CRS_TARGET_SLOTS) --S;
    if (S < CRS_MIN_SYMS) {
        S = CRS_MIN_SYMS;
        while (S > 1 && total(S) > CRS_MAX_SLOTS) --S;
    }
    if (total(S) > CRS_MAX_SLOTS) return false;
    P->syms = S;
    P->region = (S - 1) * sps + ntm + 3 + CRS_EXTRA;
    P->x_slot = P->region;
    P->w_slot = P->x_slot + S * ntm;
    P->b_slot = P->w_slot + 2 * S;
    P->t_slot = P->b_slot + (S + 1) / 2;
    *lds = (size_t)total(S) * sizeof(double2);
    return true;
}

static bool crs_shape_ok(int nh, int nfilt, int ntm, int sps)
{
    return (nh == 1 || nh == 2) && ntm >= 1 && ntm <= 257 && sps >= 1 && sps <= 256 &&
           (nfilt == 2 || nfilt == 4 || nfilt == 8 || nfilt == 16 || nfilt == 64);
}

extern "C" int wf_cpm_mf_rows_resample_geometry(int nh, int nfilt, int ntm, int sps, int64_t *h_geom)
{
    const char *who = "wf_cpm_mf_rows_resample_geometry";
    WF_REQUIRE(h_geom, "%s: NULL argument", who);
    WF_REQUIRE(crs_shape_ok(nh, nfilt, ntm, sps), "%s: nh %d nfilt %d ntm %d sps %d", who, nh, nfilt, ntm, sps);
    crs_params P;
    size_t lds = 0;
    WF_REQUIRE(crs_geometry(nh, nfilt, ntm, sps, &P, &lds), "%s: sps %d / %d-tap filters do not fit LDS staging", who, sps, ntm);
    h_geom[0] = P.syms;
    h_geom[1] = CRS_GRID_CAP;
    h_geom[2] = (int64_t)lds;
    return WF_OK;
}

extern "C" int wf_cpm_mf_rows_resample_c128(wf_ctx *ctx, const double *d_r_ri, int64_t nsamp, const double *d_templates_ri, int nh, int nfilt, int ntm,
                                            int64_t start0, int sps, int64_t ncalls, int W, const double *d_tau, int64_t nwin, double tau0,
                                            double *d_rows_ri, void *stream)
{
    const char *who = "wf_cpm_mf_rows_resample_c128";
    WF_REQUIRE(ctx && d_r_ri && d_templates_ri && d_rows_ri, "%s: NULL argument", who);
    WF_REQUIRE(crs_shape_ok(nh, nfilt, ntm, sps), "%s: nh %d (1, 2) nfilt %d (2, 4, 8, 16, 64) ntm %d (1 .. 257) sps %d (1 .. 256)", who, nh, nfilt, ntm, sps);
    WF_REQUIRE(nsamp >= 1 && nsamp <= kTimingMaxN && ncalls >= 1 && ncalls <= kTimingMaxN && start0 >= -kTimingMaxN && start0 <= kTimingMaxN,
               "%s: nsamp and ncalls must be 1 .. 2^40 and |start0| at most 2^40", who);
    WF_REQUIRE(std::isfinite(tau0), "%s: tau0 must be finite", who);
    WF_REQUIRE(!d_tau || (sync_window_ok(W) && nwin >= 1 && nwin <= kTimingMaxN), "%s: W must be a multiple of 64 from 64 to 8192 and nwin at least 1", who);
    WF_REQUIRE(!sync_mis(d_r_ri, 15) && !sync_mis(d_templates_ri, 15) && !sync_mis(d_rows_ri, 15) && !sync_mis(d_tau, 7),
               "%s: samples, templates and rows must be 16-byte and tau 8-byte aligned", who);
    crs_params P;
    size_t lds = 0;
    WF_REQUIRE(crs_geometry(nh, nfilt, ntm, sps, &P, &lds), "%s: sps %d / %d-tap filters do not fit LDS staging", who, sps, ntm);
    WF_HIP(hipSetDevice(ctx->device));
    P.nsamp = nsamp;
    P.start0 = start0;
    P.ncalls = ncalls;
    P.nwin = d_tau ? nwin : 0;
    P.sps = sps;
    P.ntm = ntm;
    P.nh = nh;
    P.W = d_tau ? W : 64;
    P.tau0 = tau0;
    P.tau = d_tau;
    P.nblk = (ncalls + P.syms - 1) / P.syms;
    const int grid = (int)(P.nblk < CRS_GRID_CAP ? P.nblk : CRS_GRID_CAP);
    using kern_t = void (*)(const double2 *, const double2 *, double2 *, crs_params);
    kern_t k;
#define CRS_PICK(NFV) (ntm == 9 ? cpm_mf_rows_resample_kernel<NFV, 9> : cpm_mf_rows_resample_kernel<NFV, 0>)
    switch (nfilt) {
    case 2: k = CRS_PICK(2); break;
    case 4: k = CRS_PICK(4); break;
    case 8: k = CRS_PICK(8); break;
    case 16: k = CRS_PICK(16); break;
    default: k = CRS_PICK(64); break;
    }
#undef CRS_PICK
    if (lds > 48 * 1024) WF_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k, dim3(grid), dim3(CRS_THREADS), lds, wf_stream(stream), reinterpret_cast<const double2 *>(d_r_ri),
                       reinterpret_cast<const double2 *>(d_templates_ri), reinterpret_cast<double2 *>(d_rows_ri), P);
    WF_LAUNCH_CHECK();
    return WF_OK;
}

extern "C" int wf_llr_stat(wf_ctx *ctx, const double *d_llr, int64_t ncalls, int bits_per_call, int W, double *d_stat, void *stream)
{
    WF_REQUIRE(ctx && d_llr && d_stat, "wf_llr_stat: NULL argument");
    WF_REQUIRE(ncalls >= 1 && ncalls <= kTimingMaxN, "wf_llr_stat: ncalls must be 1 .. 2^40");
    WF_REQUIRE(bits_per_call >= 1 && bits_per_call <= 8, "wf_llr_stat: bits_per_call must be 1 .. 8, not %d", bits_per_call);
    WF_REQUIRE(sync_window_ok(W), "wf_llr_stat: W must be a multiple of 64 from 64 to 8192");
    WF_REQUIRE(!sync_mis(d_llr, 7) && !sync_mis(d_stat, 7), "wf_llr_stat: llr and stat must be 8-byte aligned");
    WF_HIP(hipSetDevice(ctx->device));
    const int64_t nwin = (ncalls + W - 1) / W;
    hipLaunchKernelGGL(llr_stat_kernel, dim3(wf_grid_for(nwin, LSTAT_WAVES, 1 << 16)), dim3(LSTAT_THREADS), 0, wf_stream(stream), d_llr,
                       ncalls * bits_per_call, (int64_t)bits_per_call * W, nwin, d_stat);
    WF_LAUNCH_CHECK();
    return WF_OK;
}
