// wf_idd.hip — the LDPC decoder as the outer half of iterative detection and decoding (include/wfhip.h:
// wf_ldpc_decode_ext, wf_ldpc_count).  idd_decode_kernel is ldpc_decode_kernel (wf_ldpc.hip; wf_ldpc.h holds what the two
// share: geometry, check update, syndrome) with a per-codeword freeze state and an extrinsic output:
//   * a codeword whose state is 1 is not read, not decoded and not written; the test comes before any LDS or table
//     traffic, so a workgroup whose G codewords are all frozen retires after one byte load per thread and one barrier;
//   * an open codeword is decoded from a cold start exactly as wf_ldpc_decode does, its iterations are ADDED to d_iters,
//     and it leaves ±ext_sat by its decisions (and state 1) when its syndrome is zero, clamp(L - Lch) otherwise.
// Lch is RE-READ from d_llr at the end ((float)(scale * λ), the conversion the load made) instead of being kept: keeping it
// would cost n_tx x 4 B of LDS per codeword (16 KiB on top of the demo code's 48 KiB per workgroup, i.e. 2 workgroups per
// CU instead of 3), re-reading costs 8 B of global traffic per transmitted bit of an open codeword, once per call.
#include "wf_ldpc.h"

struct idd_dec_args {
    const int32_t *layer, *ell, *check_ptr, *edge_var, *var_src, *info_var, *tx_var;
    int32_t n, m, nlayers, n_tx, k, G, max_iter;
    int64_t ncw, ext_stride;
    const double *llr;
    double scale;
    float alpha, ext_clip, ext_sat;
    uint8_t *state, *info_bits;
    float *post, *ext;
    int32_t *iters;
    uint4 *gstate;          // scratch form: workgroups x G x m check states
};

template <bool LDS_STATE>
__global__ __launch_bounds__(LDPC_THREADS) void idd_decode_kernel(idd_dec_args a)
{
    extern __shared__ float4 idd_smem[];
    __shared__ int s_done[LDPC_MAX_G], s_bad[LDPC_MAX_G], s_iters[LDPC_MAX_G];
    __shared__ int s_active;
    const int n = a.n, m = a.m;
    const int span = LDPC_THREADS / a.G, g = threadIdx.x / span, r = threadIdx.x - g * span;
    const int64_t cw = (int64_t)blockIdx.x * a.G + g;
    const bool mine = cw < a.ncw && a.state[cw] == 0;          // open: this call decodes it
    if (!__syncthreads_or(mine)) return;                       // every codeword of the group frozen (or past the end)

    float *Lg = reinterpret_cast<float *>(idd_smem) + (size_t)g * n;
    uint4 *stg;
    if constexpr (LDS_STATE)
        stg = reinterpret_cast<uint4 *>(reinterpret_cast<float *>(idd_smem) + (size_t)a.G * n) + (size_t)g * m;
    else
        stg = a.gstate + ((size_t)blockIdx.x * a.G + g) * m;
    const double *llr = a.llr + cw * a.n_tx;
    if (mine) {
        for (int v = r; v < n; v += span) {
            const int src = a.var_src[v];
            Lg[v] = src < 0 ? 0.0f : (float)(a.scale * llr[src]);
        }
        for (int c = r; c < m; c += span) stg[c] = make_uint4(0u, 0u, 0u, 0u);
    }
    if (r == 0 && g < LDPC_MAX_G) {
        s_done[g] = mine ? 0 : 1;
        s_bad[g] = 0;
        s_iters[g] = 0;
    }
    if (threadIdx.x >= a.G && threadIdx.x < LDPC_MAX_G) s_done[threadIdx.x] = 1, s_bad[threadIdx.x] = 0;
    __syncthreads();

    for (int t = 0; t <= a.max_iter; ++t) {
        if (t > 0) {
            for (int l = 0; l < a.nlayers; ++l) {
                const int4 lay = reinterpret_cast<const int4 *>(a.layer)[l];      // first check, checks, ELL offset, slots
                const int32_t *ell = a.ell + lay.z;
                if (!s_done[g])
                    for (int j = r; j < lay.y; j += span) ldpc_update_check(Lg, stg + lay.x + j, ell, lay.y, j, lay.w, a.alpha);
                __syncthreads();
            }
        }
        if (!s_done[g] && ldpc_syndrome_bad(Lg, a.check_ptr, a.edge_var, m, r, span)) s_bad[g] = 1;
        __syncthreads();
        if (threadIdx.x == 0) {
            int active = 0;
            for (int q = 0; q < LDPC_MAX_G; ++q) {
                if (!s_done[q]) {
                    if (!s_bad[q]) {
                        s_done[q] = 1;
                        s_iters[q] = t;
                    } else {
                        ++active;
                    }
                }
                s_bad[q] = 0;
            }
            s_active = active;
        }
        __syncthreads();
        if (s_active == 0) break;
    }

    // outputs of the open codewords; one still running after max_iter stops there, not converged (s_done still 0)
    if (!mine) return;
    const bool conv = s_done[g] != 0;
    if (a.post)
        for (int v = r; v < n; v += span) a.post[cw * n + v] = Lg[v];
    if (a.info_bits)
        for (int i = r; i < a.k; i += span) a.info_bits[cw * a.k + i] = Lg[a.info_var[i]] < 0.0f ? 1 : 0;
    float *ext = a.ext + cw * a.ext_stride;
    for (int t = r; t < a.n_tx; t += span) {
        const float L = Lg[a.tx_var[t]];
        float x;
        if (conv) {
            x = L < 0.0f ? -a.ext_sat : a.ext_sat;
        } else {
            x = __fsub_rn(L, (float)(a.scale * llr[t]));
            x = fminf(fmaxf(x, -a.ext_clip), a.ext_clip);
        }
        ext[t] = x;
    }
    if (r == 0) {
        if (a.iters) a.iters[cw] += conv ? s_iters[g] : a.max_iter;
        if (conv) a.state[cw] = 1;
    }
}

// counts[0..3] += information bit errors, codewords with one, codewords still open, iterations summed; a workgroup per
// codeword at a time
__global__ __launch_bounds__(LDPC_THREADS) void idd_count_kernel(const uint8_t *__restrict__ info, const uint8_t *__restrict__ ref,
                                                                 const uint8_t *__restrict__ state, const int32_t *__restrict__ iters, int64_t ncw,
                                                                 int32_t k, unsigned long long *__restrict__ counts)
{
    __shared__ int s_part[LDPC_THREADS / WF_WAVE];
    const int lane = threadIdx.x & (WF_WAVE - 1), wave = threadIdx.x / WF_WAVE;
    for (int64_t cw = blockIdx.x; cw < ncw; cw += gridDim.x) {
        int err = 0;                                           // of this wave: wave-uniform
        for (int i0 = wave * WF_WAVE; i0 < k; i0 += LDPC_THREADS) {
            const int i = i0 + lane;
            err += __popcll(__ballot(i < k && (info[cw * k + i] & 1) != (ref[cw * k + i] & 1)));
        }
        if (lane == 0) s_part[wave] = err;
        __syncthreads();
        if (threadIdx.x == 0) {
            int tot = 0;
            for (int w = 0; w < LDPC_THREADS / WF_WAVE; ++w) tot += s_part[w];
            if (tot) {
                atomicAdd(counts + 0, (unsigned long long)tot);
                atomicAdd(counts + 1, 1ull);
            }
            if (state[cw] == 0) atomicAdd(counts + 2, 1ull);
            atomicAdd(counts + 3, (unsigned long long)iters[cw]);
        }
        __syncthreads();
    }
}

extern "C" int wf_ldpc_decode_ext(wf_ctx *ctx, const wf_ldpc_code *code, const double *d_llr, int64_t ncw, double scale, float alpha,
                                  int max_iter, uint8_t *d_state, uint8_t *d_info_bits, float *d_post, int32_t *d_iters, float *d_ext,
                                  int64_t ext_stride, float ext_clip, float ext_sat, void *stream)
{
    WF_REQUIRE(ctx && code && d_llr && d_state && d_ext, "wf_ldpc_decode_ext: NULL argument");
    WF_REQUIRE(ncw >= 1, "wf_ldpc_decode_ext: ncw must be at least 1");
    WF_REQUIRE(max_iter >= 1 && max_iter <= 10000, "wf_ldpc_decode_ext: max_iter = %d outside 1 .. 10000", max_iter);
    WF_REQUIRE(wf_finite_pos(scale), "wf_ldpc_decode_ext: scale must be finite and positive");
    WF_REQUIRE(wf_finite_pos(alpha), "wf_ldpc_decode_ext: alpha must be finite and positive");
    WF_REQUIRE(ext_stride >= code->n_tx, "wf_ldpc_decode_ext: ext_stride = %lld is below n_tx = %d", (long long)ext_stride, code->n_tx);
    WF_REQUIRE(ext_clip > 0.0f, "wf_ldpc_decode_ext: ext_clip must be positive (INFINITY: no clip)");
    WF_REQUIRE(wf_finite_pos(ext_sat), "wf_ldpc_decode_ext: ext_sat must be finite and positive");
    WF_REQUIRE(wf_aligned(d_llr, 8) && wf_aligned(d_post, 4) && wf_aligned(d_iters, 4) && wf_aligned(d_ext, 4),
               "wf_ldpc_decode_ext: llr must be 8-byte, post, iters and ext 4-byte aligned");
    WF_REQUIRE_SAME_DEVICE("wf_ldpc_decode_ext", code, ctx);
    ldpc_geom g;
    idd_dec_args a;
    WF_TRY(ldpc_prepare(ctx, code, ncw, reinterpret_cast<const void *>(&idd_decode_kernel<true>), reinterpret_cast<const void *>(&idd_decode_kernel<false>), &g,
                        &a.gstate));
    a.layer = code->d_layer, a.ell = code->d_ell, a.check_ptr = code->d_check_ptr, a.edge_var = code->d_edge_var;
    a.var_src = code->d_var_src, a.info_var = code->d_info_var, a.tx_var = code->d_tx_var;
    a.n = code->n, a.m = code->m, a.nlayers = code->nlayers, a.n_tx = code->n_tx, a.k = code->k, a.G = g.G, a.max_iter = max_iter;
    a.ext_stride = ext_stride;
    a.scale = scale, a.alpha = alpha, a.ext_clip = ext_clip, a.ext_sat = ext_sat;
    // slices of at most g.grid workgroups, as wf_ldpc_decode (the scratch form's check state is sized for that many)
    return wf_for_slices(ncw, g.grid * g.G, [&](int64_t b0, int64_t count) -> int {
        a.ncw = count;
        a.llr = d_llr + b0 * code->n_tx;
        a.state = d_state + b0;
        a.info_bits = d_info_bits ? d_info_bits + b0 * code->k : nullptr;
        a.post = d_post ? d_post + b0 * code->n : nullptr;
        a.iters = d_iters ? d_iters + b0 : nullptr;
        a.ext = d_ext + b0 * ext_stride;
        const unsigned grid = (unsigned)((a.ncw + g.G - 1) / g.G);
        if (g.lds_state)
            hipLaunchKernelGGL(idd_decode_kernel<true>, dim3(grid), dim3(LDPC_THREADS), g.lds_bytes, wf_stream(stream), a);
        else
            hipLaunchKernelGGL(idd_decode_kernel<false>, dim3(grid), dim3(LDPC_THREADS), g.lds_bytes, wf_stream(stream), a);
        WF_LAUNCH_CHECK();
        return WF_OK;
    });
}

extern "C" int wf_ldpc_count(wf_ctx *ctx, const wf_ldpc_code *code, const uint8_t *d_info_bits, const uint8_t *d_ref_info,
                             const uint8_t *d_state, const int32_t *d_iters, int64_t ncw, int64_t *d_counts, void *stream)
{
    WF_REQUIRE(ctx && code && d_info_bits && d_ref_info && d_state && d_iters && d_counts, "wf_ldpc_count: NULL argument");
    WF_REQUIRE(ncw >= 1, "wf_ldpc_count: ncw must be at least 1");
    WF_REQUIRE(wf_aligned(d_counts, 8) && wf_aligned(d_iters, 4), "wf_ldpc_count: counts must be 8-byte and iters 4-byte aligned");
    WF_REQUIRE_SAME_DEVICE("wf_ldpc_count", code, ctx);
    WF_HIP(hipSetDevice(ctx->device));
    const unsigned grid = (unsigned)std::min<int64_t>(ncw, (int64_t)std::max(ctx->cus, 1) * 8);
    hipLaunchKernelGGL(idd_count_kernel, dim3(grid), dim3(LDPC_THREADS), 0, wf_stream(stream), d_info_bits, d_ref_info, d_state, d_iters, ncw,
                       code->k, reinterpret_cast<unsigned long long *>(d_counts));
    WF_LAUNCH_CHECK();
    return WF_OK;
}
