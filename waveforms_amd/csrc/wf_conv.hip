// wf_conv.hip — terminated feed-forward convolutional codes of rate 1 / n_out: the encoder and the exact max-log-MAP
// soft-in / soft-out decoder (include/wfhip.h states the code, the trellis and the decoder's arithmetic).  A code is an opaque
// handle whose tables are validated once on the host and uploaded into device memory the handle owns.
//
// Decoder: one wave of 64 lanes decodes 64 / S codewords in lockstep, lane = trellis state (S = 2^(K-1) states: K = 7 fills a
// wave with one codeword, K = 3 puts 16 side by side).  The steps of a codeword are serial (the definition fixes the order of
// every sum), so all the parallelism there is are the ncw S lanes.
//   forward sweep   lane s' takes alpha of its two predecessors 2 s' mod S and 2 s' mod S + 1 by ds_bpermute and keeps
//                   alpha every CONV_C steps in the context's detector scratch (one 256-byte row per wave and checkpoint);
//   backward sweep  segment by segment from the last: alpha of the segment's steps is recomputed from its checkpoint (the same
//                   operations on the same operands: the same floats) into LDS, one row of 64 lanes per step, then lane s
//                   runs beta with the two branches that LEAVE state s: beta of its successors by ds_bpermute, its own alpha
//                   from LDS, and the 2 (n_out + 1) maxima of a step are all-reduced over the S lanes of the codeword by a
//                   DPP butterfly (quad_perm, row_half_mirror, row_mirror inside a row of 16; ds_bpermute across rows).
// The channel values of a segment, its priors, reference bits and var -> src entries are staged in LDS by all lanes before
// the segment's serial loop, so that loop holds no load from global memory.
#include "wf_conv_common.h"

#define CONV_ENC_RUN 8              // steps per encoder thread
#define CONV_ENC_THREADS 256

struct wf_conv_code {
    int device = 0;
    int32_t K = 0, nu = 0, n_out = 0, k = 0, T = 0, N = 0, n_tx = 0;
    uint32_t gen[4] = {0, 0, 0, 0};
    void *d_block = nullptr;              // both tables below, one allocation
    const int32_t *d_var_src = nullptr;   // N: transmitted position of variable v, -1 when punctured
    const int32_t *d_tx_var = nullptr;    // n_tx
};

struct conv_geom : wf_wave_geom {
    size_t lds_bytes = 0, scratch_bytes = 0;
};

static size_t conv_lds_bytes(int nu, int n_out)
{
    const size_t G = 64 >> nu;
    return 4 * (G * (CONV_C * n_out + 1) + 2 * G * (CONV_C + 1) + CONV_C * n_out + CONV_C * 64);
}

static conv_geom conv_geometry(const wf_ctx *ctx, const wf_conv_code *c, int64_t ncw)
{
    conv_geom g;
    static_cast<wf_wave_geom &>(g) = wf_wave_geometry(ctx, c->nu, c->T, ncw, 0);
    g.lds_bytes = conv_lds_bytes(c->nu, c->n_out);
    g.scratch_bytes = (size_t)(g.per_launch * g.per_wave);
    return g;
}

// One thread per (codeword, run of CONV_ENC_RUN steps): the register at the run's first step is rebuilt from the nu message
// bits in front of it, the run's code bits go to their transmitted positions (none for a punctured variable).
__global__ __launch_bounds__(CONV_ENC_THREADS) void conv_encode_kernel(const uint8_t *info, int64_t ncw, int32_t k, int32_t T, int32_t nu,
                                                                       int32_t n_out, uint32_t g0, uint32_t g1, uint32_t g2, uint32_t g3,
                                                                       int32_t n_tx, const int32_t *var_src, uint8_t *out)
{
    const int runs = (T + CONV_ENC_RUN - 1) / CONV_ENC_RUN;
    const int64_t total = ncw * runs;
    for (int64_t w = (int64_t)blockIdx.x * CONV_ENC_THREADS + threadIdx.x; w < total; w += (int64_t)gridDim.x * CONV_ENC_THREADS) {
        const int64_t cw = w / runs;
        const int i0 = (int)(w - cw * runs) * CONV_ENC_RUN, i1 = min(i0 + CONV_ENC_RUN, T);
        const uint8_t *u = info + cw * k;
        uint32_t s = 0;                    // s_i0: message bit i0 - d sits at bit nu - d
        for (int d = 1; d <= nu; ++d) {
            const int i = i0 - d;
            if (i >= 0 && i < k) s |= (uint32_t)(u[i] & 1) << (nu - d);
        }
        for (int i = i0; i < i1; ++i) {
            const uint32_t reg = ((i < k ? (uint32_t)(u[i] & 1) : 0u) << nu) | s;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < n_out) {
                    const uint32_t gj = j == 0 ? g0 : j == 1 ? g1 : j == 2 ? g2 : g3;
                    const int src = var_src[n_out * i + j];
                    if (src >= 0) out[cw * n_tx + src] = (uint8_t)(__popc(reg & gj) & 1);
                }
            }
            s = reg >> 1;
        }
    }
}

struct conv_siso_args {
    const int32_t *var_src;
    const double *llr;
    const float *prior;
    uint8_t *bits;
    float *post, *ext;
    const uint8_t *ref;
    unsigned long long *counts;
    float *ckpt;                    // waves x nseg x 64
    int64_t ncw, ext_stride;
    double scale;
    float clip;
    int32_t k, T, n_tx, nseg;
    uint32_t gen[4];
};

template <int NU, int NOUT>
__global__ __launch_bounds__(WF_WAVE) void conv_siso_kernel(conv_siso_args a)
{
    constexpr int S = 1 << NU, G = WF_WAVE / S, C = CONV_C, LSTR = C * NOUT + 1, ASTR = C + 1;
    __shared__ float sL[G * LSTR], sA[G * ASTR], sAl[C * WF_WAVE];
    __shared__ int sR[G * ASTR], sSrc[C * NOUT];
    const int lane = threadIdx.x, s = lane & (S - 1), g = lane >> NU, base = lane - s;
    const int64_t wave = blockIdx.x, cw = wave * G + g;
    const bool mine = cw < a.ncw;
    const int k = a.k, T = a.T;

    // the two branches that ENTER state s (both with input u_in = its top bit), and the two that LEAVE it (u = 0, 1)
    const bool u_in = (s >> (NU - 1)) != 0;
    const int p0 = (2 * s) & (S - 1), p1 = p0 + 1, n0 = s >> 1, n1 = n0 | (S >> 1);
    uint32_t cin0[NOUT], cin1[NOUT], cout0[NOUT], cout1[NOUT];        // all ones where the branch's code bit j is 1
#pragma unroll
    for (int j = 0; j < NOUT; ++j) {
        const uint32_t gj = a.gen[j], top = u_in ? (uint32_t)S : 0u;
        cin0[j] = 0u - (__popc((top | (uint32_t)p0) & gj) & 1u);
        cin1[j] = 0u - (__popc((top | (uint32_t)p1) & gj) & 1u);
        cout0[j] = 0u - (__popc((uint32_t)s & gj) & 1u);
        cout1[j] = 0u - (__popc(((uint32_t)S | (uint32_t)s) & gj) & 1u);
    }

    // a segment's operands into LDS, by all lanes: L (G x C x NOUT), the prior and the reference bit (G x C), var -> src
    auto stage = [&](int seg) {
        __syncthreads();
        const int i0 = seg * C;
        for (int idx = lane; idx < G * C * NOUT; idx += WF_WAVE) {
            const int gg = idx / (C * NOUT), r = idx - gg * (C * NOUT), i = i0 + r / NOUT;
            const int64_t cwg = wave * G + gg;
            float L = 0.0f;
            if (i < T && cwg < a.ncw) {
                const int src = a.var_src[NOUT * i0 + r];
                if (src >= 0) L = (float)(a.scale * a.llr[cwg * a.n_tx + src]);
            }
            sL[gg * LSTR + r] = L;
        }
        for (int idx = lane; idx < G * C; idx += WF_WAVE) {
            const int gg = idx / C, t = idx - gg * C, i = i0 + t;
            const int64_t cwg = wave * G + gg;
            const bool in = i < k && cwg < a.ncw;
            sA[gg * ASTR + t] = in && a.prior ? a.prior[cwg * k + i] : 0.0f;
            sR[gg * ASTR + t] = in && a.ref ? (a.ref[cwg * k + i] & 1) : 0;
        }
        for (int idx = lane; idx < C * NOUT; idx += WF_WAVE) sSrc[idx] = NOUT * i0 + idx < NOUT * T ? a.var_src[NOUT * i0 + idx] : -1;
        __syncthreads();
    };
    // alpha_{i+1}(s) from alpha_i, i = seg C + t
    auto forward = [&](float al, int i, int t) {
        float L[NOUT];
#pragma unroll
        for (int j = 0; j < NOUT; ++j) L[j] = sL[g * LSTR + t * NOUT + j];
        const float start = u_in ? -sA[g * ASTR + t] : 0.0f;
        const float g0 = conv_gamma<NOUT>(start, L, cin0), g1 = conv_gamma<NOUT>(start, L, cin1);
        const float a0 = __shfl(al, base + p0, WF_WAVE), a1 = __shfl(al, base + p1, WF_WAVE);
        const float an = fmaxf(__fadd_rn(a0, g0), __fadd_rn(a1, g1));
        return i >= k && u_in ? -INFINITY : an;
    };

    float *ck = a.ckpt + (size_t)wave * a.nseg * WF_WAVE + lane;
    float al = s == 0 ? 0.0f : -INFINITY;
    for (int seg = 0; seg < a.nseg; ++seg) {
        ck[(size_t)seg * WF_WAVE] = al;
        if (seg == a.nseg - 1) break;
        stage(seg);
        for (int t = 0; t < C; ++t) al = forward(al, seg * C + t, t);
    }

    float be = s == 0 ? 0.0f : -INFINITY;
    int err = 0;
    for (int seg = a.nseg - 1; seg >= 0; --seg) {
        const int i0 = seg * C, len = min(C, T - i0);
        stage(seg);
        al = ck[(size_t)seg * WF_WAVE];
        for (int t = 0; t < len; ++t) {
            sAl[t * WF_WAVE + lane] = al;           // (read back by this lane only)
            al = forward(al, i0 + t, t);
        }
        for (int t = len - 1; t >= 0; --t) {
            const int i = i0 + t;
            float L[NOUT];
#pragma unroll
            for (int j = 0; j < NOUT; ++j) L[j] = sL[g * LSTR + t * NOUT + j];
            const float A = sA[g * ASTR + t], ai = sAl[t * WF_WAVE + lane];
            const float b0 = __shfl(be, base + n0, WF_WAVE), b1 = __shfl(be, base + n1, WF_WAVE);
            const float g0 = conv_gamma<NOUT>(0.0f, L, cout0), g1 = conv_gamma<NOUT>(-A, L, cout1);
            const bool tail = i >= k;
            const float V0 = __fadd_rn(__fadd_rn(ai, g0), b0), V1 = tail ? -INFINITY : __fadd_rn(__fadd_rn(ai, g1), b1);
            const float W0 = __fadd_rn(g0, b0), W1 = tail ? -INFINITY : __fadd_rn(g1, b1);
            be = fmaxf(W0, W1);
            const float lam = conv_group_max<S>(V0) - conv_group_max<S>(V1);
            if (s == 0 && mine && !tail) {
                const int bit = lam < 0.0f ? 1 : 0;
                if (a.post) a.post[cw * k + i] = lam;
                if (a.bits) a.bits[cw * k + i] = (uint8_t)bit;
                err += bit != sR[g * ASTR + t] ? 1 : 0;
            }
#pragma unroll
            for (int j = 0; j < NOUT; ++j) {
                const float m0 = conv_group_max<S>(fmaxf(conv_drop_if(cout0[j], V0), conv_drop_if(cout1[j], V1)));
                const float m1 = conv_group_max<S>(fmaxf(conv_keep_if(cout0[j], V0), conv_keep_if(cout1[j], V1)));
                const int src = sSrc[t * NOUT + j];
                if (s == j && mine && a.ext && src >= 0) {
                    const float e = __fsub_rn(__fsub_rn(m0, m1), L[j]);
                    a.ext[cw * a.ext_stride + src] = fminf(fmaxf(e, -a.clip), a.clip);
                }
            }
        }
    }
    if (a.ref && s == 0 && mine) {
        atomicAdd(a.counts + 0, (unsigned long long)err);
        if (err) atomicAdd(a.counts + 1, 1ull);
    }
}

extern "C" int wf_conv_code_create(wf_ctx *ctx, int32_t K, int32_t n_out, const uint32_t *h_gen, int32_t k, int32_t n_tx,
                                   const int32_t *h_tx_var, wf_conv_code **out)
{
    WF_REQUIRE(ctx && h_gen && h_tx_var && out, "wf_conv_code_create: NULL argument");
    *out = nullptr;
    WF_REQUIRE(K >= 3 && K <= 7, "wf_conv_code_create: K = %d outside 3 .. 7", K);
    WF_REQUIRE(n_out >= 2 && n_out <= 4, "wf_conv_code_create: n_out = %d outside 2 .. 4", n_out);
    const int nu = K - 1;
    for (int j = 0; j < n_out; ++j)
        WF_REQUIRE(wf_tap_mask_ok(h_gen[j], K), "wf_conv_code_create: generator %d = 0%o must be a K-bit mask with bit K - 1 and bit 0 set", j, h_gen[j]);
    WF_REQUIRE(k >= 1 && (int64_t)n_out * ((int64_t)k + nu) <= CONV_MAX_N, "wf_conv_code_create: k = %d: N = n_out (k + K - 1) outside n_out K .. %d", k,
               CONV_MAX_N);
    const int32_t T = k + nu, N = n_out * T;
    WF_REQUIRE(n_tx >= 1 && n_tx <= N, "wf_conv_code_create: n_tx = %d outside 1 .. N = %d", n_tx, N);
    std::vector<int32_t> blob((size_t)N + n_tx, -1);
    WF_TRY(wf_tx_table("wf_conv_code_create", h_tx_var, n_tx, N, blob.data(), blob.data() + N));

    void *d_block;
    WF_TRY(wf_code_upload("wf_conv_code_create", ctx->device, blob.data(), blob.size() * sizeof(int32_t), &d_block));
    wf_conv_code *c = new wf_conv_code();
    c->device = ctx->device, c->d_block = d_block;
    c->K = K, c->nu = nu, c->n_out = n_out, c->k = k, c->T = T, c->N = N, c->n_tx = n_tx;
    for (int j = 0; j < n_out; ++j) c->gen[j] = h_gen[j];
    c->d_var_src = static_cast<const int32_t *>(c->d_block);
    c->d_tx_var = c->d_var_src + N;
    *out = c;
    return WF_OK;
}

extern "C" int wf_conv_code_free(wf_conv_code *code)
{
    if (!code) return WF_OK;
    const int rc = wf_code_release("wf_conv_code_free", code->device, {code->d_block});
    delete code;                          // (whatever hipFree said: the host struct never outlives the call)
    return rc;
}

extern "C" int wf_conv_encode(wf_ctx *ctx, const wf_conv_code *code, const uint8_t *d_info, int64_t ncw, uint8_t *d_tx, void *stream)
{
    WF_REQUIRE(ctx && code && d_info && d_tx, "wf_conv_encode: NULL argument");
    WF_REQUIRE(ncw >= 1, "wf_conv_encode: ncw must be at least 1");
    WF_REQUIRE_SAME_DEVICE("wf_conv_encode", code, ctx);
    WF_HIP(hipSetDevice(ctx->device));
    const int64_t work = ncw * ((code->T + CONV_ENC_RUN - 1) / CONV_ENC_RUN);
    const int grid = wf_grid_for(work, CONV_ENC_THREADS, std::max(ctx->cus, 1) * 16);
    hipLaunchKernelGGL(conv_encode_kernel, dim3(grid), dim3(CONV_ENC_THREADS), 0, wf_stream(stream), d_info, ncw, code->k, code->T, code->nu,
                       code->n_out, code->gen[0], code->gen[1], code->gen[2], code->gen[3], code->n_tx, code->d_var_src, d_tx);
    WF_LAUNCH_CHECK();
    return WF_OK;
}

extern "C" int wf_conv_siso_geometry(wf_ctx *ctx, const wf_conv_code *code, int64_t ncw, int64_t *h_geom)
{
    WF_REQUIRE(ctx && code && h_geom && ncw >= 1, "wf_conv_siso_geometry: bad argument");
    const conv_geom g = conv_geometry(ctx, code, ncw);
    h_geom[0] = g.G;
    h_geom[1] = g.waves;
    h_geom[2] = CONV_C;
    h_geom[3] = (int64_t)g.lds_bytes;
    h_geom[4] = (int64_t)g.scratch_bytes;
    return WF_OK;
}

template <int NU>
static void conv_siso_launch(int n_out, unsigned grid, hipStream_t st, const conv_siso_args &a)
{
    if (n_out == 2) hipLaunchKernelGGL((conv_siso_kernel<NU, 2>), dim3(grid), dim3(WF_WAVE), 0, st, a);
    else if (n_out == 3) hipLaunchKernelGGL((conv_siso_kernel<NU, 3>), dim3(grid), dim3(WF_WAVE), 0, st, a);
    else hipLaunchKernelGGL((conv_siso_kernel<NU, 4>), dim3(grid), dim3(WF_WAVE), 0, st, a);
}

extern "C" int wf_conv_siso(wf_ctx *ctx, const wf_conv_code *code, const double *d_llr, int64_t ncw, double scale, const float *d_info_prior,
                            uint8_t *d_info_bits, float *d_info_post, float *d_ext, int64_t ext_stride, float ext_clip,
                            const uint8_t *d_ref_info, int64_t *d_counts, void *stream)
{
    WF_REQUIRE(ctx && code && d_llr, "wf_conv_siso: NULL argument");
    WF_REQUIRE(ncw >= 1, "wf_conv_siso: ncw must be at least 1");
    WF_REQUIRE(wf_finite_pos(scale), "wf_conv_siso: scale must be finite and positive");
    WF_REQUIRE(!d_ext || (ext_stride >= code->n_tx && ext_clip > 0.0f), "wf_conv_siso: d_ext needs ext_stride >= n_tx and ext_clip > 0");
    WF_REQUIRE(!d_ref_info || d_counts, "wf_conv_siso: d_ref_info needs d_counts");
    WF_REQUIRE(wf_aligned(d_llr, 8) && wf_aligned(d_counts, 8) && wf_aligned(d_info_prior, 4) && wf_aligned(d_info_post, 4) && wf_aligned(d_ext, 4),
               "wf_conv_siso: llr and counts must be 8-byte, prior, post and ext 4-byte aligned");
    WF_REQUIRE_SAME_DEVICE("wf_conv_siso", code, ctx);
    const conv_geom g = conv_geometry(ctx, code, ncw);
    WF_HIP(hipSetDevice(ctx->device));
    WF_TRY(wf_ctx_reserve_vit(ctx, (g.scratch_bytes + 7) / 8));
    conv_siso_args a;
    a.var_src = code->d_var_src;
    a.ckpt = reinterpret_cast<float *>(ctx->d_vit_edge);
    a.ext_stride = ext_stride, a.scale = scale, a.clip = ext_clip;
    a.k = code->k, a.T = code->T, a.n_tx = code->n_tx, a.nseg = g.nseg;
    for (int j = 0; j < 4; ++j) a.gen[j] = code->gen[j];
    a.counts = reinterpret_cast<unsigned long long *>(d_counts);
    // launches of at most g.per_launch waves (the checkpoints in the scratch are sized for that many)
    return wf_for_slices(ncw, g.per_launch * g.G, [&](int64_t b0, int64_t count) -> int {
        a.ncw = count;
        a.llr = d_llr + b0 * code->n_tx;
        a.prior = d_info_prior ? d_info_prior + b0 * code->k : nullptr;
        a.bits = d_info_bits ? d_info_bits + b0 * code->k : nullptr;
        a.post = d_info_post ? d_info_post + b0 * code->k : nullptr;
        a.ext = d_ext ? d_ext + b0 * ext_stride : nullptr;
        a.ref = d_ref_info ? d_ref_info + b0 * code->k : nullptr;
        const unsigned grid = (unsigned)((a.ncw + g.G - 1) / g.G);
        const hipStream_t st = wf_stream(stream);
        switch (code->nu) {
        case 2: conv_siso_launch<2>(code->n_out, grid, st, a); break;
        case 3: conv_siso_launch<3>(code->n_out, grid, st, a); break;
        case 4: conv_siso_launch<4>(code->n_out, grid, st, a); break;
        case 5: conv_siso_launch<5>(code->n_out, grid, st, a); break;
        default: conv_siso_launch<6>(code->n_out, grid, st, a); break;
        }
        WF_LAUNCH_CHECK();
        return WF_OK;
    });
}
