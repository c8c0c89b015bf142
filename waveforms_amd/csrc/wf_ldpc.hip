// wf_ldpc.hip — LDPC codes: a systematic encoder (parity = A u over GF(2)) and a layered normalized min-sum decoder
// (include/wfhip.h states the decoder's definition).  A code is an opaque handle whose tables are validated once on the
// host and uploaded into device memory the handle owns.
//
// Decoder: a workgroup of 256 threads decodes G codewords in lockstep; the posteriors L of those codewords live in LDS as
// float32.  For each layer, a thread takes one (codeword, check) pair at a time: one pass over the check's edges forms
// T_e = L_v - R_e and the compressed check state (min, second min, argmin, signs), a second pass re-forms the same T_e and
// writes L_v = T_e + R_e.  The layers' edges are stored slot-major (slot i of every check of the layer, then slot i + 1), so
// consecutive lanes read consecutive table words and, for a quasi-cyclic layer, consecutive variables mod Z: distinct LDS
// banks.  The check state is 16 B per check and codeword: in LDS beside L when both fit in 64 KiB for the G codewords,
// otherwise in the context's detector scratch.  A separate pass over the checks forms the syndrome after each iteration.
#include "wf_ldpc.h"

struct ldpc_dec_args {
    const int32_t *layer, *ell, *check_ptr, *edge_var, *var_src, *info_var;
    int32_t n, m, nlayers, n_tx, k, G, max_iter;
    int64_t ncw;
    const double *llr;
    double scale;
    float alpha;
    uint8_t *info_bits;
    float *post;
    int32_t *iters;
    const uint8_t *ref;
    unsigned long long *counts;
    uint4 *gstate;          // scratch form: workgroups x G x m check states
};

template <bool LDS_STATE>
__global__ __launch_bounds__(LDPC_THREADS) void ldpc_decode_kernel(ldpc_dec_args a)
{
    extern __shared__ float4 ldpc_smem[];
    __shared__ int s_done[LDPC_MAX_G], s_bad[LDPC_MAX_G], s_iters[LDPC_MAX_G], s_err[LDPC_MAX_G];
    __shared__ int s_active;
    const int n = a.n, m = a.m;
    // thread -> (codeword g of the group, lane r of the span of threads that codeword has); G is a power of two
    const int span = LDPC_THREADS / a.G, g = threadIdx.x / span, r = threadIdx.x - g * span;
    float *Lg = reinterpret_cast<float *>(ldpc_smem) + (size_t)g * n;
    uint4 *stg;
    if constexpr (LDS_STATE)
        stg = reinterpret_cast<uint4 *>(reinterpret_cast<float *>(ldpc_smem) + (size_t)a.G * n) + (size_t)g * m;
    else
        stg = a.gstate + ((size_t)blockIdx.x * a.G + g) * m;      // (one launch covers at most ldpc_geom::grid workgroups)

    {
        const int64_t grp = blockIdx.x, cw = grp * a.G + g;
        const bool mine = cw < a.ncw;
        // L_v = (float)(scale * λ[src v]) (product in float64), 0 when punctured; R_e = 0
        if (mine) {
            const double *llr = a.llr + cw * a.n_tx;
            for (int v = r; v < n; v += span) {
                const int src = a.var_src[v];
                Lg[v] = src < 0 ? 0.0f : (float)(a.scale * llr[src]);
            }
            for (int c = r; c < m; c += span) stg[c] = make_uint4(0u, 0u, 0u, 0u);
        }
        if (threadIdx.x < LDPC_MAX_G) {
            s_done[threadIdx.x] = grp * a.G + threadIdx.x < a.ncw && (int)threadIdx.x < a.G ? 0 : 1;
            s_bad[threadIdx.x] = 0;
            s_iters[threadIdx.x] = 0;
            s_err[threadIdx.x] = 0;
        }
        __syncthreads();

        for (int t = 0; t <= a.max_iter; ++t) {
            if (t > 0) {
                for (int l = 0; l < a.nlayers; ++l) {
                    const int4 lay = reinterpret_cast<const int4 *>(a.layer)[l];      // first check, checks, ELL offset, slots
                    const int32_t *ell = a.ell + lay.z;
                    if (!s_done[g]) {
                        for (int j = r; j < lay.y; j += span) {
                            ldpc_update_check(Lg, stg + lay.x + j, ell, lay.y, j, lay.w, a.alpha);
                        }
                    }
                    __syncthreads();
                }
            }
            // syndrome of x̂ = [L < 0] for the codewords still running
            if (!s_done[g]) {
                if (ldpc_syndrome_bad(Lg, a.check_ptr, a.edge_var, m, r, span)) s_bad[g] = 1;
            }
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

        // outputs; a codeword still running after max_iter stops there, not converged
        if (mine) {
            if (a.post)
                for (int v = r; v < n; v += span) a.post[cw * n + v] = Lg[v];
            int err = 0;
            for (int i = r; i < a.k; i += span) {
                const uint8_t b = Lg[a.info_var[i]] < 0.0f ? 1 : 0;
                if (a.info_bits) a.info_bits[cw * a.k + i] = b;
                if (a.ref) err += b != (a.ref[cw * a.k + i] & 1) ? 1 : 0;
            }
            if (err) atomicAdd(&s_err[g], err);
        }
        __syncthreads();
        if (mine && r == 0) {
            // (s_done of a codeword that ran to max_iter is still 0 here: the last round above left it running)
            const int it = s_done[g] ? s_iters[g] : a.max_iter;
            if (a.iters) a.iters[cw] = it;
            if (a.ref && a.counts) {
                atomicAdd(a.counts + 0, (unsigned long long)s_err[g]);
                if (s_err[g]) atomicAdd(a.counts + 1, 1ull);
                if (!s_done[g]) atomicAdd(a.counts + 2, 1ull);
                atomicAdd(a.counts + 3, (unsigned long long)it);
            }
        }
        __syncthreads();
    }
}

// One workgroup per codeword: u packed by wave ballots into LDS, each parity bit the parity of the popcounts of
// A_row & u, the codeword assembled in LDS by variable and written in transmit order.
__global__ __launch_bounds__(LDPC_THREADS) void ldpc_encode_kernel(const uint8_t *info, int64_t ncw, int32_t k, int32_t kw, int32_t np,
                                                                   int32_t n_tx, const uint64_t *gen, const int32_t *info_var,
                                                                   const int32_t *par_var, const int32_t *tx_var, uint8_t *out)
{
    __shared__ uint64_t u[LDPC_MAX_N / 64];
    __shared__ uint8_t x[LDPC_MAX_N];
    const int tid = threadIdx.x, lane = tid & (WF_WAVE - 1), wave = tid / WF_WAVE;
    for (int64_t cw = blockIdx.x; cw < ncw; cw += gridDim.x) {
        const uint8_t *in = info + cw * k;
        for (int w = wave; w < kw; w += LDPC_THREADS / WF_WAVE) {
            const int i = w * 64 + lane;
            const int b = i < k ? (in[i] & 1) : 0;
            const uint64_t word = __ballot(b);
            if (lane == 0) u[w] = word;
        }
        for (int i = tid; i < k; i += LDPC_THREADS) x[info_var[i]] = in[i] & 1;
        __syncthreads();
        for (int r = tid; r < np; r += LDPC_THREADS) {
            const uint64_t *row = gen + (size_t)r * kw;
            int acc = 0;
            for (int w = 0; w < kw; ++w) acc += __popcll(row[w] & u[w]);
            x[par_var[r]] = (uint8_t)(acc & 1);
        }
        __syncthreads();
        for (int t = tid; t < n_tx; t += LDPC_THREADS) out[cw * n_tx + t] = x[tx_var[t]];
        __syncthreads();
    }
}

extern "C" int wf_ldpc_code_create(wf_ctx *ctx, int32_t n, int32_t m, const int32_t *h_check_ptr, const int32_t *h_edge_var,
                                   int32_t nlayers, const int32_t *h_layer_ptr, int32_t n_tx, const int32_t *h_tx_var, int32_t k,
                                   const int32_t *h_info_var, const uint64_t *h_parity_gen, wf_ldpc_code **out)
{
    WF_REQUIRE(ctx && h_check_ptr && h_edge_var && h_layer_ptr && h_tx_var && h_info_var && out, "wf_ldpc_code_create: NULL argument");
    *out = nullptr;
    WF_REQUIRE(n >= 2 && n <= LDPC_MAX_N, "wf_ldpc_code_create: n = %d outside 2 .. %d", n, LDPC_MAX_N);
    WF_REQUIRE(m >= 1 && m <= 4 * n, "wf_ldpc_code_create: m = %d outside 1 .. 4 n", m);
    WF_REQUIRE(nlayers >= 1 && nlayers <= m, "wf_ldpc_code_create: nlayers = %d outside 1 .. m", nlayers);
    WF_REQUIRE(n_tx >= 1 && n_tx <= n, "wf_ldpc_code_create: n_tx = %d outside 1 .. n", n_tx);
    WF_REQUIRE(k >= 1 && k < n, "wf_ldpc_code_create: k = %d outside 1 .. n - 1", k);
    WF_REQUIRE(h_check_ptr[0] == 0, "wf_ldpc_code_create: check_ptr[0] must be 0");
    for (int c = 0; c < m; ++c) {
        const int64_t d = (int64_t)h_check_ptr[c + 1] - h_check_ptr[c];
        WF_REQUIRE(d >= 2 && d <= LDPC_MAX_DEG, "wf_ldpc_code_create: check %d has degree %lld (2 .. %d)", c, (long long)d, LDPC_MAX_DEG);
    }
    const int32_t nedges = h_check_ptr[m];
    std::vector<int32_t> owner(n, -1);      // last check that touched v (distinct variables within a check)
    for (int c = 0; c < m; ++c)
        for (int e = h_check_ptr[c]; e < h_check_ptr[c + 1]; ++e) {
            const int v = h_edge_var[e];
            WF_REQUIRE(v >= 0 && v < n, "wf_ldpc_code_create: edge %d names variable %d", e, v);
            WF_REQUIRE(owner[v] != c, "wf_ldpc_code_create: check %d names variable %d twice", c, v);
            owner[v] = c;
        }
    WF_REQUIRE(h_layer_ptr[0] == 0 && h_layer_ptr[nlayers] == m, "wf_ldpc_code_create: layer_ptr must run from 0 to m");
    std::vector<int32_t> layer_of(n, -1);
    int lmax = 0, slots_total = 0;
    for (int l = 0; l < nlayers; ++l) {
        WF_REQUIRE(h_layer_ptr[l + 1] > h_layer_ptr[l], "wf_ldpc_code_create: layer %d is empty", l);
        int slots = 0;
        for (int c = h_layer_ptr[l]; c < h_layer_ptr[l + 1]; ++c) {
            slots = std::max(slots, h_check_ptr[c + 1] - h_check_ptr[c]);
            for (int e = h_check_ptr[c]; e < h_check_ptr[c + 1]; ++e) {
                const int v = h_edge_var[e];
                WF_REQUIRE(layer_of[v] != l, "wf_ldpc_code_create: variable %d appears in two checks of layer %d", v, l);
                layer_of[v] = l;
            }
        }
        lmax = std::max(lmax, h_layer_ptr[l + 1] - h_layer_ptr[l]);
        slots_total += slots * (h_layer_ptr[l + 1] - h_layer_ptr[l]);
    }
    std::vector<int32_t> var_src(n, -1);
    WF_TRY(wf_tx_table("wf_ldpc_code_create", h_tx_var, n_tx, n, var_src.data(), nullptr));
    std::vector<int32_t> is_info(n, 0);
    for (int i = 0; i < k; ++i) {
        const int v = h_info_var[i];
        WF_REQUIRE(v >= 0 && v < n && !is_info[v], "wf_ldpc_code_create: info_var[%d] = %d is out of range or repeated", i, v);
        is_info[v] = 1;
    }

    // host tables: layer records, slot-major ELL, CSR, var_src, tx_var, info_var, par_var
    std::vector<int32_t> layer(4 * (size_t)nlayers), ell((size_t)slots_total, -1), par;
    par.reserve(n - k);
    for (int v = 0; v < n; ++v)
        if (!is_info[v]) par.push_back(v);
    int off = 0;
    for (int l = 0; l < nlayers; ++l) {
        const int c0 = h_layer_ptr[l], sz = h_layer_ptr[l + 1] - c0;
        int slots = 0;
        for (int c = c0; c < c0 + sz; ++c) slots = std::max(slots, h_check_ptr[c + 1] - h_check_ptr[c]);
        layer[4 * l] = c0;
        layer[4 * l + 1] = sz;
        layer[4 * l + 2] = off;
        layer[4 * l + 3] = slots;
        for (int j = 0; j < sz; ++j)
            for (int e = h_check_ptr[c0 + j], i = 0; e < h_check_ptr[c0 + j + 1]; ++e, ++i) ell[off + (size_t)i * sz + j] = h_edge_var[e];
        off += slots * sz;
    }
    std::vector<int32_t> blob;
    auto put = [&blob](const int32_t *p, size_t cnt) {
        const size_t at = blob.size();
        blob.insert(blob.end(), p, p + cnt);
        return at;
    };
    const size_t o_layer = put(layer.data(), layer.size()), o_ell = put(ell.data(), ell.size()), o_cptr = put(h_check_ptr, (size_t)m + 1),
                 o_evar = put(h_edge_var, (size_t)nedges), o_src = put(var_src.data(), (size_t)n), o_tx = put(h_tx_var, (size_t)n_tx),
                 o_info = put(h_info_var, (size_t)k), o_par = put(par.data(), par.size());

    void *d_block, *d_gen = nullptr;
    WF_TRY(wf_code_upload("wf_ldpc_code_create", ctx->device, blob.data(), blob.size() * sizeof(int32_t), &d_block));
    if (h_parity_gen) {
        const int rc = wf_code_upload("wf_ldpc_code_create", ctx->device, h_parity_gen, (size_t)(n - k) * ((k + 63) / 64) * sizeof(uint64_t), &d_gen);
        if (rc) {
            (void)hipFree(d_block);
            return rc;
        }
    }
    wf_ldpc_code *c = new wf_ldpc_code();
    c->device = ctx->device, c->d_block = d_block, c->d_gen = static_cast<uint64_t *>(d_gen);
    c->n = n, c->m = m, c->nlayers = nlayers, c->n_tx = n_tx, c->k = k, c->kw = (k + 63) / 64, c->lmax = lmax, c->nedges = nedges;
    c->has_gen = h_parity_gen != nullptr;
    const int32_t *base = static_cast<const int32_t *>(c->d_block);
    c->d_layer = base + o_layer, c->d_ell = base + o_ell, c->d_check_ptr = base + o_cptr, c->d_edge_var = base + o_evar;
    c->d_var_src = base + o_src, c->d_tx_var = base + o_tx, c->d_info_var = base + o_info, c->d_par_var = base + o_par;
    *out = c;
    return WF_OK;
}

extern "C" int wf_ldpc_code_free(wf_ldpc_code *code)
{
    if (!code) return WF_OK;
    const int rc = wf_code_release("wf_ldpc_code_free", code->device, {code->d_block, code->d_gen});
    delete code;                          // (whatever hipFree said: the host struct never outlives the call)
    return rc;
}

extern "C" int wf_ldpc_encode(wf_ctx *ctx, const wf_ldpc_code *code, const uint8_t *d_info, int64_t ncw, uint8_t *d_tx, void *stream)
{
    WF_REQUIRE(ctx && code && d_info && d_tx, "wf_ldpc_encode: NULL argument");
    WF_REQUIRE(ncw >= 1, "wf_ldpc_encode: ncw must be at least 1");
    WF_REQUIRE(code->has_gen, "wf_ldpc_encode: the code was created without a parity generator (decode only)");
    WF_REQUIRE_SAME_DEVICE("wf_ldpc_encode", code, ctx);
    WF_HIP(hipSetDevice(ctx->device));
    const unsigned grid = (unsigned)std::min<int64_t>(ncw, (int64_t)std::max(ctx->cus, 1) * 4);
    hipLaunchKernelGGL(ldpc_encode_kernel, dim3(grid), dim3(LDPC_THREADS), 0, wf_stream(stream), d_info, ncw, code->k, code->kw,
                       code->n - code->k, code->n_tx, code->d_gen, code->d_info_var, code->d_par_var, code->d_tx_var, d_tx);
    WF_LAUNCH_CHECK();
    return WF_OK;
}

extern "C" int wf_ldpc_decode_geometry(wf_ctx *ctx, const wf_ldpc_code *code, int64_t ncw, int64_t *h_geom)
{
    WF_REQUIRE(ctx && code && h_geom && ncw >= 1, "wf_ldpc_decode_geometry: bad argument");
    const ldpc_geom g = ldpc_geometry(ctx, code, ncw);
    h_geom[0] = g.lds_state ? 0 : 1;
    h_geom[1] = g.G;
    h_geom[2] = g.grid;
    h_geom[3] = (int64_t)g.lds_bytes;
    h_geom[4] = (int64_t)g.scratch_bytes;
    return WF_OK;
}

extern "C" int wf_ldpc_decode(wf_ctx *ctx, const wf_ldpc_code *code, const double *d_llr, int64_t ncw, double scale, float alpha,
                              int max_iter, uint8_t *d_info_bits, float *d_post, int32_t *d_iters, const uint8_t *d_ref_info,
                              int64_t *d_counts, void *stream)
{
    WF_REQUIRE(ctx && code && d_llr, "wf_ldpc_decode: NULL argument");
    WF_REQUIRE(ncw >= 1, "wf_ldpc_decode: ncw must be at least 1");
    WF_REQUIRE(max_iter >= 1 && max_iter <= 10000, "wf_ldpc_decode: max_iter = %d outside 1 .. 10000", max_iter);
    WF_REQUIRE(wf_finite_pos(scale), "wf_ldpc_decode: scale must be finite and positive");
    WF_REQUIRE(wf_finite_pos(alpha), "wf_ldpc_decode: alpha must be finite and positive");
    WF_REQUIRE(!d_ref_info || d_counts, "wf_ldpc_decode: d_ref_info needs d_counts");
    WF_REQUIRE(wf_aligned(d_llr, 8) && wf_aligned(d_counts, 8) && wf_aligned(d_post, 4) && wf_aligned(d_iters, 4),
               "wf_ldpc_decode: llr and counts must be 8-byte, post and iters 4-byte aligned");
    WF_REQUIRE_SAME_DEVICE("wf_ldpc_decode", code, ctx);
    ldpc_geom g;
    ldpc_dec_args a;
    WF_TRY(ldpc_prepare(ctx, code, ncw, reinterpret_cast<const void *>(&ldpc_decode_kernel<true>), reinterpret_cast<const void *>(&ldpc_decode_kernel<false>), &g,
                        &a.gstate));
    a.layer = code->d_layer, a.ell = code->d_ell, a.check_ptr = code->d_check_ptr, a.edge_var = code->d_edge_var;
    a.var_src = code->d_var_src, a.info_var = code->d_info_var;
    a.n = code->n, a.m = code->m, a.nlayers = code->nlayers, a.n_tx = code->n_tx, a.k = code->k, a.G = g.G, a.max_iter = max_iter;
    a.scale = scale, a.alpha = alpha;
    a.counts = reinterpret_cast<unsigned long long *>(d_counts);
    // slices of at most g.grid workgroups (the scratch form's check state is sized for that many)
    return wf_for_slices(ncw, g.grid * g.G, [&](int64_t b0, int64_t count) -> int {
        a.ncw = count;
        a.llr = d_llr + b0 * code->n_tx;
        a.info_bits = d_info_bits ? d_info_bits + b0 * code->k : nullptr;
        a.post = d_post ? d_post + b0 * code->n : nullptr;
        a.iters = d_iters ? d_iters + b0 : nullptr;
        a.ref = d_ref_info ? d_ref_info + b0 * code->k : nullptr;
        const unsigned grid = (unsigned)((a.ncw + g.G - 1) / g.G);
        if (g.lds_state)
            hipLaunchKernelGGL(ldpc_decode_kernel<true>, dim3(grid), dim3(LDPC_THREADS), g.lds_bytes, wf_stream(stream), a);
        else
            hipLaunchKernelGGL(ldpc_decode_kernel<false>, dim3(grid), dim3(LDPC_THREADS), g.lds_bytes, wf_stream(stream), a);
        WF_LAUNCH_CHECK();
        return WF_OK;
    });
}
