// wf_ldpc.h — the code handle, the decoder's launch geometry and the compressed check state shared by the LDPC decoder
// (wf_ldpc.hip) and the iterative-detection form of it (wf_idd.hip).
#pragma once

#include "wf_code.h"

#define LDPC_THREADS 256
#define LDPC_MAX_G 8
#define LDPC_MAX_N 32768
#define LDPC_MAX_DEG 32
#define LDPC_LDS_CAP 65536          // LDS bytes per workgroup the decoder aims for
#define LDPC_LDS_MAX 163840         // ... and what one workgroup may hold at most (n > 16384)

struct wf_ldpc_code {
    int device = 0;
    int32_t n = 0, m = 0, nlayers = 0, n_tx = 0, k = 0, kw = 0, lmax = 0, nedges = 0;
    bool has_gen = false;
    void *d_block = nullptr;        // every int32 table below, one allocation
    uint64_t *d_gen = nullptr;      // (n - k) x kw words, or none (decode-only)
    const int32_t *d_layer = nullptr;     // nlayers x 4: first check, checks, ELL offset, ELL slots
    const int32_t *d_ell = nullptr;       // per layer: slot i of check j at offset + i * checks + j (variable, or -1 past the degree)
    const int32_t *d_check_ptr = nullptr; // m + 1 (checks in layer order)
    const int32_t *d_edge_var = nullptr;  // nedges
    const int32_t *d_var_src = nullptr;   // n: transmitted position of variable v, -1 when punctured
    const int32_t *d_tx_var = nullptr;    // n_tx
    const int32_t *d_info_var = nullptr;  // k
    const int32_t *d_par_var = nullptr;   // n - k: the non-information variables in increasing order
};

struct ldpc_geom {
    int lds_state = 1;      // 1: check state in LDS, 0: in the context's scratch
    int G = 1;
    int64_t groups = 0, grid = 0;
    size_t lds_bytes = 0, scratch_bytes = 0;
};

static ldpc_geom ldpc_geometry(const wf_ctx *ctx, const wf_ldpc_code *c, int64_t ncw)
{
    ldpc_geom g;
    const size_t l_bytes = (size_t)c->n * 4, st_bytes = (size_t)c->m * 16;
    int G = 1;                      // a power of two: the threads of a workgroup split evenly between its codewords
    while (2 * G <= LDPC_MAX_G && 2 * G * std::max(1, c->lmax) <= LDPC_THREADS) G *= 2;
    if (l_bytes + st_bytes <= LDPC_LDS_CAP) {
        while (G > 1 && (size_t)G * (l_bytes + st_bytes) > LDPC_LDS_CAP) G /= 2;
        g.lds_state = 1;
        g.lds_bytes = (size_t)G * (l_bytes + st_bytes);
    } else {
        while (G > 1 && (size_t)G * l_bytes > LDPC_LDS_CAP) G /= 2;
        g.lds_state = 0;
        g.lds_bytes = (size_t)G * l_bytes;
    }
    g.G = G;
    g.groups = (ncw + G - 1) / G;
    // the LDS form launches every group at once (a workgroup that retires early frees its CU for the next); the scratch
    // form runs in launches of as many workgroups as fit on the device at once, whose check states the scratch holds
    const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(8, LDPC_LDS_MAX / (int64_t)std::max<size_t>(g.lds_bytes, 1)));
    g.grid = g.lds_state ? g.groups : std::min<int64_t>(g.groups, (int64_t)std::max(ctx->cus, 1) * per_cu);
    g.scratch_bytes = g.lds_state ? 0 : (size_t)g.grid * G * st_bytes;
    return g;
}

// What the two decoders do before their launches: the geometry, the device, the scratch form's check states (*gstate, else
// null) and room for the dynamic LDS.  fn_lds / fn_scratch: the decoder's kernel in its two forms.
static int ldpc_prepare(wf_ctx *ctx, const wf_ldpc_code *code, int64_t ncw, const void *fn_lds, const void *fn_scratch, ldpc_geom *g, uint4 **gstate)
{
    *g = ldpc_geometry(ctx, code, ncw);
    WF_HIP(hipSetDevice(ctx->device));
    *gstate = nullptr;
    if (!g->lds_state) {
        WF_TRY(wf_ctx_reserve_vit(ctx, (g->scratch_bytes + 7) / 8));
        *gstate = reinterpret_cast<uint4 *>(ctx->d_vit_edge);
    }
    if (g->lds_bytes > LDPC_LDS_CAP - 1024)     // (the kernel's own static LDS comes on top)
        WF_HIP(hipFuncSetAttribute(g->lds_state ? fn_lds : fn_scratch, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g->lds_bytes));
    return WF_OK;
}

// R_e rebuilt bitwise from a check's state {r1, r2, argmin, sign word}
__device__ __forceinline__ float ldpc_msg(const uint4 &st, int i)
{
    const float r = __uint_as_float(i == (int)st.z ? st.y : st.x);
    return (st.w >> i) & 1u ? -r : r;
}
// One check of a layer, by one thread: a pass over the check's edges forms T_e = L_v - R_e and the new compressed state,
// a second pass re-forms the same T_e and writes L_v = T_e + R_e.  ell: the layer's slot-major table (slot i of check j
// at ell[i * checks + j]), `slots` the layer's slot count.
__device__ __forceinline__ void ldpc_update_check(float *Lg, uint4 *sp, const int32_t *ell, int checks, int j, int slots, float alpha)
{
    const uint4 st = *sp;
    float m1 = INFINITY, m2 = INFINITY;
    int e1 = 0, deg = 0;
    uint32_t neg = 0;
    for (int i = 0; i < slots; ++i) {
        const int v = ell[i * checks + j];
        if (v < 0) break;
        const float T = Lg[v] - ldpc_msg(st, i);
        const float mag = fabsf(T);
        if (mag < m1) {
            m2 = m1;
            m1 = mag;
            e1 = i;
        } else if (mag < m2) {
            m2 = mag;
        }
        neg |= (T < 0.0f ? 1u : 0u) << i;
        deg = i + 1;
    }
    const uint32_t S = __popc(neg) & 1u;
    const uint32_t mask = deg == 32 ? 0xFFFFFFFFu : ((1u << deg) - 1u);
    uint4 nst;
    nst.x = __float_as_uint(__fmul_rn(alpha, m1));
    nst.y = __float_as_uint(__fmul_rn(alpha, m2));
    nst.z = (uint32_t)e1;
    nst.w = (S ? ~neg : neg) & mask;
    for (int i = 0; i < deg; ++i) {
        const int v = ell[i * checks + j];
        const float T = Lg[v] - ldpc_msg(st, i);
        Lg[v] = __fadd_rn(T, ldpc_msg(nst, i));
    }
    *sp = nst;
}

// A codeword's share (checks r, r + span, ...) of the syndrome of x̂ = [L < 0]: true when one of them is odd.
__device__ __forceinline__ bool ldpc_syndrome_bad(const float *Lg, const int32_t *check_ptr, const int32_t *edge_var, int m, int r, int span)
{
    uint32_t p = 0;
    for (int c = r; c < m && !p; c += span)
        for (int e = check_ptr[c]; e < check_ptr[c + 1]; ++e) p ^= Lg[edge_var[e]] < 0.0f ? 1u : 0u;
    return p != 0;
}
