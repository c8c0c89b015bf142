// wf_conv_common.h — device helpers of the trellis decoders whose lanes are states (wf_conv.hip: feed-forward convolutional
// codes; wf_turbo.hip: recursive systematic constituents of a turbo code): a branch's gamma, the masked -INFINITY selects and
// the all-reduce over the S lanes of a codeword; and the launch geometry the two share on the host.
#pragma once
#include "wf_code.h"

#define CONV_MAX_N 32768
#define CONV_C 32                   // checkpoint spacing = steps per segment
#define CONV_SCRATCH_CAP (128ll << 20)   // scratch bytes one launch may use

// A wave decodes G = 64 / 2^nu codewords in lockstep, in segments of CONV_C of their T steps; one launch takes as many waves as
// the device holds at once and as the scratch cap has room for at per_wave bytes each: a 256-byte checkpoint row per segment
// plus `more_per_wave`.
struct wf_wave_geom {
    int G = 1, nseg = 0;
    int64_t waves = 0, per_launch = 0, per_wave = 0;
};

static wf_wave_geom wf_wave_geometry(const wf_ctx *ctx, int nu, int T, int64_t ncw, int64_t more_per_wave)
{
    wf_wave_geom g;
    g.G = 64 >> nu;
    g.waves = (ncw + g.G - 1) / g.G;
    g.nseg = (T + CONV_C - 1) / CONV_C;
    g.per_wave = (int64_t)g.nseg * 64 * 4 + more_per_wave;
    g.per_launch = std::max<int64_t>(1, std::min<int64_t>(g.waves, std::min<int64_t>((int64_t)std::max(ctx->cus, 1) * 64, CONV_SCRATCH_CAP / g.per_wave)));
    return g;
}

#ifdef __HIPCC__
// gamma of one branch: start (u ? -A : +0), then minus L_j where the branch's code bit j is 1, j increasing.  (x - (+0) is x
// for every x, -0 included, so +0 stands for "no subtraction".)  c[j]: all ones where the code bit is 1, else 0: L_j & c[j] is
// L_j or +0 in one instruction, and the branch's bits live in vector registers instead of one lane mask each.
template <int NOUT>
__device__ __forceinline__ float conv_gamma(float start, const float (&L)[NOUT], const uint32_t (&c)[NOUT])
{
    float g = start;
#pragma unroll
    for (int j = 0; j < NOUT; ++j) g = __fsub_rn(g, __uint_as_float(__float_as_uint(L[j]) & c[j]));
    return g;
}

// c ? -INFINITY : v and c ? v : -INFINITY for a mask c of all ones / all zeros (one v_bfi_b32 each)
__device__ __forceinline__ float conv_drop_if(uint32_t c, float v) { return __uint_as_float((c & 0xFF800000u) | (~c & __float_as_uint(v))); }
__device__ __forceinline__ float conv_keep_if(uint32_t c, float v) { return __uint_as_float((c & __float_as_uint(v)) | (~c & 0xFF800000u)); }

template <int CTRL>
__device__ __forceinline__ float conv_dpp(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}

// max over the S lanes of a codeword, in every one of them (the operands are never -0 and never NaN: the order is free)
template <int S>
__device__ __forceinline__ float conv_group_max(float v)
{
    if constexpr (S >= 2) v = fmaxf(v, conv_dpp<0xB1>(v));         // quad_perm [1, 0, 3, 2]
    if constexpr (S >= 4) v = fmaxf(v, conv_dpp<0x4E>(v));         // quad_perm [2, 3, 0, 1]
    if constexpr (S >= 8) v = fmaxf(v, conv_dpp<0x141>(v));        // row_half_mirror: the other quad of the 8
    if constexpr (S >= 16) v = fmaxf(v, conv_dpp<0x140>(v));       // row_mirror: the other 8 of the row
    if constexpr (S >= 32) v = fmaxf(v, __shfl_xor(v, 16, WF_WAVE));
    if constexpr (S >= 64) v = fmaxf(v, __shfl_xor(v, 32, WF_WAVE));
    return v;
}
#endif
