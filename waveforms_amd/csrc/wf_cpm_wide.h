// wf_cpm_wide.h — the wave-level helpers of the lane-per-state CPM detectors (wf_cpm_wide.hip: the hard wide form;
// wf_cpm_soft.hip: the max-log-MAP soft output over the full-phase trellis).
#pragma once
#include "wf_common.h"

__device__ __forceinline__ double wide_min_raw(double a, double b)
{
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// all-reduce min over the 64 lanes: row_ror 8, 4, 2, 1 inside each row, then the four row minima through the scalar file
__device__ __forceinline__ double wide_wave_min(double v)
{
    v = wide_min_raw(v, wf_dpp_f64<0x128, 0xf>(v));
    v = wide_min_raw(v, wf_dpp_f64<0x124, 0xf>(v));
    v = wide_min_raw(v, wf_dpp_f64<0x122, 0xf>(v));
    v = wide_min_raw(v, wf_dpp_f64<0x121, 0xf>(v));
    const long long b = __double_as_longlong(v);
    const int lo = (int)b, hi = (int)(b >> 32);
    double q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int l = __builtin_amdgcn_readlane(lo, 16 * k), h = __builtin_amdgcn_readlane(hi, 16 * k);
        q[k] = __longlong_as_double(((long long)h << 32) | (unsigned)l);
    }
    return wide_min_raw(wide_min_raw(q[0], q[1]), wide_min_raw(q[2], q[3]));      // (no NaNs among metrics: min is exact and order-free; fmin would quiet each bit-cast operand first)
}

__device__ __forceinline__ uint64_t wide_bperm_u64(int byte_addr, uint64_t v)
{
    const int lo = __builtin_amdgcn_ds_bpermute(byte_addr, (int)v);
    const int hi = __builtin_amdgcn_ds_bpermute(byte_addr, (int)(v >> 32));
    return ((uint64_t)(unsigned)hi << 32) | (unsigned)lo;
}

__device__ __forceinline__ void wide_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
