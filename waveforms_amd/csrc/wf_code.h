// wf_code.h — the host plumbing every code family repeats (wf_ldpc.hip + wf_idd.hip, wf_conv.hip, wf_turbo.hip, wf_rs.hip), each
// piece stated once: a handle's tables into device memory and out of it again, the transmit table, the argument predicates of
// the entry points and the loop that cuts a call into launches.  Host code only.  `fn` is the entry point's name: every message
// starts with it.
#pragma once
#include "wf_common.h"

#include <algorithm>
#include <cmath>
#include <initializer_list>

#define WF_TRY(call)             \
    do {                         \
        const int rc_ = (call);  \
        if (rc_) return rc_;     \
    } while (0)

// `bytes` of host tables into fresh memory of `device`.  On failure nothing stays allocated and *d_ptr is null.
static int wf_code_upload(const char *fn, int device, const void *host, size_t bytes, void **d_ptr)
{
    *d_ptr = nullptr;
    const char *what = "hipSetDevice";
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) what = "hipMalloc", e = hipMalloc(d_ptr, bytes);
    if (e == hipSuccess) what = "hipMemcpy", e = hipMemcpy(*d_ptr, host, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) return WF_OK;
    wf_set_error("%s: %s failed: %s", fn, what, hipGetErrorString(e));
    if (*d_ptr) (void)hipFree(*d_ptr);
    *d_ptr = nullptr;
    return WF_ERR_HIP;
}

// Frees every pointer that is not null, then reports the first failure.  The caller deletes its host struct whatever this
// returns: the struct never outlives the call.
static int wf_code_release(const char *fn, int device, std::initializer_list<void *> d_ptrs)
{
    (void)hipSetDevice(device);
    hipError_t first = hipSuccess;
    for (void *p : d_ptrs) {
        const hipError_t e = p ? hipFree(p) : hipSuccess;
        if (first == hipSuccess) first = e;
    }
    if (first == hipSuccess) return WF_OK;
    wf_set_error("%s: hipFree failed: %s", fn, hipGetErrorString(first));
    return WF_ERR_HIP;
}

// tx_var (n_tx variables of a code of N) -> var_src (N entries, -1 on entry: the transmitted position of a variable, -1 left
// where it is punctured) and, where asked for, a copy of tx_var.
static int wf_tx_table(const char *fn, const int32_t *h_tx_var, int32_t n_tx, int32_t N, int32_t *var_src, int32_t *tx_var)
{
    for (int t = 0; t < n_tx; ++t) {
        const int v = h_tx_var[t];
        WF_REQUIRE(v >= 0 && v < N, "%s: tx_var[%d] = %d outside the code", fn, t, v);
        WF_REQUIRE(var_src[v] < 0, "%s: variable %d is transmitted twice", fn, v);
        var_src[v] = t;
        if (tx_var) tx_var[t] = v;
    }
    return WF_OK;
}

// a K-bit mask with bit K - 1 and bit 0 set
static inline bool wf_tap_mask_ok(uint32_t mask, int K) { return mask < (1u << K) && ((mask >> (K - 1)) & 1u) && (mask & 1u); }

static inline bool wf_aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }   // (null is)
template <class T>
static inline bool wf_finite_pos(T x) { return std::isfinite(x) && x > 0; }

#define WF_REQUIRE_SAME_DEVICE(fn, code, ctx) \
    WF_REQUIRE((code)->device == (ctx)->device, "%s: the code lives on device %d, the context on %d", fn, (code)->device, (ctx)->device)

// A call of `total` items in launches of at most `per_launch`: launch(first, count) -> WF_OK or an error, which ends the call.
template <class F>
static int wf_for_slices(int64_t total, int64_t per_launch, F &&launch)
{
    for (int64_t first = 0; first < total; first += per_launch) WF_TRY(launch(first, std::min(per_launch, total - first)));
    return WF_OK;
}
