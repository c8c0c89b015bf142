// wf_rs.hip — Reed-Solomon codes over GF(2^8): the systematic encoder, the bounded-distance decoder (errors only, or errors and
// erasures) and the rule that declares erasures from the inner decoder's soft output, symbol-interleaved to depth I
// (include/wfhip.h states the field, the code, the frame layout and the decoders' results).  A code is an
// opaque handle whose parameters are validated once on the host; its field tables live in device memory the handle owns.
//
// Both kernels: one workgroup per frame, one wave of 64 lanes per codeword (I waves).  A lane owns the up to four symbols whose
// polynomial degrees are d = lane + 64 q, q = 0 .. 3 (symbol i of a codeword has degree n - 1 - i); the degrees n .. 254 are the
// virtual zero symbols of a shortened code.  With beta = alpha^step the tables by degree are
//   D[d] = beta^d,  W[d] = beta^(fcr d),  XI[d] = beta^(-d),  F[d] = beta^(d (1 - fcr)).
// Decoder, per wave:
//   syndromes   S_j = sum_d r_d beta^((fcr + j) d): the lane's four terms start as r_d W[d] and are multiplied by D[d] from
//               one j to the next; four syndromes are packed into a dword and all-reduced by XOR over the wave, and lane j keeps
//               S_j.  No syndrome set: the message is copied and the wave is done (the cheap path).
//   locator     inversionless Berlekamp-Massey, lane i = coefficient i of Lambda (and of the shifted B and of the syndrome
//               window); the discrepancy is an XOR all-reduce.  L > t: failure.
//   roots       Lambda(beta^(-d)) by Horner at the lane's four degrees, coefficients broadcast from their lanes; a root at a
//               virtual degree, or a root count other than L: failure.
//   values      Omega = S Lambda mod x^L (lane i = Omega_i); e_d = Omega(x) / Lambda'(x) F[d] at x = beta^(-d).
// Errors and erasures (rse_decode_kernel, the same body with ERAS = true): the lane's erased degrees enter the syndromes as 0;
//   the wave collects them by ballot (f of them; f > 2t: failure) and builds Gamma(x) = prod (1 - beta^d x) in lanes, one lane
//   shift and one product per erasure; Berlekamp-Massey then starts from Lambda = B = Gamma, L = f at syndrome f, its length
//   change taken when 2 L <= it + f; the result is the errata locator of degree L <= t + f / 2 <= 2t, still lane = coefficient.
//   Roots and values run on it unchanged; the value at an erased degree IS the symbol.  2 L - f > 2t: failure; status = L - f.
// Marking (rse_mark_kernel): one wave per codeword; rho of a symbol = min |post| over its eight bits, compared as the bit
//   patterns of non-negative floats; f_max rounds of a wave arg-min over the 64-bit key (rho, index).
// Encoder, per wave: the 2t-stage LFSR division, lane j = stage j, one step per message symbol.
// GF(256) products: log / antilog tables in LDS (MUL_TABLES = true: three byte reads and an add) or shift-and-xor in registers
// (false: 8 doublings, about 40 vector instructions).  The library is built with the form RS_MUL_TABLES names, the tables:
// measured on one MI355X on blocks of 2 443 codewords (profiles/rs_multiply_ab.json) the register form takes
// 1.5 times as long where nearly every syndrome is zero and 1.7 times where nearly every codeword is corrected.  The other
// form is a compile-time switch (-DRS_MUL_TABLES=0) kept for that comparison; both compute the same bytes.
#include "wf_code.h"

#include <cstring>

#define RS_MAX_DEPTH 8
#define RS_MAX_T 16
#define RS_TAB_EXP 0          // byte offsets in the handle's table block
#define RS_TAB_LOG 512
#define RS_TAB_D 768
#define RS_TAB_W 1024
#define RS_TAB_XI 1280
#define RS_TAB_F 1536
#define RS_TAB_GEN 1792       // g_0 .. g_{2t-1} (g is monic of degree 2t)
#define RS_TAB_BYTES (1792 + 2 * RS_MAX_T)
#define RS_MAX_GRID (1 << 20)  // frames per launch
#ifndef RS_MUL_TABLES
#define RS_MUL_TABLES 1
#endif

struct wf_rs_code {
    int device = 0;
    int32_t prim = 0, fcr = 0, step = 0, n = 0, k = 0, t = 0, depth = 0;
    uint8_t *d_tab = nullptr;
};

struct rs_args {
    const uint8_t *tab, *in, *ref, *erase;
    uint8_t *out;
    int32_t *status;
    unsigned long long *counts;
    int32_t n, k, t2, depth, bits, wide;
    uint32_t prim;
};

// ---------------------------------------------------------------- the field
template <bool MUL_TABLES>
struct rs_field {
    const uint8_t *sExp, *sLog;
    uint32_t prim;
    // (the register form walks the bits of b: pass the operand that changes from call to call there, a loop-invariant one as a —
    //  the compiler otherwise keeps one lane mask per bit of an invariant b alive across the loop, 16 scalar registers each)
    __device__ __forceinline__ uint32_t mul(uint32_t a, uint32_t b) const
    {
        if constexpr (MUL_TABLES) {
            const uint32_t v = sExp[(uint32_t)sLog[a] + (uint32_t)sLog[b]];
            return a && b ? v : 0u;
        } else {
            uint32_t p = 0;                       // Horner over the bits of b, the remainder by prim taken at every doubling
#pragma unroll
            for (int i = 7; i >= 0; --i) {
                p = (p << 1) ^ ((uint32_t)__builtin_amdgcn_sbfe((int)p, 7, 1) & prim);
                p ^= (uint32_t)__builtin_amdgcn_sbfe((int)b, i, 1) & a;
            }
            return p;
        }
    }
    __device__ __forceinline__ uint32_t inv(uint32_t a) const      // a^254 (a != 0)
    {
        uint32_t sq = mul(a, a), r = sq;                            // a^2
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            sq = mul(sq, sq);
            r = mul(r, sq);
        }
        return r;                                                   // a^(2 + 4 + .. + 128)
    }
};

__device__ __forceinline__ unsigned long long rs_wave_min(unsigned long long v)
{
#pragma unroll
    for (int d = WF_WAVE / 2; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d, WF_WAVE);
        v = o < v ? o : v;
    }
    return v;
}

__device__ __forceinline__ uint32_t rs_wave_xor(uint32_t v)
{
#pragma unroll
    for (int d = WF_WAVE / 2; d >= 1; d >>= 1) v ^= (uint32_t)__shfl_xor((int)v, d, WF_WAVE);
    return v;
}

// One symbol at symbol index `at` of a buffer in the call's bit form: a byte, or eight bytes of 0 / 1, MSB first.
__device__ __forceinline__ uint32_t rs_load(const uint8_t *p, int64_t at, int bits, int wide)
{
    if (!bits) return p[at];
    if (wide) {
        const uint64_t v = *reinterpret_cast<const uint64_t *>(p + 8 * at) & 0x0101010101010101ull;
        return (uint32_t)((v * 0x8040201008040201ull) >> 56);      // byte i (bit 8 i) lands on bit 63 - i; no two terms meet
    }
    uint32_t s = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) s |= (uint32_t)(p[8 * at + b] & 1) << (7 - b);
    return s;
}

__device__ __forceinline__ void rs_store(uint8_t *p, int64_t at, uint32_t s, int bits, int wide)
{
    if (!bits) {
        p[at] = (uint8_t)s;
    } else if (wide) {
        uint64_t v = 0;
#pragma unroll
        for (int b = 0; b < 8; ++b) v |= (uint64_t)((s >> (7 - b)) & 1u) << (8 * b);
        *reinterpret_cast<uint64_t *>(p + 8 * at) = v;
    } else {
#pragma unroll
        for (int b = 0; b < 8; ++b) p[8 * at + b] = (uint8_t)((s >> (7 - b)) & 1u);
    }
}

template <bool MUL_TABLES>
__device__ __forceinline__ rs_field<MUL_TABLES> rs_field_setup(const rs_args &a, uint8_t *sTab)
{
    if constexpr (MUL_TABLES) {                                      // 768 B = 192 dwords (both blocks are 4-byte aligned)
        for (int i = threadIdx.x; i < 192; i += blockDim.x) reinterpret_cast<uint32_t *>(sTab)[i] = reinterpret_cast<const uint32_t *>(a.tab)[i];
    }
    return rs_field<MUL_TABLES>{sTab + RS_TAB_EXP, sTab + RS_TAB_LOG, a.prim};
}

// ---------------------------------------------------------------- encoder
template <bool MUL_TABLES>
__global__ __launch_bounds__(WF_WAVE *RS_MAX_DEPTH) void rs_encode_kernel(rs_args a)
{
    __shared__ __attribute__((aligned(4))) uint8_t sTab[MUL_TABLES ? 768 : 16];      // (not allocated when unused)
    const rs_field<MUL_TABLES> gf = rs_field_setup<MUL_TABLES>(a, sTab);
    __syncthreads();
    const int lane = threadIdx.x & (WF_WAVE - 1), c = threadIdx.x >> 6, I = a.depth, n = a.n, k = a.k, t2 = a.t2;
    const int64_t in0 = (int64_t)blockIdx.x * k * I + c, out0 = (int64_t)blockIdx.x * n * I + c;

    uint32_t m[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = lane + 64 * q;
        m[q] = i < k ? rs_load(a.in, in0 + (int64_t)i * I, a.bits, a.wide) : 0u;
        if (i < k) rs_store(a.out, out0 + (int64_t)i * I, m[q], a.bits, a.wide);
    }
    const uint32_t g = lane < t2 ? a.tab[RS_TAB_GEN + lane] : 0u;
    uint32_t reg = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int cnt = min(64, k - 64 * q);
#pragma unroll 1
        for (int s = 0; s < cnt; ++s) {
            const uint32_t f = (uint32_t)__shfl((int)m[q], s, WF_WAVE) ^ (uint32_t)__shfl((int)reg, t2 - 1, WF_WAVE);
            const uint32_t up = (uint32_t)__shfl_up((int)reg, 1, WF_WAVE);
            reg = (lane ? up : 0u) ^ gf.mul(g, f);
        }
    }
    if (lane < t2) rs_store(a.out, out0 + (int64_t)(k + t2 - 1 - lane) * I, reg, a.bits, a.wide);   // stage 2t - 1 is sent first
}

// ---------------------------------------------------------------- decoder
template <bool MUL_TABLES, bool ERAS>
__device__ __forceinline__ void rs_decode_body(const rs_args &a)
{
    __shared__ __attribute__((aligned(4))) uint8_t sTab[MUL_TABLES ? 768 : 16];      // (not allocated when unused)
    __shared__ int sFrameWrong;
    const rs_field<MUL_TABLES> gf = rs_field_setup<MUL_TABLES>(a, sTab);
    if (threadIdx.x == 0) sFrameWrong = 0;
    __syncthreads();
    const int lane = threadIdx.x & (WF_WAVE - 1), c = threadIdx.x >> 6, I = a.depth, n = a.n, k = a.k, t2 = a.t2, t = t2 >> 1;
    const int64_t in0 = (int64_t)blockIdx.x * n * I + c, msg0 = (int64_t)blockIdx.x * k * I + c;

    // the lane's symbols by degree d = lane + 64 q (0 at the virtual degrees and at d = 255)
    uint32_t r[4], term[4], dk[4];
    uint32_t er = 0;                                                 // ERAS: bit q = the lane's degree lane + 64 q is erased
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int d = lane + 64 * q;
        r[q] = d < n ? rs_load(a.in, in0 + (int64_t)(n - 1 - d) * I, a.bits, a.wide) : 0u;
        if constexpr (ERAS) er |= (d < n && a.erase[in0 + (int64_t)(n - 1 - d) * I] ? 1u : 0u) << q;
        dk[q] = a.tab[RS_TAB_D + (d & 255)];
        term[q] = gf.mul(a.tab[RS_TAB_W + (d & 255)], (er >> q) & 1u ? 0u : r[q]);
    }
    unsigned long long em[4] = {0, 0, 0, 0};                         // ERAS: the wave's erased degrees, f of them
    int f = 0;
    if constexpr (ERAS) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            em[q] = __ballot((er >> q) & 1u);
            f += __popcll(em[q]);
        }
    }

    // syndromes, four to a dword; lane j keeps S_j
    uint32_t S = 0;
#pragma unroll 1
    for (int j0 = 0; j0 < t2; j0 += 4) {
        uint32_t pk = 0;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            pk |= (term[0] ^ term[1] ^ term[2] ^ term[3]) << (8 * jj);
#pragma unroll
            for (int q = 0; q < 4; ++q) term[q] = gf.mul(dk[q], term[q]);
        }
        pk = rs_wave_xor(pk);
        if ((lane >> 2) == (j0 >> 2)) S = (pk >> (8 * (lane & 3))) & 255u;
    }
    if (lane >= t2) S = 0;

    int status = 0;
    if (ERAS && f > t2) {
        status = -1;
    } else if (__ballot(S != 0) != 0) {
        // inversionless Berlekamp-Massey: Lambda <- b Lambda - delta x^m B; lane i holds coefficient i
        uint32_t lam = lane == 0 ? 1u : 0u, win = 0, b = 1;
        if constexpr (ERAS) {
            // Lambda = Gamma = prod over the erased degrees of (1 - beta^d x); the window as f iterations would have left it
#pragma unroll
            for (int q = 0; q < 4; ++q) {
#pragma unroll 1
                for (unsigned long long m = em[q]; m; m &= m - 1) {
                    const uint32_t X = (uint32_t)__shfl((int)dk[q], __builtin_ctzll(m), WF_WAVE), up = (uint32_t)__shfl_up((int)lam, 1, WF_WAVE);
                    lam ^= gf.mul(X, lane ? up : 0u);
                }
            }
            const uint32_t sw = (uint32_t)__shfl((int)S, (f - 1 - lane) & (WF_WAVE - 1), WF_WAVE);
            win = lane < f ? sw : 0u;                                // lane i: S_{f - 1 - i}
        }
        uint32_t B = lam;
        int L = f;
#pragma unroll 1
        for (int it = f; it < t2; ++it) {
            const uint32_t Bu = (uint32_t)__shfl_up((int)B, 1, WF_WAVE), wu = (uint32_t)__shfl_up((int)win, 1, WF_WAVE);
            const uint32_t sr = (uint32_t)__shfl((int)S, it, WF_WAVE);
            B = lane ? Bu : 0u;
            win = lane ? wu : sr;                                    // lane i: S_{it - i}
            const uint32_t delta = rs_wave_xor(gf.mul(lam, win));
            if (delta) {
                const uint32_t nl = gf.mul(b, lam) ^ gf.mul(delta, B);
                if (2 * L <= it + f) {
                    B = lam;
                    L = it + 1 + f - L;
                    b = delta;
                }
                lam = nl;
            }
        }
        status = ERAS ? (2 * L - f <= t2 ? L - f : -1) : (L <= t ? L : -1);      // (L = errors + erasures)
        if (ERAS ? status >= 0 : status > 0) {
            // Omega_i = sum_{j <= i} Lambda_j S_{i - j}, i < L
            uint32_t om = 0;
#pragma unroll 1
            for (int j = 0; j <= L; ++j) {
                const uint32_t lj = (uint32_t)__shfl((int)lam, j, WF_WAVE), sj = (uint32_t)__shfl_up((int)S, (unsigned)j, WF_WAVE);
                om ^= gf.mul(lj, lane >= j ? sj : 0u);
            }
            if (lane >= L) om = 0;
            // Lambda, Lambda' and Omega at x = beta^(-d) for the lane's four degrees
            uint32_t x[4], x2[4], vl[4] = {0, 0, 0, 0}, vd[4] = {0, 0, 0, 0}, vo[4] = {0, 0, 0, 0};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                x[q] = a.tab[RS_TAB_XI + ((lane + 64 * q) & 255)];
                x2[q] = gf.mul(x[q], x[q]);
            }
#pragma unroll 1
            for (int i = ERAS ? L : t; i >= 0; --i) {
                const uint32_t li = (uint32_t)__shfl((int)lam, i, WF_WAVE), oi = (uint32_t)__shfl((int)om, i, WF_WAVE);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    vl[q] = gf.mul(x[q], vl[q]) ^ li;
                    vo[q] = gf.mul(x[q], vo[q]) ^ oi;
                    if (i & 1) vd[q] = gf.mul(x2[q], vd[q]) ^ li;   // Lambda'(x) = sum over odd i of Lambda_i (x^2)^((i - 1) / 2)
                }
            }
            int roots = 0;
            bool virt = false;
            uint32_t e[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int d = lane + 64 * q;
                const bool root = d < 255 && vl[q] == 0;
                roots += __popcll(__ballot(root));
                virt = virt || (root && d >= n);
                e[q] = root && vd[q] ? gf.mul(gf.mul(vo[q], gf.inv(vd[q])), a.tab[RS_TAB_F + (d & 255)]) : 0u;
            }
            if (roots != L || __ballot(virt) != 0) {
                status = -1;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) r[q] = ((er >> q) & 1u ? 0u : r[q]) ^ e[q];
            }
        }
    } else if constexpr (ERAS) {                                     // zero syndromes: r with 0 at the erased degrees is the codeword
#pragma unroll
        for (int q = 0; q < 4; ++q) r[q] = (er >> q) & 1u ? 0u : r[q];
    }

    // the message (the received one on a failure), the status and the counts
    int diff = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int d = lane + 64 * q;
        if (d >= t2 && d < n) {
            const int64_t at = msg0 + (int64_t)(n - 1 - d) * I;
            rs_store(a.out, at, r[q], a.bits, a.wide);
            if (a.ref) diff += __popc(r[q] ^ rs_load(a.ref, at, a.bits, a.wide));
        }
    }
    if (a.status && lane == 0) a.status[(int64_t)blockIdx.x * I + c] = status;
    if (a.ref) {
        diff = (int)wf_wave_sum_i64(diff);
        if (lane == 0) {
            if (diff) {
                atomicAdd(a.counts + 0, (unsigned long long)diff);
                atomicAdd(a.counts + 1, 1ull);
                if (atomicExch(&sFrameWrong, 1) == 0) atomicAdd(a.counts + 4, 1ull);
            }
            if (status < 0) atomicAdd(a.counts + 2, 1ull);
            if (status > 0) atomicAdd(a.counts + 3, (unsigned long long)status);
            if (ERAS && status >= 0 && f > 0) atomicAdd(a.counts + 5, (unsigned long long)f);
        }
    }
}

template <bool MUL_TABLES>
__global__ __launch_bounds__(WF_WAVE *RS_MAX_DEPTH) void rs_decode_kernel(rs_args a)
{
    rs_decode_body<MUL_TABLES, false>(a);
}

template <bool MUL_TABLES>
__global__ __launch_bounds__(WF_WAVE *RS_MAX_DEPTH) void rse_decode_kernel(rs_args a)
{
    rs_decode_body<MUL_TABLES, true>(a);
}

// ---------------------------------------------------------------- erasure marking
struct rs_mark_args {
    const uint32_t *post;      // float32 bit patterns, bit form: eight per symbol
    uint8_t *erase;
    int32_t n, depth, f_max;
    uint32_t below;            // the bit pattern of `below` (0 when below <= 0: nothing is under it)
};

__global__ __launch_bounds__(WF_WAVE *RS_MAX_DEPTH) void rse_mark_kernel(rs_mark_args a)
{
    const int lane = threadIdx.x & (WF_WAVE - 1), c = threadIdx.x >> 6, I = a.depth, n = a.n;
    const int64_t sym0 = (int64_t)blockIdx.x * n * I + c;
    // rho of the lane's symbols i = lane + 64 q, as the bit pattern of a non-negative float (ordered like the value); ~0: no candidate
    uint32_t rho[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = lane + 64 * q;
        rho[q] = ~0u;
        if (i < n) {
            const uint32_t *p = a.post + 8 * (sym0 + (int64_t)i * I);
            uint32_t m = p[0] & 0x7fffffffu;
#pragma unroll
            for (int b = 1; b < 8; ++b) m = min(m, p[b] & 0x7fffffffu);
            rho[q] = m < a.below ? m : ~0u;
        }
    }
    uint32_t marked = 0;
#pragma unroll 1
    for (int round = 0; round < a.f_max; ++round) {
        unsigned long long key = ~0ull;                              // (rho, index): the smaller index wins a tie
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned long long kq = ((unsigned long long)rho[q] << 32) | (uint32_t)(lane + 64 * q);
            key = rho[q] != ~0u && kq < key ? kq : key;
        }
        const unsigned long long best = rs_wave_min(key);
        if (best == ~0ull) break;                                    // (wave-uniform)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if ((uint32_t)best == (uint32_t)(lane + 64 * q)) {
                marked |= 1u << q;
                rho[q] = ~0u;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = lane + 64 * q;
        if (i < n) a.erase[sym0 + (int64_t)i * I] = (uint8_t)((marked >> q) & 1u);
    }
}

// ---------------------------------------------------------------- host
static int rs_gcd(int a, int b) { return b ? rs_gcd(b, a % b) : a; }

extern "C" int wf_rs_code_create(wf_ctx *ctx, int32_t prim, int32_t fcr, int32_t step, int32_t n, int32_t k, int32_t depth, wf_rs_code **out)
{
    WF_REQUIRE(ctx && out, "wf_rs_code_create: NULL argument");
    *out = nullptr;
    WF_REQUIRE(prim >= 0x100 && prim < 0x200, "wf_rs_code_create: prim = 0x%x is not a polynomial of degree 8", prim);
    WF_REQUIRE(n >= 3 && n <= 255, "wf_rs_code_create: n = %d outside 3 .. 255", n);
    WF_REQUIRE(k >= 1 && k < n && (n - k) % 2 == 0 && (n - k) / 2 <= RS_MAX_T, "wf_rs_code_create: n - k = %d must be 2 t with t = 1 .. %d, k >= 1", n - k,
               RS_MAX_T);
    WF_REQUIRE(depth >= 1 && depth <= RS_MAX_DEPTH, "wf_rs_code_create: depth = %d outside 1 .. %d", depth, RS_MAX_DEPTH);
    WF_REQUIRE(fcr >= 0 && fcr <= 254, "wf_rs_code_create: fcr = %d outside 0 .. 254", fcr);
    WF_REQUIRE(step >= 1 && step <= 254 && rs_gcd(step, 255) == 1, "wf_rs_code_create: step = %d must be 1 .. 254 and prime to 255", step);
    std::vector<uint8_t> tab(RS_TAB_BYTES, 0);
    uint8_t *ex = tab.data() + RS_TAB_EXP, *lg = tab.data() + RS_TAB_LOG;
    uint32_t v = 1;
    int period = 0;
    for (int i = 0; i < 255; ++i) {                      // the powers of x: prim is primitive when they are 255 different elements
        ex[i] = (uint8_t)v;
        lg[v] = (uint8_t)i;
        v <<= 1;
        if (v & 0x100) v ^= (uint32_t)prim;
        if (v == 1 && !period) period = i + 1;
    }
    WF_REQUIRE(period == 255, "wf_rs_code_create: prim = 0x%x is not primitive (x has period %d)", prim, period);
    for (int i = 255; i < 512; ++i) ex[i] = ex[i - 255];
    lg[0] = 0;                                          // (never used: a product with 0 is selected to 0)
    const int t2 = n - k;
    for (int d = 0; d < 256; ++d) {
        const int sd = step * d % 255;
        tab[RS_TAB_D + d] = ex[sd];
        tab[RS_TAB_W + d] = ex[sd * fcr % 255];
        tab[RS_TAB_XI + d] = ex[(255 - sd) % 255];
        tab[RS_TAB_F + d] = ex[sd * ((256 - fcr) % 255) % 255];
    }
    auto mul = [&](uint32_t a, uint32_t b) -> uint32_t { return a && b ? ex[lg[a] + lg[b]] : 0u; };
    std::vector<uint32_t> g(t2 + 1, 0);                  // g(x) = prod (x - beta^(fcr + i)), g[j] = coefficient of x^j
    g[0] = 1;
    for (int i = 0; i < t2; ++i) {
        const uint32_t root = ex[step * (fcr + i) % 255];
        for (int j = i + 1; j >= 1; --j) g[j] = g[j - 1] ^ mul(g[j], root);
        g[0] = mul(g[0], root);
    }
    for (int j = 0; j < t2; ++j) tab[RS_TAB_GEN + j] = (uint8_t)g[j];

    void *d_tab;
    WF_TRY(wf_code_upload("wf_rs_code_create", ctx->device, tab.data(), tab.size(), &d_tab));
    wf_rs_code *c = new wf_rs_code();
    c->device = ctx->device, c->d_tab = static_cast<uint8_t *>(d_tab);
    c->prim = prim, c->fcr = fcr, c->step = step, c->n = n, c->k = k, c->t = t2 / 2, c->depth = depth;
    *out = c;
    return WF_OK;
}

extern "C" int wf_rs_code_free(wf_rs_code *code)
{
    if (!code) return WF_OK;
    const int rc = wf_code_release("wf_rs_code_free", code->device, {code->d_tab});
    delete code;                          // (whatever hipFree said: the host struct never outlives the call)
    return rc;
}

static rs_args rs_make_args(const wf_rs_code *code, int bits, const void *in, const void *out, const void *ref)
{
    rs_args a;
    a.tab = code->d_tab;
    a.in = a.ref = a.erase = nullptr, a.out = nullptr, a.status = nullptr, a.counts = nullptr;
    a.n = code->n, a.k = code->k, a.t2 = 2 * code->t, a.depth = code->depth, a.bits = bits, a.prim = (uint32_t)code->prim;
    a.wide = bits && ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(ref)) & 7) == 0;
    return a;
}

extern "C" int wf_rs_encode(wf_ctx *ctx, const wf_rs_code *code, const uint8_t *d_msg, int64_t nframes, int32_t bits, uint8_t *d_tx, void *stream)
{
    WF_REQUIRE(ctx && code && d_msg && d_tx, "wf_rs_encode: NULL argument");
    WF_REQUIRE(nframes >= 1, "wf_rs_encode: nframes must be at least 1");
    WF_REQUIRE(bits == 0 || bits == 1, "wf_rs_encode: bits = %d outside {0, 1}", bits);
    WF_REQUIRE_SAME_DEVICE("wf_rs_encode", code, ctx);
    WF_HIP(hipSetDevice(ctx->device));
    rs_args a = rs_make_args(code, bits, d_msg, d_tx, nullptr);
    const int64_t sym = bits ? 8 : 1, in_frame = sym * code->k * code->depth, out_frame = sym * code->n * code->depth;
    return wf_for_slices(nframes, RS_MAX_GRID, [&](int64_t f0, int64_t count) -> int {
        a.in = d_msg + f0 * in_frame;
        a.out = d_tx + f0 * out_frame;
        hipLaunchKernelGGL(rs_encode_kernel<RS_MUL_TABLES != 0>, dim3((unsigned)count), dim3(WF_WAVE * code->depth), 0, wf_stream(stream), a);
        WF_LAUNCH_CHECK();
        return WF_OK;
    });
}

extern "C" int wf_rs_decode_geometry(wf_ctx *ctx, const wf_rs_code *code, int64_t nframes, int64_t *h_geom)
{
    WF_REQUIRE(ctx && code && h_geom && nframes >= 1, "wf_rs_decode_geometry: bad argument");
    h_geom[0] = code->depth;                                             // waves (codewords) per workgroup
    h_geom[1] = nframes;                                                 // workgroups
    h_geom[2] = (nframes + RS_MAX_GRID - 1) / RS_MAX_GRID;               // launches
    h_geom[3] = RS_MUL_TABLES ? 768 + 4 : 4;                             // LDS bytes per workgroup: the tables and the frame's flag
    h_geom[4] = WF_WAVE * code->depth;                                   // threads per workgroup
    return WF_OK;
}

// wf_rs_decode (eras = false: d_erase is null and stays unread) and wf_rs_decode_erasures (eras = true)
static int rs_decode_call(const char *fn, bool eras, wf_ctx *ctx, const wf_rs_code *code, const uint8_t *d_rx, const uint8_t *d_erase, int64_t nframes,
                          int32_t bits, uint8_t *d_msg_out, int32_t *d_status, const uint8_t *d_ref_msg, int64_t *d_counts, void *stream)
{
    WF_REQUIRE(ctx && code && d_rx && (d_erase || !eras) && d_msg_out, "%s: NULL argument", fn);
    WF_REQUIRE(nframes >= 1, "%s: nframes must be at least 1", fn);
    WF_REQUIRE(bits == 0 || bits == 1, "%s: bits = %d outside {0, 1}", fn, bits);
    WF_REQUIRE(!d_ref_msg || d_counts, "%s: d_ref_msg needs d_counts", fn);
    WF_REQUIRE(wf_aligned(d_counts, 8) && wf_aligned(d_status, 4), "%s: counts must be 8-byte, status 4-byte aligned", fn);
    WF_REQUIRE_SAME_DEVICE(fn, code, ctx);
    WF_HIP(hipSetDevice(ctx->device));
    rs_args a = rs_make_args(code, bits, d_rx, d_msg_out, d_ref_msg);
    a.counts = reinterpret_cast<unsigned long long *>(d_counts);
    const int64_t sym = bits ? 8 : 1, in_frame = sym * code->n * code->depth, msg_frame = sym * code->k * code->depth;
    return wf_for_slices(nframes, RS_MAX_GRID, [&](int64_t f0, int64_t count) -> int {
        a.in = d_rx + f0 * in_frame;
        a.erase = eras ? d_erase + f0 * code->n * code->depth : nullptr;
        a.out = d_msg_out + f0 * msg_frame;
        a.ref = d_ref_msg ? d_ref_msg + f0 * msg_frame : nullptr;
        a.status = d_status ? d_status + f0 * code->depth : nullptr;
        const dim3 grid((unsigned)count), block(WF_WAVE * code->depth);
        if (!eras) hipLaunchKernelGGL(rs_decode_kernel<RS_MUL_TABLES != 0>, grid, block, 0, wf_stream(stream), a);
        else hipLaunchKernelGGL(rse_decode_kernel<RS_MUL_TABLES != 0>, grid, block, 0, wf_stream(stream), a);
        WF_LAUNCH_CHECK();
        return WF_OK;
    });
}

extern "C" int wf_rs_decode(wf_ctx *ctx, const wf_rs_code *code, const uint8_t *d_rx, int64_t nframes, int32_t bits, uint8_t *d_msg_out,
                            int32_t *d_status, const uint8_t *d_ref_msg, int64_t *d_counts, void *stream)
{
    return rs_decode_call("wf_rs_decode", false, ctx, code, d_rx, nullptr, nframes, bits, d_msg_out, d_status, d_ref_msg, d_counts, stream);
}

extern "C" int wf_rs_decode_erasures(wf_ctx *ctx, const wf_rs_code *code, const uint8_t *d_rx, const uint8_t *d_erase, int64_t nframes, int32_t bits,
                                     uint8_t *d_msg_out, int32_t *d_status, const uint8_t *d_ref_msg, int64_t *d_counts, void *stream)
{
    return rs_decode_call("wf_rs_decode_erasures", true, ctx, code, d_rx, d_erase, nframes, bits, d_msg_out, d_status, d_ref_msg, d_counts, stream);
}

extern "C" int wf_rs_mark_erasures(wf_ctx *ctx, const wf_rs_code *code, const float *d_post, int64_t nframes, int32_t f_max, float below,
                                   uint8_t *d_erase, void *stream)
{
    WF_REQUIRE(ctx && code && d_post && d_erase, "wf_rs_mark_erasures: NULL argument");
    WF_REQUIRE(nframes >= 1, "wf_rs_mark_erasures: nframes must be at least 1");
    WF_REQUIRE(f_max >= 0 && f_max <= 2 * code->t, "wf_rs_mark_erasures: f_max = %d outside 0 .. 2t = %d", f_max, 2 * code->t);
    WF_REQUIRE(std::isfinite(below), "wf_rs_mark_erasures: below must be finite");
    WF_REQUIRE(wf_aligned(d_post, 4), "wf_rs_mark_erasures: d_post must be 4-byte aligned");
    WF_REQUIRE_SAME_DEVICE("wf_rs_mark_erasures", code, ctx);
    WF_HIP(hipSetDevice(ctx->device));
    rs_mark_args a;
    a.n = code->n, a.depth = code->depth, a.f_max = f_max;
    a.below = 0;
    if (below > 0.0f) std::memcpy(&a.below, &below, 4);
    const int64_t frame = (int64_t)code->n * code->depth;
    return wf_for_slices(nframes, RS_MAX_GRID, [&](int64_t f0, int64_t count) -> int {
        a.post = reinterpret_cast<const uint32_t *>(d_post) + 8 * f0 * frame;
        a.erase = d_erase + f0 * frame;
        hipLaunchKernelGGL(rse_mark_kernel, dim3((unsigned)count), dim3(WF_WAVE * code->depth), 0, wf_stream(stream), a);
        WF_LAUNCH_CHECK();
        return WF_OK;
    });
}
