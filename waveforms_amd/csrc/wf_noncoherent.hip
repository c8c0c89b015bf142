// wf_noncoherent.hip — the multi-symbol noncoherent soft detector for PCM/FM (Osborne and Luntz): per bit, N symbols of samples
// against all 2^N hypotheses, magnitudes compared (wf_noncoherent_soft_c128).  include/wfhip.h states the definition;
// waveforms_amd/viterbi/noncoherent.py restates it in numpy.  The reference has no such detector: this is the build's own.
//
// The work is a complex product  Z[p][j] = Σ_k conj(T[p][k]) r[w_j + k]  of the 2^N x K table (K = N sps) with a Toeplitz
// operand: the windows of consecutive bits are sps samples apart.  It runs on the fp64 matrix cores as four real
// v_mfma_f64_16x16x4_f64 products per 16 hypotheses x 16 bits x 4 samples:
//     P = Σ c x,  Q = Σ s y,  R = Σ c y,  U = Σ s x   (T = c + j s, r = x + j y)   ->   Z = (P + Q) + j (R - U).
// Operand layout (MI355X_MICROARCH.md): A[i][k] in lane i + 16 k, B[k][j] in lane j + 16 k, D[i][j] in lane j + 16 (i & 3),
// register i >> 2.  A = the table (row i = hypothesis), B = the samples (column j = bit).
//
//   noncoherent_kernel<N, SPS>   one workgroup of 4 waves per tile of NC_TILE consecutive bits (grid-strided).
//       Table: a wave keeps its share of the table in REGISTERS for the whole launch, one double2 per lane, 16 hypotheses and
//       k-step: the 2^N / 16 blocks of 16 hypotheses are dealt to the waves (N = 7: two blocks a wave, N = 5: one block, two
//       waves each, N = 3: the 8 hypotheses and 8 zero rows in every wave) — the 115 KB of N = 7 never have to sit in LDS, and
//       are read from memory once per workgroup, not once per bit.
//       Samples: the tile's (NC_TILE + N - 1) sps samples go to LDS once, with coalesced 16-byte loads, NC_BATCH in flight per
//       lane; a sample outside [0, n) is stored as zero, which is the definition's edge.  One slot of padding after every sps
//       samples: the 16 lanes of a k-row read sps samples apart, sps + 1 slots is odd for every even sps.
//       Product: per group of 16 bits and k-step ONE ds_read_b128 per lane feeds 4 MFMAs per block of hypotheses.
//       Maxima: |Z| = sqrt(re² + im²) per hypothesis, the maximum per class (bit c of p) in registers over the wave's blocks,
//       across the four k-rows by two shuffles, then through LDS across the waves that share a bit; thread t writes bit t.
//   The sums are re-associated (four chains in the matrix cores' order, joined at the end): the result agrees with the host
//   statement to rounding, within 2 · 8 (K + 8) 2⁻⁵³ Σ|r| per bit (tests/test_noncoherent_gpu.py), not bit for bit.
#include "wf_common.h"

#include <cmath>

#define NC_THREADS 256
#define NC_TILE 256                                          // bits per workgroup and tile
#define NC_BATCH 8                                           // staged loads in flight per lane
#define NC_MAX_LDS (160 * 1024)
#define NC_MAX_BLOCKS_PER_CU 4

typedef double nc_d4 __attribute__((ext_vector_type(4)));

template <int N, int SPS>
struct nc_geom {
    static constexpr int K = N * SPS, KS = (K + 3) / 4, NH = 1 << N, C = (N - 1) / 2;
    static constexpr int NPB = NH >= 16 ? NH / 16 : 1;       // blocks of 16 hypotheses
    static constexpr int PW = NPB < 4 ? NPB : 4;             // waves that split the blocks,
    static constexpr int PBW = NPB / PW;                     // blocks per wave,
    static constexpr int BW = 4 / PW;                        // and waves that split a tile's groups of 16 bits
    static constexpr int COUNT = (NC_TILE + N - 1) * SPS;    // samples of a tile
    static constexpr int SLOTS = COUNT + COUNT / SPS + 1;    // ... padded
    static constexpr size_t LDS = (size_t)SLOTS * sizeof(double2) + (size_t)PW * NC_TILE * 2 * sizeof(double);
};

template <int N, int SPS>
__global__ __launch_bounds__(NC_THREADS) void noncoherent_kernel(const double2 *__restrict__ r, int64_t n, const double2 *__restrict__ T, int64_t start,
                                                                 int64_t nbits, double *__restrict__ llr, uint8_t *__restrict__ bits)
{
    using G = nc_geom<N, SPS>;
    extern __shared__ __attribute__((aligned(16))) double2 s_x[];
    double *s_max = reinterpret_cast<double *>(s_x + G::SLOTS);      // [PW][NC_TILE][2]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int i = lane & 15, kq = lane >> 4;
    const int pgroup = wave % G::PW, bgroup = wave / G::PW;

    // this wave's share of the table: row p of block pb, component 4 ks + kq (zero rows past 2^N, zero components past K)
    double2 a[G::PBW][G::KS];
#pragma unroll
    for (int pb = 0; pb < G::PBW; ++pb) {
        const int p = (pgroup * G::PBW + pb) * 16 + i;
#pragma unroll
        for (int ks = 0; ks < G::KS; ++ks) {
            const int k = 4 * ks + kq;
            a[pb][ks] = (p < G::NH && k < G::K) ? T[(size_t)p * G::K + k] : make_double2(0.0, 0.0);
        }
    }

    const int64_t ntiles = (nbits + NC_TILE - 1) / NC_TILE;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t base = start + (tile * NC_TILE - G::C) * SPS;  // the first sample of the tile's first window
        __syncthreads();                                             // the tile before has been read (samples and maxima)
        for (int k0 = t; k0 < G::COUNT; k0 += NC_BATCH * NC_THREADS) {
            double2 v[NC_BATCH];
#pragma unroll
            for (int u = 0; u < NC_BATCH; ++u) {
                const int k = k0 + u * NC_THREADS;
                const int64_t g = base + k;
                v[u] = (k < G::COUNT && g >= 0 && g < n) ? r[g] : make_double2(0.0, 0.0);
            }
#pragma unroll
            for (int u = 0; u < NC_BATCH; ++u) {
                const int k = k0 + u * NC_THREADS;
                if (k < G::COUNT) s_x[k + k / SPS] = v[u];           // k + k / SPS <= SLOTS - 2
            }
        }
        __syncthreads();
#pragma unroll 1
        for (int grp = bgroup; grp < NC_TILE / 16; grp += G::BW) {
            const int jb = grp * 16 + i;                             // the tile's bit in this lane's column: its window begins at sample jb SPS
            const double2 *xs = s_x + jb * (SPS + 1);
            nc_d4 P[G::PBW], Q[G::PBW], R[G::PBW], U[G::PBW];
#pragma unroll
            for (int pb = 0; pb < G::PBW; ++pb) P[pb] = Q[pb] = R[pb] = U[pb] = nc_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int ks = 0; ks < G::KS; ++ks) {
                const int k = 4 * ks + kq;                           // jb SPS + k <= COUNT - 1 for k < K
                const double2 x = k < G::K ? xs[k + k / SPS] : make_double2(0.0, 0.0);
#pragma unroll
                for (int pb = 0; pb < G::PBW; ++pb) {
                    P[pb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[pb][ks].x, x.x, P[pb], 0, 0, 0);
                    Q[pb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[pb][ks].y, x.y, Q[pb], 0, 0, 0);
                    R[pb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[pb][ks].x, x.y, R[pb], 0, 0, 0);
                    U[pb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[pb][ks].y, x.x, U[pb], 0, 0, 0);
                }
            }
            // this lane holds bit jb of hypotheses p = 16 block + kq + 4 reg
            double m0 = 0.0, m1 = 0.0;
#pragma unroll
            for (int pb = 0; pb < G::PBW; ++pb)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int p = (pgroup * G::PBW + pb) * 16 + kq + 4 * reg;
                    const double re = P[pb][reg] + Q[pb][reg], im = R[pb][reg] - U[pb][reg];
                    const double mag = p < G::NH ? sqrt(fma(re, re, im * im)) : 0.0;
                    if ((p >> G::C) & 1)
                        m1 = fmax(m1, mag);
                    else
                        m0 = fmax(m0, mag);
                }
#pragma unroll
            for (int d = 16; d <= 32; d <<= 1) {
                m0 = fmax(m0, __shfl_xor(m0, d, WF_WAVE));
                m1 = fmax(m1, __shfl_xor(m1, d, WF_WAVE));
            }
            if (kq == 0) {
                s_max[(pgroup * NC_TILE + jb) * 2] = m0;
                s_max[(pgroup * NC_TILE + jb) * 2 + 1] = m1;
            }
        }
        __syncthreads();
        const int64_t j = tile * NC_TILE + t;                        // NC_THREADS == NC_TILE: thread t writes bit t
        if (j < nbits) {
            double m0 = s_max[t * 2], m1 = s_max[t * 2 + 1];
#pragma unroll
            for (int pg = 1; pg < G::PW; ++pg) {
                m0 = fmax(m0, s_max[(pg * NC_TILE + t) * 2]);
                m1 = fmax(m1, s_max[(pg * NC_TILE + t) * 2 + 1]);
            }
            const double lam = m0 - m1;
            llr[j] = lam;
            bits[j] = lam < 0.0 ? 1 : 0;
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
static_assert(NC_THREADS == NC_TILE, "thread t writes bit t of the tile");

struct nc_launch {
    const void *kernel;
    size_t lds;
};

template <int N, int SPS>
static nc_launch nc_launch_of()
{
    return {reinterpret_cast<const void *>(&noncoherent_kernel<N, SPS>), nc_geom<N, SPS>::LDS};
}

template <int N>
static bool nc_select_sps(int sps, nc_launch &out)
{
    switch (sps) {
    case 4: out = nc_launch_of<N, 4>(); return true;
    case 8: out = nc_launch_of<N, 8>(); return true;
    case 10: out = nc_launch_of<N, 10>(); return true;
    case 16: out = nc_launch_of<N, 16>(); return true;
    case 20: out = nc_launch_of<N, 20>(); return true;
    default: return false;
    }
}

// the instantiation for (N, sps), or false where there is none
static bool nc_select(int N, int sps, nc_launch &out)
{
    switch (N) {
    case 3: return nc_select_sps<3>(sps, out);
    case 5: return nc_select_sps<5>(sps, out);
    case 7: return nc_select_sps<7>(sps, out);
    default: return false;
    }
}

static inline bool nc_mis(const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

static inline bool nc_overlap(const void *a, size_t abytes, const void *b, size_t bbytes)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + bbytes && y < x + abytes;
}

static const int64_t kNcMax = (int64_t)1 << 40;

static int nc_grid(int cus, int64_t nbits)
{
    const int64_t ntiles = (nbits + NC_TILE - 1) / NC_TILE, cap = (int64_t)(cus > 0 ? cus : 256) * NC_MAX_BLOCKS_PER_CU;
    return (int)(ntiles < cap ? ntiles : cap);
}

extern "C" int wf_noncoherent_geometry(wf_ctx *ctx, int N, int sps, int64_t nbits, int64_t *h_geom)
{
    const char *who = "wf_noncoherent_geometry";
    WF_REQUIRE(ctx && h_geom, "%s: NULL argument", who);
    nc_launch L;
    WF_REQUIRE(nc_select(N, sps, L), "%s: N must be 3, 5 or 7 and sps 4, 8, 10, 16 or 20, not N = %d, sps = %d", who, N, sps);
    WF_REQUIRE(nbits >= 1 && nbits <= kNcMax, "%s: nbits must be 1 .. 2^40", who);
    h_geom[0] = NC_TILE;
    h_geom[1] = nc_grid(ctx->cus, nbits);
    h_geom[2] = (int64_t)L.lds;
    return WF_OK;
}

extern "C" int wf_noncoherent_soft_c128(wf_ctx *ctx, const double *d_received_ri, int64_t n, const double *d_templates_ri, int N, int sps, int64_t start,
                                        int64_t nbits, double *d_llr, uint8_t *d_bits, void *stream)
{
    const char *who = "wf_noncoherent_soft_c128";
    WF_REQUIRE(ctx && d_received_ri && d_templates_ri && d_llr && d_bits, "%s: NULL argument", who);
    nc_launch L;
    WF_REQUIRE(nc_select(N, sps, L), "%s: N must be 3, 5 or 7 and sps 4, 8, 10, 16 or 20, not N = %d, sps = %d", who, N, sps);
    WF_REQUIRE(n >= 1 && n <= kNcMax && nbits >= 1 && nbits <= kNcMax && start >= -kNcMax && start <= kNcMax,
               "%s: n and nbits must be 1 .. 2^40 and start within ± 2^40", who);
    WF_REQUIRE(!nc_mis(d_received_ri, 15) && !nc_mis(d_templates_ri, 15) && !nc_mis(d_llr, 7), "%s: samples and templates must be 16-byte, llr 8-byte aligned",
               who);
    const size_t in_bytes = (size_t)n * 16, tab_bytes = ((size_t)N * sps << N) * 16, llr_bytes = (size_t)nbits * 8, bit_bytes = (size_t)nbits;
    WF_REQUIRE(!nc_overlap(d_llr, llr_bytes, d_received_ri, in_bytes) && !nc_overlap(d_llr, llr_bytes, d_templates_ri, tab_bytes) &&
                   !nc_overlap(d_bits, bit_bytes, d_received_ri, in_bytes) && !nc_overlap(d_bits, bit_bytes, d_templates_ri, tab_bytes) &&
                   !nc_overlap(d_llr, llr_bytes, d_bits, bit_bytes),
               "%s: the outputs overlap each other or an input", who);
    WF_REQUIRE(L.lds <= NC_MAX_LDS, "%s: a tile of sps = %d does not fit the LDS", who, sps);
    WF_HIP(hipSetDevice(ctx->device));
    if (L.lds > 48 * 1024) WF_HIP(hipFuncSetAttribute(L.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds));
    const double2 *r = reinterpret_cast<const double2 *>(d_received_ri), *T = reinterpret_cast<const double2 *>(d_templates_ri);
    void *args[] = {(void *)&r, (void *)&n, (void *)&T, (void *)&start, (void *)&nbits, (void *)&d_llr, (void *)&d_bits};
    WF_HIP(hipLaunchKernel(L.kernel, dim3(nc_grid(ctx->cus, nbits)), dim3(NC_THREADS), args, L.lds, wf_stream(stream)));
    return WF_OK;
}
