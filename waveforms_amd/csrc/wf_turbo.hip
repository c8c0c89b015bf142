// wf_turbo.hip — turbo codes: two terminated recursive systematic convolutional (RSC) constituents joined by an interleaver; the
// encoder and the max-log-MAP turbo decoder that runs EVERY half-iteration of a block in one launch (include/wfhip.h states the
// code and the decoder's arithmetic).  A code is an opaque handle whose tables are validated once on the host and uploaded into
// device memory the handle owns.
//
// Decoder: the wave of wf_conv.hip (lane = trellis state, 64 / S codewords side by side, alpha checkpoints every CONV_C steps in
// the context's detector scratch, the segment's alpha recomputed into LDS, predecessors and successors by ds_bpermute, the
// maxima of a step all-reduced over a codeword's S lanes by the DPP butterfly).  An RSC trellis has the connectivity of the
// feed-forward one and the same code-bit labels as a function of the register (a << nu) | s, with the feedback mask as
// generator 0: only the information bit u = a ^ f(s) of a branch differs, and it IS code bit 0, so the prior joins gamma where
// code bit 0 is 1 and the information bit's posterior is P of output 0.
// What is new is the loop around the two sweeps: the wave keeps its codewords through all H half-iterations.  The lane that
// owns a step's posterior writes the scaled extrinsic value straight to the OTHER constituent's prior at its interleaved
// address (A1, A2 and constituent 1's decisions live in the scratch beside the checkpoints), the next half-iteration stages
// them from there, and nothing goes back to the host.  A codeword whose two constituents agree stops: its lanes stay in the
// wave's lockstep, every write of theirs is masked, and the wave leaves the loop when all its codewords have stopped.
//
// Encoder: the register recursion is linear over GF(2), so a thread owns a run of message steps, computes the run's zero-state
// response, a scan over the codeword's runs with the powers of the run's transition matrix (the leap-ahead of wf_lfsr.hip,
// the state-map scan of wf_encode.hip) hands every run its start state, and the run is walked again to emit its bits.
#include "wf_conv_common.h"

#define TURBO_ENC_THREADS 256       // = the most runs of one constituent
#define TURBO_ENC_MIN_RUN 8         // message steps per encoder thread, at least

struct wf_turbo_code {
    int device = 0;
    int32_t K = 0, nu = 0, n_par = 0, m = 0, k = 0, T = 0, N = 0, n_tx = 0;
    uint32_t gen[4] = {0, 0, 0, 0};       // [0] the feedback mask (generator of the systematic output), [1 ..] the parity generators
    int32_t enc_run = 0, enc_nruns = 0;   // message steps per encoder thread, runs per constituent (<= TURBO_ENC_THREADS)
    uint32_t enc_pow[8] = {0};            // (M^enc_run)^(2^d), M the zero-input transition matrix: column c in bits 4 c .. 4 c + 3
    void *d_block = nullptr;              // the four tables below, one allocation
    const int32_t *d_perm = nullptr;      // k: constituent 2 encodes u[perm[i]] at step i
    const int32_t *d_inv = nullptr;       // k: perm[inv[i]] = i
    const int32_t *d_var_src = nullptr;   // N: transmitted position of variable v, -1 when punctured
    const int32_t *d_tx_var = nullptr;    // n_tx
};

// The arguments no step of the serial loops needs, parked in LDS: read from there between the loops, they hold no scalar
// registers across them (left in the argument block they stay live from the first instruction to the last).
struct turbo_cold {
    const int32_t *perm, *inv, *var_src;
    const double *llr;
    const uint8_t *ref;
    int32_t *iters;
    unsigned long long *counts;
    double scale;
    int64_t ncw;
    int32_t n_tx;
};

struct turbo_geom : wf_wave_geom {
    size_t lds_bytes = 0, scratch_bytes = 0;
    size_t off_a1 = 0, off_a2 = 0, off_d1 = 0;      // byte offsets in the scratch behind the checkpoints
};

static size_t turbo_lds_bytes(int nu, int m)
{
    const size_t G = 64 >> nu;
    return 4 * (G * (CONV_C * m + 1) + 2 * G * (CONV_C + 1) + CONV_C * 64 + CONV_C * m + 2 * CONV_C) + sizeof(turbo_cold);
}

static turbo_geom turbo_geometry(const wf_ctx *ctx, const wf_turbo_code *c, int64_t ncw)
{
    turbo_geom g;
    // per wave: the checkpoints, A1 and A2 (G x k floats each) and constituent 1's decisions (G x k bytes)
    const int64_t gk = (int64_t)(64 >> c->nu) * c->k;
    static_cast<wf_wave_geom &>(g) = wf_wave_geometry(ctx, c->nu, c->T, ncw, 9 * gk);
    g.lds_bytes = turbo_lds_bytes(c->nu, c->m);
    g.off_a1 = (size_t)(g.per_launch * g.nseg * 64 * 4);
    g.off_a2 = g.off_a1 + (size_t)(g.per_launch * gk * 4);
    g.off_d1 = g.off_a2 + (size_t)(g.per_launch * gk * 4);
    g.scratch_bytes = g.off_d1 + (size_t)(g.per_launch * gk);
    return g;
}

// ------------------------------------------------------------------------------------------------ encoder
struct turbo_enc_args {
    const uint8_t *info;
    uint8_t *out;
    const int32_t *perm, *var_src;
    int64_t ncw;
    int32_t k, T, nu, m, n_tx, run, nruns;
    uint32_t gen[4], pw[8];
};

// M z for a matrix packed by columns (column c in bits 4 c .. 4 c + 3) and a state of at most 4 bits
__host__ __device__ __forceinline__ uint32_t turbo_apply(uint32_t M, uint32_t z)
{
    uint32_t r = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) r ^= (0u - ((z >> c) & 1u)) & ((M >> (4 * c)) & 0xFu);
    return r;
}

// One workgroup per (codeword, constituent), thread t owns message steps t run .. t run + run - 1 (the thread of the last run
// also walks the nu tail steps).  Every run before the last is `run` steps long, so the state after runs 0 .. t is
// A v_{t-1} ^ z_t with the ONE matrix A = M^run: a Hillis-Steele scan with A^(2^d) at level d.
__global__ __launch_bounds__(TURBO_ENC_THREADS) void turbo_encode_kernel(turbo_enc_args a)
{
    __shared__ uint32_t sZ[TURBO_ENC_THREADS];
    const int t = threadIdx.x;
    const uint32_t fbl = a.gen[0] & ((1u << a.nu) - 1u);
    const int i0 = t * a.run, i1 = min(i0 + a.run, a.k);              // (empty for a thread past the last run)
    for (int64_t item = blockIdx.x; item < 2 * a.ncw; item += gridDim.x) {
        const int64_t cw = item >> 1;
        const int c = (int)(item & 1);
        const uint8_t *u = a.info + cw * a.k;
        uint32_t z = 0;                                               // the run's zero-state response
        for (int i = i0; i < i1; ++i) {
            const uint32_t av = (u[c ? a.perm[i] : i] & 1u) ^ (__popc(z & fbl) & 1u);
            z = ((av << a.nu) | z) >> 1;
        }
        uint32_t v = z;
        for (int d = 0, off = 1; off < a.nruns; ++d, off <<= 1) {
            sZ[t] = v;
            __syncthreads();
            if (t >= off) v ^= turbo_apply(a.pw[d], sZ[t - off]);
            __syncthreads();
        }
        sZ[t] = v;
        __syncthreads();
        uint32_t s = t ? sZ[t - 1] : 0u;                              // the state at step i0
        __syncthreads();
        if (i0 < a.k) {
            const int iend = i1 == a.k ? a.T : i1;
            for (int i = i0; i < iend; ++i) {
                const uint32_t av = i < a.k ? (u[c ? a.perm[i] : i] & 1u) ^ (__popc(s & fbl) & 1u) : 0u;
                const uint32_t reg = (av << a.nu) | s;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (j < a.m) {
                        const int src = a.var_src[2 * a.m * i + c * a.m + j];
                        if (src >= 0) a.out[cw * a.n_tx + src] = (uint8_t)(__popc(reg & a.gen[j]) & 1);
                    }
                }
                s = reg >> 1;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ decoder
struct turbo_dec_args {
    const int32_t *perm, *inv, *var_src;
    const double *llr;
    float *a1;                      // ncw x k: the caller's (in and out: have_a1), or in the scratch and starting as 0
    uint8_t *bits;
    float *post, *ext;
    int32_t *iters;
    const uint8_t *ref;
    unsigned long long *counts;
    float *ckpt;                    // waves x nseg x 64
    float *s_a2;                    // waves x G x k
    uint8_t *s_d1;                  // waves x G x k: [Λ1_i < 0]
    int64_t ncw, ext_stride;
    double scale;
    float es, clip;
    int32_t k, T, n_tx, nseg, H, early, have_a1;
    uint32_t gen[4];
};

template <int NU, int NPAR>
__global__ __launch_bounds__(WF_WAVE) void turbo_decode_kernel(turbo_dec_args a)
{
    constexpr int S = 1 << NU, G = WF_WAVE / S, C = CONV_C, M = NPAR + 1, LSTR = C * M + 1, ASTR = C + 1;
    __shared__ float sL[G * LSTR], sNA[G * ASTR], sAl[C * WF_WAVE];   // channel values, MINUS the prior (+0 in the tail), alpha
    __shared__ int sR[G * ASTR], sSrc[C * M], sSys[C], sPi[C];
    __shared__ turbo_cold sCold;
    const int lane = threadIdx.x, s = lane & (S - 1), g = lane >> NU, base = lane - s;
    const int64_t wave = blockIdx.x, cw = wave * G + g;
    const bool mine = cw < a.ncw;
    const int k = a.k, T = a.T;

    // the two branches that ENTER state s (both with register input a_in = its top bit), and the two that LEAVE it (a = 0, 1);
    // code bit 0 of a branch is its information bit u
    const bool a_in = (s >> (NU - 1)) != 0;
    const int p0 = (2 * s) & (S - 1), p1 = p0 + 1, n0 = s >> 1, n1 = n0 | (S >> 1);
    uint32_t cin0[M], cin1[M], cout0[M], cout1[M];                    // all ones where the branch's code bit j is 1
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const uint32_t gj = a.gen[j], top = a_in ? (uint32_t)S : 0u;
        cin0[j] = 0u - (__popc((top | (uint32_t)p0) & gj) & 1u);
        cin1[j] = 0u - (__popc((top | (uint32_t)p1) & gj) & 1u);
        cout0[j] = 0u - (__popc((uint32_t)s & gj) & 1u);
        cout1[j] = 0u - (__popc(((uint32_t)S | (uint32_t)s) & gj) & 1u);
        // (opaque: known to be 0 / all ones, every mask would become a lane mask in a pair of scalar registers, 16 pairs in all)
        asm volatile("" : "+v"(cin0[j]), "+v"(cin1[j]), "+v"(cout0[j]), "+v"(cout1[j]));
    }

    if (lane == 0) sCold = turbo_cold{a.perm, a.inv, a.var_src, a.llr, a.ref, a.iters, a.counts, a.scale, a.ncw, a.n_tx};
    const int64_t gk = (int64_t)G * k;
    float *A1w = a.a1 + wave * gk;                                    // codeword g of the wave at [g k + i], caller's or scratch
    float *A2w = a.s_a2 + wave * gk;
    uint8_t *D1w = a.s_d1 + wave * gk;
    float *ck = a.ckpt + (size_t)wave * a.nseg * WF_WAVE + lane;

    // a segment's operands of constituent c (0 / 1) into LDS, by all lanes.
    // A1, A2 and D1 travel from lane to lane through GLOBAL memory: one lane wrote them in the half-iteration before, any lane
    // reads them here.  What makes those writes visible is the __syncthreads() below and nothing else: it is a release /
    // acquire fence at WORKGROUP scope, and that is enough only because the workgroup is this ONE wave, whose stores and loads
    // go through the same compute unit's vector L1 in program order (write-through; no threadgroup-split mode).  A workgroup
    // of several waves still on one compute unit keeps the guarantee; waves of DIFFERENT workgroups sharing these buffers, a
    // non-temporal / cache-bypassing policy on one side only, or a barrier that orders LDS alone (wf_lds_barrier) would
    // break it silently: then the stores need an agent-scope release and the loads an agent-scope acquire.
    auto stage = [&](int c, bool zero_prior, int seg) {
        __syncthreads();
        const turbo_cold q = sCold;
        const int i0 = seg * C;
        for (int idx = lane; idx < G * C * M; idx += WF_WAVE) {
            const int gg = idx / (C * M), r = idx - gg * (C * M), t = r / M, j = r - t * M, i = i0 + t;
            const int64_t cwg = wave * G + gg;
            float L = 0.0f;
            if (i < T && cwg < q.ncw) {
                const int v = c && j == 0 && i < k ? 2 * M * q.perm[i] : 2 * M * i + c * M + j;     // Ls2_i = Ls1_π(i)
                const int src = q.var_src[v];
                if (src >= 0) L = (float)(q.scale * q.llr[cwg * q.n_tx + src]);
            }
            sL[gg * LSTR + r] = L;
        }
        for (int idx = lane; idx < G * C; idx += WF_WAVE) {
            const int gg = idx / C, t = idx - gg * C, i = i0 + t;
            const int64_t cwg = wave * G + gg;
            float A = 0.0f;
            int r = 0;
            if (i < k && cwg < q.ncw) {
                const int pi = c ? q.perm[i] : i;
                if (c) A = A2w[gg * k + i];
                else if (!zero_prior) A = A1w[gg * k + i];
                if (c) r = D1w[gg * k + pi] & 1;                      // bit 0: [Λ1_π(i) < 0]
                if (q.ref) r |= (q.ref[cwg * k + pi] & 1) << 1;       // bit 1: the reference bit this step decides
            }
            sNA[gg * ASTR + t] = i < k ? -A : 0.0f;
            sR[gg * ASTR + t] = r;
        }
        for (int idx = lane; idx < C * M; idx += WF_WAVE) {
            const int t = idx / M, i = i0 + t;
            sSrc[idx] = i < T ? q.var_src[2 * M * i + c * M + (idx - t * M)] : -1;
        }
        if (lane < C) {
            const int i = i0 + lane;
            sPi[lane] = i < k ? (c ? q.perm[i] : q.inv[i]) : 0;       // where this step's extrinsic value goes in the other prior
            sSys[lane] = c && i < k ? q.var_src[2 * M * q.perm[i]] : -1;
        }
        __syncthreads();
    };
    // alpha_{i+1}(s) from alpha_i, i = seg C + t
    auto forward = [&](float al, int i, int t) {
        float L[M];
#pragma unroll
        for (int j = 0; j < M; ++j) L[j] = sL[g * LSTR + t * M + j];
        const uint32_t nA = __float_as_uint(sNA[g * ASTR + t]);
        const float g0 = conv_gamma<M>(__uint_as_float(nA & cin0[0]), L, cin0), g1 = conv_gamma<M>(__uint_as_float(nA & cin1[0]), L, cin1);
        const float a0 = __shfl(al, base + p0, WF_WAVE), a1 = __shfl(al, base + p1, WF_WAVE);
        const float an = fmaxf(__fadd_rn(a0, g0), __fadd_rn(a1, g1));
        return i >= k && a_in ? -INFINITY : an;
    };
    auto clipped = [&](float e) { return fminf(fmaxf(e, -a.clip), a.clip); };

    bool stopped = false;
    int halves = a.H, iters = (a.H + 1) / 2, err = 0;
    for (int h = 1; h <= a.H; ++h) {
        const int c = (h & 1) ^ 1;
        const bool live = mine && !stopped, zero_prior = h == 1 && !a.have_a1;
        const bool early = a.early != 0, outs = h == a.H || (c && early);                // this half-iteration's decisions may be the codeword's last
        const bool wext = a.ext && (early || h >= a.H - 1);         // ... and so may its extrinsic values

        // one walk over the segments, up and then down: nseg - 1 forward phases that leave a checkpoint each, then every segment
        // from the last with its alpha recomputed (the same operations on the same operands) and its backward steps.  (alpha
        // goes to LDS in the forward phases too: one loop body for both.)
        // (the uniform flags in ONE scalar and the lane's role in one vector register, both opaque inside the step loop: held as
        // hoisted conditions they would take a pair of scalar registers each)
        const int flags = c | (outs ? 2 : 0) | (wext ? 4 : 0) | (a.post ? 8 : 0) | (a.bits ? 16 : 0), lrole = live ? s : -1;
        float al = s == 0 ? 0.0f : -INFINITY, be = al;
        int herr = 0, mism = 0;
        for (int ph = 0; ph < 2 * a.nseg - 1; ++ph) {
            const bool bw = ph >= a.nseg - 1;
            const int seg = bw ? 2 * a.nseg - 2 - ph : ph, i0 = seg * C, len = min(C, T - i0);
            stage(c, zero_prior, seg);
            if (!bw) ck[(size_t)seg * WF_WAVE] = al;
            else if (ph > a.nseg - 1) al = ck[(size_t)seg * WF_WAVE];
            for (int t = 0; t < len; ++t) {
                sAl[t * WF_WAVE + lane] = al;       // (read back by this lane only)
                al = forward(al, i0 + t, t);
            }
            if (!bw) continue;
            for (int t = len - 1; t >= 0; --t) {
                const int i = i0 + t;
                int f = flags, role = lrole;
                asm volatile("" : "+s"(f), "+v"(role));
                float L[M];
#pragma unroll
                for (int j = 0; j < M; ++j) L[j] = sL[g * LSTR + t * M + j];
                const float nAf = sNA[g * ASTR + t], ai = sAl[t * WF_WAVE + lane];
                const uint32_t nA = __float_as_uint(nAf);
                const float b0 = __shfl(be, base + n0, WF_WAVE), b1 = __shfl(be, base + n1, WF_WAVE);
                const float g0 = conv_gamma<M>(__uint_as_float(nA & cout0[0]), L, cout0), g1 = conv_gamma<M>(__uint_as_float(nA & cout1[0]), L, cout1);
                const bool tail = i >= k;
                const float V0 = __fadd_rn(__fadd_rn(ai, g0), b0), V1 = tail ? -INFINITY : __fadd_rn(__fadd_rn(ai, g1), b1);
                const float W0 = __fadd_rn(g0, b0), W1 = tail ? -INFINITY : __fadd_rn(g1, b1);
                be = fmaxf(W0, W1);
#pragma unroll
                for (int j = 0; j < M; ++j) {
                    const float m0 = conv_group_max<S>(fmaxf(conv_drop_if(cout0[j], V0), conv_drop_if(cout1[j], V1)));
                    const float m1 = conv_group_max<S>(fmaxf(conv_keep_if(cout0[j], V0), conv_keep_if(cout1[j], V1)));
                    const float P = __fsub_rn(m0, m1);
                    if (j == 0 && role == 0 && !tail) {          // P is Λ_i: the extrinsic value, the decision, the stop rule
                        const int pi = sPi[t], r = sR[g * ASTR + t], bit = P < 0.0f ? 1 : 0;
                        const float E = __fmul_rn(a.es, __fsub_rn(__fsub_rn(P, -nAf), L[0]));
                        const int at = f & 1 ? pi : i;                    // the information bit this step decides
                        if (f & 1) {
                            A1w[g * k + pi] = E;
                            mism += bit != (r & 1) ? 1 : 0;
                            const int sys = sSys[t];
                            if ((f & 4) && sys >= 0) a.ext[cw * a.ext_stride + sys] = clipped(__fsub_rn(P, L[0]));
                        } else {
                            A2w[g * k + pi] = E;
                            D1w[g * k + i] = (uint8_t)bit;
                        }
                        if (f & 2) {
                            if (f & 8) a.post[cw * k + at] = P;
                            if (f & 16) a.bits[cw * k + at] = (uint8_t)bit;
                            herr += bit != (r >> 1) ? 1 : 0;
                        }
                    }
                    // constituent 1's systematic variable at i < k takes its value from Λ2 (above); constituent 2's own, if it is
                    // transmitted at all, is the one variable whose channel value is not among the staged ones
                    const int src = sSrc[t * M + j];
                    if (role == j && (f & 4) && src >= 0 && !(j == 0 && !tail && !(f & 1))) {
                        const float Lown = j == 0 && !tail ? (float)(sCold.scale * sCold.llr[cw * sCold.n_tx + src]) : L[j];
                        a.ext[cw * a.ext_stride + src] = clipped(__fsub_rn(P, Lown));
                    }
                }
            }
        }
        if (outs && live) err = herr;
        if (c && early) {
            if (__shfl(live && mism == 0 ? 1 : 0, base, WF_WAVE)) {   // (the count lives in the lane of state 0)
                stopped = true;
                halves = h;
                iters = h / 2;
            }
        }
        if (__ballot(mine && !stopped) == 0ull) break;
    }
    if (s == 0 && mine) {
        const turbo_cold q = sCold;
        if (q.iters) q.iters[cw] = iters;
        if (q.ref) {
            atomicAdd(q.counts + 0, (unsigned long long)err);
            if (err) atomicAdd(q.counts + 1, 1ull);
            atomicAdd(q.counts + 2, (unsigned long long)halves);
        }
    }
}

// ------------------------------------------------------------------------------------------------ host
static uint32_t turbo_matmul(uint32_t A, uint32_t B)                  // columns of A B = A applied to the columns of B
{
    uint32_t r = 0;
    for (int c = 0; c < 4; ++c) r |= turbo_apply(A, (B >> (4 * c)) & 0xFu) << (4 * c);
    return r;
}

extern "C" int wf_turbo_code_create(wf_ctx *ctx, int32_t K, int32_t n_par, uint32_t fb, const uint32_t *h_gen, int32_t k, const int32_t *h_perm,
                                    int32_t n_tx, const int32_t *h_tx_var, wf_turbo_code **out)
{
    WF_REQUIRE(ctx && h_gen && h_perm && h_tx_var && out, "wf_turbo_code_create: NULL argument");
    *out = nullptr;
    WF_REQUIRE(K >= 3 && K <= 5, "wf_turbo_code_create: K = %d outside 3 .. 5", K);
    WF_REQUIRE(n_par >= 1 && n_par <= 3, "wf_turbo_code_create: n_par = %d outside 1 .. 3", n_par);
    const int nu = K - 1, m = 1 + n_par;
    WF_REQUIRE(wf_tap_mask_ok(fb, K), "wf_turbo_code_create: feedback mask 0%o must be a K-bit mask with bit K - 1 and bit 0 set", fb);
    for (int j = 0; j < n_par; ++j) {
        WF_REQUIRE(wf_tap_mask_ok(h_gen[j], K), "wf_turbo_code_create: parity generator %d = 0%o must be a K-bit mask with bit K - 1 and bit 0 set", j,
                   h_gen[j]);
        WF_REQUIRE(h_gen[j] != fb, "wf_turbo_code_create: parity generator %d equals the feedback mask 0%o", j, fb);
    }
    WF_REQUIRE(k >= 1 && 2 * (int64_t)m * ((int64_t)k + nu) <= CONV_MAX_N, "wf_turbo_code_create: k = %d: N = 2 m (k + K - 1) outside 2 m K .. %d", k,
               CONV_MAX_N);
    const int32_t T = k + nu, N = 2 * m * T;
    WF_REQUIRE(n_tx >= 1 && n_tx <= N, "wf_turbo_code_create: n_tx = %d outside 1 .. N = %d", n_tx, N);
    std::vector<int32_t> blob((size_t)2 * k + N + n_tx, -1);          // perm, inv, var -> src, tx_var
    for (int i = 0; i < k; ++i) {
        const int p = h_perm[i];
        WF_REQUIRE(p >= 0 && p < k, "wf_turbo_code_create: interleaver[%d] = %d outside 0 .. k - 1", i, p);
        WF_REQUIRE(blob[(size_t)k + p] < 0, "wf_turbo_code_create: the interleaver names %d twice", p);
        blob[i] = p;
        blob[(size_t)k + p] = i;
    }
    int32_t *var_src = blob.data() + 2 * (size_t)k;
    WF_TRY(wf_tx_table("wf_turbo_code_create", h_tx_var, n_tx, N, var_src, var_src + N));

    void *d_block;
    WF_TRY(wf_code_upload("wf_turbo_code_create", ctx->device, blob.data(), blob.size() * sizeof(int32_t), &d_block));
    wf_turbo_code *c = new wf_turbo_code();
    c->device = ctx->device, c->d_block = d_block;
    c->K = K, c->nu = nu, c->n_par = n_par, c->m = m, c->k = k, c->T = T, c->N = N, c->n_tx = n_tx;
    c->gen[0] = fb;
    for (int j = 0; j < n_par; ++j) c->gen[1 + j] = h_gen[j];
    // the encoder's runs and the powers of the run's zero-input transition matrix s -> ((f(s) << nu) | s) >> 1
    c->enc_run = std::max(TURBO_ENC_MIN_RUN, (k + TURBO_ENC_THREADS - 1) / TURBO_ENC_THREADS);
    c->enc_nruns = (k + c->enc_run - 1) / c->enc_run;
    const uint32_t fbl = fb & ((1u << nu) - 1u);
    uint32_t M1 = 0, A = 0x8421u;                                     // (the identity)
    for (int b = 0; b < nu; ++b) {
        const uint32_t st = 1u << b;
        M1 |= ((((uint32_t)__builtin_parity(st & fbl) << nu) | st) >> 1) << (4 * b);
    }
    for (int r = 0; r < c->enc_run; ++r) A = turbo_matmul(M1, A);
    for (int d = 0; d < 8; ++d) {
        c->enc_pow[d] = A;
        A = turbo_matmul(A, A);
    }
    c->d_perm = static_cast<const int32_t *>(c->d_block);
    c->d_inv = c->d_perm + k;
    c->d_var_src = c->d_inv + k;
    c->d_tx_var = c->d_var_src + N;
    *out = c;
    return WF_OK;
}

extern "C" int wf_turbo_code_free(wf_turbo_code *code)
{
    if (!code) return WF_OK;
    const int rc = wf_code_release("wf_turbo_code_free", code->device, {code->d_block});
    delete code;                          // (whatever hipFree said: the host struct never outlives the call)
    return rc;
}

extern "C" int wf_turbo_encode(wf_ctx *ctx, const wf_turbo_code *code, const uint8_t *d_info, int64_t ncw, uint8_t *d_tx, void *stream)
{
    WF_REQUIRE(ctx && code && d_info && d_tx, "wf_turbo_encode: NULL argument");
    WF_REQUIRE(ncw >= 1, "wf_turbo_encode: ncw must be at least 1");
    WF_REQUIRE_SAME_DEVICE("wf_turbo_encode", code, ctx);
    WF_HIP(hipSetDevice(ctx->device));
    turbo_enc_args a;
    a.info = d_info, a.out = d_tx, a.perm = code->d_perm, a.var_src = code->d_var_src, a.ncw = ncw;
    a.k = code->k, a.T = code->T, a.nu = code->nu, a.m = code->m, a.n_tx = code->n_tx, a.run = code->enc_run, a.nruns = code->enc_nruns;
    for (int j = 0; j < 4; ++j) a.gen[j] = code->gen[j];
    for (int d = 0; d < 8; ++d) a.pw[d] = code->enc_pow[d];
    const int grid = wf_grid_for(2 * ncw, 1, std::max(ctx->cus, 1) * 16);
    hipLaunchKernelGGL(turbo_encode_kernel, dim3(grid), dim3(TURBO_ENC_THREADS), 0, wf_stream(stream), a);
    WF_LAUNCH_CHECK();
    return WF_OK;
}

extern "C" int wf_turbo_decode_geometry(wf_ctx *ctx, const wf_turbo_code *code, int64_t ncw, int64_t *h_geom)
{
    WF_REQUIRE(ctx && code && h_geom && ncw >= 1, "wf_turbo_decode_geometry: bad argument");
    const turbo_geom g = turbo_geometry(ctx, code, ncw);
    h_geom[0] = g.G;
    h_geom[1] = g.waves;
    h_geom[2] = CONV_C;
    h_geom[3] = (int64_t)g.lds_bytes;
    h_geom[4] = (int64_t)g.scratch_bytes;
    return WF_OK;
}

template <int NU>
static void turbo_decode_launch(int n_par, unsigned grid, hipStream_t st, const turbo_dec_args &a)
{
    if (n_par == 1) hipLaunchKernelGGL((turbo_decode_kernel<NU, 1>), dim3(grid), dim3(WF_WAVE), 0, st, a);
    else if (n_par == 2) hipLaunchKernelGGL((turbo_decode_kernel<NU, 2>), dim3(grid), dim3(WF_WAVE), 0, st, a);
    else hipLaunchKernelGGL((turbo_decode_kernel<NU, 3>), dim3(grid), dim3(WF_WAVE), 0, st, a);
}

extern "C" int wf_turbo_decode(wf_ctx *ctx, const wf_turbo_code *code, const double *d_llr, int64_t ncw, double scale, float ext_scale,
                               int32_t half_iters, int32_t early_stop, float *d_a1, uint8_t *d_info_bits, float *d_info_post, int32_t *d_iters,
                               float *d_ext, int64_t ext_stride, float ext_clip, const uint8_t *d_ref_info, int64_t *d_counts, void *stream)
{
    WF_REQUIRE(ctx && code && d_llr, "wf_turbo_decode: NULL argument");
    WF_REQUIRE(ncw >= 1, "wf_turbo_decode: ncw must be at least 1");
    WF_REQUIRE(wf_finite_pos(scale), "wf_turbo_decode: scale must be finite and positive");
    WF_REQUIRE(wf_finite_pos(ext_scale), "wf_turbo_decode: ext_scale must be finite and positive");
    WF_REQUIRE(half_iters >= 1 && half_iters <= 64, "wf_turbo_decode: half_iters = %d outside 1 .. 64", half_iters);
    WF_REQUIRE(!d_ext || (half_iters % 2 == 0 && ext_stride >= code->n_tx && ext_clip > 0.0f),
               "wf_turbo_decode: d_ext needs an even half_iters, ext_stride >= n_tx and ext_clip > 0");
    WF_REQUIRE(!d_ref_info || d_counts, "wf_turbo_decode: d_ref_info needs d_counts");
    WF_REQUIRE(wf_aligned(d_llr, 8) && wf_aligned(d_counts, 8) && wf_aligned(d_a1, 4) && wf_aligned(d_info_post, 4) && wf_aligned(d_ext, 4) &&
                   wf_aligned(d_iters, 4),
               "wf_turbo_decode: llr and counts must be 8-byte, a1, post, ext and iters 4-byte aligned");
    WF_REQUIRE_SAME_DEVICE("wf_turbo_decode", code, ctx);
    const turbo_geom g = turbo_geometry(ctx, code, ncw);
    WF_HIP(hipSetDevice(ctx->device));
    WF_TRY(wf_ctx_reserve_vit(ctx, (g.scratch_bytes + 7) / 8));
    turbo_dec_args a;
    a.perm = code->d_perm, a.inv = code->d_inv, a.var_src = code->d_var_src;
    char *scratch = reinterpret_cast<char *>(ctx->d_vit_edge);
    a.ckpt = reinterpret_cast<float *>(scratch);
    float *s_a1 = reinterpret_cast<float *>(scratch + g.off_a1);
    a.s_a2 = reinterpret_cast<float *>(scratch + g.off_a2);
    a.s_d1 = reinterpret_cast<uint8_t *>(scratch + g.off_d1);
    a.ext_stride = ext_stride, a.scale = scale, a.es = ext_scale, a.clip = ext_clip;
    a.k = code->k, a.T = code->T, a.n_tx = code->n_tx, a.nseg = g.nseg, a.H = half_iters, a.early = early_stop ? 1 : 0, a.have_a1 = d_a1 ? 1 : 0;
    for (int j = 0; j < 4; ++j) a.gen[j] = code->gen[j];
    a.counts = reinterpret_cast<unsigned long long *>(d_counts);
    // launches of at most g.per_launch waves (the scratch is sized for that many)
    return wf_for_slices(ncw, g.per_launch * g.G, [&](int64_t b0, int64_t count) -> int {
        a.ncw = count;
        a.llr = d_llr + b0 * code->n_tx;
        a.a1 = d_a1 ? d_a1 + b0 * code->k : s_a1;
        a.bits = d_info_bits ? d_info_bits + b0 * code->k : nullptr;
        a.post = d_info_post ? d_info_post + b0 * code->k : nullptr;
        a.iters = d_iters ? d_iters + b0 : nullptr;
        a.ext = d_ext ? d_ext + b0 * ext_stride : nullptr;
        a.ref = d_ref_info ? d_ref_info + b0 * code->k : nullptr;
        const unsigned grid = (unsigned)((a.ncw + g.G - 1) / g.G);
        const hipStream_t st = wf_stream(stream);
        switch (code->nu) {
        case 2: turbo_decode_launch<2>(code->n_par, grid, st, a); break;
        case 3: turbo_decode_launch<3>(code->n_par, grid, st, a); break;
        default: turbo_decode_launch<4>(code->n_par, grid, st, a); break;
        }
        WF_LAUNCH_CHECK();
        return WF_OK;
    });
}
