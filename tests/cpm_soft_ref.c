/* cpm_soft_ref.c — the definition of wf_cpm_soft (include/wfhip.h), restated sequentially for tests/test_cpm_soft.py.
 *
 * Compiled at test time with gcc -O2 -ffp-contract=off (explicit fma() where the definition has one, no other fusion).
 * The trellis is cpm_oracle.c's with NC = p: state s = v + p c, branch (s, u) -> (v + K_old u_old) mod p + p c2, tilt and
 * pre-start variant of the global call n = first_call + k. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

typedef struct {
    int M, lgM, p, nh, K[2], Lp, S, NF, msub;
} cs_spec;

static int imod(int64_t a, int m)
{
    int r = (int)(a % m);
    return r < 0 ? r + m : r;
}

static void cs_init(cs_spec *c, int M, int p, int nh, const int *K, int Lp)
{
    c->M = M; c->lgM = M == 4 ? 2 : 1; c->p = p; c->nh = nh; c->K[0] = K[0]; c->K[1] = nh == 2 ? K[1] : K[0]; c->Lp = Lp;
    c->S = p; c->NF = M; c->msub = 1;
    for (int i = 1; i < Lp; ++i) { c->S *= M; c->NF *= M; }
    for (int i = 2; i < Lp; ++i) c->msub *= M;
}

/* (M - 1) * (sum of K over symbols 0 .. n - Lp) mod 2p, as cpm_oracle.c (ksum_mod) */
static int cs_tilt(const cs_spec *c, int64_t n)
{
    const int64_t m = n - c->Lp + 1;
    if (m <= 0) return 0;
    int per = 0;
    for (int i = 0; i < c->nh; ++i) per += c->K[i];
    int64_t acc = (m / c->nh) % (2 * c->p) * per;
    for (int i = 0; i < (int)(m % c->nh); ++i) acc += c->K[i];
    return imod((int64_t)(c->M - 1) * (acc % (2 * c->p)), 2 * c->p);
}

static int cs_end(const cs_spec *c, int64_t n, int s, int u)
{
    const int64_t m_old = n - c->Lp + 1;
    const int K_old = m_old >= 0 ? c->K[m_old % c->nh] : 0;
    const int v = s % c->p, corr = s / c->p;
    const int u_old = c->Lp == 1 ? u : corr / c->msub;
    const int corr2 = c->Lp == 1 ? 0 : u + c->M * (corr % c->msub);
    return (v + K_old * u_old) % c->p + c->p * corr2;
}

static double cs_inc(const cs_spec *c, const double *rot_cs, const double *rows_ri, int64_t k, int64_t n, int s, int u)
{
    const int v = s % c->p, corr = s / c->p;
    const int r = imod(2 * (int64_t)v - cs_tilt(c, n), 2 * c->p);
    const double *Z = rows_ri + (size_t)2 * k * c->NF;
    const int f = u + c->M * corr;
    return -fma(rot_cs[2 * r], Z[2 * f], rot_cs[2 * r + 1] * Z[2 * f + 1]);
}

/* increments inc[k][s][u] of a burst (small bursts: the brute-force test feeds them back through cpm_soft_rec) */
void cpm_soft_incs(int M, int p, int nh, const int *K, int Lp, const double *rot_cs, const double *rows_ri, int64_t n,
                   int64_t first_call, double *inc)
{
    cs_spec c;
    cs_init(&c, M, p, nh, K, Lp);
    for (int64_t k = 0; k < n; ++k)
        for (int s = 0; s < c.S; ++s)
            for (int u = 0; u < M; ++u) inc[((size_t)k * c.S + s) * M + u] = cs_inc(&c, rot_cs, rows_ri, k, first_call + k, s, u);
}

/* The recursion.  inc != NULL: increments given as inc[k][s][u]; else computed from rot_cs and rows. */
static int cs_run(const cs_spec *c, const double *inc, const double *rot_cs, const double *rows_ri, int64_t n, int64_t first_call,
                  double *llr, uint8_t *bits)
{
    const int S = c->S, M = c->M, lg = c->lgM;
    double *alpha = malloc(sizeof(double) * (size_t)n * S);
    double *a = malloc(sizeof(double) * S), *nw = malloc(sizeof(double) * S), *b = malloc(sizeof(double) * S);
    if (!alpha || !a || !nw || !b) return -1;
#define INC(k, s, u) (inc ? inc[((size_t)(k) * S + (s)) * M + (u)] : cs_inc(c, rot_cs, rows_ri, (k), first_call + (k), (s), (u)))
    for (int s = 0; s < S; ++s) a[s] = 0.0;
    for (int64_t k = 0; k < n; ++k) {
        for (int s = 0; s < S; ++s) { alpha[(size_t)k * S + s] = a[s]; nw[s] = INFINITY; }
        for (int s = 0; s < S; ++s)
            for (int u = 0; u < M; ++u) {
                const int e = cs_end(c, first_call + k, s, u);
                const double cand = a[s] + INC(k, s, u);
                if (cand < nw[e]) nw[e] = cand;
            }
        double mn = nw[0];
        for (int s = 1; s < S; ++s) mn = nw[s] < mn ? nw[s] : mn;
        for (int s = 0; s < S; ++s) a[s] = nw[s] - mn;
    }
    for (int s = 0; s < S; ++s) b[s] = 0.0;
    for (int64_t k = n - 1; k >= 0; --k) {
        double m1[2] = {INFINITY, INFINITY}, m0[2] = {INFINITY, INFINITY};
        const double *ak = alpha + (size_t)k * S;
        for (int s = 0; s < S; ++s) {
            nw[s] = INFINITY;
            for (int u = 0; u < M; ++u) {
                const int e = cs_end(c, first_call + k, s, u);
                const double x = INC(k, s, u);
                const double t = (ak[s] + x) + b[e];
                for (int i = 0; i < lg; ++i) {
                    if ((u >> (lg - 1 - i)) & 1) { if (t < m1[i]) m1[i] = t; }
                    else if (t < m0[i]) m0[i] = t;
                }
                const double y = x + b[e];
                if (y < nw[s]) nw[s] = y;
            }
        }
        for (int i = 0; i < lg; ++i) {
            llr[(size_t)lg * k + i] = m1[i] - m0[i];
            bits[(size_t)lg * k + i] = m1[i] - m0[i] < 0.0 ? 1 : 0;
        }
        double mn = nw[0];
        for (int s = 1; s < S; ++s) mn = nw[s] < mn ? nw[s] : mn;
        for (int s = 0; s < S; ++s) b[s] = nw[s] - mn;
    }
#undef INC
    free(alpha); free(a); free(nw); free(b);
    return 0;
}

int cpm_soft_rec(int M, int p, int nh, const int *K, int Lp, const double *inc, int64_t n, int64_t first_call, double *llr, uint8_t *bits)
{
    cs_spec c;
    cs_init(&c, M, p, nh, K, Lp);
    return cs_run(&c, inc, NULL, NULL, n, first_call, llr, bits);
}

int cpm_soft_rows(int M, int p, int nh, const int *K, int Lp, const double *rot_cs, const double *rows_ri, int64_t n, int64_t first_call,
                  double *llr, uint8_t *bits)
{
    cs_spec c;
    cs_init(&c, M, p, nh, K, Lp);
    return cs_run(&c, NULL, rot_cs, rows_ri, n, first_call, llr, bits);
}
