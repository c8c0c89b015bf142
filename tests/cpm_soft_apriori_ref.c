/* cpm_soft_apriori_ref.c — the definition of wf_cpm_soft_apriori (include/wfhip.h), restated sequentially for
 * tests/test_cpm_idd.py.
 *
 * Compiled at test time with gcc -O2 -ffp-contract=off (explicit fma() where the definition has one, no other fusion).
 * The trellis is wf_cpm_soft's (cpm_oracle.c with NC = p): state s = v + p c, branch (s, u) -> (v + K_old u_old) mod p + p c2,
 * tilt and pre-start variant of the global call n = first_call + k.  prior == NULL is "no prior": π = 0 everywhere. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

typedef struct {
    int M, lgM, p, nh, K[2], Lp, S, NF, msub;
} ca_spec;

static int imod(int64_t a, int m)
{
    int r = (int)(a % m);
    return r < 0 ? r + m : r;
}

static void ca_init(ca_spec *c, int M, int p, int nh, const int *K, int Lp)
{
    c->M = M; c->lgM = M == 4 ? 2 : 1; c->p = p; c->nh = nh; c->K[0] = K[0]; c->K[1] = nh == 2 ? K[1] : K[0]; c->Lp = Lp;
    c->S = p; c->NF = M; c->msub = 1;
    for (int i = 1; i < Lp; ++i) { c->S *= M; c->NF *= M; }
    for (int i = 2; i < Lp; ++i) c->msub *= M;
}

/* (M - 1) * (sum of K over symbols 0 .. n - Lp) mod 2p */
static int ca_tilt(const ca_spec *c, int64_t n)
{
    const int64_t m = n - c->Lp + 1;
    if (m <= 0) return 0;
    int per = 0;
    for (int i = 0; i < c->nh; ++i) per += c->K[i];
    int64_t acc = (m / c->nh) % (2 * c->p) * per;
    for (int i = 0; i < (int)(m % c->nh); ++i) acc += c->K[i];
    return imod((int64_t)(c->M - 1) * (acc % (2 * c->p)), 2 * c->p);
}

static int ca_end(const ca_spec *c, int64_t n, int s, int u)
{
    const int64_t m_old = n - c->Lp + 1;
    const int K_old = m_old >= 0 ? c->K[m_old % c->nh] : 0;
    const int v = s % c->p, corr = s / c->p;
    const int u_old = c->Lp == 1 ? u : corr / c->msub;
    const int corr2 = c->Lp == 1 ? 0 : u + c->M * (corr % c->msub);
    return (v + K_old * u_old) % c->p + c->p * corr2;
}

static double ca_inc(const ca_spec *c, const double *rot_cs, const double *rows_ri, int64_t k, int64_t n, int s, int u)
{
    const int v = s % c->p, corr = s / c->p;
    const int r = imod(2 * (int64_t)v - ca_tilt(c, n), 2 * c->p);
    const double *Z = rows_ri + (size_t)2 * k * c->NF;
    const int f = u + c->M * corr;
    return -fma(rot_cs[2 * r], Z[2 * f], rot_cs[2 * r + 1] * Z[2 * f + 1]);
}

static int bit_of(const ca_spec *c, int u, int i) { return (u >> (c->lgM - 1 - i)) & 1; }

/* Π_k(u): the sum of π_{k,i} over the bits of u that are 1 — u = 3 of M = 4 is the ONE addition π_0 + π_1 */
static double ca_Pi(const ca_spec *c, const double *pi, int u)
{
    if (c->M == 2) return pi[0];                        /* (u = 1) */
    return u == 3 ? pi[0] + pi[1] : (u == 2 ? pi[0] : pi[1]);
}

/* inc'_k(s,u) */
static double ca_incp(const ca_spec *c, double x, const double *pi, int u) { return u ? x + ca_Pi(c, pi, u) : x; }

/* x_{k,i}(s,u): the channel increment plus the prior of the OTHER bit of u, if u has one and it is 1 */
static double ca_x(const ca_spec *c, double x, const double *pi, int u, int i)
{
    if (c->M == 4 && bit_of(c, u, 1 - i)) return x + pi[1 - i];
    return x;
}

/* The recursion.  inc != NULL: increments given as inc[k][s][u]; else computed from rot_cs and rows. */
static int ca_run(const ca_spec *c, const double *inc, const double *rot_cs, const double *rows_ri, int64_t n, int64_t first_call,
                  const float *prior, double scale, double *ext, uint8_t *bits)
{
    const int S = c->S, M = c->M, lg = c->lgM;
    double *alpha = malloc(sizeof(double) * (size_t)n * S), *pis = malloc(sizeof(double) * (size_t)n * lg);
    double *a = malloc(sizeof(double) * S), *nw = malloc(sizeof(double) * S), *b = malloc(sizeof(double) * S);
    if (!alpha || !pis || !a || !nw || !b) return -1;
#define INC(k, s, u) (inc ? inc[((size_t)(k) * S + (s)) * M + (u)] : ca_inc(c, rot_cs, rows_ri, (k), first_call + (k), (s), (u)))
    for (int64_t j = 0; j < n * lg; ++j) pis[j] = prior ? scale * (double)prior[j] : 0.0;
    for (int s = 0; s < S; ++s) a[s] = 0.0;
    for (int64_t k = 0; k < n; ++k) {
        const double *pi = pis + (size_t)lg * k;
        for (int s = 0; s < S; ++s) { alpha[(size_t)k * S + s] = a[s]; nw[s] = INFINITY; }
        for (int s = 0; s < S; ++s)
            for (int u = 0; u < M; ++u) {
                const int e = ca_end(c, first_call + k, s, u);
                const double cand = a[s] + ca_incp(c, INC(k, s, u), pi, u);
                if (cand < nw[e]) nw[e] = cand;
            }
        double mn = nw[0];
        for (int s = 1; s < S; ++s) mn = nw[s] < mn ? nw[s] : mn;
        for (int s = 0; s < S; ++s) a[s] = nw[s] - mn;
    }
    for (int s = 0; s < S; ++s) b[s] = 0.0;
    for (int64_t k = n - 1; k >= 0; --k) {
        double m1[2] = {INFINITY, INFINITY}, m0[2] = {INFINITY, INFINITY};
        const double *ak = alpha + (size_t)k * S, *pi = pis + (size_t)lg * k;
        for (int s = 0; s < S; ++s) {
            nw[s] = INFINITY;
            for (int u = 0; u < M; ++u) {
                const int e = ca_end(c, first_call + k, s, u);
                const double x = INC(k, s, u);
                for (int i = 0; i < lg; ++i) {
                    const double t = (ak[s] + ca_x(c, x, pi, u, i)) + b[e];
                    if (bit_of(c, u, i)) { if (t < m1[i]) m1[i] = t; }
                    else if (t < m0[i]) m0[i] = t;
                }
                const double y = ca_incp(c, x, pi, u) + b[e];
                if (y < nw[s]) nw[s] = y;
            }
        }
        for (int i = 0; i < lg; ++i) {
            const double l = m1[i] - m0[i];
            ext[(size_t)lg * k + i] = l;
            bits[(size_t)lg * k + i] = l + pi[i] < 0.0 ? 1 : 0;
        }
        double mn = nw[0];
        for (int s = 1; s < S; ++s) mn = nw[s] < mn ? nw[s] : mn;
        for (int s = 0; s < S; ++s) b[s] = nw[s] - mn;
    }
#undef INC
    free(alpha); free(pis); free(a); free(nw); free(b);
    return 0;
}

/* increments given (inc[k][s][u]): what the brute-force test feeds */
int cpm_soft_apriori_rec(int M, int p, int nh, const int *K, int Lp, const double *inc, int64_t n, int64_t first_call, const float *prior,
                         double scale, double *ext, uint8_t *bits)
{
    ca_spec c;
    ca_init(&c, M, p, nh, K, Lp);
    return ca_run(&c, inc, NULL, NULL, n, first_call, prior, scale, ext, bits);
}

/* increments from the rotation table and the rows, as the entry point forms them */
int cpm_soft_apriori_rows(int M, int p, int nh, const int *K, int Lp, const double *rot_cs, const double *rows_ri, int64_t n,
                          int64_t first_call, const float *prior, double scale, double *ext, uint8_t *bits)
{
    ca_spec c;
    ca_init(&c, M, p, nh, K, Lp);
    return ca_run(&c, NULL, rot_cs, rows_ri, n, first_call, prior, scale, ext, bits);
}
