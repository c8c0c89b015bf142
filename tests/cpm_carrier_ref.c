/* cpm_carrier_ref.c — the definition of wf_cpm_soft_branch (include/wfhip.h), restated sequentially for
 * tests/test_cpm_carrier.py: the recursion of cpm_soft_ref.c with, per call, the branch b* = M s + u of the smallest
 * T_k(s,u) = (ã_k(s) + inc_k(s,u)) + b̃_{k+1}(e(s,u)) — the first one in the order s, then u, so ties go to the smallest b —
 * and the components (x, y) of q_k on it.  Compiled with gcc -O2 -ffp-contract=off, as cpm_soft_ref.c is. */
#include "cpm_soft_ref.c"

/* y of q = -Z[f] e^{-j φ_r} on branch (s, u) of call k (global call n); x is cs_inc */
static double cs_quad(const cs_spec *c, const double *rot_cs, const double *rows_ri, int64_t k, int64_t n, int s, int u)
{
    const int v = s % c->p, corr = s / c->p;
    const int r = imod(2 * (int64_t)v - cs_tilt(c, n), 2 * c->p);
    const double *Z = rows_ri + (size_t)2 * k * c->NF;
    const int f = u + c->M * corr;
    return -fma(rot_cs[2 * r], Z[2 * f + 1], -(rot_cs[2 * r + 1] * Z[2 * f]));
}

/* inc != NULL: increments given as inc[k][s][u] (no term); else computed from rot_cs and rows.  term may be NULL. */
static int csb_run(const cs_spec *c, const double *inc, const double *rot_cs, const double *rows_ri, int64_t n, int64_t first_call,
                   double *llr, uint8_t *bits, uint8_t *branch, double *term)
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
        double tbest = INFINITY, xbest = 0.0;
        int sbest = 0, ubest = 0;
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
                if (t < tbest) { tbest = t; sbest = s; ubest = u; xbest = x; }
                const double y = x + b[e];
                if (y < nw[s]) nw[s] = y;
            }
        }
        for (int i = 0; i < lg; ++i) {
            llr[(size_t)lg * k + i] = m1[i] - m0[i];
            bits[(size_t)lg * k + i] = m1[i] - m0[i] < 0.0 ? 1 : 0;
        }
        branch[k] = (uint8_t)(M * sbest + ubest);
        if (term) {
            term[2 * k] = xbest;
            term[2 * k + 1] = inc ? 0.0 : cs_quad(c, rot_cs, rows_ri, k, first_call + k, sbest, ubest);
        }
        double mn = nw[0];
        for (int s = 1; s < S; ++s) mn = nw[s] < mn ? nw[s] : mn;
        for (int s = 0; s < S; ++s) b[s] = nw[s] - mn;
    }
#undef INC
    free(alpha); free(a); free(nw); free(b);
    return 0;
}

int cpm_soft_branch_rec(int M, int p, int nh, const int *K, int Lp, const double *inc, int64_t n, int64_t first_call, double *llr, uint8_t *bits,
                        uint8_t *branch)
{
    cs_spec c;
    cs_init(&c, M, p, nh, K, Lp);
    return csb_run(&c, inc, NULL, NULL, n, first_call, llr, bits, branch, NULL);
}

int cpm_soft_branch_rows(int M, int p, int nh, const int *K, int Lp, const double *rot_cs, const double *rows_ri, int64_t n, int64_t first_call,
                         double *llr, uint8_t *bits, uint8_t *branch, double *term)
{
    cs_spec c;
    cs_init(&c, M, p, nh, K, Lp);
    return csb_run(&c, NULL, rot_cs, rows_ri, n, first_call, llr, bits, branch, term);
}
