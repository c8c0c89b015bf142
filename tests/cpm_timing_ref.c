/* The definition of wf_cpm_mf_rows_resample_c128 (include/wfhip.h) restated sequentially, every fused multiply-add an explicit
 * fma(): compiled with -ffp-contract=off, the device's rows equal these bit for bit. */
#include <math.h>
#include <stdint.h>

static void lagrange(double mu, double c[4])
{
    const double p1 = mu + 1.0, m1 = mu - 1.0, m2 = mu - 2.0;
    c[0] = -(mu * m1 * m2) / 6.0;
    c[1] = (p1 * m1 * m2) / 2.0;
    c[2] = -(p1 * mu * m2) / 2.0;
    c[3] = (p1 * mu * m1) / 6.0;
}

/* τ_n: linear between the window centres w W + (W - 1) / 2, flat outside the first and the last; each operation rounded once */
static double tau_at(const double *tau, int64_t nwin, int W, int64_t n)
{
    const double c0 = 0.5 * (double)(W - 1);
    const double tt = ((double)n - c0) / (double)W;
    if (tt <= 0.0) return tau[0];
    if (tt >= (double)(nwin - 1)) return tau[nwin - 1];
    const double fl = floor(tt);
    const int64_t w = (int64_t)fl;
    const double f = tt - fl;
    const double p0 = tau[w];
    const double d = tau[w + 1] - p0;
    const double fd = f * d;
    return p0 + fd;
}

static double sample(const double *r_ri, int64_t nsamp, int64_t g, int part) { return (g >= 0 && g < nsamp) ? r_ri[2 * g + part] : 0.0; }

int cpm_mf_rows_resample_ref(const double *r_ri, int64_t nsamp, const double *templ_ri, int nh, int nfilt, int ntm, int64_t start0, int sps,
                             int64_t ncalls, int W, const double *tau, int64_t nwin, double tau0, double *out_ri)
{
    if (ntm > 512) return 1;
    double xr[512], xi[512];
    for (int64_t n = 0; n < ncalls; ++n) {
        double t = tau0;
        if (tau) {
            const double phi = tau_at(tau, nwin, W, n);
            t = tau0 + phi;
        }
        double *o = out_ri + 2 * n * nfilt;
        if (!(fabs(t) < 4611686018427387904.0)) {
            for (int f = 0; f < 2 * nfilt; ++f) o[f] = 0.0;
            continue;
        }
        const double fl = floor(t);
        const double mu = t - fl;
        const int64_t B = start0 + n * sps + (int64_t)fl;
        double c[4];
        lagrange(mu, c);
        for (int k = 0; k < ntm; ++k) {
            const int64_t g = B + k;
            xr[k] = fma(c[3], sample(r_ri, nsamp, g + 2, 0), fma(c[2], sample(r_ri, nsamp, g + 1, 0), fma(c[1], sample(r_ri, nsamp, g, 0), c[0] * sample(r_ri, nsamp, g - 1, 0))));
            xi[k] = fma(c[3], sample(r_ri, nsamp, g + 2, 1), fma(c[2], sample(r_ri, nsamp, g + 1, 1), fma(c[1], sample(r_ri, nsamp, g, 1), c[0] * sample(r_ri, nsamp, g - 1, 1))));
        }
        const double *T = templ_ri + 2 * ((n % nh) * nfilt) * ntm;
        for (int f = 0; f < nfilt; ++f) {
            double zr = 0.0, zi = 0.0;
            for (int k = 0; k < ntm; ++k) {
                const double tr = T[2 * (f * ntm + k)], ti = T[2 * (f * ntm + k) + 1];
                zr = fma(xr[k], tr, fma(xi[k], ti, zr));
                zi = fma(-xr[k], ti, fma(xi[k], tr, zi));
            }
            o[2 * f] = zr;
            o[2 * f + 1] = zi;
        }
    }
    return 0;
}
