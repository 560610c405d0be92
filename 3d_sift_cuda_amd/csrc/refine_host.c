/*
 * refine_host.c -- host arithmetic of the guided re-matching: the least-squares similarity of
 * Umeyama (1991) over point pairs and the loop's default parameters.  Linked into libsift3d_hip.so (the loop in
 * refine_api.hip fits through it) and into libsift3d_host.so (no GPU needed).
 *
 * Everything is double until the result: centroids and the cross-covariance as sums in pair order, the 3 x 3 SVD by
 * one-sided Jacobi sweeps (Hestenes) with a fixed convergence rule, det R = +1 forced by the sign of the last singular
 * direction, then one rounding to float.
 */
#include <math.h>
#include <string.h>

#include "sift3d.h"

void sift3d_refine_defaults(sift3d_refine_params *p)
{
    p->max_rounds = 3;
    p->min_radius = 1.0f;
    p->max_radius = 16.0f;
    p->ratio_num = 4;
    p->ratio_den = 5;
    p->stop_shift = 0.01f;
    p->index_cells_max = (int64_t)1 << 26;
}

/* One-sided Jacobi on the columns of a (3 x 3, row-major): on return a = U diag(sv) (columns orthogonal) and v the
 * accumulated rotation, so that a_in = a v^T.  A pair of columns is rotated while |a_p . a_q| > 1e-15 sqrt(|a_p|^2 |a_q|^2);
 * at most 64 sweeps. */
static void jacobi3(double a[9], double v[9])
{
    for (int k = 0; k < 9; k++) v[k] = k % 4 == 0 ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 64; sweep++) {
        int rotated = 0;
        for (int p = 0; p < 2; p++)
            for (int q = p + 1; q < 3; q++) {
                double al = 0, be = 0, ga = 0;
                for (int r = 0; r < 3; r++) {
                    al += a[3 * r + p] * a[3 * r + p];
                    be += a[3 * r + q] * a[3 * r + q];
                    ga += a[3 * r + p] * a[3 * r + q];
                }
                if (!(fabs(ga) > 1e-15 * sqrt(al * be))) continue;
                rotated = 1;
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                for (int r = 0; r < 3; r++) {
                    const double x = a[3 * r + p], y = a[3 * r + q];
                    a[3 * r + p] = c * x - s * y;
                    a[3 * r + q] = s * x + c * y;
                    const double vx = v[3 * r + p], vy = v[3 * r + q];
                    v[3 * r + p] = c * vx - s * vy;
                    v[3 * r + q] = s * vx + c * vy;
                }
            }
        if (!rotated) break;
    }
}

static double det3(const double m[9])
{
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

int sift3d_fit_similarity(const float *pm, const float *pf, int64_t n, sift3d_similarity *out)
{
    if (n < 3 || !pm || !pf || !out) return -1;
    double mu_m[3] = {0, 0, 0}, mu_f[3] = {0, 0, 0};
    for (int64_t i = 0; i < n; i++)
        for (int c = 0; c < 3; c++) {
            if (!isfinite(pm[3 * i + c]) || !isfinite(pf[3 * i + c])) return -1;
            mu_m[c] += pm[3 * i + c];
            mu_f[c] += pf[3 * i + c];
        }
    for (int c = 0; c < 3; c++) {
        mu_m[c] /= (double)n;
        mu_f[c] /= (double)n;
    }
    /* cov[r][c] = mean (f - mu_f)_r (m - mu_m)_c; var_m = mean |m - mu_m|^2 */
    double cov[9] = {0}, var_m = 0;
    for (int64_t i = 0; i < n; i++) {
        double dm[3], df[3];
        for (int c = 0; c < 3; c++) {
            dm[c] = (double)pm[3 * i + c] - mu_m[c];
            df[c] = (double)pf[3 * i + c] - mu_f[c];
        }
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) cov[3 * r + c] += df[r] * dm[c];
        var_m += dm[0] * dm[0] + dm[1] * dm[1] + dm[2] * dm[2];
    }
    for (int k = 0; k < 9; k++) cov[k] /= (double)n;
    var_m /= (double)n;
    if (!(var_m > 0)) return -1;
    double a[9], v[9], u[9], sv[3];
    memcpy(a, cov, sizeof a);
    jacobi3(a, v);
    for (int c = 0; c < 3; c++) sv[c] = sqrt(a[c] * a[c] + a[3 + c] * a[3 + c] + a[6 + c] * a[6 + c]);
    /* order the singular values descending (columns of a and v with them) */
    int ord[3] = {0, 1, 2};
    for (int i = 0; i < 3; i++)
        for (int j = i + 1; j < 3; j++)
            if (sv[ord[j]] > sv[ord[i]]) {
                const int t = ord[i];
                ord[i] = ord[j];
                ord[j] = t;
            }
    double s[3], us[9], vs[9];
    for (int k = 0; k < 3; k++) {
        s[k] = sv[ord[k]];
        for (int r = 0; r < 3; r++) {
            us[3 * r + k] = a[3 * r + ord[k]];
            vs[3 * r + k] = v[3 * r + ord[k]];
        }
    }
    /* rank < 2: the centred points are collinear (or coincide) on one side */
    if (!(s[0] > 0) || !(s[1] > 1e-12 * s[0])) return -1;
    for (int k = 0; k < 2; k++)
        for (int r = 0; r < 3; r++) u[3 * r + k] = us[3 * r + k] / s[k];
    if (s[2] > 1e-12 * s[0]) {
        for (int r = 0; r < 3; r++) u[3 * r + 2] = us[3 * r + 2] / s[2];
    } else { /* a planar set: the third direction is free; complete U to a right-handed frame */
        u[2] = u[3] * u[7] - u[6] * u[4];
        u[5] = u[6] * u[1] - u[0] * u[7];
        u[8] = u[0] * u[4] - u[3] * u[1];
    }
    const double d = det3(u) * det3(vs) < 0 ? -1.0 : 1.0;
    /* R = U diag(1, 1, d) V^T; scale = (s0 + s1 + d s2) / var_m; t = mu_f - scale R mu_m */
    double R[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) R[3 * r + c] = u[3 * r] * vs[3 * c] + u[3 * r + 1] * vs[3 * c + 1] + d * u[3 * r + 2] * vs[3 * c + 2];
    const double scale = (s[0] + s[1] + d * s[2]) / var_m;
    if (!(scale > 0) || !isfinite(scale)) return -1;
    double t[3], c1[3];
    for (int r = 0; r < 3; r++) {
        t[r] = mu_f[r] - scale * (R[3 * r] * mu_m[0] + R[3 * r + 1] * mu_m[1] + R[3 * r + 2] * mu_m[2]);
        c1[r] = scale * (R[3 * r] * out->center0[0] + R[3 * r + 1] * out->center0[1] + R[3 * r + 2] * out->center0[2]) + t[r];
    }
    out->scale = (float)scale;
    for (int k = 0; k < 9; k++) out->rot[k] = (float)R[k];
    for (int r = 0; r < 3; r++) {
        out->trans[r] = (float)t[r];
        out->center1[r] = (float)c1[r];
    }
    return 0;
}
