/*
 * field_host.c -- host arithmetic of the nonrigid alignment: the default parameters, the node grid
 * of a sample set, the samples of accepted pairs, the terms of the warp, the interpolation of a field at key positions and
 * its fold count.  Linked into libsift3d_hip.so (field_api.hip uses all of it) and into libsift3d_host.so (no GPU needed).
 */
#include <math.h>
#include <string.h>

#include "sift3d.h"

void sift3d_field_defaults(sift3d_field_params *p)
{
    p->spacing = 4.0f;
    p->radius = 20.0f;
    p->lambda = 0.1f;
    p->search_radius = 8.0f;
    p->min_tol = 1.0f;
    p->ratio_num = 4;
    p->ratio_den = 5;
    p->max_nodes = (int64_t)1 << 26;
    p->index_cells_max = (int64_t)1 << 26;
}

static int finite3(const float *a) { return isfinite(a[0]) && isfinite(a[1]) && isfinite(a[2]); }

int sift3d_field_size(const float *y, int64_t n, const sift3d_field_params *p, sift3d_field *f)
{
    if (!p || !f || n < 0 || (n > 0 && !y)) return SIFT3D_ERR_ARG;
    const float h = p->spacing, R = p->radius;
    if (!(h > 0) || !isfinite(h) || !(R > 0) || !isfinite(R) || !(p->lambda >= 0) || !isfinite(p->lambda) || p->max_nodes < 1) return SIFT3D_ERR_ARG;
    double mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
    int any = 0;
    for (int64_t i = 0; i < n; i++) {
        if (!finite3(y + 3 * i)) continue;
        for (int k = 0; k < 3; k++) {
            const double v = y[3 * i + k];
            if (!any || v < mn[k]) mn[k] = v;
            if (!any || v > mx[k]) mx[k] = v;
        }
        any = 1;
    }
    double total = 1;
    for (int k = 0; k < 3; k++) {
        const double c = floor((mx[k] - mn[k] + 2.0 * (double)R) / (double)h) + 2.0;
        if (!(c <= (double)(1 << 24))) return SIFT3D_ERR_ARG;
        f->n[k] = (int64_t)c;
        f->origin[k] = (float)(mn[k] - (double)R);
        total *= c;
    }
    f->spacing = h;
    return total <= (double)p->max_nodes ? SIFT3D_OK : SIFT3D_ERR_ARG;
}

/* T^-1(y) = c0 + rot^T (y - c1) / scale in double */
static void inverse_point(const sift3d_similarity *t, const float y[3], double out[3])
{
    double d[3];
    for (int k = 0; k < 3; k++) d[k] = (double)y[k] - (double)t->center1[k];
    for (int r = 0; r < 3; r++) {
        const double o = ((double)t->rot[r] * d[0] + (double)t->rot[3 + r] * d[1]) + (double)t->rot[6 + r] * d[2];
        out[r] = (double)t->center0[r] + o / (double)t->scale;
    }
}

void sift3d_field_samples(const sift3d_similarity *t, const float *pf, const float *pm, int64_t n, float *y, float *v)
{
    for (int64_t i = 0; i < n; i++) {
        double q[3];
        inverse_point(t, pf + 3 * i, q);
        for (int k = 0; k < 3; k++) {
            y[3 * i + k] = pf[3 * i + k];
            v[3 * i + k] = (float)((double)pm[3 * i + k] - q[k]);
        }
    }
}

int sift3d_field_warp_terms(const float fv[16], const float mv[16], float c[12], float k[9])
{
    static const float eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const float *F = fv ? fv : eye, *M = mv ? mv : eye;
    if (F[12] != 0 || F[13] != 0 || F[14] != 0 || F[15] != 1 || M[12] != 0 || M[13] != 0 || M[14] != 0 || M[15] != 1) return -1;
    for (int r = 0; r < 12; r++) c[r] = F[r];
    /* the inverse of the linear part by its adjugate, in double */
    double a[9];
    for (int r = 0; r < 3; r++)
        for (int q = 0; q < 3; q++) a[3 * r + q] = M[4 * r + q];
    const double c0 = a[4] * a[8] - a[5] * a[7], c1 = a[5] * a[6] - a[3] * a[8], c2 = a[3] * a[7] - a[4] * a[6];
    const double det = a[0] * c0 + a[1] * c1 + a[2] * c2;
    if (!(det != 0) || !isfinite(det)) return -1;
    const double inv[9] = {c0, a[2] * a[7] - a[1] * a[8], a[1] * a[5] - a[2] * a[4],
                           c1, a[0] * a[8] - a[2] * a[6], a[2] * a[3] - a[0] * a[5],
                           c2, a[1] * a[6] - a[0] * a[7], a[0] * a[4] - a[1] * a[3]};
    for (int r = 0; r < 9; r++) k[r] = (float)(inv[r] / det);
    return 0;
}

/* the interpolation at grid coordinates g (inside the grid): section 7c's floor, weights, clamp and x -> y -> z order */
static void interp(const sift3d_field *f, const float g[3], float out[3])
{
    int64_t lo[3], hi[3];
    float w[3];
    for (int r = 0; r < 3; r++) {
        const float fl = floorf(g[r]);
        w[r] = g[r] - fl;
        lo[r] = (int64_t)fl;
        hi[r] = lo[r] + 1 <= f->n[r] - 1 ? lo[r] + 1 : f->n[r] - 1;
    }
    const int64_t n0 = f->n[0], n1 = f->n[1], N = n0 * n1 * f->n[2];
#define AT(c, x, y, z) f->disp[(c) * N + ((z) * n1 + (y)) * n0 + (x)]
    for (int c = 0; c < 3; c++) {
        const float u0 = 1.0f - w[0], u1 = 1.0f - w[1], u2 = 1.0f - w[2];
        const float e00 = u0 * AT(c, lo[0], lo[1], lo[2]) + w[0] * AT(c, hi[0], lo[1], lo[2]);
        const float e10 = u0 * AT(c, lo[0], hi[1], lo[2]) + w[0] * AT(c, hi[0], hi[1], lo[2]);
        const float e01 = u0 * AT(c, lo[0], lo[1], hi[2]) + w[0] * AT(c, hi[0], lo[1], hi[2]);
        const float e11 = u0 * AT(c, lo[0], hi[1], hi[2]) + w[0] * AT(c, hi[0], hi[1], hi[2]);
        const float a = u1 * e00 + w[1] * e10, b = u1 * e01 + w[1] * e11;
        out[c] = u2 * a + w[2] * b;
    }
#undef AT
}

void sift3d_field_eval(const sift3d_field *f, const float *y, int64_t n, float *out)
{
    for (int64_t i = 0; i < n; i++) {
        float g[3];
        int inside = 1;
        for (int r = 0; r < 3; r++) {
            g[r] = (y[3 * i + r] - f->origin[r]) / f->spacing;
            inside &= g[r] >= 0.0f && g[r] <= (float)(f->n[r] - 1);
        }
        if (inside) interp(f, g, out + 3 * i);
        else out[3 * i] = out[3 * i + 1] = out[3 * i + 2] = 0.0f;
    }
}

int64_t sift3d_field_folds(const sift3d_similarity *t, const sift3d_field *f, double *max_disp)
{
    const int64_t n0 = f->n[0], n1 = f->n[1], n2 = f->n[2], N = n0 * n1 * n2;
    const double h2 = 2.0 * (double)f->spacing, s = (double)t->scale;
    int64_t folds = 0;
    double big = 0;
    for (int64_t c = 0; c < n2; c++)
        for (int64_t b = 0; b < n1; b++)
            for (int64_t a = 0; a < n0; a++) {
                const int64_t i = (c * n1 + b) * n0 + a;
                const int64_t at[3] = {a, b, c}, step[3] = {1, n0, n0 * n1}, top[3] = {n0, n1, n2};
                double J[9];
                for (int q = 0; q < 3; q++) /* column q: d phi / d y_q */
                    for (int r = 0; r < 3; r++) {
                        const double up = at[q] + 1 < top[q] ? (double)f->disp[r * N + i + step[q]] : 0.0;
                        const double dn = at[q] > 0 ? (double)f->disp[r * N + i - step[q]] : 0.0;
                        J[3 * r + q] = (double)t->rot[3 * q + r] / s + (up - dn) / h2;
                    }
                const double det = J[0] * (J[4] * J[8] - J[5] * J[7]) - J[1] * (J[3] * J[8] - J[5] * J[6]) + J[2] * (J[3] * J[7] - J[4] * J[6]);
                if (!(det > 0)) folds++;
                const double v0 = f->disp[i], v1 = f->disp[N + i], v2 = f->disp[2 * N + i];
                const double m = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
                if (m > big) big = m;
            }
    if (max_disp) *max_disp = big;
    return folds;
}
