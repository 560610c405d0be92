/*
 * blockmatch_host.c -- host arithmetic of the intensity refinement: the default parameters, the
 * quantisation range, the node lattice, the output grid, the gates and samples from the kernel's integer words and the fold
 * count under a 4 x 4 transform.  Linked into libsift3d_hip.so (blockmatch_api.hip uses all of it) and into
 * libsift3d_host.so (no GPU needed).
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "sift3d.h"

void sift3d_blockmatch_defaults(sift3d_blockmatch_params *p)
{
    sift3d_field_params f;
    sift3d_field_defaults(&f);
    p->stride = 4;
    p->block = 4;
    p->search = 3;
    p->rounds = 2;
    p->variance_quantile = 0.25f;
    p->cost_fraction = 0.8f;
    p->spacing = f.spacing;
    p->radius = f.radius;
    p->lambda = f.lambda;
    p->min_tol = f.min_tol;
    p->max_nodes = f.max_nodes;
}

static int params_ok(const sift3d_blockmatch_params *p)
{
    return p && p->stride >= 1 && p->block >= 1 && p->block <= SIFT3D_BLOCKMATCH_MAX_B && p->search >= 1 && p->search <= SIFT3D_BLOCKMATCH_MAX_R &&
           p->rounds >= 0 && p->rounds <= SIFT3D_BLOCKMATCH_MAX_ROUNDS && p->variance_quantile >= 0 && p->variance_quantile < 1 &&
           p->cost_fraction > 0 && isfinite(p->cost_fraction) && p->spacing > 0 && isfinite(p->spacing) && p->radius > 0 && isfinite(p->radius) &&
           p->lambda >= 0 && isfinite(p->lambda) && p->min_tol >= 0 && isfinite(p->min_tol) && p->max_nodes >= 1;
}

int sift3d_blockmatch_range(const float *f, int64_t n, float *lo, float *hi)
{
    float a = 0, b = 0;
    int any = 0;
    for (int64_t i = 0; i < n; i++) {
        const float v = f[i];
        if (!isfinite(v)) continue;
        if (!any || v < a) a = v;
        if (!any || v > b) b = v;
        any = 1;
    }
    if (lo) *lo = a;
    if (hi) *hi = b;
    return any && b > a;
}

int sift3d_blockmatch_lattice(int64_t nx, int64_t ny, int64_t nz, const sift3d_blockmatch_params *p, int64_t first[3], int64_t count[3])
{
    if (!params_ok(p) || !first || !count) return -1;
    const int64_t n[3] = {nx, ny, nz}, m = (int64_t)p->block + p->search;
    for (int k = 0; k < 3; k++) {
        if (n[k] < 2 * m + 1) return -1;
        first[k] = m;
        count[k] = (n[k] - 1 - 2 * m) / p->stride + 1;
    }
    return 0;
}

static const float bm_eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

int sift3d_blockmatch_grid(int64_t nx, int64_t ny, int64_t nz, const float fixed_vox2key[16], const sift3d_blockmatch_params *p, sift3d_field *f)
{
    if (!params_ok(p) || !f || nx < 1 || ny < 1 || nz < 1) return SIFT3D_ERR_ARG;
    const float *c = fixed_vox2key ? fixed_vox2key : bm_eye;
    float y[24];
    for (int i = 0; i < 8; i++) {
        const float px = (i & 1) ? (float)(nx - 1) : 0.0f, py = (i & 2) ? (float)(ny - 1) : 0.0f, pz = (i & 4) ? (float)(nz - 1) : 0.0f;
        for (int r = 0; r < 3; r++) y[3 * i + r] = ((c[4 * r] * px + c[4 * r + 1] * py) + c[4 * r + 2] * pz) + c[4 * r + 3];
    }
    sift3d_field_params fp;
    sift3d_field_defaults(&fp);
    fp.spacing = p->spacing;
    fp.radius = p->radius;
    fp.lambda = p->lambda;
    fp.max_nodes = p->max_nodes;
    return sift3d_field_size(y, 8, &fp, f);
}

/* L = inverse of the linear part of m (4 x 4 row-major), by its adjugate in double; 0, or -1 where it is singular */
static int inverse_linear(const float m[16], double L[9])
{
    double a[9];
    for (int r = 0; r < 3; r++)
        for (int q = 0; q < 3; q++) a[3 * r + q] = m[4 * r + q];
    const double c0 = a[4] * a[8] - a[5] * a[7], c1 = a[5] * a[6] - a[3] * a[8], c2 = a[3] * a[7] - a[4] * a[6];
    const double det = a[0] * c0 + a[1] * c1 + a[2] * c2;
    if (!(det != 0) || !isfinite(det)) return -1;
    const double inv[9] = {c0, a[2] * a[7] - a[1] * a[8], a[1] * a[5] - a[2] * a[4],
                           c1, a[0] * a[8] - a[2] * a[6], a[2] * a[3] - a[0] * a[5],
                           c2, a[1] * a[6] - a[0] * a[7], a[0] * a[4] - a[1] * a[3]};
    for (int r = 0; r < 9; r++) L[r] = inv[r] / det;
    return 0;
}

static int by_i64(const void *a, const void *b)
{
    const int64_t u = *(const int64_t *)a, v = *(const int64_t *)b;
    return u < v ? -1 : (u > v ? 1 : 0);
}

int64_t sift3d_blockmatch_samples(const uint32_t *words, int64_t nx, int64_t ny, int64_t nz, const sift3d_blockmatch_params *p,
                                  const float fixed_vox2key[16], const float moving_to_fixed[16], const sift3d_field *in, float *y, float *v,
                                  int64_t counts[4])
{
    int64_t first[3], cnt[3];
    double L[9];
    if (!words || !y || !v || !moving_to_fixed || sift3d_blockmatch_lattice(nx, ny, nz, p, first, cnt) != 0 ||
        inverse_linear(moving_to_fixed, L) != 0)
        return -1;
    const float *c = fixed_vox2key ? fixed_vox2key : bm_eye;
    const int64_t N = cnt[0] * cnt[1] * cnt[2];
    const int64_t side = 2 * (int64_t)p->block + 1, vol = side * side * side;
    int64_t tally[4] = {0, 0, 0, 0};
    /* the variance threshold over the unflagged nodes */
    int64_t *var = (int64_t *)malloc(sizeof(int64_t) * (size_t)(N > 0 ? N : 1));
    if (!var) return -1;
    int64_t m = 0;
    for (int64_t i = 0; i < N; i++) {
        const uint32_t *w = words + SIFT3D_BLOCKMATCH_WORDS * i;
        if (!w[3]) var[m++] = vol * (int64_t)w[13] - (int64_t)w[12] * (int64_t)w[12];
    }
    int64_t thr = 0;
    if (m > 0) {
        qsort(var, (size_t)m, sizeof(int64_t), by_i64);
        int64_t at = (int64_t)floor((double)p->variance_quantile * (double)m);
        if (at > m - 1) at = m - 1;
        thr = var[at];
    }
    free(var);
    int64_t ns = 0;
    for (int64_t i = 0; i < N; i++) {
        const uint32_t *w = words + SIFT3D_BLOCKMATCH_WORDS * i;
        if (w[3]) {
            tally[0]++;
            continue;
        }
        if (!(vol * (int64_t)w[13] - (int64_t)w[12] * (int64_t)w[12] > thr)) {
            tally[1]++;
            continue;
        }
        const int32_t s[3] = {(int32_t)w[0], (int32_t)w[1], (int32_t)w[2]};
        if (abs(s[0]) >= p->search || abs(s[1]) >= p->search || abs(s[2]) >= p->search) {
            tally[2]++;
            continue;
        }
        if ((s[0] || s[1] || s[2]) && !((double)w[4] < (double)p->cost_fraction * (double)w[5])) {
            tally[3]++;
            continue;
        }
        double D[3];
        for (int k = 0; k < 3; k++) {
            const double cm = (double)w[6 + 2 * k], cp = (double)w[7 + 2 * k], c0 = (double)w[4];
            const double den = (cm - 2.0 * c0) + cp;
            D[k] = (double)s[k] + (den > 0 ? 0.5 * (cm - cp) / den : 0.0);
        }
        const int64_t a = i % cnt[0], b = (i / cnt[0]) % cnt[1], cc = i / (cnt[0] * cnt[1]);
        const double P[3] = {(double)(first[0] + a * p->stride), (double)(first[1] + b * p->stride), (double)(first[2] + cc * p->stride)};
        double ky[3], kd[3];
        float kf[3], vin[3] = {0, 0, 0};
        for (int r = 0; r < 3; r++) {
            ky[r] = (((double)c[4 * r] * P[0] + (double)c[4 * r + 1] * P[1]) + (double)c[4 * r + 2] * P[2]) + (double)c[4 * r + 3];
            kd[r] = ((double)c[4 * r] * D[0] + (double)c[4 * r + 1] * D[1]) + (double)c[4 * r + 2] * D[2];
            kf[r] = (float)(ky[r] + kd[r]);
        }
        if (in) sift3d_field_eval(in, kf, 1, vin);
        for (int r = 0; r < 3; r++) {
            y[3 * ns + r] = (float)ky[r];
            v[3 * ns + r] = (float)((double)vin[r] + ((L[3 * r] * kd[0] + L[3 * r + 1] * kd[1]) + L[3 * r + 2] * kd[2]));
        }
        ns++;
    }
    if (counts) memcpy(counts, tally, sizeof tally);
    return ns;
}

int64_t sift3d_blockmatch_folds(const float moving_to_fixed[16], const sift3d_field *f, double *max_disp)
{
    double L[9];
    if (!moving_to_fixed || !f || inverse_linear(moving_to_fixed, L) != 0) return -1;
    const int64_t n0 = f->n[0], n1 = f->n[1], n2 = f->n[2], N = n0 * n1 * n2;
    const double h2 = 2.0 * (double)f->spacing;
    int64_t folds = 0;
    double big = 0;
    for (int64_t c = 0; c < n2; c++)
        for (int64_t b = 0; b < n1; b++)
            for (int64_t a = 0; a < n0; a++) {
                const int64_t i = (c * n1 + b) * n0 + a;
                const int64_t at[3] = {a, b, c}, step[3] = {1, n0, n0 * n1}, top[3] = {n0, n1, n2};
                double J[9];
                for (int q = 0; q < 3; q++)
                    for (int r = 0; r < 3; r++) {
                        const double up = at[q] + 1 < top[q] ? (double)f->disp[r * N + i + step[q]] : 0.0;
                        const double dn = at[q] > 0 ? (double)f->disp[r * N + i - step[q]] : 0.0;
                        J[3 * r + q] = L[3 * r + q] + (up - dn) / h2;
                    }
                const double det = J[0] * (J[4] * J[8] - J[5] * J[7]) - J[1] * (J[3] * J[8] - J[5] * J[6]) + J[2] * (J[3] * J[7] - J[4] * J[6]);
                if (!(det > 0)) folds++;
                const double v0 = f->disp[i], v1 = f->disp[N + i], v2 = f->disp[2 * N + i];
                const double mg = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
                if (mg > big) big = mg;
            }
    if (max_disp) *max_disp = big;
    return folds;
}
