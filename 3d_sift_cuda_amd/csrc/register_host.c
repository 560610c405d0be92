/*
 * register_host.c -- host side of the affine registration by mutual information: the default parameters and
 * their check, the transform family theta -> map and theta -> result, the candidates of one iteration, the lattice and its units,
 * and the report as text.  One stated sequence of double operations, built with -ffp-contract=off; tests/register_oracle.c
 * restates it with the same libm calls in the same order.  Linked into libsift3d_hip.so (register_api.hip uses it) and into
 * libsift3d_host.so (no GPU needed).
 */
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "sift3d.h"

void sift3d_register_defaults(sift3d_register_params *p)
{
    static const int32_t stride[SIFT3D_REGISTER_MAX_LEVELS] = {4, 2, 1, 1};
    static const double first[SIFT3D_REGISTER_MAX_LEVELS] = {4.0, 1.0, 0.25, 0.0625}, last[SIFT3D_REGISTER_MAX_LEVELS] = {1.0, 0.25, 0.0625, 0.0625};
    memset(p, 0, sizeof *p);
    p->dof = 12;
    p->metric = SIFT3D_REGISTER_METRIC_NMI;
    p->bins = 32;
    p->n_levels = 3;
    for (int l = 0; l < SIFT3D_REGISTER_MAX_LEVELS; l++) {
        p->stride[l] = stride[l];
        p->first_step[l] = first[l];
        p->last_step[l] = last[l];
    }
    p->max_iterations = 200;
    p->device = 0;
    p->form = SIFT3D_REGISTER_FORM_DEFAULT;
    p->min_overlap = 0.25;
}

__attribute__((format(printf, 3, 4))) static int refuse(char *err, int64_t err_len, const char *fmt, ...)
{
    if (err && err_len > 0) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, (size_t)err_len, fmt, ap);
        va_end(ap);
    }
    return -1;
}

static int stride_ok(int32_t s) { return s == 1 || s == 2 || s == 4 || s == 8; }

/* the number of active parameters, 0 for a dof that is none of the five */
static int active_of(int32_t dof, int idx[SIFT3D_REGISTER_THETA])
{
    if (dof != 3 && dof != 6 && dof != 7 && dof != 9 && dof != 12) return 0;
    int n = 0;
    for (int k = 0; k < (dof == 7 ? 7 : dof); k++) idx[n++] = k; /* 7: index 6 stands for the shared scale */
    return n;
}

int sift3d_register_check(const sift3d_register_params *p, char *err, int64_t err_len)
{
    int idx[SIFT3D_REGISTER_THETA];
    if (!p) return refuse(err, err_len, "null pointer");
    if (active_of(p->dof, idx) == 0) return refuse(err, err_len, "dof = %d: 3, 6, 7, 9 or 12", (int)p->dof);
    if (p->metric != SIFT3D_REGISTER_METRIC_MI && p->metric != SIFT3D_REGISTER_METRIC_NMI) return refuse(err, err_len, "metric = %d: 0 (mi) or 1 (nmi)", (int)p->metric);
    if (p->bins != 8 && p->bins != 16 && p->bins != 32 && p->bins != 64) return refuse(err, err_len, "bins = %d: 8, 16, 32 or 64", (int)p->bins);
    if (p->n_levels < 1 || p->n_levels > SIFT3D_REGISTER_MAX_LEVELS) return refuse(err, err_len, "n_levels = %d: 1 .. %d", (int)p->n_levels, SIFT3D_REGISTER_MAX_LEVELS);
    for (int l = 0; l < p->n_levels; l++) {
        if (!stride_ok(p->stride[l])) return refuse(err, err_len, "stride[%d] = %d: 1, 2, 4 or 8", l, (int)p->stride[l]);
        if (!(isfinite(p->first_step[l]) && p->first_step[l] > 0.0)) return refuse(err, err_len, "first_step[%d] = %g: finite and above 0", l, p->first_step[l]);
        if (!(p->last_step[l] > 0.0 && p->last_step[l] <= p->first_step[l]))
            return refuse(err, err_len, "last_step[%d] = %g: above 0 and at most first_step = %g", l, p->last_step[l], p->first_step[l]);
    }
    if (p->max_iterations < 1) return refuse(err, err_len, "max_iterations = %d: at least 1", (int)p->max_iterations);
    if (!(p->min_overlap >= 0.0 && p->min_overlap <= 1.0)) return refuse(err, err_len, "min_overlap = %g: 0 .. 1", p->min_overlap);
    if (p->form != SIFT3D_REGISTER_FORM_DEFAULT && (p->form < 0 || p->form > (SIFT3D_REGISTER_FORM_BY_MAP | SIFT3D_REGISTER_FORM_PLANE)))
        return refuse(err, err_len, "form = %d: -1 or 0 .. 3", (int)p->form);
    return 0;
}

/* ---- 4 x 4 arithmetic: sift3d_resample_map's (align_host.c), restated because those functions are that file's own ---- */
static int affine_inverse(const double a[16], double o[16])
{
    if (a[12] != 0.0 || a[13] != 0.0 || a[14] != 0.0 || a[15] != 1.0) return -1;
    const double c00 = a[5] * a[10] - a[6] * a[9], c01 = a[6] * a[8] - a[4] * a[10], c02 = a[4] * a[9] - a[5] * a[8];
    const double det = a[0] * c00 + a[1] * c01 + a[2] * c02;
    if (!(det != 0.0) || !isfinite(det)) return -1;
    const double inv[9] = {c00, a[2] * a[9] - a[1] * a[10], a[1] * a[6] - a[2] * a[5],
                           c01, a[0] * a[10] - a[2] * a[8], a[2] * a[4] - a[0] * a[6],
                           c02, a[1] * a[8] - a[0] * a[9], a[0] * a[5] - a[1] * a[4]};
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) o[4 * r + c] = inv[3 * r + c] / det;
        o[4 * r + 3] = -(o[4 * r] * a[3] + o[4 * r + 1] * a[7] + o[4 * r + 2] * a[11]);
        if (!isfinite(o[4 * r]) || !isfinite(o[4 * r + 1]) || !isfinite(o[4 * r + 2]) || !isfinite(o[4 * r + 3])) return -1;
    }
    o[12] = o[13] = o[14] = 0.0;
    o[15] = 1.0;
    return 0;
}

static void mul44(const double a[16], const double b[16], double o[16])
{
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) o[4 * r + c] = a[4 * r] * b[c] + a[4 * r + 1] * b[4 + c] + a[4 * r + 2] * b[8 + c] + a[4 * r + 3] * b[12 + c];
}

static void load44(const float *m, double o[16])
{
    for (int k = 0; k < 16; k++) o[k] = m ? (double)m[k] : (k % 5 == 0 ? 1.0 : 0.0);
}

static void mul33(const double a[9], const double b[9], double o[9])
{
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) o[3 * r + c] = (a[3 * r] * b[c] + a[3 * r + 1] * b[3 + c]) + a[3 * r + 2] * b[6 + c];
}

/* D(theta) about the centre of the fixed volume, as include/sift3d.h states it */
static void theta_matrix(const double *th, int64_t nx, int64_t ny, int64_t nz, const double fv[16], double d[16])
{
    const double *t = th, *r = th + 3, *s = th + 6, *g = th + 9;
    const double ctr[3] = {(double)(nx - 1) / 2.0, (double)(ny - 1) / 2.0, (double)(nz - 1) / 2.0};
    double c[3];
    for (int i = 0; i < 3; i++) c[i] = ((fv[4 * i] * ctr[0] + fv[4 * i + 1] * ctr[1]) + fv[4 * i + 2] * ctr[2]) + fv[4 * i + 3];
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const double a = sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
    if (a > 0.0) {
        const double K[9] = {0.0, -r[2], r[1], r[2], 0.0, -r[0], -r[1], r[0], 0.0};
        double KK[9];
        mul33(K, K, KK);
        const double A = sin(a) / a, B = (1.0 - cos(a)) / (a * a);
        for (int k = 0; k < 9; k++) R[k] = (R[k] + A * K[k]) + B * KK[k];
    }
    const double G[9] = {1.0, g[0], g[1], 0.0, 1.0, g[2], 0.0, 0.0, 1.0};
    const double e[3] = {exp(s[0]), exp(s[1]), exp(s[2])};
    double RG[9];
    mul33(R, G, RG);
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) d[4 * i + j] = RG[3 * i + j] * e[j];
        d[4 * i + 3] = (c[i] - ((d[4 * i] * c[0] + d[4 * i + 1] * c[1]) + d[4 * i + 2] * c[2])) + t[i];
    }
    d[12] = d[13] = d[14] = 0.0;
    d[15] = 1.0;
}

int sift3d_register_map(const double theta[SIFT3D_REGISTER_THETA], int64_t nx, int64_t ny, int64_t nz, const float fixed_vox2key[16],
                        const float moving_vox2key[16], const float initial[16], float map[12])
{
    double t[16], fv[16], mv[16], ti[16], mvi[16], d[16], e[16], p[16], a[16];
    if (!theta || !map) return -1;
    load44(initial, t);
    load44(fixed_vox2key, fv);
    load44(moving_vox2key, mv);
    if (affine_inverse(t, ti) != 0 || affine_inverse(mv, mvi) != 0 || affine_inverse(fv, p) != 0) return -1; /* p: scratch */
    theta_matrix(theta, nx, ny, nz, fv, d);
    mul44(d, fv, e);
    mul44(ti, e, p);
    mul44(mvi, p, a);
    for (int k = 0; k < 12; k++) {
        if (!isfinite(a[k])) return -1;
        map[k] = (float)a[k];
    }
    return 0;
}

int sift3d_register_result(const double theta[SIFT3D_REGISTER_THETA], int64_t nx, int64_t ny, int64_t nz, const float fixed_vox2key[16],
                           const float initial[16], float result[16])
{
    double t[16], fv[16], d[16], di[16], m[16];
    if (!theta || !result) return -1;
    load44(initial, t);
    load44(fixed_vox2key, fv);
    if (t[12] != 0.0 || t[13] != 0.0 || t[14] != 0.0 || t[15] != 1.0) return -1;
    theta_matrix(theta, nx, ny, nz, fv, d);
    if (affine_inverse(d, di) != 0) return -1;
    mul44(di, t, m);
    for (int k = 0; k < 12; k++)
        if (!isfinite(m[k])) return -1;
    for (int k = 0; k < 16; k++) result[k] = (float)m[k];
    return 0;
}

int sift3d_register_candidates(const double theta[SIFT3D_REGISTER_THETA], int32_t dof, double u, double rho, double *cand)
{
    int idx[SIFT3D_REGISTER_THETA];
    const int n = active_of(dof, idx);
    if (n == 0 || !theta || !cand) return -1;
    for (int k = 0; k < n; k++) {
        const double step = idx[k] < 3 ? u : u / rho;
        for (int sign = 0; sign < 2; sign++) {
            double *c = cand + (size_t)(2 * k + sign) * SIFT3D_REGISTER_THETA;
            memcpy(c, theta, sizeof(double) * SIFT3D_REGISTER_THETA);
            const double v = sign == 0 ? theta[idx[k]] + step : theta[idx[k]] - step;
            c[idx[k]] = v;
            if (dof == 7 && idx[k] == 6) c[7] = c[8] = v; /* the shared scale */
        }
    }
    return 2 * n;
}

int64_t sift3d_register_lattice(int64_t nx, int64_t ny, int64_t nz, int32_t stride, const float fixed_vox2key[16], int64_t n[3], double *h, double *rho)
{
    if (nx < 1 || ny < 1 || nz < 1 || !stride_ok(stride)) return -1;
    const int64_t ext[3] = {nx, ny, nz};
    int64_t count = 1;
    double fv[16], least = 0.0, edge = 0.0;
    load44(fixed_vox2key, fv);
    for (int a = 0; a < 3; a++) {
        const int64_t pts = (ext[a] - 1) / stride + 1;
        if (n) n[a] = pts;
        count *= pts;
        const double col = sqrt((fv[a] * fv[a] + fv[4 + a] * fv[4 + a]) + fv[8 + a] * fv[8 + a]);
        if (!(col > 0.0) || !isfinite(col)) return -1;
        if (a == 0 || col < least) least = col;
        const double e = (double)(ext[a] - 1) * col;
        if (e > edge) edge = e;
    }
    if (h) *h = least;
    if (rho) *rho = edge > 0.0 ? edge / 2.0 : least / 2.0;
    return count;
}

/* appends to buf[at ..) what fits, returns the position the whole text has reached */
__attribute__((format(printf, 4, 5))) static int64_t put(char *buf, int64_t len, int64_t at, const char *fmt, ...)
{
    char line[320];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(line, sizeof line, fmt, ap);
    va_end(ap);
    const int64_t n = (int64_t)strlen(line);
    for (int64_t i = 0; i < n; i++)
        if (buf && at + i < len - 1) buf[at + i] = line[i];
    return at + n;
}

static int64_t put_double(char *buf, int64_t len, int64_t at, double v, const char *after)
{
    if (isnan(v)) return put(buf, len, at, "nan%s", after);
    return put(buf, len, at, "%.12g%s", v, after);
}

static int64_t put_record(char *buf, int64_t len, int64_t at, const char *name, const sift3d_similarity_record *r, int64_t outside)
{
    at = put(buf, len, at, "%s %lld %lld %lld ", name, (long long)r->sums[0], (long long)r->excluded, (long long)outside);
    at = put_double(buf, len, at, r->mi, " ");
    at = put_double(buf, len, at, r->nmi, " ");
    return put_double(buf, len, at, r->rho, "\n");
}

int64_t sift3d_register_report_text(const sift3d_register_report *r, char *buf, int64_t len)
{
    if (!r || r->n_levels < 0 || r->n_levels > SIFT3D_REGISTER_MAX_LEVELS) return -1;
    int64_t at = put(buf, len, 0, "# dof %d metric %s bins %d stop %d\n", (int)r->dof, r->metric == SIFT3D_REGISTER_METRIC_MI ? "mi" : "nmi", (int)r->bins, (int)r->stop);
    at = put(buf, len, at, "# h %.12g rho %.12g\n", r->h, r->rho);
    at = put(buf, len, at, "# level stride lattice iterations evaluations stop score_in score_out last_step device_ms\n");
    for (int l = 0; l < r->n_levels; l++) {
        const sift3d_register_level *v = &r->level[l];
        at = put(buf, len, at, "%d %d %lld %d %d %d ", l, (int)v->stride, (long long)v->n_lattice, (int)v->iterations, (int)v->evaluations, (int)v->stop);
        at = put_double(buf, len, at, v->score_in, " ");
        at = put_double(buf, len, at, v->score_out, " ");
        at = put(buf, len, at, "%.12g %.3f\n", v->last_step, v->device_ms);
    }
    at = put(buf, len, at, "# theta t r s g\n");
    for (int k = 0; k < SIFT3D_REGISTER_THETA; k++) at = put_double(buf, len, at, r->theta[k], k % 3 == 2 ? "\n" : " ");
    at = put(buf, len, at, "# result\n");
    for (int k = 0; k < 16; k++) at = put(buf, len, at, "%.9g%s", (double)r->result[k], k % 4 == 3 ? "\n" : " ");
    at = put(buf, len, at, "# record n excluded outside mi nmi rho\n");
    at = put_record(buf, len, at, "before", &r->before, r->outside_before);
    at = put_record(buf, len, at, "after", &r->after, r->outside_after);
    if (buf && len > 0) buf[at < len - 1 ? at : len - 1] = 0;
    return at;
}
