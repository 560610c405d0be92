/*
 * average_host.c -- host side of the template from warped images: the default parameters and their check, the
 * report's counts from the mask plane, the report as text, and the node-wise mean of K displacement fields in one stated sequence
 * of double operations (built with -ffp-contract=off; tests/average_oracle.c restates it).  Linked into libsift3d_hip.so
 * (average_api.hip uses it) and into libsift3d_host.so (no GPU needed).
 */
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "sift3d.h"

void sift3d_average_defaults(sift3d_average_params *p)
{
    memset(p, 0, sizeof *p);
    p->trim = 0;
    p->min_count = 1;
    p->fill = NAN;
    p->device = 0;
    p->max_voxels = 1ll << 32;
    p->form = SIFT3D_AVERAGE_FORM_DEFAULT;
}

__attribute__((format(printf, 4, 5))) static int refuse(char *err, int64_t err_len, int rc, const char *fmt, ...)
{
    if (err && err_len > 0) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, (size_t)err_len, fmt, ap);
        va_end(ap);
    }
    return rc;
}

int sift3d_average_check(const sift3d_average_params *p, int32_t K, char *err, int64_t err_len)
{
    if (!p) return refuse(err, err_len, -1, "null pointer");
    if (K < 1 || K > SIFT3D_AVERAGE_MAX_IMAGES) return refuse(err, err_len, -1, "K = %d images: 1 .. %d", (int)K, SIFT3D_AVERAGE_MAX_IMAGES);
    if (p->trim < 0 || p->trim > SIFT3D_AVERAGE_MAX_TRIM) return refuse(err, err_len, -1, "trim = %d: 0 .. %d", (int)p->trim, SIFT3D_AVERAGE_MAX_TRIM);
    if (p->min_count < 1 || p->min_count > K) return refuse(err, err_len, -1, "min_count = %d: 1 .. K = %d", (int)p->min_count, (int)K);
    if (p->max_voxels < 1) return refuse(err, err_len, -1, "max_voxels = %lld: at least 1", (long long)p->max_voxels);
    if (p->form != SIFT3D_AVERAGE_FORM_DEFAULT && p->form != SIFT3D_AVERAGE_FORM_COLUMN)
        return refuse(err, err_len, -1, "form = %d: -1 or 0", (int)p->form);
    return 0;
}

int sift3d_average_counts(const uint32_t *mask, int64_t n, int32_t K, int32_t trim, int32_t min_count, sift3d_average_report *r)
{
    if (!mask || !r || n < 0 || K < 1 || K > SIFT3D_AVERAGE_MAX_IMAGES) return -1;
    r->images = K;
    r->trim = trim;
    r->min_count = min_count;
    r->voxels = n;
    r->none = r->below = 0;
    memset(r->count, 0, sizeof r->count);
    for (int k = 0; k < SIFT3D_AVERAGE_MAX_IMAGES; k++) r->image[k].contributing = 0;
    for (int64_t i = 0; i < n; i++) {
        const uint32_t m = mask[i];
        if (K < 32 && (m >> K) != 0) return -1;
        int c = 0;
        for (int k = 0; k < K; k++)
            if ((m >> k) & 1u) {
                c++;
                r->image[k].contributing++;
            }
        r->count[c]++;
        r->none += c == 0;
        r->below += c < min_count;
    }
    return 0;
}

/* appends to buf[at ..) what fits, returns the position the whole text has reached */
__attribute__((format(printf, 4, 5))) static int64_t put(char *buf, int64_t len, int64_t at, const char *fmt, ...)
{
    char line[160];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(line, sizeof line, fmt, ap);
    va_end(ap);
    const int64_t n = (int64_t)strlen(line);
    for (int64_t i = 0; i < n; i++)
        if (buf && at + i < len - 1) buf[at + i] = line[i];
    return at + n;
}

int64_t sift3d_average_report_text(const sift3d_average_report *r, char *buf, int64_t len)
{
    if (!r || r->images < 1 || r->images > SIFT3D_AVERAGE_MAX_IMAGES) return -1;
    int64_t at = put(buf, len, 0, "# images %d trim %d min_count %d\n", (int)r->images, (int)r->trim, (int)r->min_count);
    at = put(buf, len, at, "# voxels %lld none %lld below %lld\n", (long long)r->voxels, (long long)r->none, (long long)r->below);
    at = put(buf, len, at, "# image contributing upload_ms\n");
    for (int k = 0; k < r->images; k++) at = put(buf, len, at, "%d %lld %.3f\n", k + 1, (long long)r->image[k].contributing, r->image[k].upload_ms);
    at = put(buf, len, at, "# n voxels\n");
    for (int c = 0; c <= r->images; c++) at = put(buf, len, at, "%d %lld\n", c, (long long)r->count[c]);
    at = put(buf, len, at, "# kernel_ms wall_ms\n%.3f %.3f\n", r->kernel_ms, r->wall_ms);
    if (buf && len > 0) buf[at < len - 1 ? at : len - 1] = 0;
    return at;
}

static uint32_t bits_of(float v)
{
    uint32_t u;
    memcpy(&u, &v, sizeof u);
    return u;
}

int sift3d_mean_field(int32_t K, const sift3d_field *fields, sift3d_field *out, char *err, int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (K < 1 || K > SIFT3D_AVERAGE_MAX_IMAGES) return refuse(err, err_len, SIFT3D_ERR_ARG, "K = %d fields: 1 .. %d", (int)K, SIFT3D_AVERAGE_MAX_IMAGES);
    if (!fields || !out) return refuse(err, err_len, SIFT3D_ERR_ARG, "null pointer");
    const sift3d_field *f0 = &fields[0];
    for (int a = 0; a < 3; a++)
        if (f0->n[a] < 2 || f0->n[a] > (1 << 24)) return refuse(err, err_len, SIFT3D_ERR_ARG, "field 0: n[%d] = %lld: 2 .. 2^24 nodes per axis", a, (long long)f0->n[a]);
    if (f0->n[0] * f0->n[1] > (1ll << 40) / f0->n[2]) return refuse(err, err_len, SIFT3D_ERR_ARG, "field 0: more than 2^40 nodes");
    const int64_t N = f0->n[0] * f0->n[1] * f0->n[2];
    for (int k = 0; k < K; k++) {
        const sift3d_field *f = &fields[k];
        for (int a = 0; a < 3; a++) {
            if (f->n[a] != f0->n[a])
                return refuse(err, err_len, SIFT3D_ERR_ARG, "field %d: n[%d] = %lld differs from field 0's %lld", k, a, (long long)f->n[a], (long long)f0->n[a]);
            if (bits_of(f->origin[a]) != bits_of(f0->origin[a]))
                return refuse(err, err_len, SIFT3D_ERR_ARG, "field %d: origin[%d] = %.9g differs from field 0's %.9g", k, a, (double)f->origin[a], (double)f0->origin[a]);
        }
        if (bits_of(f->spacing) != bits_of(f0->spacing))
            return refuse(err, err_len, SIFT3D_ERR_ARG, "field %d: spacing = %.9g differs from field 0's %.9g", k, (double)f->spacing, (double)f0->spacing);
        if (!f->disp || f->capacity < 3 * N) return refuse(err, err_len, SIFT3D_ERR_ARG, "field %d: disp holds fewer than 3 n0 n1 n2 floats", k);
    }
    for (int a = 0; a < 3; a++) {
        out->n[a] = f0->n[a];
        out->origin[a] = f0->origin[a];
    }
    out->spacing = f0->spacing;
    if (!out->disp || out->capacity < 3 * N) return refuse(err, err_len, SIFT3D_ERR_CAPACITY, "out holds fewer than 3 n0 n1 n2 = %lld floats", (long long)(3 * N));
    for (int64_t i = 0; i < 3 * N; i++) {
        double s = 0.0;
        for (int k = 0; k < K; k++) s = s + (double)fields[k].disp[i];
        out->disp[i] = (float)(s / (double)K);
    }
    return SIFT3D_OK;
}
