/*
 * normalize_host.c -- host side of the intensity matching: the default parameters and their check, the transfer
 * table from the two histograms and the six sums in one stated sequence of double operations (built with -ffp-contract=off;
 * tests/normalize_oracle.c restates it), the check of a table and the report as text.  Linked into libsift3d_hip.so (normalize_api.hip
 * uses it) and into libsift3d_host.so (no GPU needed).
 */
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "quantize.h"
#include "sift3d.h"

void sift3d_normalize_defaults(sift3d_normalize_params *p)
{
    memset(p, 0, sizeof *p);
    p->mode = SIFT3D_NORMALIZE_LINEAR;
    p->knots = 64;
    p->device = 0;
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

int sift3d_normalize_check(const sift3d_normalize_params *p, char *err, int64_t err_len)
{
    if (!p) return refuse(err, err_len, "null pointer");
    if (p->mode != SIFT3D_NORMALIZE_LINEAR && p->mode != SIFT3D_NORMALIZE_HIST) return refuse(err, err_len, "mode = %d: 0 (linear) or 1 (hist)", (int)p->mode);
    if (p->mode == SIFT3D_NORMALIZE_HIST && (p->knots < 2 || p->knots > SIFT3D_NORMALIZE_MAX_KNOTS - 1))
        return refuse(err, err_len, "knots = %d: 2 .. %d", (int)p->knots, SIFT3D_NORMALIZE_MAX_KNOTS - 1);
    return 0;
}

static int range_ok(const float r[2]) { return isfinite(r[0]) && isfinite(r[1]) && r[1] > r[0]; }

/* the position of rank r in the histogram h, in quantiser units: section 7s's x_j */
static double quantile(const int64_t *h, int64_t r)
{
    int64_t below = 0;
    int i = 0;
    while (i < SIFT3D_NORMALIZE_BINS - 1 && below + h[i] <= r) below += h[i++];
    return ((double)i - 0.5) + ((double)(r - below) + 0.5) / (double)h[i];
}

int sift3d_normalize_transfer(int32_t mode, int32_t knots, const int64_t *hist_a, const int64_t *hist_b, const int64_t *sums, const float a_range[2],
                              const float b_range[2], sift3d_transfer *t, char *err, int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (!hist_a || !hist_b || !sums || !a_range || !b_range || !t) return refuse(err, err_len, "null pointer");
    sift3d_normalize_params p;
    sift3d_normalize_defaults(&p);
    p.mode = mode;
    p.knots = knots;
    if (sift3d_normalize_check(&p, err, err_len) != 0) return -1;
    if (!range_ok(a_range)) return refuse(err, err_len, "a_range = %g %g: finite, hi > lo", (double)a_range[0], (double)a_range[1]);
    if (!range_ok(b_range)) return refuse(err, err_len, "b_range = %g %g: finite, hi > lo", (double)b_range[0], (double)b_range[1]);
    const int64_t n = sums[0];
    int64_t ta = 0, tb = 0;
    for (int i = 0; i < SIFT3D_NORMALIZE_BINS; i++) {
        if (hist_a[i] < 0 || hist_b[i] < 0) return refuse(err, err_len, "bin %d holds a negative count", i);
        ta += hist_a[i];
        tb += hist_b[i];
    }
    if (n < 0 || ta != n || tb != n)
        return refuse(err, err_len, "sums[0] = %lld, hist_a holds %lld and hist_b %lld voxels: they must agree", (long long)n, (long long)ta, (long long)tb);
    memset(t, 0, sizeof *t);
    t->mode = mode;
    t->a_lo = a_range[0];
    t->a_hi = a_range[1];
    t->b_lo = b_range[0];
    t->b_hi = b_range[1];
    t->wa = ((double)a_range[1] - (double)a_range[0]) / (double)QMAX;
    if (n < 2) return refuse(err, err_len, "%lld voxels are counted: at least 2 are needed", (long long)n);
    if (mode == SIFT3D_NORMALIZE_LINEAR) {
        const __int128 N = n, Sa = sums[1], Sb = sums[2];
        const __int128 Va = N * (__int128)sums[3] - Sa * Sa, Vb = N * (__int128)sums[4] - Sb * Sb;
        if (!(Va > 0)) return refuse(err, err_len, "the counted voxels of the reference all fall in one bin: no variance to match");
        if (!(Vb > 0)) return refuse(err, err_len, "the counted voxels of the image all fall in one bin: no variance to match");
        const double ma = (double)sums[1] / (double)n, mb = (double)sums[2] / (double)n;
        const double g = sqrt((double)Va) / sqrt((double)Vb);
        t->m = 2;
        t->xb[0] = 0.0;
        t->xb[1] = (double)QMAX;
        t->xa[0] = ma + (0.0 - mb) * g;
        t->xa[1] = ma + ((double)QMAX - mb) * g;
    } else {
        int m = 0;
        for (int j = 0; j <= knots; j++) {
            const int64_t r = (int64_t)(((__int128)j * (__int128)(n - 1)) / knots);
            const double xa = quantile(hist_a, r), xb = quantile(hist_b, r);
            if (m > 0 && !(xb > t->xb[m - 1])) continue;
            t->xa[m] = xa;
            t->xb[m] = xb;
            m++;
        }
        t->m = m;
        if (m < 2) return refuse(err, err_len, "the counted voxels of the image all fall at one position: fewer than two knots");
        if (t->xa[0] == t->xa[m - 1]) return refuse(err, err_len, "the counted voxels of the reference all fall at one position: nothing to match to");
    }
    for (int k = 0; k + 1 < t->m; k++) t->slope[k] = (t->xa[k + 1] - t->xa[k]) / (t->xb[k + 1] - t->xb[k]);
    t->tail = (t->xa[t->m - 1] - t->xa[0]) / (t->xb[t->m - 1] - t->xb[0]);
    return 0;
}

int sift3d_transfer_check(const sift3d_transfer *t, char *err, int64_t err_len)
{
    if (!t) return refuse(err, err_len, "null pointer");
    if (t->m < 2 || t->m > SIFT3D_NORMALIZE_MAX_KNOTS) return refuse(err, err_len, "table: m = %d knots: 2 .. %d", (int)t->m, SIFT3D_NORMALIZE_MAX_KNOTS);
    const float ra[2] = {t->a_lo, t->a_hi}, rb[2] = {t->b_lo, t->b_hi};
    if (!range_ok(ra) || !range_ok(rb)) return refuse(err, err_len, "table: a range is not finite or has hi <= lo");
    if (!isfinite(t->wa) || !isfinite(t->tail)) return refuse(err, err_len, "table: wa or tail is not finite");
    for (int k = 0; k < t->m; k++) {
        if (!isfinite(t->xb[k]) || !isfinite(t->xa[k]) || !isfinite(t->slope[k])) return refuse(err, err_len, "table: knot %d is not finite", k);
        if (k > 0 && !(t->xb[k] > t->xb[k - 1])) return refuse(err, err_len, "table: xb[%d] is not above xb[%d]", k, k - 1);
        if (k > 0 && t->xa[k] < t->xa[k - 1]) return refuse(err, err_len, "table: xa[%d] is below xa[%d]", k, k - 1);
    }
    return 0;
}

/* appends to buf[at ..) what fits, returns the position the whole text has reached */
__attribute__((format(printf, 4, 5))) static int64_t put(char *buf, int64_t len, int64_t at, const char *fmt, ...)
{
    char line[200];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(line, sizeof line, fmt, ap);
    va_end(ap);
    const int64_t n = (int64_t)strlen(line);
    for (int64_t i = 0; i < n; i++)
        if (buf && at + i < len - 1) buf[at + i] = line[i];
    return at + n;
}

int64_t sift3d_normalize_report_text(const sift3d_normalize_report *r, char *buf, int64_t len)
{
    if (!r || r->table.m < 2 || r->table.m > SIFT3D_NORMALIZE_MAX_KNOTS) return -1;
    const sift3d_transfer *t = &r->table;
    int64_t at = put(buf, len, 0, "# mode %s knots %d kept %d\n", r->mode == SIFT3D_NORMALIZE_HIST ? "hist" : "linear", (int)r->knots, (int)t->m);
    at = put(buf, len, at, "# range_reference %.9g %.9g\n# range_image %.9g %.9g\n", (double)t->a_lo, (double)t->a_hi, (double)t->b_lo, (double)t->b_hi);
    at = put(buf, len, at, "# reference_voxels %lld counted %lld masked %lld outside %lld excluded %lld\n", (long long)r->reference_voxels, (long long)r->sums[0],
             (long long)r->counts[0], (long long)r->counts[1], (long long)r->counts[2]);
    at = put(buf, len, at, "# image_voxels %lld\n# knot xb xa slope\n", (long long)r->image_voxels);
    for (int k = 0; k < t->m; k++) at = put(buf, len, at, "%d %.17g %.17g %.17g\n", k, t->xb[k], t->xa[k], t->slope[k]);
    at = put(buf, len, at, "# tail wa\n%.17g %.17g\n", t->tail, t->wa);
    at = put(buf, len, at, "# hist_ms apply_ms wall_ms\n%.3f %.3f %.3f\n", r->hist_ms, r->apply_ms, r->wall_ms);
    if (buf && len > 0) buf[at < len - 1 ? at : len - 1] = 0;
    return at;
}
