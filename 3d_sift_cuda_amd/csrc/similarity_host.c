/*
 * similarity_host.c -- host side of the image similarity: the default parameters and their check, the derived
 * values of a joint histogram and its integer sums -- one stated sequence of double operations, built with -ffp-contract=off -- and
 * the report as text.  The GPU never computes a logarithm.  Linked into libsift3d_hip.so (similarity_api.hip uses it) and into
 * libsift3d_host.so (no GPU needed).
 */
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "sift3d.h"
#include "quantize.h"

void sift3d_similarity_defaults(sift3d_similarity_params *p)
{
    p->bins = 64;
    p->same_scale = 0;
    p->max_labels = SIFT3D_SIMILARITY_MAX_LABELS;
    p->device = 0;
    p->flush = 1; /* the faster of the two at 512^3 */
    p->reserved = 0;
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

static int bins_ok(int32_t bins) { return bins == 8 || bins == 16 || bins == 32 || bins == 64; }

int sift3d_similarity_check(const sift3d_similarity_params *p, char *err, int64_t err_len)
{
    if (!p) return refuse(err, err_len, "null pointer");
    if (!bins_ok(p->bins)) return refuse(err, err_len, "bins = %d: 8, 16, 32 or 64", (int)p->bins);
    if (p->same_scale != 0 && p->same_scale != 1) return refuse(err, err_len, "same_scale = %d: 0 or 1", (int)p->same_scale);
    if (p->max_labels < 1 || p->max_labels > SIFT3D_SIMILARITY_MAX_LABELS)
        return refuse(err, err_len, "max_labels = %d: 1 .. %d", (int)p->max_labels, SIFT3D_SIMILARITY_MAX_LABELS);
    if (p->flush != 0 && p->flush != 1) return refuse(err, err_len, "flush = %d: 0 or 1", (int)p->flush);
    return 0;
}

/* rho and rms of six sums, as include/sift3d.h states them */
static void rho_rms(const int64_t *s, float lo, float hi, int32_t same_scale, double *rho, double *rms)
{
    const int64_t n = s[0];
    *rho = NAN;
    *rms = NAN;
    if (n <= 0) return;
    if (same_scale) {
        const int64_t d = s[3] - 2 * s[5] + s[4];
        *rms = sqrt((double)d / (double)n) * (((double)hi - (double)lo) / (double)QMAX);
    }
    const __int128 c = (__int128)n * s[5] - (__int128)s[1] * s[2];
    const __int128 va = (__int128)n * s[3] - (__int128)s[1] * s[1];
    const __int128 vb = (__int128)n * s[4] - (__int128)s[2] * s[2];
    if (va > 0 && vb > 0) *rho = (double)c / (sqrt((double)va) * sqrt((double)vb));
}

/* H of count cells that add up to n > 0 */
static double entropy(const int64_t *c, int count, int64_t n)
{
    double s = 0.0;
    for (int k = 0; k < count; k++)
        if (c[k] > 0) s += (double)c[k] * log((double)c[k]);
    return log((double)n) - s / (double)n;
}

int sift3d_similarity_measures(const int64_t *hist, int32_t bins, const int64_t *sums, float lo, float hi, int32_t same_scale,
                               sift3d_similarity_record *record)
{
    if (!hist || !sums || !record || !bins_ok(bins)) return -1;
    int64_t s[SIFT3D_SIMILARITY_SUMS];
    memcpy(s, sums, sizeof s);
    record->bins = bins;
    record->same_scale = same_scale ? 1 : 0;
    record->mi = record->nmi = record->h_a = record->h_b = record->h_ab = NAN;
    rho_rms(s, lo, hi, same_scale, &record->rho, &record->rms);
    const int64_t n = s[0];
    if (n > 0) {
        int64_t row[SIFT3D_SIMILARITY_MAX_BINS], col[SIFT3D_SIMILARITY_MAX_BINS];
        memset(row, 0, sizeof row);
        memset(col, 0, sizeof col);
        for (int i = 0; i < bins; i++)
            for (int j = 0; j < bins; j++) {
                row[i] += hist[i * bins + j];
                col[j] += hist[i * bins + j];
            }
        record->h_a = entropy(row, bins, n);
        record->h_b = entropy(col, bins, n);
        record->h_ab = entropy(hist, bins * bins, n);
        record->mi = (record->h_a + record->h_b) - record->h_ab;
        if (record->h_ab > 0) record->nmi = (record->h_a + record->h_b) / record->h_ab;
    }
    memcpy(record->sums, s, sizeof s);
    return 0;
}

void sift3d_similarity_label_measures(int32_t label, const int64_t *sums, float lo, float hi, int32_t same_scale, sift3d_similarity_label_record *rec)
{
    int64_t s[SIFT3D_SIMILARITY_SUMS];
    memcpy(s, sums, sizeof s);
    rec->label = label;
    rec->reserved = 0;
    rho_rms(s, lo, hi, same_scale, &rec->rho, &rec->rms);
    memcpy(rec->sums, s, sizeof s);
}

/* appends to buf[at ..) what fits, returns the position the whole text has reached */
static int64_t put_text(char *buf, int64_t len, int64_t at, const char *text)
{
    const int64_t n = (int64_t)strlen(text);
    for (int64_t i = 0; i < n; i++)
        if (buf && at + i < len - 1) buf[at + i] = text[i];
    return at + n;
}

__attribute__((format(printf, 4, 5))) static int64_t put(char *buf, int64_t len, int64_t at, const char *fmt, ...)
{
    char line[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(line, sizeof line, fmt, ap);
    va_end(ap);
    return put_text(buf, len, at, line);
}

/* a double with 12 significant digits and what follows it; a NaN of either sign as nan */
static int64_t put_double(char *buf, int64_t len, int64_t at, double v, const char *after)
{
    if (isnan(v)) return put(buf, len, at, "nan%s", after);
    return put(buf, len, at, "%.12g%s", v, after);
}

int64_t sift3d_similarity_report_text(const sift3d_similarity_record *r, const sift3d_similarity_label_record *lr, int32_t n_labels, char *buf, int64_t len)
{
    if (!r) return -1;
    int64_t at = put(buf, len, 0, "# range_a %.9g %.9g\n", (double)r->a_lo, (double)r->a_hi);
    at = put(buf, len, at, "# range_b %.9g %.9g\n", (double)r->b_lo, (double)r->b_hi);
    at = put(buf, len, at, "# same_scale %d\n", r->same_scale ? 1 : 0);
    at = put(buf, len, at, "# voxels %lld %lld\n", (long long)r->sums[0], (long long)r->excluded);
    const double v[7] = {r->mi, r->nmi, r->rho, r->rms, r->h_a, r->h_b, r->h_ab};
    for (int k = 0; k < 7; k++) at = put_double(buf, len, at, v[k], k < 6 ? " " : "\n");
    if (lr && n_labels >= 0) {
        at = put(buf, len, at, "# label n rho rms\n");
        const int count = n_labels > SIFT3D_SIMILARITY_MAX_LABELS ? SIFT3D_SIMILARITY_MAX_LABELS : n_labels;
        for (int k = 0; k < count; k++) {
            at = put(buf, len, at, "%d %lld ", (int)lr[k].label, (long long)lr[k].sums[0]);
            at = put_double(buf, len, at, lr[k].rho, " ");
            at = put_double(buf, len, at, lr[k].rms, "\n");
        }
    }
    if (buf && len > 0) buf[at < len - 1 ? at : len - 1] = 0;
    return at;
}
