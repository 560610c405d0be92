/*
 * similarity_oracle.c -- CPU restatement of the image similarity of DESIGN.md section 7o (test infrastructure; written from that text,
 * it includes none of the product's headers).  Built with cc -O2 -ffp-contract=off by tests/similarity_cases.py.
 *
 * osim_range: lo, hi = the least and the largest finite value; 1 where hi > lo, else 0.
 * osim_q: -1 where v is not finite, else t = (((double)v - lo) / (hi - lo)) * 1023; 0 for t <= 0, 1023 for t >= 1023, else rint(t).
 * osim_count: every voxel in index order, serially.  A voxel counts when both q are >= 0.  hist[i bins + j] counts the voxels with
 *   qA >> s = i and qB >> s = j, s = 10 - log2 bins; sums = n, sum qA, sum qB, sum qA^2, sum qB^2, sum qA qB over the counted voxels;
 *   the return value is the number of the other voxels.  With labels (finite: an integer 0 .. 65535) lab_sums[6 l ..] holds the same
 *   six sums over the counted voxels whose label is l; 65536 x 6 words, cleared here.
 * osim_measures: out = mi, nmi, rho, rms, h_a, h_b, h_ab.  osim_rho_rms: out = rho, rms of six sums.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

int osim_range(const float *f, int64_t n, float *lo, float *hi)
{
    int any = 0;
    float a = 0, b = 0;
    for (int64_t i = 0; i < n; i++) {
        if (!isfinite(f[i])) continue;
        if (!any || f[i] < a) a = f[i];
        if (!any || f[i] > b) b = f[i];
        any = 1;
    }
    *lo = a;
    *hi = b;
    return any && b > a;
}

int osim_q(float v, float lo, float hi)
{
    if (!isfinite(v)) return -1;
    const double t = (((double)v - (double)lo) / ((double)hi - (double)lo)) * 1023.0;
    return t <= 0.0 ? 0 : (t >= 1023.0 ? 1023 : (int)rint(t));
}

int64_t osim_count(const float *a, const float *b, const float *labels, int64_t n, float alo, float ahi, float blo, float bhi, int bins, int64_t *hist,
                   int64_t *sums, int64_t *lab_sums)
{
    int s = 10;
    for (int k = bins; k > 1; k >>= 1) s--;
    memset(hist, 0, sizeof(int64_t) * (size_t)(bins * bins));
    memset(sums, 0, sizeof(int64_t) * 6);
    if (labels) memset(lab_sums, 0, sizeof(int64_t) * 6 * 65536);
    int64_t excluded = 0;
    for (int64_t i = 0; i < n; i++) {
        const int64_t qa = osim_q(a[i], alo, ahi), qb = osim_q(b[i], blo, bhi);
        if (qa < 0 || qb < 0) {
            excluded++;
            continue;
        }
        const int64_t term[6] = {1, qa, qb, qa * qa, qb * qb, qa * qb};
        hist[(qa >> s) * bins + (qb >> s)]++;
        for (int j = 0; j < 6; j++) sums[j] += term[j];
        if (labels && isfinite(labels[i]))
            for (int j = 0; j < 6; j++) lab_sums[6 * (int64_t)labels[i] + j] += term[j];
    }
    return excluded;
}

void osim_rho_rms(const int64_t *s, float lo, float hi, int same_scale, double *out)
{
    out[0] = out[1] = NAN;
    const int64_t n = s[0];
    if (n <= 0) return;
    const __int128 cov = (__int128)n * s[5] - (__int128)s[1] * s[2];
    const __int128 va = (__int128)n * s[3] - (__int128)s[1] * s[1], vb = (__int128)n * s[4] - (__int128)s[2] * s[2];
    if (va > 0 && vb > 0) out[0] = (double)cov / (sqrt((double)va) * sqrt((double)vb));
    if (same_scale) out[1] = sqrt((double)(s[3] - 2 * s[5] + s[4]) / (double)n) * (((double)hi - (double)lo) / 1023.0);
}

static double entropy_of(const int64_t *c, int count, int64_t n)
{
    double sum = 0.0;
    for (int k = 0; k < count; k++)
        if (c[k] > 0) sum += (double)c[k] * log((double)c[k]);
    return log((double)n) - sum / (double)n;
}

void osim_measures(const int64_t *hist, int bins, const int64_t *s, float lo, float hi, int same_scale, double *out)
{
    for (int k = 0; k < 7; k++) out[k] = NAN;
    const int64_t n = s[0];
    if (n <= 0) return;
    osim_rho_rms(s, lo, hi, same_scale, out + 2);
    int64_t rows[64], cols[64];
    for (int i = 0; i < bins; i++) {
        rows[i] = cols[i] = 0;
        for (int j = 0; j < bins; j++) {
            rows[i] += hist[i * bins + j];
            cols[i] += hist[j * bins + i];
        }
    }
    const double ha = entropy_of(rows, bins, n), hb = entropy_of(cols, bins, n), hab = entropy_of(hist, bins * bins, n);
    out[4] = ha;
    out[5] = hb;
    out[6] = hab;
    out[0] = (ha + hb) - hab;
    if (hab > 0) out[1] = (ha + hb) / hab;
}
