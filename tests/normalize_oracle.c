/*
 * normalize_oracle.c -- CPU restatement of the intensity matching of DESIGN.md section 7s (test infrastructure; written from that
 * text, it includes none of the product's headers).  Built with cc -O2 -ffp-contract=off by tests/normalize_cases.py.  The sampler is
 * the resampling oracle's and the field oracle's, compiled beside it (their file-local helpers renamed apart).
 *
 * onm_range: the least and greatest finite value.  onm_overlap: the two histograms, the six sums and the three counts, voxel by
 * voxel and serially.  onm_transfer: the table of either mode.  onm_apply: the table on every voxel, with a linear search for the
 * segment.
 */
#include <string.h>

#define at orc_at
#define lerp orc_lerp
#define one_voxel orc_one_voxel
#include "resample_oracle.c"
#undef at
#undef lerp
#undef one_voxel
#define at ofd_at
#define lerp ofd_lerp
#define one_voxel ofd_one_voxel
#include "field_oracle.c"
#undef at
#undef lerp
#undef one_voxel

int onm_range(const float *v, int64_t n, float *lo, float *hi)
{
    int any = 0;
    float a = 0, b = 0;
    for (int64_t i = 0; i < n; i++) {
        if (!isfinite(v[i])) continue;
        if (!any) a = b = v[i];
        if (v[i] < a) a = v[i];
        if (v[i] > b) b = v[i];
        any = 1;
    }
    *lo = a;
    *hi = b;
    return any && b > a;
}

static int onm_q(float v, float lo, float hi)
{
    if (!isfinite(v)) return -1;
    const double t = (((double)v - (double)lo) / ((double)hi - (double)lo)) * 1023.0;
    if (t <= 0.0) return 0;
    if (t >= 1023.0) return 1023;
    return (int)rint(t);
}

/* 1 where the position of the reference voxel (i, j, k) passes the sampler's inside test */
static int onm_inside(int64_t mx, int64_t my, int64_t mz, const float *A, const float *C, const float *K, const float *disp, const int64_t *nn, const float *o,
                      float h, int64_t i, int64_t j, int64_t k)
{
    const float p[3] = {(float)i, (float)j, (float)k};
    const int64_t n[3] = {mx, my, mz};
    float q[3], g[3], d[3];
    for (int r = 0; r < 3; r++) {
        float s = A[4 * r] * p[0];
        s = s + A[4 * r + 1] * p[1];
        s = s + A[4 * r + 2] * p[2];
        q[r] = s + A[4 * r + 3];
    }
    if (disp) {
        for (int r = 0; r < 3; r++) {
            float c = C[4 * r] * p[0];
            c = c + C[4 * r + 1] * p[1];
            c = c + C[4 * r + 2] * p[2];
            g[r] = ((c + C[4 * r + 3]) - o[r]) / h;
        }
        if (field_at(disp, nn, g, d))
            for (int r = 0; r < 3; r++) {
                float s = K[3 * r] * d[0];
                s = s + K[3 * r + 1] * d[1];
                s = s + K[3 * r + 2] * d[2];
                q[r] = q[r] + s;
            }
    }
    for (int r = 0; r < 3; r++)
        if (!(q[r] >= 0.0f) || !(q[r] <= (float)(n[r] - 1))) return 0;
    return 1;
}

/* hist_a, hist_b: 1024 words each; sums: n Sa Sb Saa Sbb Sab; counts: masked outside excluded.  disp NULL: no field */
int onm_overlap(const float *R, int64_t nx, int64_t ny, int64_t nz, const float *mask, const float *B, int64_t mx, int64_t my, int64_t mz, const float *A,
                const float *C, const float *K, const float *disp, const int64_t *nn, const float *o, float h, float alo, float ahi, float blo, float bhi,
                int64_t *hist_a, int64_t *hist_b, int64_t *sums, int64_t *counts)
{
    if (nx < 1 || ny < 1 || nz < 1 || mx < 1 || my < 1 || mz < 1) return -1;
    for (int e = 0; e < 1024; e++) hist_a[e] = hist_b[e] = 0;
    for (int e = 0; e < 6; e++) sums[e] = 0;
    for (int e = 0; e < 3; e++) counts[e] = 0;
    for (int64_t k = 0; k < nz; k++)
        for (int64_t j = 0; j < ny; j++)
            for (int64_t i = 0; i < nx; i++) {
                const int64_t x = (k * ny + j) * nx + i;
                if (mask && (!isfinite(mask[x]) || mask[x] == 0.0f)) {
                    counts[0]++;
                    continue;
                }
                if (!onm_inside(mx, my, mz, A, C, K, disp, nn, o, h, i, j, k)) {
                    counts[1]++;
                    continue;
                }
                const float b = disp ? ofd_one_voxel(B, mx, my, mz, A, C, K, disp, nn, o, h, 0, NAN, i, j, k) : orc_one_voxel(B, mx, my, mz, A, 0, NAN, i, j, k);
                const int qa = onm_q(R[x], alo, ahi), qb = onm_q(b, blo, bhi);
                if (qa < 0 || qb < 0) {
                    counts[2]++;
                    continue;
                }
                hist_a[qa]++;
                hist_b[qb]++;
                sums[0] += 1;
                sums[1] += qa;
                sums[2] += qb;
                sums[3] += (int64_t)qa * qa;
                sums[4] += (int64_t)qb * qb;
                sums[5] += (int64_t)qa * qb;
            }
    return 0;
}

/* x_j of rank r in h */
static double onm_knot(const int64_t *h, int64_t r)
{
    int64_t cum = 0;
    for (int i = 0; i < 1024; i++) {
        if (cum + h[i] > r) return ((double)i - 0.5) + ((double)(r - cum) + 0.5) / (double)h[i];
        cum += h[i];
    }
    return NAN; /* r is not below the histogram's total */
}

/* 0 and the table (xb, xa, slope: room for 257; slope's first m - 1 are set); -2: n < 2; -3: no variance in the reference (linear) or
 * equal first and last xa (hist); -4: no variance in the image (linear) or fewer than two knots (hist) */
int onm_transfer(int mode, int Q, const int64_t *hist_a, const int64_t *hist_b, const int64_t *sums, float alo, float ahi, int *m_out, double *xb, double *xa,
                 double *slope, double *tail, double *wa)
{
    const int64_t n = sums[0];
    *wa = ((double)ahi - (double)alo) / 1023.0;
    *m_out = 0;
    if (n < 2) return -2;
    int m = 0;
    if (mode == 0) {
        const __int128 va = (__int128)n * sums[3] - (__int128)sums[1] * sums[1], vb = (__int128)n * sums[4] - (__int128)sums[2] * sums[2];
        if (va <= 0) return -3;
        if (vb <= 0) return -4;
        const double ma = (double)sums[1] / (double)n, mb = (double)sums[2] / (double)n;
        const double g = sqrt((double)va) / sqrt((double)vb);
        xb[0] = 0.0;
        xb[1] = 1023.0;
        xa[0] = ma + (0.0 - mb) * g;
        xa[1] = ma + (1023.0 - mb) * g;
        m = 2;
    } else {
        for (int j = 0; j <= Q; j++) {
            const int64_t r = ((int64_t)j * (n - 1)) / Q;
            const double a = onm_knot(hist_a, r), b = onm_knot(hist_b, r);
            if (j == 0 || b > xb[m - 1]) {
                xa[m] = a;
                xb[m] = b;
                m++;
            }
        }
        if (m < 2) return -4;
        if (xa[0] == xa[m - 1]) return -3;
    }
    for (int k = 0; k < m - 1; k++) slope[k] = (xa[k + 1] - xa[k]) / (xb[k + 1] - xb[k]);
    *tail = (xa[m - 1] - xa[0]) / (xb[m - 1] - xb[0]);
    *m_out = m;
    return 0;
}

void onm_apply(const float *v, int64_t n, int m, const double *xb, const double *xa, const double *slope, double tail, double wa, float alo, float blo, float bhi,
               float *out)
{
    for (int64_t i = 0; i < n; i++) {
        if (!isfinite(v[i])) {
            memcpy(&out[i], &v[i], sizeof(float));
            continue;
        }
        const double u = (((double)v[i] - (double)blo) / ((double)bhi - (double)blo)) * 1023.0;
        double y;
        if (u < xb[0]) y = xa[0] + (u - xb[0]) * tail;
        else if (u >= xb[m - 1]) y = xa[m - 1] + (u - xb[m - 1]) * tail;
        else {
            int k = 0;
            while (k + 1 < m && xb[k + 1] <= u) k++;
            y = fmin(xa[k] + (u - xb[k]) * slope[k], xa[k + 1]);
        }
        out[i] = (float)((double)alo + y * wa);
    }
}
