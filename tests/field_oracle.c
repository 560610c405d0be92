/*
 * field_oracle.c -- CPU restatement of the displacement field of DESIGN.md section 7e (test infrastructure; written from
 * that text, it includes none of the product's headers).  Built with cc -O2 -ffp-contract=off by tests/field_cases.py.
 *
 * ofd_fit: every node against every finite sample (all six components finite), in float:
 *   P = o + (float)a h per axis; dx = y.x - P.x; d2 = ((dx dx + dy dy) + dz dz); only d2 < R R counts;
 *   t = 1 - d2 / (R R), w = (t t) t; W += rint(w 2^24), V_c += rint((w v_c) 2^24) in int64;
 *   v_c = (float)((double)V_c / ((double)W + lambda 2^24)), 0 where that denominator is 0.
 * The samples are visited in order of y.x and only those within 2R along x of the node are tested: a sample farther away has
 * |dx| >= R, so d2 >= R R in float, and contributes nothing.  The sums are integers: the order does not matter.
 * ofd_eval: the interpolation of a field at key positions (section 7c's floor, weights, clamp, x -> y -> z), 0 outside.
 * ofd_warp: section 7c's resampler with the field term, output planes [z0, z1).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

static const float *g_sort_y;
static int by_x(const void *a, const void *b)
{
    const float u = g_sort_y[3 * *(const int64_t *)a], v = g_sort_y[3 * *(const int64_t *)b];
    return u < v ? -1 : (u > v ? 1 : 0);
}

int ofd_fit(const float *y, const float *v, int64_t n, const float *o, float h, const int64_t *nn, float R, float lambda, float *disp)
{
    int64_t *idx = (int64_t *)malloc(sizeof(int64_t) * (size_t)(n > 0 ? n : 1));
    float *xs = (float *)malloc(sizeof(float) * (size_t)(n > 0 ? n : 1));
    if (!idx || !xs) return -1;
    int64_t m = 0;
    for (int64_t i = 0; i < n; i++) {
        int ok = 1;
        for (int k = 0; k < 3; k++) ok &= isfinite(y[3 * i + k]) && isfinite(v[3 * i + k]);
        if (ok) idx[m++] = i;
    }
    g_sort_y = y;
    qsort(idx, (size_t)m, sizeof(int64_t), by_x);
    for (int64_t s = 0; s < m; s++) xs[s] = y[3 * idx[s]];
    const float rr = R * R;
    const double den_l = (double)lambda * 16777216.0;
    const int64_t N = nn[0] * nn[1] * nn[2];
    for (int64_t c = 0; c < nn[2]; c++)
        for (int64_t b = 0; b < nn[1]; b++)
            for (int64_t a = 0; a < nn[0]; a++) {
                const float P[3] = {o[0] + (float)a * h, o[1] + (float)b * h, o[2] + (float)c * h};
                /* first sample with x >= P.x - 2R */
                const double lo = (double)P[0] - 2.0 * (double)R, hi = (double)P[0] + 2.0 * (double)R;
                int64_t L = 0, U = m;
                while (L < U) {
                    const int64_t mid = (L + U) / 2;
                    if ((double)xs[mid] < lo) L = mid + 1;
                    else U = mid;
                }
                int64_t W = 0, V[3] = {0, 0, 0};
                for (int64_t s = L; s < m && (double)xs[s] <= hi; s++) {
                    const float *q = y + 3 * idx[s], *e = v + 3 * idx[s];
                    const float dx = q[0] - P[0], dy = q[1] - P[1], dz = q[2] - P[2];
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    if (!(d2 < rr)) continue;
                    const float t = 1.0f - d2 / rr;
                    const float w = (t * t) * t;
                    W += (int64_t)rintf(w * 16777216.0f);
                    for (int k = 0; k < 3; k++) V[k] += (int64_t)rintf((w * e[k]) * 16777216.0f);
                }
                const double den = (double)W + den_l;
                const int64_t i = (c * nn[1] + b) * nn[0] + a;
                for (int k = 0; k < 3; k++) disp[k * N + i] = den == 0.0 ? 0.0f : (float)((double)V[k] / den);
            }
    free(idx);
    free(xs);
    return 0;
}

static float lerp(float a, float b, float w) { return (1.0f - w) * a + w * b; }

/* v at grid coordinates g; 0 (and 0 returned) outside */
static int field_at(const float *disp, const int64_t *nn, const float g[3], float out[3])
{
    out[0] = out[1] = out[2] = 0.0f;
    for (int r = 0; r < 3; r++)
        if (!(g[r] >= 0.0f) || !(g[r] <= (float)(nn[r] - 1))) return 0;
    int64_t lo[3], hi[3];
    float w[3];
    for (int r = 0; r < 3; r++) {
        const float f = floorf(g[r]);
        w[r] = g[r] - f;
        lo[r] = (int64_t)f;
        hi[r] = lo[r] + 1 <= nn[r] - 1 ? lo[r] + 1 : nn[r] - 1;
    }
    const int64_t N = nn[0] * nn[1] * nn[2];
    for (int c = 0; c < 3; c++) {
        const float *d = disp + c * N;
#define AT(x, y, z) d[((z) * nn[1] + (y)) * nn[0] + (x)]
        const float e00 = lerp(AT(lo[0], lo[1], lo[2]), AT(hi[0], lo[1], lo[2]), w[0]);
        const float e10 = lerp(AT(lo[0], hi[1], lo[2]), AT(hi[0], hi[1], lo[2]), w[0]);
        const float e01 = lerp(AT(lo[0], lo[1], hi[2]), AT(hi[0], lo[1], hi[2]), w[0]);
        const float e11 = lerp(AT(lo[0], hi[1], hi[2]), AT(hi[0], hi[1], hi[2]), w[0]);
#undef AT
        out[c] = lerp(lerp(e00, e10, w[1]), lerp(e01, e11, w[1]), w[2]);
    }
    return 1;
}

void ofd_eval(const float *disp, const int64_t *nn, const float *o, float h, const float *y, int64_t n, float *out)
{
    for (int64_t i = 0; i < n; i++) {
        float g[3];
        for (int r = 0; r < 3; r++) g[r] = (y[3 * i + r] - o[r]) / h;
        field_at(disp, nn, g, out + 3 * i);
    }
}

static float at(const float *v, int64_t nx, int64_t ny, int64_t x, int64_t y, int64_t z) { return v[(z * ny + y) * nx + x]; }

static float one_voxel(const float *src, int64_t nx, int64_t ny, int64_t nz, const float *A, const float *C, const float *K, const float *disp,
                       const int64_t *nn, const float *o, float h, int interp, float fill, int64_t i, int64_t j, int64_t k)
{
    const float p[3] = {(float)i, (float)j, (float)k};
    const int64_t n[3] = {nx, ny, nz};
    float q[3], kap[3], g[3], d[3];
    for (int r = 0; r < 3; r++) {
        float s = A[4 * r] * p[0];
        s = s + A[4 * r + 1] * p[1];
        s = s + A[4 * r + 2] * p[2];
        q[r] = s + A[4 * r + 3];
        float c = C[4 * r] * p[0];
        c = c + C[4 * r + 1] * p[1];
        c = c + C[4 * r + 2] * p[2];
        kap[r] = c + C[4 * r + 3];
        g[r] = (kap[r] - o[r]) / h;
    }
    if (field_at(disp, nn, g, d))
        for (int r = 0; r < 3; r++) {
            float s = K[3 * r] * d[0];
            s = s + K[3 * r + 1] * d[1];
            s = s + K[3 * r + 2] * d[2];
            q[r] = q[r] + s;
        }
    for (int r = 0; r < 3; r++) {
        const float top = (float)(n[r] - 1);
        if (!(q[r] >= 0.0f) || !(q[r] <= top)) return fill;
    }
    if (interp == 1) {
        int64_t c[3];
        for (int r = 0; r < 3; r++) {
            c[r] = (int64_t)floorf(q[r] + 0.5f);
            if (c[r] > n[r] - 1) c[r] = n[r] - 1;
        }
        return at(src, nx, ny, c[0], c[1], c[2]);
    }
    int64_t lo[3], hi[3];
    float w[3];
    for (int r = 0; r < 3; r++) {
        const float f = floorf(q[r]);
        w[r] = q[r] - f;
        lo[r] = (int64_t)f;
        hi[r] = lo[r] + 1 <= n[r] - 1 ? lo[r] + 1 : n[r] - 1;
    }
    const float e00 = lerp(at(src, nx, ny, lo[0], lo[1], lo[2]), at(src, nx, ny, hi[0], lo[1], lo[2]), w[0]);
    const float e10 = lerp(at(src, nx, ny, lo[0], hi[1], lo[2]), at(src, nx, ny, hi[0], hi[1], lo[2]), w[0]);
    const float e01 = lerp(at(src, nx, ny, lo[0], lo[1], hi[2]), at(src, nx, ny, hi[0], lo[1], hi[2]), w[0]);
    const float e11 = lerp(at(src, nx, ny, lo[0], hi[1], hi[2]), at(src, nx, ny, hi[0], hi[1], hi[2]), w[0]);
    return lerp(lerp(e00, e10, w[1]), lerp(e01, e11, w[1]), w[2]);
}

int ofd_warp(const float *src, int64_t nx, int64_t ny, int64_t nz, float *dst, int64_t ox, int64_t oy, int64_t oz, const float *A, const float *C,
             const float *K, const float *disp, const int64_t *nn, const float *o, float h, int interp, float fill, int64_t z0, int64_t z1)
{
    if (nx < 1 || ny < 1 || nz < 1 || ox < 1 || oy < 1 || oz < 1 || z0 < 0 || z1 > oz || z1 < z0 || (interp != 0 && interp != 1)) return -1;
    for (int64_t k = z0; k < z1; k++)
        for (int64_t j = 0; j < oy; j++)
            for (int64_t i = 0; i < ox; i++)
                dst[((k - z0) * oy + j) * ox + i] = one_voxel(src, nx, ny, nz, A, C, K, disp, nn, o, h, interp, fill, i, j, k);
    return 0;
}
