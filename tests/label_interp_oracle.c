/*
 * label_interp_oracle.c -- CPU restatement of the label-aware linear interpolation of DESIGN.md section 7n (test infrastructure;
 * written from that text, it includes none of the product's headers).  Built with cc -O2 -ffp-contract=off by
 * tests/label_interp_cases.py.
 *
 * Position, inside test, fill, f = floorf(q), w = q - f, i0, i1 = min(i0 + 1, n - 1) and u = 1.0f - w are section 7c's.  Corner
 * c = a + 2b + 4d has the value L_c = src[(z_d ny + y_b) nx + x_a] and the weight W_c = (X_a * Y_b) * Z_d.  The classes are built
 * one by one, each from its lowest-numbered corner; a class' score is ((t_0 + t_1) + ...) + t_7 with t_c = W_c for its corners and
 * 0.0f for the others; the winner is taken by the rule, serially.
 *
 * orc_label_resample: output planes [z0, z1) of an (ox, oy, oz) output through the affine map A.
 * orc_label_warp:     the same through A and a displacement field (section 7e's position arithmetic, restated here).
 * orc_label_scores:   per output voxel the winner's score and the largest score among the other classes (-1.0f where there is
 *                     no other class, both -1.0f where the voxel maps outside); returns the number of inside voxels.
 */
#include <math.h>
#include <stdint.h>

static float at(const float *v, int64_t nx, int64_t ny, int64_t x, int64_t y, int64_t z) { return v[(z * ny + y) * nx + x]; }

static int one_class(float a, float b)
{
    const int fa = isfinite(a), fb = isfinite(b);
    if (fa && fb) return a == b;
    return !fa && !fb;
}

/* 1: class a (value va, score sa) is before class b under the winner rule */
static int before(float va, float sa, float vb, float sb)
{
    if (sa > sb) return 1;
    if (sa < sb) return 0;
    const int fa = isfinite(va), fb = isfinite(vb);
    if (fa != fb) return fa;
    return fa && va < vb;
}

/* q inside the source: the vote at q; top / second (may be NULL): the winner's score and the best other class' */
static float vote_at(const float *src, int64_t nx, int64_t ny, int64_t nz, const float q[3], float *top, float *second)
{
    const int64_t n[3] = {nx, ny, nz};
    int64_t lo[3], hi[3];
    float w[3], u[3];
    for (int r = 0; r < 3; r++) {
        const float f = floorf(q[r]);
        w[r] = q[r] - f;
        u[r] = 1.0f - w[r];
        lo[r] = (int64_t)f;
        hi[r] = lo[r] + 1 <= n[r] - 1 ? lo[r] + 1 : n[r] - 1;
    }
    float L[8], W[8];
    for (int c = 0; c < 8; c++) {
        const int a = c & 1, b = (c >> 1) & 1, d = c >> 2;
        L[c] = at(src, nx, ny, a ? hi[0] : lo[0], b ? hi[1] : lo[1], d ? hi[2] : lo[2]);
        const float xy = (a ? w[0] : u[0]) * (b ? w[1] : u[1]);
        W[c] = xy * (d ? w[2] : u[2]);
    }
    /* the classes, each named by its lowest-numbered corner */
    int head[8], nc = 0;
    float score[8];
    for (int c = 0; c < 8; c++) {
        int seen = 0;
        for (int e = 0; e < c; e++) seen |= one_class(L[e], L[c]);
        if (seen) continue;
        float s = one_class(L[c], L[0]) ? W[0] : 0.0f;
        for (int e = 1; e < 8; e++) s = s + (one_class(L[c], L[e]) ? W[e] : 0.0f);
        head[nc] = c;
        score[nc] = s;
        nc++;
    }
    int win = 0;
    for (int k = 1; k < nc; k++)
        if (before(L[head[k]], score[k], L[head[win]], score[win])) win = k;
    if (top) *top = score[win];
    if (second) {
        float s2 = -1.0f;
        for (int k = 0; k < nc; k++)
            if (k != win && score[k] > s2) s2 = score[k];
        *second = s2;
    }
    return isfinite(L[head[win]]) ? L[head[win]] : NAN;
}

static void affine_position(const float *A, int64_t i, int64_t j, int64_t k, float q[3])
{
    const float p[3] = {(float)i, (float)j, (float)k};
    for (int r = 0; r < 3; r++) {
        float s = A[4 * r] * p[0];
        s = s + A[4 * r + 1] * p[1];
        s = s + A[4 * r + 2] * p[2];
        q[r] = s + A[4 * r + 3];
    }
}

static int inside(const float q[3], int64_t nx, int64_t ny, int64_t nz)
{
    const int64_t n[3] = {nx, ny, nz};
    for (int r = 0; r < 3; r++) {
        const float top = (float)(n[r] - 1);
        if (!(q[r] >= 0.0f) || !(q[r] <= top)) return 0; /* NaN fails both */
    }
    return 1;
}

int orc_label_resample(const float *src, int64_t nx, int64_t ny, int64_t nz, float *dst, int64_t ox, int64_t oy, int64_t oz, const float *A,
                       float fill, int64_t z0, int64_t z1)
{
    if (nx < 1 || ny < 1 || nz < 1 || ox < 1 || oy < 1 || oz < 1 || z0 < 0 || z1 > oz || z1 < z0) return -1;
    for (int64_t k = z0; k < z1; k++)
        for (int64_t j = 0; j < oy; j++)
            for (int64_t i = 0; i < ox; i++) {
                float q[3];
                affine_position(A, i, j, k, q);
                dst[((k - z0) * oy + j) * ox + i] = inside(q, nx, ny, nz) ? vote_at(src, nx, ny, nz, q, 0, 0) : fill;
            }
    return 0;
}

int64_t orc_label_scores(const float *src, int64_t nx, int64_t ny, int64_t nz, int64_t ox, int64_t oy, int64_t oz, const float *A, float *top,
                         float *second)
{
    if (nx < 1 || ny < 1 || nz < 1 || ox < 1 || oy < 1 || oz < 1) return -1;
    int64_t in = 0;
    for (int64_t k = 0; k < oz; k++)
        for (int64_t j = 0; j < oy; j++)
            for (int64_t i = 0; i < ox; i++) {
                const int64_t o = (k * oy + j) * ox + i;
                float q[3];
                affine_position(A, i, j, k, q);
                top[o] = second[o] = -1.0f;
                if (!inside(q, nx, ny, nz)) continue;
                vote_at(src, nx, ny, nz, q, top + o, second + o);
                in++;
            }
    return in;
}

/* ---- through a field: section 7e's position ---- */

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

int orc_label_warp(const float *src, int64_t nx, int64_t ny, int64_t nz, float *dst, int64_t ox, int64_t oy, int64_t oz, const float *A, const float *C,
                   const float *K, const float *disp, const int64_t *nn, const float *o, float h, float fill, int64_t z0, int64_t z1)
{
    if (nx < 1 || ny < 1 || nz < 1 || ox < 1 || oy < 1 || oz < 1 || z0 < 0 || z1 > oz || z1 < z0) return -1;
    for (int64_t k = z0; k < z1; k++)
        for (int64_t j = 0; j < oy; j++)
            for (int64_t i = 0; i < ox; i++) {
                float q[3], kap[3], g[3], d[3];
                affine_position(A, i, j, k, q);
                affine_position(C, i, j, k, kap);
                for (int r = 0; r < 3; r++) g[r] = (kap[r] - o[r]) / h;
                if (field_at(disp, nn, g, d))
                    for (int r = 0; r < 3; r++) {
                        float s = K[3 * r] * d[0];
                        s = s + K[3 * r + 1] * d[1];
                        s = s + K[3 * r + 2] * d[2];
                        q[r] = q[r] + s;
                    }
                dst[((k - z0) * oy + j) * ox + i] = inside(q, nx, ny, nz) ? vote_at(src, nx, ny, nz, q, 0, 0) : fill;
            }
    return 0;
}
