/*
 * resample_oracle.c -- CPU restatement of the resampling contract of DESIGN.md section 7c (test infrastructure; written
 * from that text, it includes none of the product's headers).  Built with cc -O2 -ffp-contract=off by
 * tests/resample_cases.py.
 *
 * orc_resample: output planes [z0, z1) of an (ox, oy, oz) output into dst ((z1 - z0) * oy * ox floats), so that outputs too
 * big for the host can be checked plane by plane.  interp 0: linear, 1: nearest.
 */
#include <math.h>
#include <stdint.h>

static float at(const float *v, int64_t nx, int64_t ny, int64_t x, int64_t y, int64_t z) { return v[(z * ny + y) * nx + x]; }

static float lerp(float a, float b, float w) { return (1.0f - w) * a + w * b; }

static float one_voxel(const float *src, int64_t nx, int64_t ny, int64_t nz, const float *A, int interp, float fill, int64_t i,
                       int64_t j, int64_t k)
{
    const float p[3] = {(float)i, (float)j, (float)k};
    const int64_t n[3] = {nx, ny, nz};
    float q[3];
    for (int r = 0; r < 3; r++) {
        float s = A[4 * r] * p[0];
        s = s + A[4 * r + 1] * p[1];
        s = s + A[4 * r + 2] * p[2];
        q[r] = s + A[4 * r + 3];
    }
    for (int r = 0; r < 3; r++) {
        const float top = (float)(n[r] - 1);
        if (!(q[r] >= 0.0f) || !(q[r] <= top)) return fill; /* NaN fails both */
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
    /* x first (four lines), then y (two), then z */
    const float e00 = lerp(at(src, nx, ny, lo[0], lo[1], lo[2]), at(src, nx, ny, hi[0], lo[1], lo[2]), w[0]);
    const float e10 = lerp(at(src, nx, ny, lo[0], hi[1], lo[2]), at(src, nx, ny, hi[0], hi[1], lo[2]), w[0]);
    const float e01 = lerp(at(src, nx, ny, lo[0], lo[1], hi[2]), at(src, nx, ny, hi[0], lo[1], hi[2]), w[0]);
    const float e11 = lerp(at(src, nx, ny, lo[0], hi[1], hi[2]), at(src, nx, ny, hi[0], hi[1], hi[2]), w[0]);
    return lerp(lerp(e00, e10, w[1]), lerp(e01, e11, w[1]), w[2]);
}

int orc_resample(const float *src, int64_t nx, int64_t ny, int64_t nz, float *dst, int64_t ox, int64_t oy, int64_t oz, const float *A,
                 int interp, float fill, int64_t z0, int64_t z1)
{
    if (nx < 1 || ny < 1 || nz < 1 || ox < 1 || oy < 1 || oz < 1 || z0 < 0 || z1 > oz || z1 < z0 || (interp != 0 && interp != 1)) return -1;
    for (int64_t k = z0; k < z1; k++)
        for (int64_t j = 0; j < oy; j++)
            for (int64_t i = 0; i < ox; i++) dst[((k - z0) * oy + j) * ox + i] = one_voxel(src, nx, ny, nz, A, interp, fill, i, j, k);
    return 0;
}
