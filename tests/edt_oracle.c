/*
 * edt_oracle.c -- CPU oracle of the distance map and the surface distances (include/sift3d.h, "exact
 * Euclidean distance map").  Test infrastructure: built by tests/_helpers.c_oracle, never linked into the product.
 *
 * The map is a true brute force: every voxel against the list of all sites, three differences, three squares, one minimum.  It is
 * not separable and has no passes, tiles or chunks, so it shares no structure with the kernels.  The surface rule and the two
 * directed lists are written out serially, in voxel order.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

/* d2: one uint64 per voxel, written at every voxel (only NULL) or at those flagged in only; 0, or -1 without memory */
static int brute(const uint8_t *sites, const uint8_t *only, int64_t nx, int64_t ny, int64_t nz, const uint32_t sp[3], uint64_t *d2)
{
    const int64_t n = nx * ny * nz;
    int64_t ns = 0;
    for (int64_t i = 0; i < n; i++) ns += sites[i] != 0;
    int32_t *at = (int32_t *)malloc(sizeof(int32_t) * 3 * (size_t)(ns > 0 ? ns : 1));
    if (!at) return -1;
    ns = 0;
    for (int64_t z = 0; z < nz; z++)
        for (int64_t y = 0; y < ny; y++)
            for (int64_t x = 0; x < nx; x++)
                if (sites[(z * ny + y) * nx + x]) {
                    at[3 * ns] = (int32_t)x;
                    at[3 * ns + 1] = (int32_t)y;
                    at[3 * ns + 2] = (int32_t)z;
                    ns++;
                }
    for (int64_t z = 0; z < nz; z++)
        for (int64_t y = 0; y < ny; y++)
            for (int64_t x = 0; x < nx; x++) {
                if (only && !only[(z * ny + y) * nx + x]) continue;
                uint64_t best = UINT64_MAX;
                for (int64_t s = 0; s < ns; s++) {
                    const int64_t ax = (int64_t)sp[0] * (x - at[3 * s]), ay = (int64_t)sp[1] * (y - at[3 * s + 1]), az = (int64_t)sp[2] * (z - at[3 * s + 2]);
                    const uint64_t d = (uint64_t)(ax * ax) + (uint64_t)(ay * ay) + (uint64_t)(az * az);
                    if (d < best) best = d;
                }
                d2[(z * ny + y) * nx + x] = best;
            }
    free(at);
    return 0;
}

int oed_map(const uint8_t *sites, int64_t nx, int64_t ny, int64_t nz, const uint32_t sp[3], uint64_t *d2) { return brute(sites, NULL, nx, ny, nz, sp, d2); }

static int carries(const float *lab, int64_t nx, int64_t ny, int64_t nz, int64_t x, int64_t y, int64_t z, int32_t l)
{
    if (x < 0 || x >= nx || y < 0 || y >= ny || z < 0 || z >= nz) return 0;
    const float v = lab[(z * ny + y) * nx + x];
    return isfinite(v) && v == (float)l;
}

/* flags: 1 at the surface voxels of l; returns their number */
int64_t oed_surface(const float *lab, int64_t nx, int64_t ny, int64_t nz, int32_t l, uint8_t *flags)
{
    int64_t count = 0;
    for (int64_t z = 0; z < nz; z++)
        for (int64_t y = 0; y < ny; y++)
            for (int64_t x = 0; x < nx; x++) {
                const int s = carries(lab, nx, ny, nz, x, y, z, l) &&
                              !(carries(lab, nx, ny, nz, x - 1, y, z, l) && carries(lab, nx, ny, nz, x + 1, y, z, l) && carries(lab, nx, ny, nz, x, y - 1, z, l) &&
                                carries(lab, nx, ny, nz, x, y + 1, z, l) && carries(lab, nx, ny, nz, x, y, z - 1, l) && carries(lab, nx, ny, nz, x, y, z + 1, l));
                flags[(z * ny + y) * nx + x] = (uint8_t)s;
                count += s;
            }
    return count;
}

/* The two directed lists of the label l, each with room for nx ny nz values, in voxel order: list_ab[i] is the distance of the i-th
 * surface voxel of l in a to the nearest one in b (UINT64_MAX where b has none).  0, or -1 without memory. */
int oed_lists(const float *a, const float *b, int64_t nx, int64_t ny, int64_t nz, const uint32_t sp[3], int32_t l, uint64_t *list_ab, int64_t *n_a,
              uint64_t *list_ba, int64_t *n_b)
{
    const int64_t n = nx * ny * nz;
    uint8_t *fa = (uint8_t *)malloc((size_t)n), *fb = (uint8_t *)malloc((size_t)n);
    uint64_t *d2 = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)n);
    int rc = -1;
    if (fa && fb && d2) {
        oed_surface(a, nx, ny, nz, l, fa);
        oed_surface(b, nx, ny, nz, l, fb);
        *n_a = *n_b = 0;
        rc = brute(fb, fa, nx, ny, nz, sp, d2);
        for (int64_t i = 0; i < n && rc == 0; i++)
            if (fa[i]) list_ab[(*n_a)++] = d2[i];
        if (rc == 0) rc = brute(fa, fb, nx, ny, nz, sp, d2);
        for (int64_t i = 0; i < n && rc == 0; i++)
            if (fb[i]) list_ba[(*n_b)++] = d2[i];
    }
    free(fa);
    free(fb);
    free(d2);
    return rc;
}
