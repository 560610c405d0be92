/*
 * keypoint_math_check.cpp -- the scalar arithmetic of the per-keypoint kernels (3d_sift_cuda_amd/csrc/keypoint_math.h) on the
 * CPU.  Stand-alone (tests/test_keypoint_math_cpu.py builds it with the oracle's source, once plain and once under
 * AddressSanitizer + UndefinedBehaviorSanitizer).  The header's functions, compiled for the host, against the oracle's, bit for
 * bit (memcmp), on inputs from a fixed-seed generator:
 *   svd3_sort_eig      svd3 + sort_eig against o3_svd3 + o3_sort_eig: float Gram matrices of 3 .. 39 gradient triples, summed
 *                      in float in index order as the kernel's nine chains sum them, at scales 1e-3, 1 and 1e3; fixed shares
 *                      with one component zero throughout (rank 2), with two components equal throughout, and all zero; w
 *                      and v start at zero on both sides, as the kernel starts them
 *   invert3            against o3_invert3: the sorted eigenvector matrices of the family above, then 2 000 matrices that are
 *                      not orthogonal, with determinants down to 1e-6
 *   interp_quadratic   against o3_interp_quadratic: integer abscissae x - 1, x, x + 1 (x = 0 .. 99) and the three sigmas of a
 *                      level (1.6 * 2^(l/3)); random ordinates, and fixed shares with f1 == f0 (no strict extremum), all
 *                      zero, and collinear
 *   interp_point_patch against o3_interp_point on an 11^3 grid: every interior voxel of 20 random grids
 * and one property that has no oracle export:
 *   in_radius          485 of the 1331 voxels (NRAD: the lattice points with x^2 + y^2 + z^2 < 25, counted here from that
 *                      definition in integers), each with its three coordinates in 1 .. 9, the set symmetric under the
 *                      negation of each axis
 * Prints "<family> <cases> <bad>" per family; exits 1 if any case was bad.
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "keypoint_math.h"
#include "sift3d_oracle.h"

#define PD KEYPOINT_MATH_PD
#define PV (PD * PD * PD)

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd32()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 32);
}
static float rndu() { return (float)(rnd32() >> 8) * (1.0f / 16777216.0f); } /* [0, 1) */
static float rnds() { return 2.0f * rndu() - 1.0f; }

static int report(const char *family, int n, int bad)
{
    printf("%s %d %d\n", family, n, bad);
    return bad;
}

/* both sides' inverse of the row-major 3x3 m */
static bool invert_agrees(const float *m)
{
    float mine[9], in[3][3], theirs[3][3];
    memcpy(in, m, sizeof(in));
    invert3(m, mine);
    o3_invert3(in, theirs);
    return memcmp(mine, theirs, sizeof(mine)) == 0;
}

int main()
{
    int any_bad = 0;
    {
        const int n = 200000;
        const float scales[3] = {1e-3f, 1.0f, 1e3f};
        int bad_svd = 0, bad_inv = 0;
        for (int k = 0; k < n; k++) {
            const int kind = k % 1000 == 2 ? 3 : (k % 16 == 0 ? 1 : (k % 16 == 1 ? 2 : 0)); /* 1: rank 2, 2: two equal, 3: zero */
            const float scale = scales[(k / 16) % 3];
            const int terms = 3 + (int)(rnd32() % 37u), zeroed = (int)(rnd32() % 3u);
            float mat[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
            for (int t = 0; t < terms; t++) {
                float g[3] = {scale * rnds(), scale * rnds(), scale * rnds()};
                if (kind == 1) g[zeroed] = 0;
                if (kind == 2) g[(zeroed + 1) % 3] = g[zeroed];
                if (kind == 3) g[0] = g[1] = g[2] = 0;
                for (int i = 0; i < 3; i++)
                    for (int j = 0; j < 3; j++) mat[i][j] += g[i] * g[j];
            }
            float a[3][3], w[3] = {0, 0, 0}, v[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
            float oa[3][3], ow[3] = {0, 0, 0}, ov[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
            memcpy(a, mat, sizeof(a));
            memcpy(oa, mat, sizeof(oa));
            svd3(a, w, v);
            sort_eig(w, v);
            o3_svd3(oa, ow, ov);
            o3_sort_eig(ow, ov);
            if (memcmp(w, ow, sizeof(w)) != 0 || memcmp(v, ov, sizeof(v)) != 0) bad_svd++;
            if (!invert_agrees(&v[0][0])) bad_inv++;
        }
        any_bad |= report("svd3_sort_eig", n, bad_svd);
        const int skewed = 2000;
        for (int k = 0; k < skewed; k++) { /* the third row: a combination of the first two plus a little of its own */
            float m[9];
            for (int i = 0; i < 6; i++) m[i] = rnds();
            const float own = powf(10.0f, -6.0f * rndu()), c0 = rnds(), c1 = rnds();
            for (int i = 0; i < 3; i++) m[6 + i] = c0 * m[i] + c1 * m[3 + i] + own * rnds();
            if (!invert_agrees(m)) bad_inv++;
        }
        any_bad |= report("invert3", n + skewed, bad_inv);
    }
    {
        const int n = 200000;
        int bad = 0;
        float sigma[6];
        for (int l = 0; l < 6; l++) sigma[l] = (float)(1.6 * pow(2.0, l / 3.0));
        for (int k = 0; k < n; k++) {
            double x0, x1, x2;
            if (k % 2 == 0) {
                const int x = (int)(rnd32() % 100u);
                x0 = x - 1; x1 = x; x2 = x + 1;
            } else { /* higher, centre, lower -- and the other way round */
                const int l = (int)(rnd32() % 4u);
                x0 = sigma[l + 2]; x1 = sigma[l + 1]; x2 = sigma[l];
                if (k % 4 == 3) { const double t = x0; x0 = x2; x2 = t; }
            }
            float f0 = rnds(), f1 = rnds(), f2 = rnds();
            if (k % 10 == 4) f1 = f0;
            if (k % 10 == 5) f0 = f1 = f2 = 0;
            if (k % 10 == 6) { /* on one line over the abscissae */
                const float slope = k % 20 == 6 ? 0.0f : rnds();
                f0 = (float)(f1 + slope * (x0 - x1));
                f2 = (float)(f1 + slope * (x2 - x1));
            }
            const double mine = interp_quadratic(x0, x1, x2, f0, f1, f2), theirs = o3_interp_quadratic(x0, x1, x2, f0, f1, f2);
            if (memcmp(&mine, &theirs, sizeof(mine)) != 0) bad++;
        }
        any_bad |= report("interp_quadratic", n, bad);
    }
    {
        static float grid[PV];
        int n = 0, bad = 0;
        for (int g = 0; g < 20; g++) {
            for (int s = 0; s < PV; s++) grid[s] = g % 5 == 4 && rnd32() % 3u == 0 ? 0.0f : rnds();
            for (int z = 1; z < PD - 1; z++)
                for (int y = 1; y < PD - 1; y++)
                    for (int x = 1; x < PD - 1; x++) {
                        float mine[3], theirs[3];
                        interp_point_patch(grid, (z * PD + y) * PD + x, mine);
                        o3_interp_point(grid, PD, PD, PD, x, y, z, &theirs[0], &theirs[1], &theirs[2]);
                        if (memcmp(mine, theirs, sizeof(mine)) != 0) bad++;
                        n++;
                    }
        }
        any_bad |= report("interp_point_patch", n, bad);
    }
    {
        int inside = 0, lattice = 0, bad = 0;
        for (int s = 0; s < PV; s++) {
            const int x = s % PD, y = (s / PD) % PD, z = s / (PD * PD), h = PD / 2;
            const bool in = in_radius(s);
            inside += in ? 1 : 0;
            lattice += (x - h) * (x - h) + (y - h) * (y - h) + (z - h) * (z - h) < h * h ? 1 : 0;
            if (in && (x < 1 || x > PD - 2 || y < 1 || y > PD - 2 || z < 1 || z > PD - 2)) bad++;
            if (in != in_radius((z * PD + y) * PD + (PD - 1 - x)) || in != in_radius((z * PD + (PD - 1 - y)) * PD + x) ||
                in != in_radius(((PD - 1 - z) * PD + y) * PD + x))
                bad++;
        }
        if (inside != 485 || lattice != 485) bad++;
        any_bad |= report("in_radius", PV, bad);
    }
    return any_bad ? 1 : 0;
}
