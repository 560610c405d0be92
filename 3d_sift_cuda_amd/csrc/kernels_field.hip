/*
 * kernels_field.hip -- the nonrigid alignment's hot path for gfx950 (MI355X): the fit of a keypoint displacement field on a
 * node grid and the warp of a volume through a similarity plus that field.  Beyond the reference.
 *
 * field_fit_kernel.  One node per lane.  A 256-thread workgroup owns a brick of 8 x 8 x 4 nodes and each wave a 4 x 4 x 4
 * part of it (16 key units a side at the default spacing, less than one cell), so the lanes of a wave walk nearly the same
 * cells and read the same samples.  The samples are binned on the host into cells of edge >= R (1 + 2^-10), sorted by cell,
 * positions and values as float4; a lane walks the 3 x 3 rows of three cells around its node's cell.  Per sample, in float:
 *   dx = y.x - P.x, d2 = ((dx dx + dy dy) + dz dz); only d2 < R R counts; t = 1 - d2 / (R R), w = (t t) t;
 *   W += rint(w 2^24), V_c += rint((w v_c) 2^24) in int64.
 * The sums are integers, so the walking order does not matter; the node's value is (float)((double)V_c / ((double)W +
 * lambda 2^24)), 0 where the denominator is 0.  Only + - x / on floats: no transcendental differs between host and device.
 *
 * field_warp_kernel.  section 7c's resampler (kernels_resample.hip: the brick of 32 x 8 x 4 voxels, four x voxels per thread,
 * the XCD dealing) with one added term: the fixed key position kappa = C p (the map's order), g = (kappa - o) / h, and where
 * 0 <= g <= n - 1 on every axis the trilinear interpolation v of the float4 nodes (one dwordx4 load per corner; section 7c's
 * floor, weights, clamp and x -> y -> z order), added as q_r += ((K[r][0] v0 + K[r][1] v1) + K[r][2] v2).  Outside the grid
 * q is left as it is.
 *
 * -ffp-contract=off and no -fno-honor-nans (Makefile): a NaN position fails the inside test, a NaN node reaches q.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#define FF_BX 8
#define FF_BY 8
#define FF_BZ 4
#define FF_MAX_GRID (1u << 20)

struct ff_cells {
    double o[3], edge;
    long long n[3];
};

struct ff_nodes {
    float o[3], h;
    long long n[3];
};

__global__ __launch_bounds__(256) void field_fit_kernel(const float4 *__restrict__ ys, const float4 *__restrict__ vs, const int *__restrict__ start,
                                                        ff_cells cg, ff_nodes g, float rr, double lam24, float *__restrict__ out, long long nb0,
                                                        long long nb1, long long nbricks)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int lx = (lane & 3) + (wv & 1) * 4, ly = ((lane >> 2) & 3) + (wv >> 1) * 4, lz = lane >> 4;
    const long long N = g.n[0] * g.n[1] * g.n[2];
    for (long long L = blockIdx.x; L < nbricks; L += gridDim.x) {
        const long long bx = L % nb0, t0 = L / nb0, by = t0 % nb1, bz = t0 / nb1;
        const long long a = bx * FF_BX + lx, b = by * FF_BY + ly, c = bz * FF_BZ + lz;
        if (a >= g.n[0] || b >= g.n[1] || c >= g.n[2]) continue;
        const float p[3] = {g.o[0] + (float)a * g.h, g.o[1] + (float)b * g.h, g.o[2] + (float)c * g.h};
        long long lo[3], hi[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            /* the node's cell, possibly outside the cell grid by a few cells (the nodes reach R past the samples) */
            const double u = floor(((double)p[k] - cg.o[k]) / cg.edge);
            const long long ci = u < -2.0 ? -2 : (u > (double)(cg.n[k] + 1) ? cg.n[k] + 1 : (long long)u);
            lo[k] = ci - 1 > 0 ? ci - 1 : 0;
            hi[k] = ci + 1 < cg.n[k] - 1 ? ci + 1 : cg.n[k] - 1;
        }
        long long W = 0, V0 = 0, V1 = 0, V2 = 0;
        if (lo[0] <= hi[0])
            for (long long cz = lo[2]; cz <= hi[2]; cz++)
                for (long long cy = lo[1]; cy <= hi[1]; cy++) {
                    const long long row = (cz * cg.n[1] + cy) * cg.n[0];
                    const int s1 = start[row + hi[0] + 1];
                    for (int s = start[row + lo[0]]; s < s1; s++) {
                        const float4 y = ys[s];
                        const float dx = y.x - p[0], dy = y.y - p[1], dz = y.z - p[2];
                        const float d2 = (dx * dx + dy * dy) + dz * dz;
                        if (!(d2 < rr)) continue;
                        const float t = 1.0f - d2 / rr;
                        const float w = (t * t) * t;
                        const float4 v = vs[s];
                        W += (long long)rintf(w * 16777216.0f);
                        V0 += (long long)rintf((w * v.x) * 16777216.0f);
                        V1 += (long long)rintf((w * v.y) * 16777216.0f);
                        V2 += (long long)rintf((w * v.z) * 16777216.0f);
                    }
                }
        const double den = (double)W + lam24;
        const long long i = (c * g.n[1] + b) * g.n[0] + a;
        out[i] = den == 0.0 ? 0.0f : (float)((double)V0 / den);
        out[N + i] = den == 0.0 ? 0.0f : (float)((double)V1 / den);
        out[2 * N + i] = den == 0.0 ? 0.0f : (float)((double)V2 / den);
    }
}

/* The sample cells: cg.n cells, start[cg.n0 cg.n1 cg.n2 + 1]; out: 3 N floats, component-major. */
hipError_t sift3d_launch_field_fit(hipStream_t s, const float4 *ys, const float4 *vs, const int *start, const double co[3], double edge,
                                   const long long cn[3], const float o[3], float h, const long long n[3], float rr, double lam24, float *out)
{
    ff_cells cg;
    ff_nodes g;
    for (int k = 0; k < 3; k++) {
        cg.o[k] = co[k];
        cg.n[k] = cn[k];
        g.o[k] = o[k];
        g.n[k] = n[k];
    }
    cg.edge = edge;
    g.h = h;
    const long long nb0 = (n[0] + FF_BX - 1) / FF_BX, nb1 = (n[1] + FF_BY - 1) / FF_BY, nb2 = (n[2] + FF_BZ - 1) / FF_BZ;
    const long long nbricks = nb0 * nb1 * nb2;
    const unsigned grid = (unsigned)(nbricks < (long long)FF_MAX_GRID ? nbricks : FF_MAX_GRID);
    hipLaunchKernelGGL(field_fit_kernel, dim3(grid), dim3(256), 0, s, ys, vs, start, cg, g, rr, lam24, out, nb0, nb1, nbricks);
    return hipGetLastError();
}

#define FW_TX 8
#define FW_VX 4
#define FW_BX (FW_TX * FW_VX)
#define FW_BY 8
#define FW_BZ 4
#define FW_MAX_GRID (1u << 22)

struct fw_map {
    float a[12]; /* output voxel -> moving voxel (section 7c) */
    float c[12]; /* output voxel -> fixed key */
    float k[9];  /* moving key displacement -> moving voxel displacement */
    float o[3], h;
    float top[3]; /* (float)(n - 1) of the node grid */
    long long n[3];
};

template <int NEAREST>
__global__ __launch_bounds__(256) void field_warp_kernel(const float *__restrict__ src, long long nx, long long ny, long long nz, float *__restrict__ dst,
                                                         long long ox, long long oy, long long oz, fw_map m, const float4 *__restrict__ nodes, float fill,
                                                         long long nbx, long long nby, long long nbricks, int vec)
{
    const unsigned grid = gridDim.x, b = blockIdx.x;
    const long long slot0 = (long long)(b & 7u) * (grid >> 3) + (b >> 3);
    const int tx = threadIdx.x & (FW_TX - 1), ty = (threadIdx.x / FW_TX) & (FW_BY - 1), tz = threadIdx.x / (FW_TX * FW_BY);
    const float hx = (float)(nx - 1), hy = (float)(ny - 1), hz = (float)(nz - 1);
    const long long gn0 = m.n[0], gn1 = m.n[1];
    for (long long L = slot0; L < nbricks; L += grid) {
        const long long bx = L % nbx, t = L / nbx, by = t % nby, bz = t / nby;
        const long long i0 = bx * FW_BX + tx * FW_VX, j = by * FW_BY + ty, k = bz * FW_BZ + tz;
        if (j >= oy || k >= oz || i0 >= ox) continue;
        const float py = (float)j, pz = (float)k;
        float r[FW_VX];
#pragma unroll
        for (int v = 0; v < FW_VX; v++) {
            const float px = (float)(i0 + v);
            float qx = ((m.a[0] * px + m.a[1] * py) + m.a[2] * pz) + m.a[3];
            float qy = ((m.a[4] * px + m.a[5] * py) + m.a[6] * pz) + m.a[7];
            float qz = ((m.a[8] * px + m.a[9] * py) + m.a[10] * pz) + m.a[11];
            const float kx = ((m.c[0] * px + m.c[1] * py) + m.c[2] * pz) + m.c[3];
            const float ky = ((m.c[4] * px + m.c[5] * py) + m.c[6] * pz) + m.c[7];
            const float kz = ((m.c[8] * px + m.c[9] * py) + m.c[10] * pz) + m.c[11];
            const float gx = (kx - m.o[0]) / m.h, gy = (ky - m.o[1]) / m.h, gz = (kz - m.o[2]) / m.h;
            if (gx >= 0.0f && gx <= m.top[0] && gy >= 0.0f && gy <= m.top[1] && gz >= 0.0f && gz <= m.top[2]) {
                const float fx = floorf(gx), fy = floorf(gy), fz = floorf(gz);
                const float wx = gx - fx, wy = gy - fy, wz = gz - fz;
                const long long x0 = (int)fx, y0 = (int)fy, z0 = (int)fz;
                const long long x1 = x0 + 1 < gn0 - 1 ? x0 + 1 : gn0 - 1, y1 = y0 + 1 < gn1 - 1 ? y0 + 1 : gn1 - 1,
                                z1 = z0 + 1 < m.n[2] - 1 ? z0 + 1 : m.n[2] - 1;
                const float4 *r00 = nodes + (z0 * gn1 + y0) * gn0, *r10 = nodes + (z0 * gn1 + y1) * gn0, *r01 = nodes + (z1 * gn1 + y0) * gn0,
                             *r11 = nodes + (z1 * gn1 + y1) * gn0;
                const float4 a00 = r00[x0], b00 = r00[x1], a10 = r10[x0], b10 = r10[x1], a01 = r01[x0], b01 = r01[x1], a11 = r11[x0],
                             b11 = r11[x1];
                const float ux = 1.0f - wx, uy = 1.0f - wy, uz = 1.0f - wz;
                float d[3];
#define FW_COMP(C, f)                                                                                  \
    {                                                                                                  \
        const float c00 = ux * a00.f + wx * b00.f, c10 = ux * a10.f + wx * b10.f;                       \
        const float c01 = ux * a01.f + wx * b01.f, c11 = ux * a11.f + wx * b11.f;                       \
        const float c0 = uy * c00 + wy * c10, c1 = uy * c01 + wy * c11;                                 \
        d[C] = uz * c0 + wz * c1;                                                                      \
    }
                FW_COMP(0, x)
                FW_COMP(1, y)
                FW_COMP(2, z)
#undef FW_COMP
                qx = qx + ((m.k[0] * d[0] + m.k[1] * d[1]) + m.k[2] * d[2]);
                qy = qy + ((m.k[3] * d[0] + m.k[4] * d[1]) + m.k[5] * d[2]);
                qz = qz + ((m.k[6] * d[0] + m.k[7] * d[1]) + m.k[8] * d[2]);
            }
            r[v] = fill;
            if (!(qx >= 0.0f && qx <= hx && qy >= 0.0f && qy <= hy && qz >= 0.0f && qz <= hz)) continue;
            if (NEAREST) {
                long long ix = (int)floorf(qx + 0.5f), iy = (int)floorf(qy + 0.5f), iz = (int)floorf(qz + 0.5f);
                ix = ix < nx - 1 ? ix : nx - 1;
                iy = iy < ny - 1 ? iy : ny - 1;
                iz = iz < nz - 1 ? iz : nz - 1;
                r[v] = src[(iz * ny + iy) * nx + ix];
            } else {
                const float fx = floorf(qx), fy = floorf(qy), fz = floorf(qz);
                const float wx = qx - fx, wy = qy - fy, wz = qz - fz;
                const long long x0 = (int)fx, y0 = (int)fy, z0 = (int)fz;
                const long long x1 = x0 + 1 < nx - 1 ? x0 + 1 : nx - 1, y1 = y0 + 1 < ny - 1 ? y0 + 1 : ny - 1,
                                z1 = z0 + 1 < nz - 1 ? z0 + 1 : nz - 1;
                const float *r00 = src + (z0 * ny + y0) * nx, *r10 = src + (z0 * ny + y1) * nx, *r01 = src + (z1 * ny + y0) * nx,
                            *r11 = src + (z1 * ny + y1) * nx;
                const float ux = 1.0f - wx, uy = 1.0f - wy, uz = 1.0f - wz;
                const float c00 = ux * r00[x0] + wx * r00[x1];
                const float c10 = ux * r10[x0] + wx * r10[x1];
                const float c01 = ux * r01[x0] + wx * r01[x1];
                const float c11 = ux * r11[x0] + wx * r11[x1];
                const float c0 = uy * c00 + wy * c10, c1 = uy * c01 + wy * c11;
                r[v] = uz * c0 + wz * c1;
            }
        }
        float *o = dst + (k * oy + j) * ox + i0;
        if (vec && i0 + FW_VX <= ox) {
            *reinterpret_cast<float4 *>(o) = make_float4(r[0], r[1], r[2], r[3]);
        } else {
#pragma unroll
            for (int v = 0; v < FW_VX; v++)
                if (i0 + v < ox) o[v] = r[v];
        }
    }
}

/* map, c: 12 floats (3 x 4 row-major); k: 9; the node grid n (each 2 .. 2^24), origin o, spacing h; nodes: float4 (v0, v1,
 * v2, 0), x fastest.  The caller has checked the shapes. */
hipError_t sift3d_launch_field_warp(hipStream_t s, const float *src, int64_t nx, int64_t ny, int64_t nz, float *dst, int64_t ox, int64_t oy,
                                    int64_t oz, const float *map, const float *c, const float *k, const float o[3], float h, const int64_t n[3],
                                    const float4 *nodes, int nearest, float fill)
{
    fw_map m;
    for (int r = 0; r < 12; r++) {
        m.a[r] = map[r];
        m.c[r] = c[r];
    }
    for (int r = 0; r < 9; r++) m.k[r] = k[r];
    for (int r = 0; r < 3; r++) {
        m.o[r] = o[r];
        m.n[r] = n[r];
        m.top[r] = (float)(n[r] - 1);
    }
    m.h = h;
    const long long nbx = (ox + FW_BX - 1) / FW_BX, nby = (oy + FW_BY - 1) / FW_BY, nbz = (oz + FW_BZ - 1) / FW_BZ;
    const long long nbricks = nbx * nby * nbz;
    long long g = (nbricks + 7) / 8 * 8;
    if (g > (long long)FW_MAX_GRID) g = FW_MAX_GRID;
    const int vec = (ox % FW_VX) == 0 && ((uintptr_t)dst % 16) == 0;
    if (nearest)
        hipLaunchKernelGGL(field_warp_kernel<1>, dim3((unsigned)g), dim3(256), 0, s, src, (long long)nx, (long long)ny, (long long)nz, dst,
                           (long long)ox, (long long)oy, (long long)oz, m, nodes, fill, nbx, nby, nbricks, vec);
    else
        hipLaunchKernelGGL(field_warp_kernel<0>, dim3((unsigned)g), dim3(256), 0, s, src, (long long)nx, (long long)ny, (long long)nz, dst,
                           (long long)ox, (long long)oy, (long long)oz, m, nodes, fill, nbx, nby, nbricks, vec);
    return hipGetLastError();
}
