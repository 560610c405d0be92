/*
 * kernels_field.hip -- the nonrigid alignment's hot path for gfx950 (MI355X): the fit of a keypoint displacement field on a
 * node grid and the warp of a volume through a similarity plus that field.  Beyond the reference.
 *
 * field_fit_kernel.  One node per lane, in warp_device.h's brick of 8 x 8 x 4 nodes: a wave's 4 x 4 x 4 part is 16 key units
 * a side at the default spacing, less than one cell, so the lanes of a wave walk nearly the same cells and read the same
 * samples.  The samples are binned on the host into cells of edge >= R (1 + 2^-10), sorted by cell,
 * positions and values as float4; a lane walks the 3 x 3 rows of three cells around its node's cell.  Per sample, in float:
 *   dx = y.x - P.x, d2 = ((dx dx + dy dy) + dz dz); only d2 < R R counts; t = 1 - d2 / (R R), w = (t t) t;
 *   W += rint(w 2^24), V_c += rint((w v_c) 2^24) in int64.
 * The sums are integers, so the walking order does not matter; the node's value is (float)((double)V_c / ((double)W +
 * lambda 2^24)), 0 where the denominator is 0.  Only + - x / on floats: no transcendental differs between host and device.
 *
 * field_warp_kernel.  section 7c's resampler with the field's term added to the position: warp_device.h's brick of output
 * voxels, warp_position<1> and sample_volume; its header states the contract.
 *
 * -ffp-contract=off and no -fno-honor-nans (Makefile): a NaN position fails the inside test, a NaN node reaches q.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "warp_device.h"

struct ff_cells {
    double o[3], edge;
    long long n[3];
};

__global__ __launch_bounds__(256) void field_fit_kernel(const float4 *__restrict__ ys, const float4 *__restrict__ vs, const int *__restrict__ start,
                                                        ff_cells cg, node_grid g, float rr, double lam24, float *__restrict__ out, long long nb0,
                                                        long long nb1, long long nbricks)
{
    int lx, ly, lz;
    node_lane(lx, ly, lz);
    const long long N = g.n[0] * g.n[1] * g.n[2];
    for (long long L = blockIdx.x; L < nbricks; L += gridDim.x) {
        long long a, b, c;
        node_of_slot(L, nb0, nb1, lx, ly, lz, a, b, c);
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
                                   const long long cn[3], const float o[3], float h, const int64_t n[3], float rr, double lam24, float *out)
{
    ff_cells cg;
    node_grid g;
    for (int k = 0; k < 3; k++) {
        cg.o[k] = co[k];
        cg.n[k] = cn[k];
    }
    cg.edge = edge;
    fill_node_grid(g, o, h, n);
    const node_launch b = node_launch_of(n);
    hipLaunchKernelGGL(field_fit_kernel, dim3(b.grid), dim3(256), 0, s, ys, vs, start, cg, g, rr, lam24, out, b.nb0, b.nb1, b.nbricks);
    return hipGetLastError();
}

template <int MODE>
__global__ __launch_bounds__(256) void field_warp_kernel(const float *__restrict__ src, long long nx, long long ny, long long nz, float *__restrict__ dst,
                                                         long long ox, long long oy, long long oz, warp_map m, const float4 *__restrict__ nodes, float fill,
                                                         long long nbx, long long nby, long long nbricks, int vec)
{
    int tx, ty, tz;
    brick_lane(tx, ty, tz);
    const float hx = (float)(nx - 1), hy = (float)(ny - 1), hz = (float)(nz - 1);
    for (long long L = brick_slot0(); L < nbricks; L += gridDim.x) {
        long long i0, j, k;
        brick_voxel(L, nbx, nby, tx, ty, tz, i0, j, k);
        if (j >= oy || k >= oz || i0 >= ox) continue;
        float r[BRICK_VX];
#pragma unroll
        for (int v = 0; v < BRICK_VX; v++) {
            float q[3];
            warp_position<1>(m, nodes, (float)(i0 + v), (float)j, (float)k, q);
            r[v] = sample_volume<MODE>(src, nx, ny, nz, hx, hy, hz, q[0], q[1], q[2], fill);
        }
        store_row4(dst + (k * oy + j) * ox + i0, ox, i0, r, vec);
    }
}

/* map, c: 12 floats (3 x 4 row-major); k: 9; the node grid n (each 2 .. 2^24), origin o, spacing h; nodes: float4 (v0, v1,
 * v2, 0), x fastest; mode: a sift3d_interp.  The caller has checked the shapes and the mode. */
hipError_t sift3d_launch_field_warp(hipStream_t s, const float *src, int64_t nx, int64_t ny, int64_t nz, float *dst, int64_t ox, int64_t oy,
                                    int64_t oz, const float *map, const float *c, const float *k, const float o[3], float h, const int64_t n[3],
                                    const float4 *nodes, int mode, float fill)
{
    warp_map m;
    fill_warp_map(m, map, c, k, true, o, h, n);
    const brick_launch b = brick_launch_of(dst, ox, oy, oz);
    auto kernel = mode == WARP_LABEL ? field_warp_kernel<WARP_LABEL> : mode == WARP_NEAREST ? field_warp_kernel<WARP_NEAREST> : field_warp_kernel<WARP_LINEAR>;
    hipLaunchKernelGGL(kernel, dim3(b.grid), dim3(256), 0, s, src, (long long)nx, (long long)ny, (long long)nz, dst, (long long)ox, (long long)oy,
                       (long long)oz, m, nodes, fill, b.nbx, b.nby, b.nbricks, b.vec);
    return hipGetLastError();
}
