/*
 * kernels_invert.hip -- the reverse direction of the nonrigid alignment for gfx950 (MI355X): the inverse of a displacement
 * field on a node grid of its own, and the Jacobian determinant map of a warp.  Beyond the reference.
 *
 * field_invert_kernel.  One node per lane, in warp_device.h's brick of 8 x 8 x 4 nodes, so the eight gathers of a wave's lanes
 * fall on neighbouring forward nodes (nodes_at, one dwordx4 load per corner).  Per node z (its float position, widened), with P = inv(M'),
 * Q = inv(M) and A = lin(M) as doubles from the host:
 *   b_r = ((P[r][0] z0 + P[r][1] z1) + P[r][2] z2) + P[r][3];  u = 0;  k = 0
 *   loop:  y = b + u;  v = the forward field at (float)y (nodes_at's float arithmetic; 0 outside its grid)
 *          r_c = ((((Q[c][0] y0 + Q[c][1] y1) + Q[c][2] y2) + Q[c][3]) + (double)v_c) - z_c;  rr = (r0 r0 + r1 r1) + r2 r2
 *          rr <= tol^2: converged, stop.  k == max_iter: not converged, stop.
 *          u_c = u_c - ((A[c][0] r0 + A[c][1] r1) + A[c][2] r2);  k = k + 1
 *          a component of u not within +-SIFT3D_FIELD_MAX_DISP (NaN included): u = 0, diverged, stop.
 * Written per node: (float)u, the word k | state << 16 (0 converged, 1 not converged, 2 diverged) and the last rr.  A lane
 * leaves the loop when its node stops, so a wave runs until its last lane has.
 *
 * jacobian_map_kernel<FORM>.  warp_device.h's brick of 32 x 8 x 4 output voxels.  q(p) is warp_position, the position that
 * field_warp_kernel samples the image at.  Per voxel D[r][a] = (q_r(p + e_a) - q_r(p - e_a)) 0.5f in float, the
 * determinant in double in sift3d_blockmatch_folds' order, times one double factor, rounded to float once.  FORM 0 evaluates q
 * six times per voxel; FORM 1 evaluates the brick and a one-voxel halo once into LDS (34 x 10 x 6 positions, 24 480 bytes)
 * and takes the differences from there.  Both give the same numbers: q at a position does not depend on who asks.
 *
 * -ffp-contract=off and no -fno-honor-nans (Makefile): a NaN position fails the inside test, a NaN node reaches u and J.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "warp_device.h"

#define FI_MAX_DISP 128.0 /* SIFT3D_FIELD_MAX_DISP */

struct fi_maps {
    double p[12], q[12], a[9], tol2;
    int max_iter, has_field;
};

__global__ __launch_bounds__(256) void field_invert_kernel(const float4 *__restrict__ fwd, node_grid f, node_grid g, fi_maps m, float *__restrict__ u_out,
                                                           unsigned *__restrict__ status, double *__restrict__ res2, long long nb0, long long nb1,
                                                           long long nbricks)
{
    int lx, ly, lz;
    node_lane(lx, ly, lz);
    const long long N = g.n[0] * g.n[1] * g.n[2];
    for (long long L = blockIdx.x; L < nbricks; L += gridDim.x) {
        long long a, b, c;
        node_of_slot(L, nb0, nb1, lx, ly, lz, a, b, c);
        if (a >= g.n[0] || b >= g.n[1] || c >= g.n[2]) continue;
        const double z0 = (double)(g.o[0] + (float)a * g.h), z1 = (double)(g.o[1] + (float)b * g.h), z2 = (double)(g.o[2] + (float)c * g.h);
        const double b0 = ((m.p[0] * z0 + m.p[1] * z1) + m.p[2] * z2) + m.p[3];
        const double b1 = ((m.p[4] * z0 + m.p[5] * z1) + m.p[6] * z2) + m.p[7];
        const double b2 = ((m.p[8] * z0 + m.p[9] * z1) + m.p[10] * z2) + m.p[11];
        double u0 = 0.0, u1 = 0.0, u2 = 0.0, rr;
        unsigned st;
        int k = 0;
        for (;;) {
            const double y0 = b0 + u0, y1 = b1 + u1, y2 = b2 + u2;
            float d[3] = {0.0f, 0.0f, 0.0f};
            bool inside;
            if (m.has_field) nodes_at(fwd, f.o, f.h, f.top, f.n, (float)y0, (float)y1, (float)y2, d, inside);
            const double r0 = ((((m.q[0] * y0 + m.q[1] * y1) + m.q[2] * y2) + m.q[3]) + (double)d[0]) - z0;
            const double r1 = ((((m.q[4] * y0 + m.q[5] * y1) + m.q[6] * y2) + m.q[7]) + (double)d[1]) - z1;
            const double r2 = ((((m.q[8] * y0 + m.q[9] * y1) + m.q[10] * y2) + m.q[11]) + (double)d[2]) - z2;
            rr = (r0 * r0 + r1 * r1) + r2 * r2;
            if (rr <= m.tol2) {
                st = (unsigned)k;
                break;
            }
            if (k == m.max_iter) {
                st = (unsigned)k | (1u << 16);
                break;
            }
            u0 = u0 - ((m.a[0] * r0 + m.a[1] * r1) + m.a[2] * r2);
            u1 = u1 - ((m.a[3] * r0 + m.a[4] * r1) + m.a[5] * r2);
            u2 = u2 - ((m.a[6] * r0 + m.a[7] * r1) + m.a[8] * r2);
            k++;
            if (!(u0 <= FI_MAX_DISP && u0 >= -FI_MAX_DISP && u1 <= FI_MAX_DISP && u1 >= -FI_MAX_DISP && u2 <= FI_MAX_DISP && u2 >= -FI_MAX_DISP)) {
                u0 = u1 = u2 = 0.0;
                st = (unsigned)k | (2u << 16);
                break;
            }
        }
        const long long i = (c * g.n[1] + b) * g.n[0] + a;
        u_out[i] = (float)u0;
        u_out[N + i] = (float)u1;
        u_out[2 * N + i] = (float)u2;
        status[i] = st;
        res2[i] = rr;
    }
}

/* p = inv(M'), q = inv(M): 3 x 4 row-major doubles; a = lin(M): 3 x 3.  fwd NULL: no forward field (fo, fh, fn unused).  The
 * inverse grid go, gh, gn; out: u 3 N floats component-major, status N words, res2 N doubles.  The caller has checked the shapes. */
hipError_t sift3d_launch_field_invert(hipStream_t s, const float4 *fwd, const float fo[3], float fh, const int64_t fn[3], const float go[3], float gh,
                                      const int64_t gn[3], const double p[12], const double q[12], const double a[9], double tol2, int max_iter,
                                      float *u, unsigned *status, double *res2)
{
    node_grid f, g;
    fi_maps m;
    if (fwd) fill_node_grid(f, fo, fh, fn);
    else fill_no_node_grid(f);
    fill_node_grid(g, go, gh, gn);
    for (int k = 0; k < 12; k++) {
        m.p[k] = p[k];
        m.q[k] = q[k];
    }
    for (int k = 0; k < 9; k++) m.a[k] = a[k];
    m.tol2 = tol2;
    m.max_iter = max_iter;
    m.has_field = fwd != nullptr;
    const node_launch b = node_launch_of(gn);
    hipLaunchKernelGGL(field_invert_kernel, dim3(b.grid), dim3(256), 0, s, fwd, f, g, m, u, status, res2, b.nb0, b.nb1, b.nbricks);
    return hipGetLastError();
}

#define JM_HX (BRICK_BX + 2)
#define JM_HY (BRICK_BY + 2)
#define JM_HZ (BRICK_BZ + 2)
#define JM_HALO (JM_HX * JM_HY * JM_HZ)

/* warp_position at the output position (px, py, pz), the field's term by the map's run-time has_field */
__device__ __forceinline__ void jm_q(const warp_map &m, const float4 *__restrict__ nodes, float px, float py, float pz, float q[3])
{
    if (m.has_field) warp_position<1>(m, nodes, px, py, pz, q);
    else warp_position<0>(m, nodes, px, py, pz, q);
}

/* J from the six neighbouring positions: xp, xm, yp, ym, zp, zm */
__device__ __forceinline__ float jm_det(const float xp[3], const float xm[3], const float yp[3], const float ym[3], const float zp[3],
                                        const float zm[3], double factor)
{
    double J[9];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        J[3 * r] = (double)((xp[r] - xm[r]) * 0.5f);
        J[3 * r + 1] = (double)((yp[r] - ym[r]) * 0.5f);
        J[3 * r + 2] = (double)((zp[r] - zm[r]) * 0.5f);
    }
    const double det = J[0] * (J[4] * J[8] - J[5] * J[7]) - J[1] * (J[3] * J[8] - J[5] * J[6]) + J[2] * (J[3] * J[7] - J[4] * J[6]);
    return (float)(det * factor);
}

template <int FORM>
__global__ __launch_bounds__(256) void jacobian_map_kernel(float *__restrict__ dst, long long ox, long long oy, long long oz, warp_map m,
                                                           const float4 *__restrict__ nodes, double factor, long long nbx, long long nby,
                                                           long long nbricks, int vec)
{
    __shared__ float sq[FORM ? 3 * JM_HALO : 1];
    int tx, ty, tz;
    brick_lane(tx, ty, tz);
    for (long long L = brick_slot0(); L < nbricks; L += gridDim.x) {
        long long i0, j, k;
        brick_voxel(L, nbx, nby, tx, ty, tz, i0, j, k);
        const bool mine = j < oy && k < oz && i0 < ox;
        float r[BRICK_VX];
        if (FORM) {
            long long x0, y0, z0; /* the brick's first voxel: the halo starts one voxel before it */
            brick_origin(L, nbx, nby, x0, y0, z0);
            for (int e = threadIdx.x; e < JM_HALO; e += 256) {
                const int ex = e % JM_HX, ey = (e / JM_HX) % JM_HY, ez = e / (JM_HX * JM_HY);
                float q[3];
                jm_q(m, nodes, (float)(x0 + ex - 1), (float)(y0 + ey - 1), (float)(z0 + ez - 1), q);
                sq[e] = q[0];
                sq[JM_HALO + e] = q[1];
                sq[2 * JM_HALO + e] = q[2];
            }
            __syncthreads();
            if (mine) {
#pragma unroll
                for (int v = 0; v < BRICK_VX; v++) {
                    const int at = ((tz + 1) * JM_HY + (ty + 1)) * JM_HX + (tx * BRICK_VX + v + 1);
                    float xp[3], xm[3], yp[3], ym[3], zp[3], zm[3];
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        const float *s = sq + c * JM_HALO + at;
                        xp[c] = s[1];
                        xm[c] = s[-1];
                        yp[c] = s[JM_HX];
                        ym[c] = s[-JM_HX];
                        zp[c] = s[JM_HX * JM_HY];
                        zm[c] = s[-JM_HX * JM_HY];
                    }
                    r[v] = jm_det(xp, xm, yp, ym, zp, zm, factor);
                }
            }
            __syncthreads();
        } else if (mine) {
            const float py = (float)j, pz = (float)k;
#pragma unroll
            for (int v = 0; v < BRICK_VX; v++) {
                const float px = (float)(i0 + v);
                float xp[3], xm[3], yp[3], ym[3], zp[3], zm[3];
                jm_q(m, nodes, (float)(i0 + v + 1), py, pz, xp);
                jm_q(m, nodes, (float)(i0 + v - 1), py, pz, xm);
                jm_q(m, nodes, px, (float)(j + 1), pz, yp);
                jm_q(m, nodes, px, (float)(j - 1), pz, ym);
                jm_q(m, nodes, px, py, (float)(k + 1), zp);
                jm_q(m, nodes, px, py, (float)(k - 1), zm);
                r[v] = jm_det(xp, xm, yp, ym, zp, zm, factor);
            }
        }
        if (mine) store_row4(dst + (k * oy + j) * ox + i0, ox, i0, r, vec);
    }
}

/* map, c: 12 floats; k: 9; nodes NULL: no field (o, h, n unused), else float4 (v0, v1, v2, 0) on the grid n (2 .. 2^24 per
 * axis), origin o, spacing h.  form 0: six evaluations per voxel; 1: the brick and its halo through LDS.  The caller has checked
 * the shapes. */
hipError_t sift3d_launch_jacobian_map(hipStream_t s, float *dst, int64_t ox, int64_t oy, int64_t oz, const float *map, const float *c, const float *k,
                                      const float o[3], float h, const int64_t n[3], const float4 *nodes, double factor, int form)
{
    warp_map m;
    fill_warp_map(m, map, c, k, nodes != nullptr, o, h, n);
    const brick_launch b = brick_launch_of(dst, ox, oy, oz);
    auto kernel = form ? jacobian_map_kernel<1> : jacobian_map_kernel<0>;
    hipLaunchKernelGGL(kernel, dim3(b.grid), dim3(256), 0, s, dst, (long long)ox, (long long)oy, (long long)oz, m, nodes, factor, b.nbx, b.nby,
                       b.nbricks, b.vec);
    return hipGetLastError();
}
