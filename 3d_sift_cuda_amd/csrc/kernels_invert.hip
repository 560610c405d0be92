/*
 * kernels_invert.hip -- the reverse direction of the nonrigid alignment for gfx950 (MI355X): the inverse of a displacement
 * field on a node grid of its own, and the Jacobian determinant map of a warp.  Beyond the reference.
 *
 * field_invert_kernel.  One node per lane; a 256-thread workgroup owns a brick of 8 x 8 x 4 nodes and each wave a 4 x 4 x 4
 * part of it (field_fit_kernel's mapping), so the eight gathers of a wave's lanes fall on neighbouring forward nodes.  The
 * forward nodes are float4, one dwordx4 load per corner.  Per node z (its float position, widened), with P = inv(M'),
 * Q = inv(M) and A = lin(M) as doubles from the host:
 *   b_r = ((P[r][0] z0 + P[r][1] z1) + P[r][2] z2) + P[r][3];  u = 0;  k = 0
 *   loop:  y = b + u;  v = the forward field at (float)y (field_warp_kernel's float arithmetic; 0 outside its grid)
 *          r_c = ((((Q[c][0] y0 + Q[c][1] y1) + Q[c][2] y2) + Q[c][3]) + (double)v_c) - z_c;  rr = (r0 r0 + r1 r1) + r2 r2
 *          rr <= tol^2: converged, stop.  k == max_iter: not converged, stop.
 *          u_c = u_c - ((A[c][0] r0 + A[c][1] r1) + A[c][2] r2);  k = k + 1
 *          a component of u not within +-SIFT3D_FIELD_MAX_DISP (NaN included): u = 0, diverged, stop.
 * Written per node: (float)u, the word k | state << 16 (0 converged, 1 not converged, 2 diverged) and the last rr.  A lane
 * leaves the loop when its node stops, so a wave runs until its last lane has.
 *
 * jacobian_map_kernel<FORM>.  section 7c's brick of 32 x 8 x 4 output voxels.  q(p) is field_warp_kernel's position
 * arithmetic without the gather of the image.  Per voxel D[r][a] = (q_r(p + e_a) - q_r(p - e_a)) 0.5f in float, the
 * determinant in double in sift3d_blockmatch_folds' order, times one double factor, rounded to float once.  FORM 0 evaluates q
 * six times per voxel; FORM 1 evaluates the brick and a one-voxel halo once into LDS (34 x 10 x 6 positions, 24 480 bytes)
 * and takes the differences from there.  Both give the same numbers: q at a position does not depend on who asks.
 *
 * -ffp-contract=off and no -fno-honor-nans (Makefile): a NaN position fails the inside test, a NaN node reaches u and J.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#define FI_BX 8
#define FI_BY 8
#define FI_BZ 4
#define FI_MAX_GRID (1u << 20)
#define FI_MAX_DISP 128.0 /* SIFT3D_FIELD_MAX_DISP */

struct fi_nodes {
    float o[3], h;
    float top[3]; /* (float)(n - 1) */
    long long n[3];
};

struct fi_maps {
    double p[12], q[12], a[9], tol2;
    int max_iter, has_field;
};

/* the trilinear interpolation of the float4 nodes at the key position (kx, ky, kz): field_warp_kernel's arithmetic; 0 outside */
__device__ __forceinline__ void nodes_at(const float4 *__restrict__ nodes, const float o[3], float h, const float top[3], const long long n[3],
                                         float kx, float ky, float kz, float d[3], bool &inside)
{
    const float gx = (kx - o[0]) / h, gy = (ky - o[1]) / h, gz = (kz - o[2]) / h;
    inside = gx >= 0.0f && gx <= top[0] && gy >= 0.0f && gy <= top[1] && gz >= 0.0f && gz <= top[2];
    d[0] = d[1] = d[2] = 0.0f;
    if (!inside) return;
    const long long gn0 = n[0], gn1 = n[1];
    const float fx = floorf(gx), fy = floorf(gy), fz = floorf(gz);
    const float wx = gx - fx, wy = gy - fy, wz = gz - fz;
    const long long x0 = (int)fx, y0 = (int)fy, z0 = (int)fz;
    const long long x1 = x0 + 1 < gn0 - 1 ? x0 + 1 : gn0 - 1, y1 = y0 + 1 < gn1 - 1 ? y0 + 1 : gn1 - 1, z1 = z0 + 1 < n[2] - 1 ? z0 + 1 : n[2] - 1;
    const float4 *r00 = nodes + (z0 * gn1 + y0) * gn0, *r10 = nodes + (z0 * gn1 + y1) * gn0, *r01 = nodes + (z1 * gn1 + y0) * gn0,
                 *r11 = nodes + (z1 * gn1 + y1) * gn0;
    const float4 a00 = r00[x0], b00 = r00[x1], a10 = r10[x0], b10 = r10[x1], a01 = r01[x0], b01 = r01[x1], a11 = r11[x0], b11 = r11[x1];
    const float ux = 1.0f - wx, uy = 1.0f - wy, uz = 1.0f - wz;
#define FI_COMP(C, f)                                                                                  \
    {                                                                                                  \
        const float c00 = ux * a00.f + wx * b00.f, c10 = ux * a10.f + wx * b10.f;                       \
        const float c01 = ux * a01.f + wx * b01.f, c11 = ux * a11.f + wx * b11.f;                       \
        const float c0 = uy * c00 + wy * c10, c1 = uy * c01 + wy * c11;                                 \
        d[C] = uz * c0 + wz * c1;                                                                      \
    }
    FI_COMP(0, x)
    FI_COMP(1, y)
    FI_COMP(2, z)
#undef FI_COMP
}

__global__ __launch_bounds__(256) void field_invert_kernel(const float4 *__restrict__ fwd, fi_nodes f, fi_nodes g, fi_maps m, float *__restrict__ u_out,
                                                           unsigned *__restrict__ status, double *__restrict__ res2, long long nb0, long long nb1,
                                                           long long nbricks)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int lx = (lane & 3) + (wv & 1) * 4, ly = ((lane >> 2) & 3) + (wv >> 1) * 4, lz = lane >> 4;
    const long long N = g.n[0] * g.n[1] * g.n[2];
    for (long long L = blockIdx.x; L < nbricks; L += gridDim.x) {
        const long long bx = L % nb0, t0 = L / nb0, by = t0 % nb1, bz = t0 / nb1;
        const long long a = bx * FI_BX + lx, b = by * FI_BY + ly, c = bz * FI_BZ + lz;
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

static void fill_nodes(fi_nodes &d, const float o[3], float h, const int64_t n[3])
{
    for (int k = 0; k < 3; k++) {
        d.o[k] = o[k];
        d.n[k] = n[k];
        d.top[k] = (float)(n[k] - 1);
    }
    d.h = h;
}

/* p = inv(M'), q = inv(M): 3 x 4 row-major doubles; a = lin(M): 3 x 3.  fwd NULL: no forward field (fo, fh, fn unused).  The
 * inverse grid go, gh, gn; out: u 3 N floats component-major, status N words, res2 N doubles.  The caller has checked the shapes. */
hipError_t sift3d_launch_field_invert(hipStream_t s, const float4 *fwd, const float fo[3], float fh, const int64_t fn[3], const float go[3], float gh,
                                      const int64_t gn[3], const double p[12], const double q[12], const double a[9], double tol2, int max_iter,
                                      float *u, unsigned *status, double *res2)
{
    fi_nodes f, g;
    fi_maps m;
    static const float zero3[3] = {0, 0, 0};
    static const int64_t two3[3] = {2, 2, 2};
    fill_nodes(f, fwd ? fo : zero3, fwd ? fh : 1.0f, fwd ? fn : two3);
    fill_nodes(g, go, gh, gn);
    for (int k = 0; k < 12; k++) {
        m.p[k] = p[k];
        m.q[k] = q[k];
    }
    for (int k = 0; k < 9; k++) m.a[k] = a[k];
    m.tol2 = tol2;
    m.max_iter = max_iter;
    m.has_field = fwd != nullptr;
    const long long nb0 = (gn[0] + FI_BX - 1) / FI_BX, nb1 = (gn[1] + FI_BY - 1) / FI_BY, nb2 = (gn[2] + FI_BZ - 1) / FI_BZ;
    const long long nbricks = nb0 * nb1 * nb2;
    const unsigned grid = (unsigned)(nbricks < (long long)FI_MAX_GRID ? nbricks : FI_MAX_GRID);
    hipLaunchKernelGGL(field_invert_kernel, dim3(grid), dim3(256), 0, s, fwd, f, g, m, u, status, res2, nb0, nb1, nbricks);
    return hipGetLastError();
}

#define JM_TX 8
#define JM_VX 4
#define JM_BX (JM_TX * JM_VX)
#define JM_BY 8
#define JM_BZ 4
#define JM_HX (JM_BX + 2)
#define JM_HY (JM_BY + 2)
#define JM_HZ (JM_BZ + 2)
#define JM_HALO (JM_HX * JM_HY * JM_HZ)
#define JM_MAX_GRID (1u << 22)

struct jm_map {
    float a[12]; /* output voxel -> source voxel (section 7c) */
    float c[12]; /* output voxel -> output key */
    float k[9];  /* source key displacement -> source voxel displacement */
    float o[3], h;
    float top[3];
    long long n[3];
    int has_field;
};

/* field_warp_kernel's position arithmetic at the output position (px, py, pz) */
__device__ __forceinline__ void jm_q(const jm_map &m, const float4 *__restrict__ nodes, float px, float py, float pz, float q[3])
{
    q[0] = ((m.a[0] * px + m.a[1] * py) + m.a[2] * pz) + m.a[3];
    q[1] = ((m.a[4] * px + m.a[5] * py) + m.a[6] * pz) + m.a[7];
    q[2] = ((m.a[8] * px + m.a[9] * py) + m.a[10] * pz) + m.a[11];
    if (!m.has_field) return;
    const float kx = ((m.c[0] * px + m.c[1] * py) + m.c[2] * pz) + m.c[3];
    const float ky = ((m.c[4] * px + m.c[5] * py) + m.c[6] * pz) + m.c[7];
    const float kz = ((m.c[8] * px + m.c[9] * py) + m.c[10] * pz) + m.c[11];
    float d[3];
    bool inside;
    nodes_at(nodes, m.o, m.h, m.top, m.n, kx, ky, kz, d, inside);
    if (inside) {
        q[0] = q[0] + ((m.k[0] * d[0] + m.k[1] * d[1]) + m.k[2] * d[2]);
        q[1] = q[1] + ((m.k[3] * d[0] + m.k[4] * d[1]) + m.k[5] * d[2]);
        q[2] = q[2] + ((m.k[6] * d[0] + m.k[7] * d[1]) + m.k[8] * d[2]);
    }
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
__global__ __launch_bounds__(256) void jacobian_map_kernel(float *__restrict__ dst, long long ox, long long oy, long long oz, jm_map m,
                                                           const float4 *__restrict__ nodes, double factor, long long nbx, long long nby,
                                                           long long nbricks, int vec)
{
    __shared__ float sq[FORM ? 3 * JM_HALO : 1];
    const unsigned grid = gridDim.x, b = blockIdx.x;
    const long long slot0 = (long long)(b & 7u) * (grid >> 3) + (b >> 3);
    const int tx = threadIdx.x & (JM_TX - 1), ty = (threadIdx.x / JM_TX) & (JM_BY - 1), tz = threadIdx.x / (JM_TX * JM_BY);
    for (long long L = slot0; L < nbricks; L += grid) {
        const long long bx = L % nbx, t = L / nbx, by = t % nby, bz = t / nby;
        const long long i0 = bx * JM_BX + tx * JM_VX, j = by * JM_BY + ty, k = bz * JM_BZ + tz;
        const bool mine = j < oy && k < oz && i0 < ox;
        float r[JM_VX];
        if (FORM) {
            for (int e = threadIdx.x; e < JM_HALO; e += 256) {
                const int ex = e % JM_HX, ey = (e / JM_HX) % JM_HY, ez = e / (JM_HX * JM_HY);
                float q[3];
                jm_q(m, nodes, (float)(bx * JM_BX + ex - 1), (float)(by * JM_BY + ey - 1), (float)(bz * JM_BZ + ez - 1), q);
                sq[e] = q[0];
                sq[JM_HALO + e] = q[1];
                sq[2 * JM_HALO + e] = q[2];
            }
            __syncthreads();
            if (mine) {
#pragma unroll
                for (int v = 0; v < JM_VX; v++) {
                    const int at = ((tz + 1) * JM_HY + (ty + 1)) * JM_HX + (tx * JM_VX + v + 1);
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
            for (int v = 0; v < JM_VX; v++) {
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
        if (!mine) continue;
        float *o = dst + (k * oy + j) * ox + i0;
        if (vec && i0 + JM_VX <= ox) {
            *reinterpret_cast<float4 *>(o) = make_float4(r[0], r[1], r[2], r[3]);
        } else {
#pragma unroll
            for (int v = 0; v < JM_VX; v++)
                if (i0 + v < ox) o[v] = r[v];
        }
    }
}

/* map, c: 12 floats; k: 9; nodes NULL: no field (o, h, n unused), else float4 (v0, v1, v2, 0) on the grid n (2 .. 2^24 per
 * axis), origin o, spacing h.  form 0: six evaluations per voxel; 1: the brick and its halo through LDS.  The caller has checked
 * the shapes. */
hipError_t sift3d_launch_jacobian_map(hipStream_t s, float *dst, int64_t ox, int64_t oy, int64_t oz, const float *map, const float *c, const float *k,
                                      const float o[3], float h, const int64_t n[3], const float4 *nodes, double factor, int form)
{
    jm_map m;
    for (int r = 0; r < 12; r++) {
        m.a[r] = map[r];
        m.c[r] = c[r];
    }
    for (int r = 0; r < 9; r++) m.k[r] = k[r];
    for (int r = 0; r < 3; r++) {
        m.o[r] = nodes ? o[r] : 0.0f;
        m.n[r] = nodes ? n[r] : 2;
        m.top[r] = (float)(m.n[r] - 1);
    }
    m.h = nodes ? h : 1.0f;
    m.has_field = nodes != nullptr;
    const long long nbx = (ox + JM_BX - 1) / JM_BX, nby = (oy + JM_BY - 1) / JM_BY, nbz = (oz + JM_BZ - 1) / JM_BZ;
    const long long nbricks = nbx * nby * nbz;
    long long g = (nbricks + 7) / 8 * 8;
    if (g > (long long)JM_MAX_GRID) g = JM_MAX_GRID;
    const int vec = (ox % JM_VX) == 0 && ((uintptr_t)dst % 16) == 0;
    if (form)
        hipLaunchKernelGGL(jacobian_map_kernel<1>, dim3((unsigned)g), dim3(256), 0, s, dst, (long long)ox, (long long)oy, (long long)oz, m, nodes,
                           factor, nbx, nby, nbricks, vec);
    else
        hipLaunchKernelGGL(jacobian_map_kernel<0>, dim3((unsigned)g), dim3(256), 0, s, dst, (long long)ox, (long long)oy, (long long)oz, m, nodes,
                           factor, nbx, nby, nbricks, vec);
    return hipGetLastError();
}
