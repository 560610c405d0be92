/*
 * kernels_compose.hip -- the composition of two alignments for gfx950 (MI355X): the displacement field of phi2 o phi1 on a node
 * grid of its own, and the interpolation residual of that grid cell by cell.  Beyond the reference.
 *
 * Pair 1 is (M1, v1), A key -> B key: phi1(y) = inv(M1) y + v1(y).  Pair 2 is (M2, v2), B key -> C key.  Mc' is the written
 * composite matrix as a reader gets it back.  With P1 = inv(M1), P2 = inv(M2), Pc = inv(Mc') as doubles from the host, at a
 * float position y widened to double (compose_chain):
 *   a_r = ((P1[r][0] y0 + P1[r][1] y1) + P1[r][2] y2) + P1[r][3];  v1 = field 1 at y (nodes_at's float arithmetic; 0 outside)
 *   s_r = a_r + (double)v1_r
 *   b_r = ((P2[r][0] s0 + P2[r][1] s1) + P2[r][2] s2) + P2[r][3];  v2 = field 2 at (float)s
 *   t_r = b_r + (double)v2_r
 *   c_r = ((Pc[r][0] y0 + Pc[r][1] y1) + Pc[r][2] y2) + Pc[r][3]
 *
 * field_compose_kernel.  One node per lane, in warp_device.h's brick of 8 x 8 x 4 nodes, so the gathers of a wave's lanes into
 * v1 fall on neighbouring nodes (one dwordx4 load per corner).  y = origin + (float)index h; w = t - c; the node's value is
 * (float)w and its status word bit 0: field 1 given and y outside its grid, bit 1: field 2 given and s outside its grid, bit 2:
 * a component of w not within +-SIFT3D_FIELD_MAX_DISP (NaN included), the node then written as 0.  The nodes are written
 * component-major for the host and, where asked, as the float4 nodes the residual kernel gathers from.
 *
 * compose_residual_kernel.  One cell per lane over the n - 1 cells per axis, the same brick.  z = origin + ((float)index +
 * 0.5f) h; wt = nodes_at of the composite float4 nodes at z; e_r = t_r(z) - (c_r(z) + (double)wt_r); the cell's value is the
 * double (e0 e0 + e1 e1) + e2 e2.
 *
 * -ffp-contract=off and no -fno-honor-nans (Makefile): a NaN position fails the inside test, a NaN node reaches w (weight 0
 * included) and fails the bound.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "warp_device.h"

#define FC_MAX_DISP 128.0 /* SIFT3D_FIELD_MAX_DISP */

struct fc_maps {
    double p1[12], p2[12], pc[12];
    int has1, has2;
};

/* t = phi2(phi1(y)) and c = inv(Mc') y at the float position (yx, yy, yz); st: bits 0 and 1 of the status word */
__device__ __forceinline__ void compose_chain(const float4 *__restrict__ f1, const float4 *__restrict__ f2, const node_grid &g1, const node_grid &g2,
                                              const fc_maps &m, float yx, float yy, float yz, double t[3], double c[3], unsigned &st)
{
    const double y0 = (double)yx, y1 = (double)yy, y2 = (double)yz;
    const double a0 = ((m.p1[0] * y0 + m.p1[1] * y1) + m.p1[2] * y2) + m.p1[3];
    const double a1 = ((m.p1[4] * y0 + m.p1[5] * y1) + m.p1[6] * y2) + m.p1[7];
    const double a2 = ((m.p1[8] * y0 + m.p1[9] * y1) + m.p1[10] * y2) + m.p1[11];
    float d[3] = {0.0f, 0.0f, 0.0f};
    bool inside;
    st = 0u;
    if (m.has1) {
        nodes_at(f1, g1.o, g1.h, g1.top, g1.n, yx, yy, yz, d, inside);
        if (!inside) st |= 1u;
    }
    const double s0 = a0 + (double)d[0], s1 = a1 + (double)d[1], s2 = a2 + (double)d[2];
    const double b0 = ((m.p2[0] * s0 + m.p2[1] * s1) + m.p2[2] * s2) + m.p2[3];
    const double b1 = ((m.p2[4] * s0 + m.p2[5] * s1) + m.p2[6] * s2) + m.p2[7];
    const double b2 = ((m.p2[8] * s0 + m.p2[9] * s1) + m.p2[10] * s2) + m.p2[11];
    d[0] = d[1] = d[2] = 0.0f;
    if (m.has2) {
        nodes_at(f2, g2.o, g2.h, g2.top, g2.n, (float)s0, (float)s1, (float)s2, d, inside);
        if (!inside) st |= 2u;
    }
    t[0] = b0 + (double)d[0];
    t[1] = b1 + (double)d[1];
    t[2] = b2 + (double)d[2];
    c[0] = ((m.pc[0] * y0 + m.pc[1] * y1) + m.pc[2] * y2) + m.pc[3];
    c[1] = ((m.pc[4] * y0 + m.pc[5] * y1) + m.pc[6] * y2) + m.pc[7];
    c[2] = ((m.pc[8] * y0 + m.pc[9] * y1) + m.pc[10] * y2) + m.pc[11];
}

__global__ __launch_bounds__(256) void field_compose_kernel(const float4 *__restrict__ f1, const float4 *__restrict__ f2, node_grid g1, node_grid g2,
                                                            node_grid g, fc_maps m, float *__restrict__ w_out, float4 *__restrict__ w4_out,
                                                            unsigned *__restrict__ status, long long nb0, long long nb1, long long nbricks)
{
    int lx, ly, lz;
    node_lane(lx, ly, lz);
    const long long N = g.n[0] * g.n[1] * g.n[2];
    for (long long L = blockIdx.x; L < nbricks; L += gridDim.x) {
        long long a, b, c;
        node_of_slot(L, nb0, nb1, lx, ly, lz, a, b, c);
        if (a >= g.n[0] || b >= g.n[1] || c >= g.n[2]) continue;
        double t[3], q[3];
        unsigned st;
        compose_chain(f1, f2, g1, g2, m, g.o[0] + (float)a * g.h, g.o[1] + (float)b * g.h, g.o[2] + (float)c * g.h, t, q, st);
        double w0 = t[0] - q[0], w1 = t[1] - q[1], w2 = t[2] - q[2];
        if (!(w0 <= FC_MAX_DISP && w0 >= -FC_MAX_DISP && w1 <= FC_MAX_DISP && w1 >= -FC_MAX_DISP && w2 <= FC_MAX_DISP && w2 >= -FC_MAX_DISP)) {
            w0 = w1 = w2 = 0.0;
            st |= 4u;
        }
        const long long i = (c * g.n[1] + b) * g.n[0] + a;
        const float x0 = (float)w0, x1 = (float)w1, x2 = (float)w2;
        w_out[i] = x0;
        w_out[N + i] = x1;
        w_out[2 * N + i] = x2;
        if (w4_out) w4_out[i] = make_float4(x0, x1, x2, 0.0f);
        status[i] = st;
    }
}

/* cn: the cells per axis, g.n - 1 each; wn: the composite nodes on g */
__global__ __launch_bounds__(256) void compose_residual_kernel(const float4 *__restrict__ f1, const float4 *__restrict__ f2,
                                                               const float4 *__restrict__ wn, node_grid g1, node_grid g2, node_grid g, fc_maps m,
                                                               double *__restrict__ res2, long long cn0, long long cn1, long long cn2, long long nb0,
                                                               long long nb1, long long nbricks)
{
    int lx, ly, lz;
    node_lane(lx, ly, lz);
    for (long long L = blockIdx.x; L < nbricks; L += gridDim.x) {
        long long a, b, c;
        node_of_slot(L, nb0, nb1, lx, ly, lz, a, b, c);
        if (a >= cn0 || b >= cn1 || c >= cn2) continue;
        const float zx = g.o[0] + ((float)a + 0.5f) * g.h, zy = g.o[1] + ((float)b + 0.5f) * g.h, zz = g.o[2] + ((float)c + 0.5f) * g.h;
        double t[3], q[3];
        unsigned st;
        compose_chain(f1, f2, g1, g2, m, zx, zy, zz, t, q, st);
        float d[3];
        bool inside;
        nodes_at(wn, g.o, g.h, g.top, g.n, zx, zy, zz, d, inside);
        const double e0 = t[0] - (q[0] + (double)d[0]), e1 = t[1] - (q[1] + (double)d[1]), e2 = t[2] - (q[2] + (double)d[2]);
        res2[(c * cn1 + b) * cn0 + a] = (e0 * e0 + e1 * e1) + e2 * e2;
    }
}

static void fill_fc(fc_maps &m, node_grid &g1, node_grid &g2, const float4 *f1, const float o1[3], float h1, const int64_t n1[3], const float4 *f2,
                    const float o2[3], float h2, const int64_t n2[3], const double p1[12], const double p2[12], const double pc[12])
{
    if (f1) fill_node_grid(g1, o1, h1, n1);
    else fill_no_node_grid(g1);
    if (f2) fill_node_grid(g2, o2, h2, n2);
    else fill_no_node_grid(g2);
    for (int k = 0; k < 12; k++) {
        m.p1[k] = p1[k];
        m.p2[k] = p2[k];
        m.pc[k] = pc[k];
    }
    m.has1 = f1 != nullptr;
    m.has2 = f2 != nullptr;
}

/* p1 = inv(M1), p2 = inv(M2), pc = inv(Mc'): 3 x 4 row-major doubles.  f1, f2 NULL: no field (its o, h, n unused).  The composite
 * grid go, gh, gn; out: w 3 N floats component-major, w4 N float4 (may be NULL), status N words.  The caller has checked the shapes. */
hipError_t sift3d_launch_field_compose(hipStream_t s, const float4 *f1, const float o1[3], float h1, const int64_t n1[3], const float4 *f2,
                                       const float o2[3], float h2, const int64_t n2[3], const float go[3], float gh, const int64_t gn[3],
                                       const double p1[12], const double p2[12], const double pc[12], float *w, float4 *w4, unsigned *status)
{
    node_grid g1, g2, g;
    fc_maps m;
    fill_fc(m, g1, g2, f1, o1, h1, n1, f2, o2, h2, n2, p1, p2, pc);
    fill_node_grid(g, go, gh, gn);
    const node_launch b = node_launch_of(gn);
    hipLaunchKernelGGL(field_compose_kernel, dim3(b.grid), dim3(256), 0, s, f1, f2, g1, g2, g, m, w, w4, status, b.nb0, b.nb1, b.nbricks);
    return hipGetLastError();
}

/* the residual of the composite nodes w4 (N float4 on the grid go, gh, gn, each axis >= 2) into res2, (gn0 - 1)(gn1 - 1)(gn2 - 1)
 * doubles, x fastest */
hipError_t sift3d_launch_compose_residual(hipStream_t s, const float4 *f1, const float o1[3], float h1, const int64_t n1[3], const float4 *f2,
                                          const float o2[3], float h2, const int64_t n2[3], const float go[3], float gh, const int64_t gn[3],
                                          const double p1[12], const double p2[12], const double pc[12], const float4 *w4, double *res2)
{
    node_grid g1, g2, g;
    fc_maps m;
    fill_fc(m, g1, g2, f1, o1, h1, n1, f2, o2, h2, n2, p1, p2, pc);
    fill_node_grid(g, go, gh, gn);
    const int64_t cn[3] = {gn[0] - 1, gn[1] - 1, gn[2] - 1};
    const node_launch b = node_launch_of(cn);
    hipLaunchKernelGGL(compose_residual_kernel, dim3(b.grid), dim3(256), 0, s, f1, f2, w4, g1, g2, g, m, res2, (long long)cn[0], (long long)cn[1],
                       (long long)cn[2], b.nb0, b.nb1, b.nbricks);
    return hipGetLastError();
}
