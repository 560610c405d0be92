/*
 * kernels_refine.hip -- the guided search of the re-matching step for gfx950 (MI355X).
 *
 * guided_kernel.  One query (moving record) per lane, 256-thread workgroups, no LDS, no atomics.  The queries are dealt in
 * the cell order of their MOVING position (sorted once per call on the host): a similarity keeps neighbours together, so
 * neighbouring lanes predict into the same few fixed cells in every round and read the same fixed rows from L1 / L2.  A lane
 *   - predicts q = am_sim_point(x_m, center0, center1, rot, scale) and the scale product m.scale * scale (align_math.h, the
 *     operations the host and the CPU oracle perform),
 *   - finds the cell of q on the fixed grid (double, as the host binned the fixed records) and walks the 3 x 3 rows of
 *     three cells around it; the three cells of a row are adjacent in the cell order, so a row is one run of records,
 *   - tests each record: equal line flags, the scale ratio in [lo, hi], the squared distance below radius^2 -- all in float,
 *     NaN failing every comparison,
 *   - for a record that passes reads its 64-byte row as four global_load_dwordx4 and forms d = |q|^2 + |f|^2 - 2 q.f
 *     exactly with v_dot4_u32_u8 (the components are 0..127), the query row held in sixteen VGPRs,
 *   - keeps the best two by (d, original fixed index), so the result does not depend on the order of the visit.
 * The fixed records sit in cell order (SoA positions, scales, info, row norms and original indices); the rows stay in the
 * caller's order and a passing candidate's row is read through its original index (12 MB at 185 k records: they stay in L2
 * and the Infinity Cache).  A dense cell-start table (ncell + 1 entries) gives a run by two loads; the sorted form keeps one
 * int64 cell key per record and finds a run by two binary searches.
 *
 * Exactness: this file honours NaN (no -fno-honor-nans) and is built with -ffp-contract=off.
 */
#include <stdint.h>

#include "align_math.h"
#include "sift3d_internal.h"

typedef unsigned int r_v4u __attribute__((ext_vector_type(4)));

struct refine_grid {
    double ox, oy, oz, edge; /* origin (the fixed records' finite minimum) and cell edge */
    long long nx, ny, nz;    /* cells per axis */
    int dense;               /* 1: cell_start has nx * ny * nz + 1 entries; 0: keys holds each record's cell key */
};

struct refine_xform {
    float c0[3], c1[3], rot[9], s;
};

__device__ __forceinline__ long long rf_cell(float v, double o, double edge, long long n)
{
    double c = floor(((double)v - o) / edge);
    /* a position far outside the grid: any clamp outside [-1, n] keeps the 3-cell window empty */
    c = c < -2.0 ? -2.0 : (c > (double)n + 1.0 ? (double)n + 1.0 : c);
    return (long long)c;
}

/* first record whose key is >= k */
__device__ __forceinline__ int rf_lower(const long long *__restrict__ keys, int n, long long k)
{
    int a = 0, b = n;
    while (a < b) {
        const int m = a + ((b - a) >> 1);
        if (keys[m] < k) a = m + 1;
        else b = m;
    }
    return a;
}

__global__ __launch_bounds__(256) void guided_kernel(const r_v4u *__restrict__ f_rows, const int *__restrict__ f_norm,
                                                     const float *__restrict__ f_pos, const unsigned *__restrict__ f_info,
                                                     const int *__restrict__ f_idx, int n_f, const int *__restrict__ cell_start,
                                                     const long long *__restrict__ keys, refine_grid g, const r_v4u *__restrict__ m_rows,
                                                     const float *__restrict__ m_pos, const unsigned *__restrict__ m_info,
                                                     const int *__restrict__ order, int n_m, refine_xform t, float rr, float lo, float hi,
                                                     int *__restrict__ o_i1, int *__restrict__ o_d1, int *__restrict__ o_i2,
                                                     int *__restrict__ o_d2, int *__restrict__ o_visited)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_m) return;
    const int mi = order[k];
    const long long nm = n_m, nf = n_f;
    const float p[3] = {m_pos[mi], m_pos[nm + mi], m_pos[2 * nm + mi]};
    float q[3];
    am_sim_point(p, q, t.c0, t.c1, t.rot, t.s);
    const float ms = m_pos[3 * nm + mi] * t.s;
    const unsigned line = m_info[mi] & AM_INFO_LINE;
    int i1 = -1, d1 = 0x7fffffff, i2 = -1, d2 = 0x7fffffff, visited = 0;
    if (isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]) && n_f > 0) {
        r_v4u qr[4];
#pragma unroll
        for (int c = 0; c < 4; c++) qr[c] = m_rows[4 * (long long)mi + c];
        unsigned qn = 0;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            qn = __builtin_amdgcn_udot4(qr[c].x, qr[c].x, qn, false);
            qn = __builtin_amdgcn_udot4(qr[c].y, qr[c].y, qn, false);
            qn = __builtin_amdgcn_udot4(qr[c].z, qr[c].z, qn, false);
            qn = __builtin_amdgcn_udot4(qr[c].w, qr[c].w, qn, false);
        }
        const long long cx = rf_cell(q[0], g.ox, g.edge, g.nx), cy = rf_cell(q[1], g.oy, g.edge, g.ny), cz = rf_cell(q[2], g.oz, g.edge, g.nz);
        const long long x0 = cx - 1 < 0 ? 0 : cx - 1, x1 = cx + 1 >= g.nx ? g.nx - 1 : cx + 1;
        for (long long z = cz - 1; z <= cz + 1; z++) {
            if (z < 0 || z >= g.nz || x0 > x1) continue;
            for (long long y = cy - 1; y <= cy + 1; y++) {
                if (y < 0 || y >= g.ny) continue;
                const long long kb = (z * g.ny + y) * g.nx;
                int a, b;
                if (g.dense) {
                    a = cell_start[kb + x0];
                    b = cell_start[kb + x1 + 1];
                } else {
                    a = rf_lower(keys, n_f, kb + x0);
                    b = rf_lower(keys, n_f, kb + x1 + 1);
                }
                visited += b - a;
                for (int j = a; j < b; j++) {
                    if ((f_info[j] & AM_INFO_LINE) != line) continue;
                    const float r = f_pos[3 * nf + j] / ms;
                    if (!(r >= lo && r <= hi)) continue;
                    const float dx = f_pos[j] - q[0], dy = f_pos[nf + j] - q[1], dz = f_pos[2 * nf + j] - q[2];
                    if (!((dx * dx + dy * dy) + dz * dz < rr)) continue;
                    const int fi = f_idx[j];
                    unsigned dot = 0;
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        const r_v4u fr = f_rows[4 * (long long)fi + c];
                        dot = __builtin_amdgcn_udot4(qr[c].x, fr.x, dot, false);
                        dot = __builtin_amdgcn_udot4(qr[c].y, fr.y, dot, false);
                        dot = __builtin_amdgcn_udot4(qr[c].z, fr.z, dot, false);
                        dot = __builtin_amdgcn_udot4(qr[c].w, fr.w, dot, false);
                    }
                    const int d = (int)qn + f_norm[j] - 2 * (int)dot;
                    if (d < d1 || (d == d1 && fi < i1)) {
                        d2 = d1;
                        i2 = i1;
                        d1 = d;
                        i1 = fi;
                    } else if (d < d2 || (d == d2 && fi < i2)) {
                        d2 = d;
                        i2 = fi;
                    }
                }
            }
        }
    }
    o_i1[mi] = i1;
    o_d1[mi] = d1;
    o_i2[mi] = i2;
    o_d2[mi] = d2;
    if (o_visited) o_visited[mi] = visited;
}

hipError_t sift3d_launch_guided(hipStream_t s, const void *f_rows, const int *f_norm, const float *f_pos, const unsigned *f_info, const int *f_idx,
                                int n_f, const int *cell_start, const long long *keys, const double grid_o[3], double edge, const long long grid_n[3],
                                int dense, const void *m_rows, const float *m_pos, const unsigned *m_info, const int *order, int n_m,
                                const float c0[3], const float c1[3], const float rot[9], float scale, float radius, float lo, float hi, int *i1,
                                int *d1, int *i2, int *d2, int *visited)
{
    if (n_m <= 0) return hipSuccess;
    refine_grid g;
    g.ox = grid_o[0];
    g.oy = grid_o[1];
    g.oz = grid_o[2];
    g.edge = edge;
    g.nx = grid_n[0];
    g.ny = grid_n[1];
    g.nz = grid_n[2];
    g.dense = dense;
    refine_xform t;
    for (int k = 0; k < 3; k++) {
        t.c0[k] = c0[k];
        t.c1[k] = c1[k];
    }
    for (int k = 0; k < 9; k++) t.rot[k] = rot[k];
    t.s = scale;
    const float rr = radius * radius;
    hipLaunchKernelGGL(guided_kernel, dim3((unsigned)((n_m + 255) / 256)), dim3(256), 0, s, (const r_v4u *)f_rows, f_norm, f_pos, f_info, f_idx, n_f,
                       cell_start, keys, g, (const r_v4u *)m_rows, m_pos, m_info, order, n_m, t, rr, lo, hi, i1, d1, i2, d2, visited);
    return hipGetLastError();
}
