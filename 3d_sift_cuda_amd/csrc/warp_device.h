/*
 * warp_device.h -- the arithmetic and the thread mappings that the warp family shares on gfx950 (MI355X): the image sampler,
 * the gather of a displacement field's nodes, the position of an output voxel under a map and a field, the brick of output
 * voxels and the brick of nodes.  Included by kernels_resample.hip, kernels_field.hip, kernels_invert.hip and kernels_fuse.hip
 * (which takes the brick of output voxels alone) only; every
 * function is __device__ __forceinline__, or a host inline that fills one of the structs or sizes a launch (marked "host"), so
 * each kernel keeps its own code.  tests/resample_oracle.c,
 * tests/field_oracle.c and tests/invert_oracle.c restate the arithmetic on the CPU, operation for operation.
 *
 * The sampler.  An output voxel p = (i, j, k), converted to float, has the source position
 *   q_r = ((A[r][0] * i + A[r][1] * j) + A[r][2] * k) + A[r][3];
 * a sample only where 0 <= q <= n - 1 on every axis (NaN fails), `fill` elsewhere.  Linear: f = floorf(q), w = q - f,
 * i0 = (int64)f, i1 = min(i0 + 1, n - 1), interpolated along x, then y, then z, each step (1 - w) * a + w * b; all eight
 * corners are read and weighed, so a NaN or infinite corner of weight 0 still reaches the result (IEEE, no -fno-honor-nans).
 * Nearest: i = min((int64)floorf(q + 0.5f), n - 1).  No texture sampler: its filter weights are fixed-point.
 * Label (section 7n): linear's eight corners c = a + 2b + 4d with the weights W_c = (X_a * Y_b) * Z_d (X_0 = ux, X_1 = wx, ...).
 * Corners of equal value (==) are one class, the non-finite ones together the unlabelled class; a class' score is the sum
 * ((t_0 + t_1) + ... + t_7), t_c = W_c for its corners and 0.0f for the others.  The largest score wins, at equal scores a
 * labelled class before the unlabelled one and the smaller value before the larger; the result is the value of the winner's
 * lowest-numbered corner with its bits, a quiet NaN for the unlabelled class.  In registers and without a branch: the masked sum
 * of every corner, then one pass over the corners under that rule.  tests/label_interp_oracle.c restates it.
 *
 * The field's term (section 7e).  The key position kappa = C p (the map's order), g = (kappa - o) / h, and where
 * 0 <= g <= n - 1 on every axis the trilinear interpolation v of the float4 nodes (one dwordx4 load per corner; the
 * sampler's floor, weights, clamp and x -> y -> z order), added as q_r = q_r + ((K[r][0] v0 + K[r][1] v1) + K[r][2] v2).
 * Outside the grid q is left as it is, and v reads as 0.
 *
 * The brick of output voxels.  A workgroup of 256 threads owns a brick of 32 x 8 x 4 output voxels; a thread owns four
 * consecutive x voxels of one row (one 16-byte store when the row allows it).  The bricks are numbered x fastest, then y,
 * then z, and the launch deals block b to brick slot (b % 8) * (grid / 8) + b / 8: blocks are dealt round-robin over the
 * eight XCDs, so each XCD walks one contiguous run of bricks -- a slab of output planes whose source footprint stays compact
 * under any rotation and is shared through that XCD's L2.  The placement is for speed only.  Larger outputs than one grid
 * loop over the brick slots in strides of the grid.  All voxel indices are 64-bit.
 *
 * The brick of nodes.  One node per lane; a workgroup of 256 threads owns a brick of 8 x 8 x 4 nodes and each wave a
 * 4 x 4 x 4 part of it, so the lanes of a wave read neighbouring samples (the fit) or neighbouring forward nodes (the
 * inverse).  Block b takes the brick slots b, b + grid, ...
 *
 * -ffp-contract=off and no -fno-honor-nans (Makefile): the order of the float operations above is binding.
 */
#ifndef SIFT3D_WARP_DEVICE_H
#define SIFT3D_WARP_DEVICE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

/* ---- the node grid and the gather of its nodes ---- */

struct node_grid {
    float o[3], h;
    float top[3]; /* (float)(n - 1) */
    long long n[3];
};

/* host: the grid of n nodes per axis at origin o with spacing h */
inline void fill_node_grid(node_grid &g, const float o[3], float h, const int64_t n[3])
{
    for (int k = 0; k < 3; k++) {
        g.o[k] = o[k];
        g.n[k] = n[k];
        g.top[k] = (float)(n[k] - 1);
    }
    g.h = h;
}

/* host: where there is no field, a placeholder (origin 0, spacing 1, 2 nodes per axis) that is never gathered from */
inline void fill_no_node_grid(node_grid &g)
{
    static const float zero3[3] = {0, 0, 0};
    static const int64_t two3[3] = {2, 2, 2};
    fill_node_grid(g, zero3, 1.0f, two3);
}

/* the trilinear interpolation of the float4 nodes at the key position (kx, ky, kz); 0 outside */
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
#define NODES_COMP(C, f)                                                                               \
    {                                                                                                  \
        const float c00 = ux * a00.f + wx * b00.f, c10 = ux * a10.f + wx * b10.f;                       \
        const float c01 = ux * a01.f + wx * b01.f, c11 = ux * a11.f + wx * b11.f;                       \
        const float c0 = uy * c00 + wy * c10, c1 = uy * c01 + wy * c11;                                 \
        d[C] = uz * c0 + wz * c1;                                                                      \
    }
    NODES_COMP(0, x)
    NODES_COMP(1, y)
    NODES_COMP(2, z)
#undef NODES_COMP
}

/* ---- the position of an output voxel ---- */

struct warp_map {
    float a[12]; /* output voxel -> source voxel */
    float c[12]; /* output voxel -> output key */
    float k[9];  /* source key displacement -> source voxel displacement */
    node_grid g;
    int has_field;
};

/* host: map, c: 12 floats (3 x 4 row-major); k: 9; has_field: the node grid n (each 2 .. 2^24), origin o, spacing h, which are
 * not read without it */
inline void fill_warp_map(warp_map &m, const float *map, const float *c, const float *k, bool has_field, const float o[3], float h,
                          const int64_t n[3])
{
    for (int r = 0; r < 12; r++) {
        m.a[r] = map[r];
        m.c[r] = c[r];
    }
    for (int r = 0; r < 9; r++) m.k[r] = k[r];
    if (has_field) fill_node_grid(m.g, o, h, n);
    else fill_no_node_grid(m.g);
    m.has_field = has_field;
}

/* q = A p at the output position (px, py, pz) and, with FIELD, q += K v where the key position C p is inside the node grid.
 * Without FIELD only m.a is read: any struct with an a[12] serves as the map. */
template <int FIELD, class MAP>
__device__ __forceinline__ void warp_position(const MAP &m, const float4 *__restrict__ nodes, float px, float py, float pz, float q[3])
{
    q[0] = ((m.a[0] * px + m.a[1] * py) + m.a[2] * pz) + m.a[3];
    q[1] = ((m.a[4] * px + m.a[5] * py) + m.a[6] * pz) + m.a[7];
    q[2] = ((m.a[8] * px + m.a[9] * py) + m.a[10] * pz) + m.a[11];
    if constexpr (FIELD) {
        const float kx = ((m.c[0] * px + m.c[1] * py) + m.c[2] * pz) + m.c[3];
        const float ky = ((m.c[4] * px + m.c[5] * py) + m.c[6] * pz) + m.c[7];
        const float kz = ((m.c[8] * px + m.c[9] * py) + m.c[10] * pz) + m.c[11];
        float d[3];
        bool inside;
        nodes_at(nodes, m.g.o, m.g.h, m.g.top, m.g.n, kx, ky, kz, d, inside);
        if (inside) {
            q[0] = q[0] + ((m.k[0] * d[0] + m.k[1] * d[1]) + m.k[2] * d[2]);
            q[1] = q[1] + ((m.k[3] * d[0] + m.k[4] * d[1]) + m.k[5] * d[2]);
            q[2] = q[2] + ((m.k[6] * d[0] + m.k[7] * d[1]) + m.k[8] * d[2]);
        }
    }
}

/* ---- the image sampler ---- */

#define WARP_LINEAR 0  /* include/sift3d.h: sift3d_interp */
#define WARP_NEAREST 1
#define WARP_LABEL 2

/* the label-aware vote over eight corner values L and their weights W (the header's "Label") */
__device__ __forceinline__ float label_vote(const float (&L)[8], const float (&W)[8])
{
    /* The class key: the value itself, +inf for every non-finite one.  Then two corners are of one class exactly when their keys
     * compare equal (-0 == 0, inf == inf, no NaN left), a labelled class is one whose key is below +inf, and "labelled before
     * unlabelled, then the smaller value" is one comparison of keys.  A finite key has its corner's bits. */
    const float inf = __builtin_inff();
    float K[8];
#pragma unroll
    for (int c = 0; c < 8; c++) K[c] = fabsf(L[c]) < inf ? L[c] : inf;
    float best = K[0], best_s = 0.0f;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        float s = 0.0f;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            /* each pair is compared once: the indices are compile-time constants after unrolling */
            const float t = e == c ? W[e] : (K[c < e ? c : e] == K[c < e ? e : c] ? W[e] : 0.0f);
            s = e == 0 ? t : s + t;
        }
        /* corner 0 opens; a later corner takes over only when its class is strictly better, so a class keeps its lowest corner.
         * & and |, not && and ||: selects, no branches */
        const bool better = (c == 0) | (s > best_s) | ((s == best_s) & (K[c] < best));
        best = better ? K[c] : best;
        best_s = better ? s : best_s;
    }
    return best < inf ? best : __builtin_nanf("");
}

/* src (nx x ny x nz, x fastest) at the position (qx, qy, qz); hx = (float)(nx - 1) and so on; `fill` outside.  MODE: WARP_* */
template <int MODE>
__device__ __forceinline__ float sample_volume(const float *__restrict__ src, long long nx, long long ny, long long nz, float hx, float hy, float hz,
                                               float qx, float qy, float qz, float fill)
{
    static_assert(MODE == WARP_LINEAR || MODE == WARP_NEAREST || MODE == WARP_LABEL, "sample_volume: unknown mode");
    if (!(qx >= 0.0f && qx <= hx && qy >= 0.0f && qy <= hy && qz >= 0.0f && qz <= hz)) return fill;
    if (MODE == WARP_NEAREST) {
        /* q <= n - 1 <= 2^24 - 1 here: the int conversions give the values of (int64) ones, in one instruction */
        long long ix = (int)floorf(qx + 0.5f), iy = (int)floorf(qy + 0.5f), iz = (int)floorf(qz + 0.5f);
        ix = ix < nx - 1 ? ix : nx - 1;
        iy = iy < ny - 1 ? iy : ny - 1;
        iz = iz < nz - 1 ? iz : nz - 1;
        return src[(iz * ny + iy) * nx + ix];
    }
    const float fx = floorf(qx), fy = floorf(qy), fz = floorf(qz);
    const float wx = qx - fx, wy = qy - fy, wz = qz - fz;
    const long long x0 = (int)fx, y0 = (int)fy, z0 = (int)fz;
    const long long x1 = x0 + 1 < nx - 1 ? x0 + 1 : nx - 1, y1 = y0 + 1 < ny - 1 ? y0 + 1 : ny - 1, z1 = z0 + 1 < nz - 1 ? z0 + 1 : nz - 1;
    const float *r00 = src + (z0 * ny + y0) * nx, *r10 = src + (z0 * ny + y1) * nx, *r01 = src + (z1 * ny + y0) * nx,
                *r11 = src + (z1 * ny + y1) * nx;
    const float ux = 1.0f - wx, uy = 1.0f - wy, uz = 1.0f - wz;
    if constexpr (MODE == WARP_LABEL) {
        /* linear's eight gathers; corner c = a + 2b + 4d */
        const float L[8] = {r00[x0], r00[x1], r10[x0], r10[x1], r01[x0], r01[x1], r11[x0], r11[x1]};
        const float xy00 = ux * uy, xy10 = wx * uy, xy01 = ux * wy, xy11 = wx * wy;
        const float W[8] = {xy00 * uz, xy10 * uz, xy01 * uz, xy11 * uz, xy00 * wz, xy10 * wz, xy01 * wz, xy11 * wz};
        return label_vote(L, W);
    } else {
        const float c00 = ux * r00[x0] + wx * r00[x1]; /* (y0, z0) */
        const float c10 = ux * r10[x0] + wx * r10[x1]; /* (y1, z0) */
        const float c01 = ux * r01[x0] + wx * r01[x1]; /* (y0, z1) */
        const float c11 = ux * r11[x0] + wx * r11[x1]; /* (y1, z1) */
        const float c0 = uy * c00 + wy * c10, c1 = uy * c01 + wy * c11;
        return uz * c0 + wz * c1;
    }
}

/* ---- the brick of output voxels ---- */

#define BRICK_TX 8                     /* threads along x */
#define BRICK_VX 4                     /* consecutive x voxels per thread */
#define BRICK_BX (BRICK_TX * BRICK_VX) /* 32 */
#define BRICK_BY 8
#define BRICK_BZ 4                     /* BRICK_TX * BRICK_BY * BRICK_BZ = 256 threads */
#define BRICK_MAX_GRID (1u << 22)

/* the first brick slot of this block; the next ones follow in strides of the grid */
__device__ __forceinline__ long long brick_slot0()
{
    const unsigned grid = gridDim.x, b = blockIdx.x;
    return (long long)(b & 7u) * (grid >> 3) + (b >> 3);
}

/* this thread's place in its brick: its four voxels start at x = BRICK_VX * tx */
__device__ __forceinline__ void brick_lane(int &tx, int &ty, int &tz)
{
    tx = threadIdx.x & (BRICK_TX - 1);
    ty = (threadIdx.x / BRICK_TX) & (BRICK_BY - 1);
    tz = threadIdx.x / (BRICK_TX * BRICK_BY);
}

/* brick slot L -> the brick's first voxel (x0, y0, z0): the same for every thread of the block, so scalar arithmetic */
__device__ __forceinline__ void brick_origin(long long L, long long nbx, long long nby, long long &x0, long long &y0, long long &z0)
{
    const long long bx = L % nbx, t = L / nbx, by = t % nby, bz = t / nby;
    x0 = bx * BRICK_BX;
    y0 = by * BRICK_BY;
    z0 = bz * BRICK_BZ;
}

/* brick slot L -> the first of this thread's four voxels, (i0, j, k); it may lie outside the output */
__device__ __forceinline__ void brick_voxel(long long L, long long nbx, long long nby, int tx, int ty, int tz, long long &i0, long long &j,
                                            long long &k)
{
    long long x0, y0, z0;
    brick_origin(L, nbx, nby, x0, y0, z0);
    i0 = x0 + tx * BRICK_VX;
    j = y0 + ty;
    k = z0 + tz;
}

/* r[0 .. 3] to the row's voxels i0 .. i0 + 3 at dst, as far as the row (ox voxels) reaches */
__device__ __forceinline__ void store_row4(float *__restrict__ dst, long long ox, long long i0, const float r[BRICK_VX], int vec)
{
    if (vec && i0 + BRICK_VX <= ox) {
        *reinterpret_cast<float4 *>(dst) = make_float4(r[0], r[1], r[2], r[3]);
    } else {
#pragma unroll
        for (int v = 0; v < BRICK_VX; v++)
            if (i0 + v < ox) dst[v] = r[v];
    }
}

struct brick_launch {
    long long nbx, nby, nbricks;
    unsigned grid; /* a multiple of the XCD count: grid / 8 slots per XCD */
    int vec;       /* 16-byte stores: rows of whole float4s and an aligned base */
};

/* host */
inline brick_launch brick_launch_of(const float *dst, int64_t ox, int64_t oy, int64_t oz)
{
    brick_launch b;
    b.nbx = (ox + BRICK_BX - 1) / BRICK_BX;
    b.nby = (oy + BRICK_BY - 1) / BRICK_BY;
    b.nbricks = b.nbx * b.nby * ((oz + BRICK_BZ - 1) / BRICK_BZ);
    const long long g = (b.nbricks + 7) / 8 * 8;
    b.grid = g > (long long)BRICK_MAX_GRID ? BRICK_MAX_GRID : (unsigned)g;
    b.vec = (ox % BRICK_VX) == 0 && ((uintptr_t)dst % 16) == 0;
    return b;
}

/* ---- the brick of nodes ---- */

#define NODE_BX 8
#define NODE_BY 8
#define NODE_BZ 4
#define NODE_MAX_GRID (1u << 20)

/* this lane's place in its brick of nodes: each wave a 4 x 4 x 4 part */
__device__ __forceinline__ void node_lane(int &lx, int &ly, int &lz)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    lx = (lane & 3) + (wv & 1) * 4;
    ly = ((lane >> 2) & 3) + (wv >> 1) * 4;
    lz = lane >> 4;
}

/* brick slot L -> this lane's node (a, b, c); it may lie outside the grid */
__device__ __forceinline__ void node_of_slot(long long L, long long nb0, long long nb1, int lx, int ly, int lz, long long &a, long long &b,
                                             long long &c)
{
    const long long bx = L % nb0, t0 = L / nb0, by = t0 % nb1, bz = t0 / nb1;
    a = bx * NODE_BX + lx;
    b = by * NODE_BY + ly;
    c = bz * NODE_BZ + lz;
}

struct node_launch {
    long long nb0, nb1, nbricks;
    unsigned grid;
};

/* host */
inline node_launch node_launch_of(const int64_t n[3])
{
    node_launch b;
    b.nb0 = (n[0] + NODE_BX - 1) / NODE_BX;
    b.nb1 = (n[1] + NODE_BY - 1) / NODE_BY;
    b.nbricks = b.nb0 * b.nb1 * ((n[2] + NODE_BZ - 1) / NODE_BZ);
    b.grid = (unsigned)(b.nbricks < (long long)NODE_MAX_GRID ? b.nbricks : NODE_MAX_GRID);
    return b;
}

#endif
