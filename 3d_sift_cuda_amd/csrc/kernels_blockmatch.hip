/*
 * kernels_blockmatch.hip -- the block search of the intensity refinement (tests/blockmatch_oracle.c
 * restates it as a serial brute force).  Two kernels: bm_quantize_kernel maps a float volume to 10-bit integers (-1: not
 * finite) with the affine map the host fixed, and block_match_kernel<B, R, P> finds, per lattice node, the integer shift of
 * the least sum of squared differences.  Every sum is an integer below 2^32, so no result depends on the order of the
 * additions, the tiling or the wave layout.
 *
 * Mapping.  A workgroup of 256 lanes owns a brick of up to 4 x 4 x 2 neighbouring nodes (the launcher shrinks the brick
 * until its tiles fit 64 KiB of LDS).  It stages the brick's F tile and W tile (the union of the nodes' blocks and search
 * windows, which overlap heavily at stride 4) as int16 once, then
 *   pass 1: one lane per (node, row of the F block / the W window): flag and the block's sums, by LDS atomics;
 *   pass 2: one lane per (node, sz, sy): the 2r+1 costs along sx.  With B, R > 0 (compile-time b, r) the lane keeps a row of
 *           F (2b+1 values) and of W (2b+1+2r) in registers per block row, so 2b+1+2b+1+2r LDS reads feed (2r+1)(2b+1)
 *           multiply-adds, and with P != 0 takes the differences two at a time (v_pk_sub_i16) into v_dot2_i32_i16; B = R = 0 is
 *           the form for any b, r (two LDS reads per multiply-add).  The lane's best shift goes
 *           into the node's 64-bit key cost << 19 | |s|^2 << 12 | (sz+r) << 8 | (sy+r) << 4 | (sx+r) by an LDS atomic min: the
 *           least key is the least cost, ties by the least |s|^2, then z, y, x;
 *   pass 3: one lane per (node, axis neighbour of the argmin): that cost again from the tiles (6 of the (2r+1)^3 shifts).
 * block_match_ncc_kernel<B, R>, further down, is the same search under the correlation cost of DESIGN.md section 7g.
 */
#include "sift3d_internal.h"

#define BM_THREADS 256
#define BM_QMAX 1023
#define BM_LDS_MAX 65536
#define BM_NONE 0xffffffffu

struct bm_args {
    int nx, ny, nz;        /* the volumes' extents */
    int f0[3], st, n[3];   /* the lattice: first node (x, y, z), stride, count per axis */
    int b, r;
    int nb[3];             /* nodes per brick and axis */
    int bricks[3];         /* bricks per axis */
};

__global__ __launch_bounds__(256) void bm_quantize_kernel(const float *__restrict__ src, long long n, double lo, double hi, short *__restrict__ dst)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = src[i];
    short q = -1;
    if (isfinite(v)) {
        const double t = (((double)v - lo) / (hi - lo)) * (double)BM_QMAX;
        q = t <= 0.0 ? (short)0 : (t >= (double)BM_QMAX ? (short)BM_QMAX : (short)(int)rint(t));
    }
    dst[i] = q;
}

/* Sum over one block of (F(p + u) - W(p + u + s))^2 from the tiles: f at the block's first voxel, w at the window's first
 * voxel of this shift */
__device__ __forceinline__ unsigned bm_cost_at(const short *f, const short *w, int side, int fx, int fxy, int wx, int wxy)
{
    unsigned c = 0;
    for (int z = 0; z < side; z++)
        for (int y = 0; y < side; y++) {
            const short *fr = f + z * fxy + y * fx, *wr = w + z * wxy + y * wx;
            for (int x = 0; x < side; x++) {
                const int d = (int)fr[x] - (int)wr[x];
                c += (unsigned)__mul24(d, d);
            }
        }
    return c;
}

typedef short bm_s2 __attribute__((ext_vector_type(2)));

/* P != 0: the row of differences two at a time (v_pk_sub_i16) into v_dot2_i32_i16, whose 32-bit sum wraps as the unsigned one does */
template <int B, int R, int P> __global__ __launch_bounds__(BM_THREADS) void block_match_kernel(const short *__restrict__ qf, const short *__restrict__ qw, bm_args a, unsigned *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char bm_lds[];
    const int b = B > 0 ? B : a.b, r = R > 0 ? R : a.r;
    const int side = 2 * b + 1, S = 2 * r + 1, S2 = S * S;
    const int NN = a.nb[0] * a.nb[1] * a.nb[2];
    /* tiles: F over the bricks' blocks, W over their windows */
    const int fx = (a.nb[0] - 1) * a.st + side, fy = (a.nb[1] - 1) * a.st + side, fz = (a.nb[2] - 1) * a.st + side;
    const int wx = fx + 2 * r, wy = fy + 2 * r, wz = fz + 2 * r;
    const int fxy = fx * fy, wxy = wx * wy, fvol = fxy * fz, wvol = wxy * wz;
    unsigned long long *key = reinterpret_cast<unsigned long long *>(bm_lds);
    unsigned *c0 = reinterpret_cast<unsigned *>(key + NN), *flag = c0 + NN, *sf = flag + NN, *sf2 = sf + NN;
    short *tf = reinterpret_cast<short *>(sf2 + NN), *tw = tf + ((fvol + 1) & ~1);

    const long long L = blockIdx.x;
    const int bx = (int)(L % a.bricks[0]), by = (int)((L / a.bricks[0]) % a.bricks[1]), bz = (int)(L / ((long long)a.bricks[0] * a.bricks[1]));
    const int na0 = bx * a.nb[0], nb0 = by * a.nb[1], nc0 = bz * a.nb[2];                                /* first node of the brick */
    const int px = a.f0[0] + na0 * a.st, py = a.f0[1] + nb0 * a.st, pz = a.f0[2] + nc0 * a.st; /* its voxel */
    const int tid = threadIdx.x;

    for (int i = tid; i < NN; i += BM_THREADS) {
        key[i] = ~0ull;
        c0[i] = 0;
        flag[i] = 0;
        sf[i] = 0;
        sf2[i] = 0;
    }
    for (int i = tid; i < fvol; i += BM_THREADS) {
        const int x = i % fx, t = i / fx, y = t % fy, z = t / fy;
        const int gx = px - b + x, gy = py - b + y, gz = pz - b + z;
        short v = -1;
        if (gx >= 0 && gx < a.nx && gy >= 0 && gy < a.ny && gz >= 0 && gz < a.nz) v = qf[((long long)gz * a.ny + gy) * a.nx + gx];
        tf[i] = v;
    }
    for (int i = tid; i < wvol; i += BM_THREADS) {
        const int x = i % wx, t = i / wx, y = t % wy, z = t / wy;
        const int gx = px - b - r + x, gy = py - b - r + y, gz = pz - b - r + z;
        short v = -1;
        if (gx >= 0 && gx < a.nx && gy >= 0 && gy < a.ny && gz >= 0 && gz < a.nz) v = qw[((long long)gz * a.ny + gy) * a.nx + gx];
        tw[i] = v;
    }
    __syncthreads();

    /* pass 1: flags and the block's sums */
    {
        const int frows = side * side, wside = side + 2 * r, wrows = wside * wside;
        for (int it = tid; it < NN * frows; it += BM_THREADS) {
            const int nd = it / frows, row = it - nd * frows;
            const int la = nd % a.nb[0], lb = (nd / a.nb[0]) % a.nb[1], lc = nd / (a.nb[0] * a.nb[1]);
            if (na0 + la >= a.n[0] || nb0 + lb >= a.n[1] || nc0 + lc >= a.n[2]) continue;
            const short *p = tf + (lc * a.st + row / side) * fxy + (lb * a.st + row % side) * fx + la * a.st;
            unsigned s1 = 0, s2 = 0;
            int bad = 0;
            for (int x = 0; x < side; x++) {
                const int v = p[x];
                bad |= v < 0;
                s1 += (unsigned)v;
                s2 += (unsigned)__mul24(v, v);
            }
            if (bad) atomicOr(&flag[nd], 1u);
            atomicAdd(&sf[nd], s1);
            atomicAdd(&sf2[nd], s2);
        }
        for (int it = tid; it < NN * wrows; it += BM_THREADS) {
            const int nd = it / wrows, row = it - nd * wrows;
            const int la = nd % a.nb[0], lb = (nd / a.nb[0]) % a.nb[1], lc = nd / (a.nb[0] * a.nb[1]);
            if (na0 + la >= a.n[0] || nb0 + lb >= a.n[1] || nc0 + lc >= a.n[2]) continue;
            const short *p = tw + (lc * a.st + row / wside) * wxy + (lb * a.st + row % wside) * wx + la * a.st;
            int bad = 0;
            for (int x = 0; x < wside; x++) bad |= p[x] < 0;
            if (bad) atomicOr(&flag[nd], 1u);
        }
    }
    __syncthreads();

    /* pass 2: the costs of every shift; the least key per node */
    for (int it = tid; it < NN * S2; it += BM_THREADS) {
        const int nd = it / S2, rem = it - nd * S2, sz = rem / S, sy = rem - sz * S; /* sz, sy in 0 .. 2r */
        const int la = nd % a.nb[0], lb = (nd / a.nb[0]) % a.nb[1], lc = nd / (a.nb[0] * a.nb[1]);
        if (na0 + la >= a.n[0] || nb0 + lb >= a.n[1] || nc0 + lc >= a.n[2] || flag[nd]) continue;
        const short *f = tf + (lc * a.st) * fxy + (lb * a.st) * fx + la * a.st;
        const short *w = tw + (lc * a.st + sz) * wxy + (lb * a.st + sy) * wx + la * a.st;
        const int dz = sz - r, dy = sy - r;
        const unsigned zy2 = (unsigned)(dz * dz + dy * dy);
        unsigned long long best = ~0ull;
        if constexpr (B > 0 && R > 0) {
            unsigned c[2 * R + 1];
#pragma unroll
            for (int s = 0; s < 2 * R + 1; s++) c[s] = 0;
            for (int z = 0; z < 2 * B + 1; z++)
                for (int y = 0; y < 2 * B + 1; y++) {
                    const short *fr = f + z * fxy + y * fx, *wr = w + z * wxy + y * wx;
                    int fv[2 * B + 1], wv[2 * B + 1 + 2 * R];
#pragma unroll
                    for (int x = 0; x < 2 * B + 1; x++) fv[x] = fr[x];
#pragma unroll
                    for (int x = 0; x < 2 * B + 1 + 2 * R; x++) wv[x] = wr[x];
                    if constexpr (P != 0) {
                        bm_s2 fp[B], wp[2 * B + 2 * R];
#pragma unroll
                        for (int x = 0; x < B; x++) fp[x] = bm_s2{(short)fv[2 * x], (short)fv[2 * x + 1]};
#pragma unroll
                        for (int x = 0; x < 2 * B + 2 * R; x++) wp[x] = bm_s2{(short)wv[x], (short)wv[x + 1]};
#pragma unroll
                        for (int s = 0; s < 2 * R + 1; s++) {
                            int acc = (int)c[s];
#pragma unroll
                            for (int x = 0; x < B; x++) {
                                const bm_s2 d = fp[x] - wp[2 * x + s];
                                acc = __builtin_amdgcn_sdot2(d, d, acc, false);
                            }
                            const int d = fv[2 * B] - wv[2 * B + s];
                            c[s] = (unsigned)acc + (unsigned)__mul24(d, d);
                        }
                    } else {
#pragma unroll
                        for (int s = 0; s < 2 * R + 1; s++)
#pragma unroll
                            for (int x = 0; x < 2 * B + 1; x++) {
                                const int d = fv[x] - wv[x + s];
                                c[s] += (unsigned)__mul24(d, d);
                            }
                    }
                }
#pragma unroll
            for (int s = 0; s < 2 * R + 1; s++) {
                const int dx = s - R;
                const unsigned long long k = ((unsigned long long)c[s] << 19) | ((unsigned long long)(zy2 + (unsigned)(dx * dx)) << 12) |
                                             (unsigned long long)((sz << 8) | (sy << 4) | s);
                best = k < best ? k : best;
                if (dz == 0 && dy == 0 && dx == 0) c0[nd] = c[s];
            }
        } else {
            for (int s = 0; s < S; s++) {
                const unsigned c = bm_cost_at(f, w + s, side, fx, fxy, wx, wxy);
                const int dx = s - r;
                const unsigned long long k = ((unsigned long long)c << 19) | ((unsigned long long)(zy2 + (unsigned)(dx * dx)) << 12) |
                                             (unsigned long long)((sz << 8) | (sy << 4) | s);
                best = k < best ? k : best;
                if (dz == 0 && dy == 0 && dx == 0) c0[nd] = c;
            }
        }
        atomicMin(&key[nd], best);
    }
    __syncthreads();

    /* pass 3: the costs beside the argmin; the records */
    for (int it = tid; it < NN * 8; it += BM_THREADS) {
        const int nd = it >> 3, slot = it & 7;
        const int la = nd % a.nb[0], lb = (nd / a.nb[0]) % a.nb[1], lc = nd / (a.nb[0] * a.nb[1]);
        if (na0 + la >= a.n[0] || nb0 + lb >= a.n[1] || nc0 + lc >= a.n[2]) continue;
        const long long node = ((long long)(nc0 + lc) * a.n[1] + (nb0 + lb)) * a.n[0] + (na0 + la);
        unsigned *o = out + node * 16;
        const int fl = flag[nd] != 0;
        const unsigned long long k = key[nd];
        const int ax = (int)(k & 15u), ay = (int)((k >> 4) & 15u), az = (int)((k >> 8) & 15u); /* the argmin, 0 .. 2r */
        if (slot < 6) {
            unsigned c = 0;
            if (!fl) {
                int s[3] = {ax, ay, az};
                s[slot >> 1] += (slot & 1) ? 1 : -1;
                c = BM_NONE;
                if (s[0] >= 0 && s[0] < S && s[1] >= 0 && s[1] < S && s[2] >= 0 && s[2] < S)
                    c = bm_cost_at(tf + (lc * a.st) * fxy + (lb * a.st) * fx + la * a.st,
                                   tw + (lc * a.st + s[2]) * wxy + (lb * a.st + s[1]) * wx + la * a.st + s[0], side, fx, fxy, wx, wxy);
            }
            o[6 + slot] = c;
        } else if (slot == 6) {
            o[0] = fl ? 0u : (unsigned)(ax - r);
            o[1] = fl ? 0u : (unsigned)(ay - r);
            o[2] = fl ? 0u : (unsigned)(az - r);
            o[3] = (unsigned)fl;
            o[4] = fl ? 0u : (unsigned)(k >> 19);
            o[5] = fl ? 0u : c0[nd];
        } else {
            o[12] = fl ? 0u : sf[nd];
            o[13] = fl ? 0u : sf2[nd];
            o[14] = 0u;
            o[15] = 0u;
        }
    }
}

/* ---- the correlation cost (tests/blockmatch_ncc_oracle.c restates it) ------------------------------------
 * cost(s) = rint((1 - rho^2(s)) 2^31) of the zero-mean normalised cross-correlation rho of the F block and the shifted W block,
 * from five integer sums.  Widths: Sw < 2^22 and Sww, Sfw <= 13^3 1023^2 < 2^32 for b <= 6, as the squared differences were, so
 * they are accumulated in 32 bits; A = N Sfw - Sf Sw and the variances Vf, Vw do not fit (|A|, V <= (13^3 1023)^2 < 2^43) and are
 * formed in int64.  Each converts to double exactly; the rest is one sequence of IEEE double operations (multiply, multiply,
 * divide, subtract, multiply by 2^31, rint), which the host restates operation for operation: this file is compiled with
 * -ffp-contract=off and without fast-math, and fp64 multiply and divide are correctly rounded on the device.
 * block_match_kernel above is left exactly as it was: this kernel repeats its staging, pass 1, key and record rather than share
 * helpers with it, so that the SSD code objects keep their instruction streams. */
__device__ __forceinline__ unsigned bm_ncc_cost(long long N, long long Sf, long long Vf, unsigned Sw, unsigned Sww, unsigned Sfw)
{
    const long long A = N * (long long)Sfw - Sf * (long long)Sw;
    const long long Vw = N * (long long)Sww - (long long)Sw * (long long)Sw;
    double q = 0.0;
    if (A > 0 && Vf > 0 && Vw > 0) q = ((double)A * (double)A) / ((double)Vf * (double)Vw);
    q = q > 1.0 ? 1.0 : q;
    return (unsigned)rint((1.0 - q) * 2147483648.0);
}

/* Sw, Sww, Sfw over one block from the tiles: f at the block's first voxel, w at the window's first voxel of this shift */
__device__ __forceinline__ void bm_ncc_sums_at(const short *f, const short *w, int side, int fx, int fxy, int wx, int wxy, unsigned &sw,
                                               unsigned &sww, unsigned &sfw)
{
    unsigned a = 0, b = 0, c = 0;
    for (int z = 0; z < side; z++)
        for (int y = 0; y < side; y++) {
            const short *fr = f + z * fxy + y * fx, *wr = w + z * wxy + y * wx;
            for (int x = 0; x < side; x++) {
                const int fv = fr[x], wv = wr[x];
                a += (unsigned)wv;
                b += (unsigned)__mul24(wv, wv);
                c += (unsigned)__mul24(fv, wv);
            }
        }
    sw = a;
    sww = b;
    sfw = c;
}

/* B, R > 0: pass 2 keeps the rows in registers as block_match_kernel<B, R, 1> does and reads the same tile values.  Per block
 * row it adds every W value and its square (squared once per row) to a sum per window column, and the products to a sum per
 * shift, two at a time through v_dot2_i32_i16 on the packed pairs; after the last row the column sums slide into the 2r + 1
 * window sums.  B = R = 0: any b, r, three sums per shift straight from the tiles. */
template <int B, int R> __global__ __launch_bounds__(BM_THREADS) void block_match_ncc_kernel(const short *__restrict__ qf, const short *__restrict__ qw, bm_args a, unsigned *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char bm_lds[];
    const int b = B > 0 ? B : a.b, r = R > 0 ? R : a.r;
    const int side = 2 * b + 1, S = 2 * r + 1, S2 = S * S;
    const long long N = (long long)side * side * side;
    const int NN = a.nb[0] * a.nb[1] * a.nb[2];
    const int fx = (a.nb[0] - 1) * a.st + side, fy = (a.nb[1] - 1) * a.st + side, fz = (a.nb[2] - 1) * a.st + side;
    const int wx = fx + 2 * r, wy = fy + 2 * r, wz = fz + 2 * r;
    const int fxy = fx * fy, wxy = wx * wy, fvol = fxy * fz, wvol = wxy * wz;
    unsigned long long *key = reinterpret_cast<unsigned long long *>(bm_lds);
    unsigned *c0 = reinterpret_cast<unsigned *>(key + NN), *flag = c0 + NN, *sf = flag + NN, *sf2 = sf + NN;
    short *tf = reinterpret_cast<short *>(sf2 + NN), *tw = tf + ((fvol + 1) & ~1);

    const long long L = blockIdx.x;
    const int bx = (int)(L % a.bricks[0]), by = (int)((L / a.bricks[0]) % a.bricks[1]), bz = (int)(L / ((long long)a.bricks[0] * a.bricks[1]));
    const int na0 = bx * a.nb[0], nb0 = by * a.nb[1], nc0 = bz * a.nb[2];
    const int px = a.f0[0] + na0 * a.st, py = a.f0[1] + nb0 * a.st, pz = a.f0[2] + nc0 * a.st;
    const int tid = threadIdx.x;

    for (int i = tid; i < NN; i += BM_THREADS) {
        key[i] = ~0ull;
        c0[i] = 0;
        flag[i] = 0;
        sf[i] = 0;
        sf2[i] = 0;
    }
    for (int i = tid; i < fvol; i += BM_THREADS) {
        const int x = i % fx, t = i / fx, y = t % fy, z = t / fy;
        const int gx = px - b + x, gy = py - b + y, gz = pz - b + z;
        short v = -1;
        if (gx >= 0 && gx < a.nx && gy >= 0 && gy < a.ny && gz >= 0 && gz < a.nz) v = qf[((long long)gz * a.ny + gy) * a.nx + gx];
        tf[i] = v;
    }
    for (int i = tid; i < wvol; i += BM_THREADS) {
        const int x = i % wx, t = i / wx, y = t % wy, z = t / wy;
        const int gx = px - b - r + x, gy = py - b - r + y, gz = pz - b - r + z;
        short v = -1;
        if (gx >= 0 && gx < a.nx && gy >= 0 && gy < a.ny && gz >= 0 && gz < a.nz) v = qw[((long long)gz * a.ny + gy) * a.nx + gx];
        tw[i] = v;
    }
    __syncthreads();

    /* pass 1: flags and the F block's sums */
    {
        const int frows = side * side, wside = side + 2 * r, wrows = wside * wside;
        for (int it = tid; it < NN * frows; it += BM_THREADS) {
            const int nd = it / frows, row = it - nd * frows;
            const int la = nd % a.nb[0], lb = (nd / a.nb[0]) % a.nb[1], lc = nd / (a.nb[0] * a.nb[1]);
            if (na0 + la >= a.n[0] || nb0 + lb >= a.n[1] || nc0 + lc >= a.n[2]) continue;
            const short *p = tf + (lc * a.st + row / side) * fxy + (lb * a.st + row % side) * fx + la * a.st;
            unsigned s1 = 0, s2 = 0;
            int bad = 0;
            for (int x = 0; x < side; x++) {
                const int v = p[x];
                bad |= v < 0;
                s1 += (unsigned)v;
                s2 += (unsigned)__mul24(v, v);
            }
            if (bad) atomicOr(&flag[nd], 1u);
            atomicAdd(&sf[nd], s1);
            atomicAdd(&sf2[nd], s2);
        }
        for (int it = tid; it < NN * wrows; it += BM_THREADS) {
            const int nd = it / wrows, row = it - nd * wrows;
            const int la = nd % a.nb[0], lb = (nd / a.nb[0]) % a.nb[1], lc = nd / (a.nb[0] * a.nb[1]);
            if (na0 + la >= a.n[0] || nb0 + lb >= a.n[1] || nc0 + lc >= a.n[2]) continue;
            const short *p = tw + (lc * a.st + row / wside) * wxy + (lb * a.st + row % wside) * wx + la * a.st;
            int bad = 0;
            for (int x = 0; x < wside; x++) bad |= p[x] < 0;
            if (bad) atomicOr(&flag[nd], 1u);
        }
    }
    __syncthreads();

    /* pass 2: the costs of every shift; the least key per node */
    for (int it = tid; it < NN * S2; it += BM_THREADS) {
        const int nd = it / S2, rem = it - nd * S2, sz = rem / S, sy = rem - sz * S; /* sz, sy in 0 .. 2r */
        const int la = nd % a.nb[0], lb = (nd / a.nb[0]) % a.nb[1], lc = nd / (a.nb[0] * a.nb[1]);
        if (na0 + la >= a.n[0] || nb0 + lb >= a.n[1] || nc0 + lc >= a.n[2] || flag[nd]) continue;
        const short *f = tf + (lc * a.st) * fxy + (lb * a.st) * fx + la * a.st;
        const short *w = tw + (lc * a.st + sz) * wxy + (lb * a.st + sy) * wx + la * a.st;
        const int dz = sz - r, dy = sy - r;
        const unsigned zy2 = (unsigned)(dz * dz + dy * dy);
        const long long Sf = (long long)sf[nd], Vf = N * (long long)sf2[nd] - Sf * Sf;
        unsigned long long best = ~0ull;
        if constexpr (B > 0 && R > 0) {
            constexpr int WN = 2 * B + 1 + 2 * R;
            unsigned cw[WN], cww[WN];
            int cfw[2 * R + 1];
#pragma unroll
            for (int x = 0; x < WN; x++) cw[x] = cww[x] = 0;
#pragma unroll
            for (int s = 0; s < 2 * R + 1; s++) cfw[s] = 0;
            for (int z = 0; z < 2 * B + 1; z++)
                for (int y = 0; y < 2 * B + 1; y++) {
                    const short *fr = f + z * fxy + y * fx, *wr = w + z * wxy + y * wx;
                    int fv[2 * B + 1], wv[WN];
#pragma unroll
                    for (int x = 0; x < 2 * B + 1; x++) fv[x] = fr[x];
#pragma unroll
                    for (int x = 0; x < WN; x++) wv[x] = wr[x];
#pragma unroll
                    for (int x = 0; x < WN; x++) {
                        cw[x] += (unsigned)wv[x];
                        cww[x] += (unsigned)__mul24(wv[x], wv[x]);
                    }
                    bm_s2 fp[B], wp[2 * B + 2 * R];
#pragma unroll
                    for (int x = 0; x < B; x++) fp[x] = bm_s2{(short)fv[2 * x], (short)fv[2 * x + 1]};
#pragma unroll
                    for (int x = 0; x < 2 * B + 2 * R; x++) wp[x] = bm_s2{(short)wv[x], (short)wv[x + 1]};
#pragma unroll
                    for (int s = 0; s < 2 * R + 1; s++) {
                        int acc = cfw[s];
#pragma unroll
                        for (int x = 0; x < B; x++) acc = __builtin_amdgcn_sdot2(fp[x], wp[2 * x + s], acc, false);
                        cfw[s] = acc + __mul24(fv[2 * B], wv[2 * B + s]);
                    }
                }
            unsigned sw = 0, sww = 0;
#pragma unroll
            for (int x = 0; x < 2 * B + 1; x++) {
                sw += cw[x];
                sww += cww[x];
            }
#pragma unroll
            for (int s = 0; s < 2 * R + 1; s++) {
                const unsigned c = bm_ncc_cost(N, Sf, Vf, sw, sww, (unsigned)cfw[s]);
                const int dx = s - R;
                const unsigned long long k = ((unsigned long long)c << 19) | ((unsigned long long)(zy2 + (unsigned)(dx * dx)) << 12) |
                                             (unsigned long long)((sz << 8) | (sy << 4) | s);
                best = k < best ? k : best;
                if (dz == 0 && dy == 0 && dx == 0) c0[nd] = c;
                if (s < 2 * R) {
                    sw += cw[s + 2 * B + 1] - cw[s];
                    sww += cww[s + 2 * B + 1] - cww[s];
                }
            }
        } else {
            for (int s = 0; s < S; s++) {
                unsigned sw, sww, sfw;
                bm_ncc_sums_at(f, w + s, side, fx, fxy, wx, wxy, sw, sww, sfw);
                const unsigned c = bm_ncc_cost(N, Sf, Vf, sw, sww, sfw);
                const int dx = s - r;
                const unsigned long long k = ((unsigned long long)c << 19) | ((unsigned long long)(zy2 + (unsigned)(dx * dx)) << 12) |
                                             (unsigned long long)((sz << 8) | (sy << 4) | s);
                best = k < best ? k : best;
                if (dz == 0 && dy == 0 && dx == 0) c0[nd] = c;
            }
        }
        atomicMin(&key[nd], best);
    }
    __syncthreads();

    /* pass 3: the costs beside the argmin; the records */
    for (int it = tid; it < NN * 8; it += BM_THREADS) {
        const int nd = it >> 3, slot = it & 7;
        const int la = nd % a.nb[0], lb = (nd / a.nb[0]) % a.nb[1], lc = nd / (a.nb[0] * a.nb[1]);
        if (na0 + la >= a.n[0] || nb0 + lb >= a.n[1] || nc0 + lc >= a.n[2]) continue;
        const long long node = ((long long)(nc0 + lc) * a.n[1] + (nb0 + lb)) * a.n[0] + (na0 + la);
        unsigned *o = out + node * 16;
        const int fl = flag[nd] != 0;
        const unsigned long long k = key[nd];
        const int ax = (int)(k & 15u), ay = (int)((k >> 4) & 15u), az = (int)((k >> 8) & 15u); /* the argmin, 0 .. 2r */
        if (slot < 6) {
            unsigned c = 0;
            if (!fl) {
                int s[3] = {ax, ay, az};
                s[slot >> 1] += (slot & 1) ? 1 : -1;
                c = BM_NONE;
                if (s[0] >= 0 && s[0] < S && s[1] >= 0 && s[1] < S && s[2] >= 0 && s[2] < S) {
                    unsigned sw, sww, sfw;
                    bm_ncc_sums_at(tf + (lc * a.st) * fxy + (lb * a.st) * fx + la * a.st,
                                   tw + (lc * a.st + s[2]) * wxy + (lb * a.st + s[1]) * wx + la * a.st + s[0], side, fx, fxy, wx, wxy, sw, sww, sfw);
                    const long long Sf = (long long)sf[nd];
                    c = bm_ncc_cost(N, Sf, N * (long long)sf2[nd] - Sf * Sf, sw, sww, sfw);
                }
            }
            o[6 + slot] = c;
        } else if (slot == 6) {
            o[0] = fl ? 0u : (unsigned)(ax - r);
            o[1] = fl ? 0u : (unsigned)(ay - r);
            o[2] = fl ? 0u : (unsigned)(az - r);
            o[3] = (unsigned)fl;
            o[4] = fl ? 0u : (unsigned)(k >> 19);
            o[5] = fl ? 0u : c0[nd];
        } else {
            o[12] = fl ? 0u : sf[nd];
            o[13] = fl ? 0u : sf2[nd];
            o[14] = 0u;
            o[15] = 0u;
        }
    }
}

hipError_t sift3d_launch_bm_quantize(hipStream_t s, const float *src, int64_t n, double lo, double hi, short *dst)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(bm_quantize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, (long long)n, lo, hi, dst);
    return hipGetLastError();
}

static size_t bm_lds_bytes(const int nb[3], int st, int b, int r)
{
    const size_t NN = (size_t)nb[0] * nb[1] * nb[2];
    size_t f = 1, w = 1;
    for (int k = 0; k < 3; k++) {
        f *= (size_t)(nb[k] - 1) * st + 2 * b + 1;
        w *= (size_t)(nb[k] - 1) * st + 2 * b + 1 + 2 * r;
    }
    return NN * 24 + 2 * ((f + 1) & ~(size_t)1) + 2 * w;
}

/* The brick and the grid of a launch: 4 x 4 x 2 nodes, shrunk (z, then y, then x) until the tiles fit */
static hipError_t bm_plan(int64_t nx, int64_t ny, int64_t nz, const int64_t first[3], int64_t stride, const int64_t n[3], int b, int r, bm_args &a,
                          size_t &lds, long long &bricks)
{
    a.nx = (int)nx;
    a.ny = (int)ny;
    a.nz = (int)nz;
    a.st = (int)stride;
    a.b = b;
    a.r = r;
    int nb[3] = {4, 4, 2};
    for (int k = 0; k < 3; k++) {
        a.f0[k] = (int)first[k];
        a.n[k] = (int)n[k];
        if (n[k] < nb[k]) nb[k] = (int)n[k];
    }
    while (bm_lds_bytes(nb, a.st, b, r) > BM_LDS_MAX) {
        const int k = nb[2] > 1 ? 2 : (nb[1] > 1 ? 1 : 0);
        if (nb[k] == 1) return hipErrorInvalidValue;
        nb[k] = (nb[k] + 1) / 2;
    }
    bricks = 1;
    for (int k = 0; k < 3; k++) {
        a.nb[k] = nb[k];
        a.bricks[k] = (a.n[k] + nb[k] - 1) / nb[k];
        bricks *= a.bricks[k];
    }
    if (bricks > 0x7fffffffll) return hipErrorInvalidValue;
    lds = bm_lds_bytes(nb, a.st, b, r);
    return hipSuccess;
}

/* qf, qw: the quantised volumes (nx ny nz int16, x fastest); first, stride, n: the lattice; out: 16 words per node.  The caller
 * has checked 1 <= b <= 6, 1 <= r <= 6, stride >= 1, the extents (each below 2^31 / 16) and n (each >= 1, product below 2^31).
 * generic: 0 the specialised form where there is one (packed differences); 1 the form for any b, r; 2 the specialised form with
 * one multiply-add per instruction (kept for the measurement).  The tests compare all three. */
hipError_t sift3d_launch_block_match(hipStream_t s, const short *qf, const short *qw, int64_t nx, int64_t ny, int64_t nz, const int64_t first[3],
                                     int64_t stride, const int64_t n[3], int b, int r, int generic, unsigned *out)
{
    bm_args a;
    size_t lds;
    long long bricks;
    const hipError_t e = bm_plan(nx, ny, nz, first, stride, n, b, r, a, lds, bricks);
    if (e != hipSuccess) return e;
    const dim3 g((unsigned)bricks), t(BM_THREADS);
    if (generic == 0 && b == 4 && r == 3) hipLaunchKernelGGL((block_match_kernel<4, 3, 1>), g, t, lds, s, qf, qw, a, out);
    else if (generic == 0 && b == 4 && r == 4) hipLaunchKernelGGL((block_match_kernel<4, 4, 1>), g, t, lds, s, qf, qw, a, out);
    else if (generic == 2 && b == 4 && r == 3) hipLaunchKernelGGL((block_match_kernel<4, 3, 0>), g, t, lds, s, qf, qw, a, out);
    else if (generic == 2 && b == 4 && r == 4) hipLaunchKernelGGL((block_match_kernel<4, 4, 0>), g, t, lds, s, qf, qw, a, out);
    else hipLaunchKernelGGL((block_match_kernel<0, 0, 0>), g, t, lds, s, qf, qw, a, out);
    return hipGetLastError();
}

/* The same search under the correlation cost.  generic: 0 the register form where there is one ((b, r) = (4, 3), (4, 4)); any
 * other value the form for any b, r.  Same words from both. */
hipError_t sift3d_launch_block_match_ncc(hipStream_t s, const short *qf, const short *qw, int64_t nx, int64_t ny, int64_t nz, const int64_t first[3],
                                         int64_t stride, const int64_t n[3], int b, int r, int generic, unsigned *out)
{
    bm_args a;
    size_t lds;
    long long bricks;
    const hipError_t e = bm_plan(nx, ny, nz, first, stride, n, b, r, a, lds, bricks);
    if (e != hipSuccess) return e;
    const dim3 g((unsigned)bricks), t(BM_THREADS);
    if (generic == 0 && b == 4 && r == 3) hipLaunchKernelGGL((block_match_ncc_kernel<4, 3>), g, t, lds, s, qf, qw, a, out);
    else if (generic == 0 && b == 4 && r == 4) hipLaunchKernelGGL((block_match_ncc_kernel<4, 4>), g, t, lds, s, qf, qw, a, out);
    else hipLaunchKernelGGL((block_match_ncc_kernel<0, 0>), g, t, lds, s, qf, qw, a, out);
    return hipGetLastError();
}
