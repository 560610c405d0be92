/*
 * kernels_blockmatch.hip -- the block search of the intensity refinement (DESIGN.md sections 7f, 7g; tests/blockmatch_oracle.c
 * and tests/blockmatch_ncc_oracle.c restate it as serial brute forces).  bm_quantize_kernel maps a float volume to 10-bit integers
 * (-1: not finite) with the affine map the host fixed; block_match_kernel<B, R, P> and block_match_ncc_kernel<B, R> find, per
 * lattice node, the integer shift of the least cost: the sum of squared differences, or the correlation cost of section 7g.
 * Both are bm_search over a cost type (bm_ssd, bm_ncc); everything but the cost is written once.  Every sum is an integer below
 * 2^32, so no result depends on the order of the additions, the tiling or the wave layout.
 *
 * Mapping.  A workgroup of 256 lanes owns a brick of up to 4 x 4 x 2 neighbouring nodes (the launcher shrinks the brick
 * until its tiles fit 64 KiB of LDS).  It stages the brick's F tile and W tile (the union of the nodes' blocks and search
 * windows, which overlap heavily at stride 4) as int16 once, then
 *   pass 1: one lane per (node, row of the F block / the W window): flag and the block's sums, by LDS atomics;
 *   pass 2: one lane per (node, sz, sy): the 2r+1 costs along sx.  With B, R > 0 (compile-time b, r) the lane keeps a row of
 *           F (2b+1 values) and of W (2b+1+2r) in registers per block row (the costs' along_x); B = R = 0 is the form for any
 *           b, r, every shift straight from the tiles (the costs' at).  The lane's best shift goes into the node's 64-bit key
 *           (bm_key) by an LDS atomic min: the least key is the least cost, ties by the least |s|^2, then z, y, x;
 *   pass 3: one lane per (node, axis neighbour of the argmin): that cost again from the tiles (6 of the (2r+1)^3 shifts), and
 *           the node's record.
 */
#include "sift3d_internal.h"
#include "patch_cost.h"
#include "quantize.h"

#define BM_THREADS 256
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
    dst[i] = (short)quantize(src[i], lo, hi);
}

/* A workgroup's brick: the search's sizes, the F and W tiles' extents and strides, the brick's first node and its voxel, and the
 * carve-up of the dynamic LDS (bm_lds_bytes on the host: 24 bytes per node, then the two tiles) */
struct bm_tiles {
    int b, r, side, S, NN;
    int fx, fy, fz, fxy, fvol;
    int wx, wy, wz, wxy, wvol;
    int n0[3], p0[3];
    unsigned long long *key;
    unsigned *c0, *flag, *sf, *sf2;
    short *tf, *tw;
};

__device__ __forceinline__ bm_tiles bm_setup(const bm_args &a, int b, int r, unsigned char *lds)
{
    bm_tiles t;
    t.b = b;
    t.r = r;
    t.side = 2 * b + 1;
    t.S = 2 * r + 1;
    t.NN = a.nb[0] * a.nb[1] * a.nb[2];
    t.fx = (a.nb[0] - 1) * a.st + t.side;
    t.fy = (a.nb[1] - 1) * a.st + t.side;
    t.fz = (a.nb[2] - 1) * a.st + t.side;
    t.wx = t.fx + 2 * r;
    t.wy = t.fy + 2 * r;
    t.wz = t.fz + 2 * r;
    t.fxy = t.fx * t.fy;
    t.wxy = t.wx * t.wy;
    t.fvol = t.fxy * t.fz;
    t.wvol = t.wxy * t.wz;
    const long long L = blockIdx.x;
    const int brick[3] = {(int)(L % a.bricks[0]), (int)((L / a.bricks[0]) % a.bricks[1]), (int)(L / ((long long)a.bricks[0] * a.bricks[1]))};
    for (int k = 0; k < 3; k++) {
        t.n0[k] = brick[k] * a.nb[k];
        t.p0[k] = a.f0[k] + t.n0[k] * a.st;
    }
    t.key = reinterpret_cast<unsigned long long *>(lds);
    t.c0 = reinterpret_cast<unsigned *>(t.key + t.NN);
    t.flag = t.c0 + t.NN;
    t.sf = t.flag + t.NN;
    t.sf2 = t.sf + t.NN;
    t.tf = reinterpret_cast<short *>(t.sf2 + t.NN);
    t.tw = t.tf + ((t.fvol + 1) & ~1);
    return t;
}

__device__ __forceinline__ void bm_clear(const bm_tiles &t)
{
    for (int i = threadIdx.x; i < t.NN; i += BM_THREADS) {
        t.key[i] = ~0ull;
        t.c0[i] = 0;
        t.flag[i] = 0;
        t.sf[i] = 0;
        t.sf2[i] = 0;
    }
}

/* ex x ey x (vol / (ex ey)) values of src from voxel o on into the tile; -1 outside the volume */
__device__ __forceinline__ void bm_load_tile(const short *__restrict__ src, const bm_args &a, const int o[3], int back, int ex, int ey, int vol, short *tile)
{
    for (int i = threadIdx.x; i < vol; i += BM_THREADS) {
        const int x = i % ex, t = i / ex, y = t % ey, z = t / ey;
        const int gx = o[0] - back + x, gy = o[1] - back + y, gz = o[2] - back + z;
        short v = -1;
        if (gx >= 0 && gx < a.nx && gy >= 0 && gy < a.ny && gz >= 0 && gz < a.nz) v = src[((long long)gz * a.ny + gy) * a.nx + gx];
        tile[i] = v;
    }
}

/* Node nd of the brick: its place in the brick, whether the lattice has it, and the first voxel of its block in the F tile and
 * of its window in the W tile */
struct bm_node {
    int l[3];
    bool in;
    const short *f, *w;
};

__device__ __forceinline__ bm_node bm_local(const bm_args &a, const bm_tiles &t, int nd)
{
    bm_node n;
    n.l[0] = nd % a.nb[0];
    n.l[1] = (nd / a.nb[0]) % a.nb[1];
    n.l[2] = nd / (a.nb[0] * a.nb[1]);
    n.in = t.n0[0] + n.l[0] < a.n[0] && t.n0[1] + n.l[1] < a.n[1] && t.n0[2] + n.l[2] < a.n[2];
    n.f = t.tf + (n.l[2] * a.st) * t.fxy + (n.l[1] * a.st) * t.fx + n.l[0] * a.st;
    n.w = t.tw + (n.l[2] * a.st) * t.wxy + (n.l[1] * a.st) * t.wx + n.l[0] * a.st;
    return n;
}

/* pass 1: flags and the F block's sums */
__device__ __forceinline__ void bm_pass1(const bm_args &a, const bm_tiles &t)
{
    const int frows = t.side * t.side, wside = t.side + 2 * t.r, wrows = wside * wside;
    for (int it = threadIdx.x; it < t.NN * frows; it += BM_THREADS) {
        const int nd = it / frows, row = it - nd * frows;
        const bm_node n = bm_local(a, t, nd);
        if (!n.in) continue;
        const short *p = n.f + (row / t.side) * t.fxy + (row % t.side) * t.fx;
        unsigned s1 = 0, s2 = 0;
        int bad = 0;
        for (int x = 0; x < t.side; x++) {
            const int v = p[x];
            bad |= v < 0;
            s1 += (unsigned)v;
            s2 += (unsigned)__mul24(v, v);
        }
        if (bad) atomicOr(&t.flag[nd], 1u);
        atomicAdd(&t.sf[nd], s1);
        atomicAdd(&t.sf2[nd], s2);
    }
    for (int it = threadIdx.x; it < t.NN * wrows; it += BM_THREADS) {
        const int nd = it / wrows, row = it - nd * wrows;
        const bm_node n = bm_local(a, t, nd);
        if (!n.in) continue;
        const short *p = n.w + (row / wside) * t.wxy + (row % wside) * t.wx;
        int bad = 0;
        for (int x = 0; x < wside; x++) bad |= p[x] < 0;
        if (bad) atomicOr(&t.flag[nd], 1u);
    }
}

/* The key of the shift (sx, sy, sz) in 0 .. 2r: the least key is the least cost, ties by the least |s|^2, then z, y, x */
__device__ __forceinline__ unsigned long long bm_key(unsigned cost, int r, int sx, int sy, int sz)
{
    const int dx = sx - r, dy = sy - r, dz = sz - r;
    return ((unsigned long long)cost << 19) | ((unsigned long long)(unsigned)(dz * dz + dy * dy + dx * dx) << 12) |
           (unsigned long long)((sz << 8) | (sy << 4) | sx);
}

/* pass 2's step: the lesser of best and the key of this shift and its cost; the zero shift's cost goes to the node's c0 */
__device__ __forceinline__ unsigned long long bm_take(const bm_tiles &t, int nd, unsigned long long best, unsigned cost, int sx, int sy, int sz)
{
    const unsigned long long k = bm_key(cost, t.r, sx, sy, sz);
    if (sx == t.r && sy == t.r && sz == t.r) t.c0[nd] = cost;
    return k < best ? k : best;
}

typedef short bm_s2 __attribute__((ext_vector_type(2)));

/* ---- the costs ----------------------------------------------------------------------------------------------------------------
 * A cost is made for one node after pass 1 and gives
 *   at<B>(f, w, t):      the cost of one shift straight from the tiles, f at the block's first voxel, w at the window's first
 *                        voxel of this shift.  B > 0: the caller knows b at compile time (pass 3 of the register forms), and
 *                        the rows go three to a loop iteration.  Left to itself the compiler unrolls all (2B + 1)^3 voxels
 *                        there and hoists the loads: under bm_ncc that spilled, and a whole plane of 2B + 1 rows per
 *                        iteration still took about 100 VGPRs in every form;
 *   along_x<B, R, P>():  the 2R + 1 costs along sx, w at the window's first voxel of sx = 0, a row of F and of W in registers
 *                        per block row.  The two loops over the rows stay loops: that is the code whose time is recorded in
 *                        DESIGN.md sections 7f and 7g, and the compiler otherwise unrolls one of them in some forms only. */

/* The sum of squared differences.  P != 0: the row of differences two at a time (v_pk_sub_i16) into v_dot2_i32_i16, whose 32-bit
 * sum wraps as the unsigned one does; P == 0: one multiply-add per instruction (kept for the measurement) */
struct bm_ssd {
    __device__ __forceinline__ bm_ssd(const bm_tiles &, int) {}

    template <int B> __device__ __forceinline__ unsigned at(const short *f, const short *w, const bm_tiles &t) const
    {
        constexpr int ROWS = B > 0 ? 3 : 1;
        unsigned c = 0;
#pragma unroll 1
        for (int z = 0; z < t.side; z++)
#pragma unroll ROWS
            for (int y = 0; y < t.side; y++) {
                const short *fr = f + z * t.fxy + y * t.fx, *wr = w + z * t.wxy + y * t.wx;
                for (int x = 0; x < t.side; x++) {
                    const int d = (int)fr[x] - (int)wr[x];
                    c += (unsigned)__mul24(d, d);
                }
            }
        return c;
    }

    template <int B, int R, int P> __device__ __forceinline__ void along_x(const short *f, const short *w, const bm_tiles &t, unsigned (&c)[2 * R + 1]) const
    {
#pragma unroll
        for (int s = 0; s < 2 * R + 1; s++) c[s] = 0;
#pragma unroll 1
        for (int z = 0; z < 2 * B + 1; z++)
#pragma unroll 1
            for (int y = 0; y < 2 * B + 1; y++) {
                const short *fr = f + z * t.fxy + y * t.fx, *wr = w + z * t.wxy + y * t.wx;
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
    }
};

/* The correlation cost: cost(s) = rint((1 - rho^2(s)) 2^31) of the zero-mean normalised cross-correlation
 * rho of the F block and the shifted W block, from five integer sums.  N is the block's voxel count; Sf and Vf = N Sff - Sf^2 come
 * from the node's words of pass 1.  Widths: Sw < 2^22 and Sww, Sfw <= 13^3 1023^2 < 2^32 for b <= 6, as the squared differences
 * are, so they are accumulated in 32 bits; A = N Sfw - Sf Sw and the variances Vf, Vw do not fit (|A|, V <= (13^3 1023)^2 < 2^43) and
 * are formed in int64.  What they cost is patch_cost.h's pc_ncc_cost, the one sequence of double operations. */
struct bm_ncc {
    long long N, Sf, Vf;

    __device__ __forceinline__ bm_ncc(const bm_tiles &t, int nd)
    {
        N = (long long)t.side * t.side * t.side;
        Sf = (long long)t.sf[nd];
        Vf = N * (long long)t.sf2[nd] - Sf * Sf;
    }

    __device__ __forceinline__ unsigned cost(unsigned Sw, unsigned Sww, unsigned Sfw) const
    {
        const long long A = N * (long long)Sfw - Sf * (long long)Sw;
        const long long Vw = N * (long long)Sww - (long long)Sw * (long long)Sw;
        return pc_ncc_cost(A, Vf, Vw);
    }

    template <int B> __device__ __forceinline__ unsigned at(const short *f, const short *w, const bm_tiles &t) const
    {
        constexpr int ROWS = B > 0 ? 3 : 1;
        unsigned sw = 0, sww = 0, sfw = 0;
#pragma unroll 1
        for (int z = 0; z < t.side; z++)
#pragma unroll ROWS
            for (int y = 0; y < t.side; y++) {
                const short *fr = f + z * t.fxy + y * t.fx, *wr = w + z * t.wxy + y * t.wx;
                for (int x = 0; x < t.side; x++) {
                    const int fv = fr[x], wv = wr[x];
                    sw += (unsigned)wv;
                    sww += (unsigned)__mul24(wv, wv);
                    sfw += (unsigned)__mul24(fv, wv);
                }
            }
        return cost(sw, sww, sfw);
    }

    /* Reads the tile values bm_ssd's does.  Per block row it adds every W value and its square (squared once per row) to a sum per
     * window column, and the products to a sum per shift, two at a time through v_dot2_i32_i16 on the packed pairs; after the last
     * row the column sums slide into the 2R + 1 window sums. */
    template <int B, int R, int P> __device__ __forceinline__ void along_x(const short *f, const short *w, const bm_tiles &t, unsigned (&c)[2 * R + 1]) const
    {
        constexpr int WN = 2 * B + 1 + 2 * R;
        unsigned cw[WN], cww[WN];
        int cfw[2 * R + 1];
#pragma unroll
        for (int x = 0; x < WN; x++) cw[x] = cww[x] = 0;
#pragma unroll
        for (int s = 0; s < 2 * R + 1; s++) cfw[s] = 0;
#pragma unroll 1
        for (int z = 0; z < 2 * B + 1; z++)
#pragma unroll 1
            for (int y = 0; y < 2 * B + 1; y++) {
                const short *fr = f + z * t.fxy + y * t.fx, *wr = w + z * t.wxy + y * t.wx;
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
            c[s] = cost(sw, sww, (unsigned)cfw[s]);
            if (s < 2 * R) {
                sw += cw[s + 2 * B + 1] - cw[s];
                sww += cww[s + 2 * B + 1] - cww[s];
            }
        }
    }
};

/* pass 3: the costs beside the argmin; the records */
template <class COST, int B> __device__ __forceinline__ void bm_pass3(const bm_args &a, const bm_tiles &t, unsigned *__restrict__ out)
{
    for (int it = threadIdx.x; it < t.NN * 8; it += BM_THREADS) {
        const int nd = it >> 3, slot = it & 7;
        const bm_node n = bm_local(a, t, nd);
        if (!n.in) continue;
        const long long node = ((long long)(t.n0[2] + n.l[2]) * a.n[1] + (t.n0[1] + n.l[1])) * a.n[0] + (t.n0[0] + n.l[0]);
        unsigned *o = out + node * 16;
        const int fl = t.flag[nd] != 0;
        const unsigned long long k = t.key[nd];
        const int ax = (int)(k & 15u), ay = (int)((k >> 4) & 15u), az = (int)((k >> 8) & 15u); /* the argmin, 0 .. 2r */
        if (slot < 6) {
            unsigned c = 0;
            if (!fl) {
                int s[3] = {ax, ay, az};
                s[slot >> 1] += (slot & 1) ? 1 : -1;
                c = BM_NONE;
                if (s[0] >= 0 && s[0] < t.S && s[1] >= 0 && s[1] < t.S && s[2] >= 0 && s[2] < t.S)
                    c = COST(t, nd).template at<B>(n.f, n.w + s[2] * t.wxy + s[1] * t.wx + s[0], t);
            }
            o[6 + slot] = c;
        } else if (slot == 6) {
            o[0] = fl ? 0u : (unsigned)(ax - t.r);
            o[1] = fl ? 0u : (unsigned)(ay - t.r);
            o[2] = fl ? 0u : (unsigned)(az - t.r);
            o[3] = (unsigned)fl;
            o[4] = fl ? 0u : (unsigned)(k >> 19);
            o[5] = fl ? 0u : t.c0[nd];
        } else {
            o[12] = fl ? 0u : t.sf[nd];
            o[13] = fl ? 0u : t.sf2[nd];
            o[14] = 0u;
            o[15] = 0u;
        }
    }
}

/* The search of one brick under COST.  B, R > 0: b, r at compile time and pass 2 with the rows in registers; B = R = 0: any b, r */
template <class COST, int B, int R, int P> __device__ __forceinline__ void bm_search(const short *__restrict__ qf, const short *__restrict__ qw, const bm_args &a, unsigned *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char bm_lds[];
    const bm_tiles t = bm_setup(a, B > 0 ? B : a.b, R > 0 ? R : a.r, bm_lds);
    const int S2 = t.S * t.S;

    bm_clear(t);
    bm_load_tile(qf, a, t.p0, t.b, t.fx, t.fy, t.fvol, t.tf);
    bm_load_tile(qw, a, t.p0, t.b + t.r, t.wx, t.wy, t.wvol, t.tw);
    __syncthreads();

    bm_pass1(a, t);
    __syncthreads();

    /* pass 2: the costs of every shift; the least key per node */
    for (int it = threadIdx.x; it < t.NN * S2; it += BM_THREADS) {
        const int nd = it / S2, rem = it - nd * S2, sz = rem / t.S, sy = rem - sz * t.S; /* sz, sy in 0 .. 2r */
        const bm_node n = bm_local(a, t, nd);
        if (!n.in || t.flag[nd]) continue;
        const short *w = n.w + sz * t.wxy + sy * t.wx;
        const COST cost(t, nd);
        unsigned long long best = ~0ull;
        if constexpr (B > 0 && R > 0) {
            unsigned c[2 * R + 1];
            cost.template along_x<B, R, P>(n.f, w, t, c);
#pragma unroll
            for (int s = 0; s < 2 * R + 1; s++) best = bm_take(t, nd, best, c[s], s, sy, sz);
        } else {
            for (int s = 0; s < t.S; s++) best = bm_take(t, nd, best, cost.template at<0>(n.f, w + s, t), s, sy, sz);
        }
        atomicMin(&t.key[nd], best);
    }
    __syncthreads();

    bm_pass3<COST, B>(a, t, out);
}

template <int B, int R, int P> __global__ __launch_bounds__(BM_THREADS) void block_match_kernel(const short *__restrict__ qf, const short *__restrict__ qw, bm_args a, unsigned *__restrict__ out)
{
    bm_search<bm_ssd, B, R, P>(qf, qw, a, out);
}

template <int B, int R> __global__ __launch_bounds__(BM_THREADS) void block_match_ncc_kernel(const short *__restrict__ qf, const short *__restrict__ qw, bm_args a, unsigned *__restrict__ out)
{
    bm_search<bm_ncc, B, R, 1>(qf, qw, a, out);
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

typedef void (*bm_kernel)(const short *, const short *, bm_args, unsigned *);

/* qf, qw: the quantised volumes (nx ny nz int16, x fastest); first, stride, n: the lattice; out: 16 words per node.  The caller
 * has checked 1 <= b <= 6, 1 <= r <= 6, stride >= 1, the extents (each below 2^31 / 16) and n (each >= 1, product below 2^31). */
static hipError_t bm_launch(bm_kernel k, hipStream_t s, const short *qf, const short *qw, int64_t nx, int64_t ny, int64_t nz, const int64_t first[3],
                            int64_t stride, const int64_t n[3], int b, int r, unsigned *out)
{
    bm_args a;
    size_t lds;
    long long bricks;
    const hipError_t e = bm_plan(nx, ny, nz, first, stride, n, b, r, a, lds, bricks);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3((unsigned)bricks), dim3(BM_THREADS), lds, s, qf, qw, a, out);
    return hipGetLastError();
}

/* The search under the sum of squared differences.  generic: 0 the specialised form where there is one ((b, r) = (4, 3), (4, 4);
 * packed differences); 1 the form for any b, r; 2 the specialised form with one multiply-add per instruction (kept for the
 * measurement).  The tests compare all three. */
hipError_t sift3d_launch_block_match(hipStream_t s, const short *qf, const short *qw, int64_t nx, int64_t ny, int64_t nz, const int64_t first[3],
                                     int64_t stride, const int64_t n[3], int b, int r, int generic, unsigned *out)
{
    bm_kernel k = block_match_kernel<0, 0, 0>;
    if (generic == 0 && b == 4 && r == 3) k = block_match_kernel<4, 3, 1>;
    else if (generic == 0 && b == 4 && r == 4) k = block_match_kernel<4, 4, 1>;
    else if (generic == 2 && b == 4 && r == 3) k = block_match_kernel<4, 3, 0>;
    else if (generic == 2 && b == 4 && r == 4) k = block_match_kernel<4, 4, 0>;
    return bm_launch(k, s, qf, qw, nx, ny, nz, first, stride, n, b, r, out);
}

/* The same search under the correlation cost.  generic: 0 the register form where there is one ((b, r) = (4, 3), (4, 4)); any
 * other value the form for any b, r.  Same words from both. */
hipError_t sift3d_launch_block_match_ncc(hipStream_t s, const short *qf, const short *qw, int64_t nx, int64_t ny, int64_t nz, const int64_t first[3],
                                         int64_t stride, const int64_t n[3], int b, int r, int generic, unsigned *out)
{
    bm_kernel k = block_match_ncc_kernel<0, 0>;
    if (generic == 0 && b == 4 && r == 3) k = block_match_ncc_kernel<4, 3>;
    else if (generic == 0 && b == 4 && r == 4) k = block_match_ncc_kernel<4, 4>;
    return bm_launch(k, s, qf, qw, nx, ny, nz, first, stride, n, b, r, out);
}
