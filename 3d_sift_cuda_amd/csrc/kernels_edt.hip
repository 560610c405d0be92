/*
 * kernels_edt.hip -- the exact Euclidean distance map and the surface kernels for gfx950 (MI355X; DESIGN.md section 7l;
 * tests/edt_oracle.c restates them as a serial brute force).  Everything is integer arithmetic and every result a minimum, a
 * count or a flag, so nothing depends on the tiling, the pass order or the wave layout.
 *
 * edt_surface_kernel    one launch per label: the surface flags of the label in both volumes and their two counts, from the two
 *                       label planes (kernels_label.hip's label_plane_kernel, once per volume).
 * edt_x_kernel          a wave per row: the row's site flags become a bit mask in LDS (one ballot per 64 voxels), every word
 *                       learns the nearest site in the words before and after it, and a voxel finds its nearest site to either
 *                       side with one count-leading-zeros and one find-first-set.  uint16 |dx|, EDT_DX_NONE for a row without a
 *                       site.
 * edt_line_kernel       the y and the z pass: the minimum along a line of (value at the candidate) + (s d)^2.  A workgroup owns 64
 *                       consecutive x of one line position of the other axis, so every global load and store is one row of 64
 *                       lanes; wave w holds the outputs j0 + w + 4k (k < 16) of its lane's line in registers while the line's
 *                       candidates pass through LDS in chunks of EDT_CHUNK, each read once for the sixteen outputs: a candidate
 *                       costs a 64-bit multiply-add and a 64-bit compare-select per output.  A candidate without a value is
 *                       staged as 2^62: above every distance (< 2^58), and 2^62 + (s d)^2 does not wrap, so the loop has no
 *                       test.  FIRST: the input is edt_x_kernel's uint16 plane and the staged value (sx dx)^2.
 * edt_gather_kernel     the map's value at every flagged voxel into a compact list, in the order the atomics fall.
 */
#include <algorithm>

#include "sift3d_internal.h"
#include "label_plane.h"

#define EDT_THREADS 256
#define EDT_TX 64    /* lanes along x of a line tile: one wave */
#define EDT_TY 4     /* waves of a workgroup */
#define EDT_CHUNK 64 /* candidates of a line staged at a time: 64 x 64 x 8 bytes = 32 KiB */
#define EDT_OPT 16   /* outputs a thread holds per sweep over the line's candidates */
#define EDT_OUTS (EDT_TY * EDT_OPT)
#define EDT_BIG (1ull << 62)
#define EDT_NONE 0xffffffffffffffffull
#define EDT_DX_NONE 0xffffu
#define EDT_MAX_WORDS 64 /* 4096 voxels of a row / 64 */

__device__ __forceinline__ bool edt_carries(const unsigned short *lab, const unsigned long long *valid, long long i, unsigned l)
{
    return lab[i] == l && label_valid(valid, i);
}

/* counts[0], counts[1]: the surface voxels of l in A and in B (the caller has zeroed them) */
__global__ __launch_bounds__(EDT_THREADS) void edt_surface_kernel(const unsigned short *__restrict__ lab_a, const unsigned long long *__restrict__ valid_a,
                                                                  const unsigned short *__restrict__ lab_b, const unsigned long long *__restrict__ valid_b,
                                                                  long long nx, long long ny, long long nz, unsigned l, unsigned char *__restrict__ sites_a,
                                                                  unsigned char *__restrict__ sites_b, unsigned *__restrict__ counts)
{
    const long long n = nx * ny * nz, i = (long long)blockIdx.x * EDT_THREADS + threadIdx.x;
    const bool in = i < n;
    const long long x = i % nx, y = i / nx % ny, z = i / (nx * ny), sy = nx, sz = nx * ny;
    for (int v = 0; v < 2; v++) {
        const unsigned short *lab = v ? lab_b : lab_a;
        const unsigned long long *valid = v ? valid_b : valid_a;
        bool s = false;
        if (in && edt_carries(lab, valid, i, l))
            s = x == 0 || x == nx - 1 || y == 0 || y == ny - 1 || z == 0 || z == nz - 1 || !edt_carries(lab, valid, i - 1, l) ||
                !edt_carries(lab, valid, i + 1, l) || !edt_carries(lab, valid, i - sy, l) || !edt_carries(lab, valid, i + sy, l) ||
                !edt_carries(lab, valid, i - sz, l) || !edt_carries(lab, valid, i + sz, l);
        if (in) (v ? sites_b : sites_a)[i] = s ? 1 : 0;
        const unsigned long long m = __ballot(s);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(&counts[v], (unsigned)__popcll(m));
    }
}

__global__ __launch_bounds__(EDT_THREADS) void edt_x_kernel(const unsigned char *__restrict__ sites, long long nx, long long nrows,
                                                            unsigned short *__restrict__ dx)
{
    __shared__ unsigned long long mask[EDT_TY][EDT_MAX_WORDS];
    __shared__ int before[EDT_TY][EDT_MAX_WORDS], after[EDT_TY][EDT_MAX_WORDS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int words = (int)((nx + 63) >> 6);
    for (long long base = (long long)blockIdx.x * EDT_TY; base < nrows; base += (long long)gridDim.x * EDT_TY) {
        const long long row = base + w;
        const bool live = row < nrows;
        __syncthreads(); /* the masks of the rows before are no longer read */
        for (int c = 0; c < words; c++) {
            const long long x = (long long)c * 64 + lane;
            const bool s = live && x < nx && sites[row * nx + x] != 0;
            const unsigned long long m = __ballot(s);
            if (lane == 0) mask[w][c] = m;
        }
        __syncthreads();
        if (lane < words) { /* the nearest site in the words before this one and in those after it, -1 for none */
            int p = -1, q = -1;
            for (int c = lane - 1; c >= 0 && p < 0; c--)
                if (mask[w][c]) p = c * 64 + 63 - __clzll((long long)mask[w][c]);
            for (int c = lane + 1; c < words && q < 0; c++)
                if (mask[w][c]) q = c * 64 + __ffsll((unsigned long long)mask[w][c]) - 1;
            before[w][lane] = p;
            after[w][lane] = q;
        }
        __syncthreads();
        if (!live) continue; /* the barriers are at the top of the loop, which every wave runs equally often */
        for (int c = 0; c < words; c++) {
            const int x = c * 64 + lane;
            if (x >= nx) break;
            const unsigned long long m = mask[w][c];
            const unsigned long long lo = m & (~0ull >> (63 - lane)), hi = m & (~0ull << lane);
            const int left = lo ? c * 64 + 63 - __clzll((long long)lo) : before[w][c];
            const int right = hi ? c * 64 + __ffsll(hi) - 1 : after[w][c];
            unsigned d = EDT_DX_NONE;
            if (left >= 0) d = (unsigned)(x - left);
            if (right >= 0) d = min(d, (unsigned)(right - x));
            dx[row * nx + x] = (unsigned short)d;
        }
    }
}

/* in: FIRST the uint16 plane of edt_x_kernel, else the 64-bit plane of the pass before (EDT_NONE: no value).  The line runs over L
 * positions lstride elements apart; the other axis over nouter positions ostride apart; ntx tiles of 64 along x. */
template <int FIRST>
__global__ __launch_bounds__(EDT_THREADS) void edt_line_kernel(const void *__restrict__ in, unsigned long long *__restrict__ out, long long nx, long long L,
                                                               long long lstride, long long nouter, long long ostride, unsigned s_x, unsigned s, long long ntx)
{
    __shared__ __attribute__((aligned(16))) unsigned long long tile[EDT_CHUNK * EDT_TX];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const long long ntiles = ntx * nouter;
    const int step = (int)s * EDT_TY;
    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const long long x = t % ntx * EDT_TX + tx;
        const bool live = x < nx;
        const long long base = t / ntx * ostride + x;
        for (long long j0 = 0; j0 < L; j0 += EDT_OUTS) {
            unsigned long long best[EDT_OPT];
#pragma unroll
            for (int k = 0; k < EDT_OPT; k++) best[k] = EDT_BIG;
            for (long long c0 = 0; c0 < L; c0 += EDT_CHUNK) {
                const int cn = (int)min((long long)EDT_CHUNK, L - c0);
                __syncthreads(); /* the chunk before is no longer read */
                for (int i = ty; i < cn; i += EDT_TY) {
                    unsigned long long f = EDT_BIG;
                    if (live) {
                        const long long at = base + (c0 + i) * lstride;
                        if (FIRST) {
                            const unsigned d = ((const unsigned short *)in)[at];
                            const unsigned long long g = (unsigned long long)d * s_x;
                            if (d != EDT_DX_NONE) f = g * g;
                        } else {
                            f = min(((const unsigned long long *)in)[at], EDT_BIG);
                        }
                    }
                    tile[i * EDT_TX + tx] = f;
                }
                __syncthreads();
                const int rel = (int)(j0 - c0) + ty; /* the thread's first output, counted from the chunk's first candidate */
                for (int i = 0; i < cn; i++) {
                    const unsigned long long f = tile[i * EDT_TX + tx];
                    const int t0 = (rel - i) * (int)s; /* |t| < 2^29: 4159 voxels of at most 65535 um */
#pragma unroll
                    for (int k = 0; k < EDT_OPT; k++) {
                        const long long d = t0 + k * step;
                        const unsigned long long v = f + (unsigned long long)(d * d);
                        best[k] = v < best[k] ? v : best[k];
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < EDT_OPT; k++) {
                const long long j = j0 + ty + k * EDT_TY;
                if (live && j < L) out[base + j * lstride] = best[k] >= EDT_BIG ? EDT_NONE : best[k];
            }
        }
    }
}

/* list[0 .. cap): d2 at the voxels flagged in `at`, cap of them by edt_surface_kernel's count; *cursor zeroed by the caller */
__global__ __launch_bounds__(EDT_THREADS) void edt_gather_kernel(const unsigned char *__restrict__ at, const unsigned long long *__restrict__ d2, long long n,
                                                                 unsigned cap, unsigned *__restrict__ cursor, unsigned long long *__restrict__ list)
{
    const long long i = (long long)blockIdx.x * EDT_THREADS + threadIdx.x;
    if (i >= n || !at[i]) return;
    const unsigned pos = atomicAdd(cursor, 1u);
    if (pos < cap) list[pos] = d2[i];
}

static unsigned edt_blocks(long long n) { return (unsigned)((n + EDT_THREADS - 1) / EDT_THREADS); }

/* the callers have checked the extents (1 .. 4096 each, at most 2^30 voxels) and the spacings (1 .. 65535) */
hipError_t sift3d_launch_edt_surface(hipStream_t s, const unsigned short *lab_a, const unsigned long long *valid_a, const unsigned short *lab_b,
                                     const unsigned long long *valid_b, int64_t nx, int64_t ny, int64_t nz, unsigned l, unsigned char *sites_a,
                                     unsigned char *sites_b, unsigned *counts)
{
    hipLaunchKernelGGL(edt_surface_kernel, dim3(edt_blocks(nx * ny * nz)), dim3(EDT_THREADS), 0, s, lab_a, valid_a, lab_b, valid_b, (long long)nx, (long long)ny,
                       (long long)nz, l, sites_a, sites_b, counts);
    return hipGetLastError();
}

hipError_t sift3d_launch_edt_x(hipStream_t s, const unsigned char *sites, int64_t nx, int64_t ny, int64_t nz, unsigned short *dx)
{
    if (nx > 64 * EDT_MAX_WORDS) return hipErrorInvalidValue;
    const long long nrows = ny * nz;
    const unsigned grid = (unsigned)std::min<long long>((nrows + EDT_TY - 1) / EDT_TY, 2048);
    hipLaunchKernelGGL(edt_x_kernel, dim3(grid), dim3(EDT_THREADS), 0, s, sites, (long long)nx, nrows, dx);
    return hipGetLastError();
}

/* axis 1: the y pass, dx (uint16) to out; axis 2: the z pass, in (uint64) to out */
hipError_t sift3d_launch_edt_line(hipStream_t s, int axis, const void *in, unsigned long long *out, int64_t nx, int64_t ny, int64_t nz, unsigned s_x,
                                  unsigned s_axis)
{
    const long long ntx = (nx + EDT_TX - 1) / EDT_TX;
    const long long nouter = axis == 1 ? nz : ny;
    const unsigned grid = (unsigned)std::min<long long>(ntx * nouter, 2048);
    if (axis == 1)
        hipLaunchKernelGGL(edt_line_kernel<1>, dim3(grid), dim3(EDT_THREADS), 0, s, in, out, (long long)nx, (long long)ny, (long long)nx, nouter,
                           (long long)(nx * ny), s_x, s_axis, ntx);
    else
        hipLaunchKernelGGL(edt_line_kernel<0>, dim3(grid), dim3(EDT_THREADS), 0, s, in, out, (long long)nx, (long long)nz, (long long)(nx * ny), nouter,
                           (long long)nx, s_x, s_axis, ntx);
    return hipGetLastError();
}

hipError_t sift3d_launch_edt_gather(hipStream_t s, const unsigned char *at, const unsigned long long *d2, int64_t n, unsigned cap, unsigned *cursor,
                                    unsigned long long *list)
{
    hipLaunchKernelGGL(edt_gather_kernel, dim3(edt_blocks(n)), dim3(EDT_THREADS), 0, s, at, d2, (long long)n, cap, cursor, list);
    return hipGetLastError();
}
