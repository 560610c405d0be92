/*
 * kernels_fuse.hip -- the hot path of multi-atlas label fusion for gfx950 (MI355X; tests/fuse_oracle.c
 * restates it as a serial brute force).  fuse_weight_kernel<B, METRIC> gives every target voxel its similarity u (0 .. 32768) to
 * one warped atlas from the integer sums over the voxel's clipped patch (patch_sums.h; what they are worth: patch_cost.h);
 * fuse_label_kernel turns the warped float labels into a uint16 plane and marks the voxels where the atlas does not vote;
 * fuse_vote_kernel votes over the K planes.  Everything is integer arithmetic but patch_cost.h's one sequence of double
 * operations, so no result depends on the tiling, the order of the additions or the wave layout.
 *
 * fuse_weight_kernel.  A workgroup of 256 threads owns warp_device.h's brick of 32 x 8 x 4 target voxels (a thread four
 * consecutive x voxels, the bricks dealt over the XCDs) and stages the brick plus a halo of b of qT and qW in LDS, one dword per
 * voxel: the two int16 values side by side and the joint validity in bit 31.  A voxel outside the volume, or with q = -1 in
 * either volume, is staged as 0: it adds nothing to any sum, so a clipped or holed patch needs no test in the loops, and all
 * sums are plain box sums.
 *   B > 0 (b at compile time; instantiated for 2), the sliding form: per row (dz, dy) of the patch a thread reads the 4 + 2b
 *   dwords under its four windows once and adds each column's terms to that column's sums; after the (2b + 1)^2 rows the column
 *   sums slide into the four windows.  (4 + 2b) / 4 column updates per voxel and row instead of 2b + 1.
 *   B = 0 (any b <= 6): every patch voxel straight from the tile, per output voxel.  The column sums of the sliding form would be
 *   arrays indexed by a run-time b, which the compiler keeps in scratch.
 *
 * fuse_vote_kernel.  One voxel per lane.  The lane copies its K (label, u) pairs into its own column of LDS (dword k * 256 + lane:
 * lanes on consecutive banks, and no lane reads another's, so no barrier), then walks them in atlas order: for the first voter of
 * each label it adds up that label's weights over the later voters.  K is a run-time count up to 32: in registers the pairs would
 * be an array under a run-time index (scratch), and re-reading global memory costs K^2 / 2 loads per voxel.
 */
#include "sift3d_internal.h"
#include "label_plane.h"
#include "patch_sums.h"

#define FUSE_THREADS 256
#define FUSE_U_NONE 0xffffu  /* in a u plane: the atlas does not vote here */
#define FUSE_VALID 0x80000000u
#define FUSE_BIT_FALLBACK (1u << 30)
#define FUSE_BIT_NONE (1u << 31)

template <int B, int NCC>
__global__ __launch_bounds__(FUSE_THREADS) void fuse_weight_kernel(const short *__restrict__ qt, const short *__restrict__ qw, long long nx, long long ny,
                                                                   long long nz, int b_any, unsigned short *__restrict__ u, long long nbx, long long nby,
                                                                   long long nbricks)
{
    extern __shared__ __attribute__((aligned(16))) unsigned fuse_tile[];
    const int b = B > 0 ? B : b_any, side = 2 * b + 1;
    const int ex = BRICK_BX + 2 * b, ey = BRICK_BY + 2 * b, ez = BRICK_BZ + 2 * b, exy = ex * ey, vol = exy * ez;
    int tx, ty, tz;
    brick_lane(tx, ty, tz);
    for (long long L = brick_slot0(); L < nbricks; L += gridDim.x) {
        long long x0, y0, z0;
        brick_origin(L, nbx, nby, x0, y0, z0);
        __syncthreads(); /* the tile of the brick before is no longer read */
        for (int i = threadIdx.x; i < vol; i += FUSE_THREADS) {
            const int x = i % ex, t = i / ex, y = t % ey, z = t / ey;
            const long long gx = x0 - b + x, gy = y0 - b + y, gz = z0 - b + z;
            unsigned v = 0;
            if (gx >= 0 && gx < nx && gy >= 0 && gy < ny && gz >= 0 && gz < nz) {
                const long long at = (gz * ny + gy) * nx + gx;
                const int f = qt[at], w = qw[at];
                if (f >= 0 && w >= 0) v = FUSE_VALID | ((unsigned)w << 16) | (unsigned)f;
            }
            fuse_tile[i] = v;
        }
        __syncthreads();
        const long long i0 = x0 + tx * BRICK_VX, j = y0 + ty, k = z0 + tz;
        if (j >= ny || k >= nz || i0 >= nx) continue; /* no barrier below this line */
        const unsigned *row0 = fuse_tile + tz * exy + ty * ex + tx * BRICK_VX; /* the patch's first voxel of output voxel 0 */
        patch_sums out[BRICK_VX];
        if constexpr (B > 0) {
            constexpr int COLS = BRICK_VX + 2 * B;
            patch_sums col[COLS];
#pragma unroll
            for (int c = 0; c < COLS; c++) col[c] = patch_sums{0, 0, 0, 0, 0, 0, 0};
#pragma unroll 1
            for (int dz = 0; dz < 2 * B + 1; dz++)
#pragma unroll 1
                for (int dy = 0; dy < 2 * B + 1; dy++) {
                    const unsigned *r = row0 + dz * exy + dy * ex;
                    unsigned x[COLS];
#pragma unroll
                    for (int c = 0; c < COLS; c++) x[c] = r[c];
#pragma unroll
                    for (int c = 0; c < COLS; c++) ps_add_packed<NCC>(col[c], x[c]);
                }
            ps_slide<B, NCC>(col, out);
        } else {
#pragma unroll
            for (int v = 0; v < BRICK_VX; v++) {
                patch_sums s = patch_sums{0, 0, 0, 0, 0, 0, 0};
#pragma unroll 1
                for (int dz = 0; dz < side; dz++)
#pragma unroll 1
                    for (int dy = 0; dy < side; dy++) {
                        const unsigned *r = row0 + dz * exy + dy * ex + v;
                        for (int dx = 0; dx < side; dx++) ps_add_packed<NCC>(s, r[dx]);
                    }
                out[v] = s;
            }
        }
        unsigned short *dst = u + (k * ny + j) * nx + i0;
#pragma unroll
        for (int v = 0; v < BRICK_VX; v++)
            if (i0 + v < nx) dst[v] = (unsigned short)ps_u<NCC>(out[v]);
    }
}

/* Warped float labels (finite: an integer 0 .. 65535, which the host has checked on the atlas; nearest-neighbour warping picks
 * atlas values or the NaN fill) to the uint16 plane.  Where the label is not finite the atlas does not vote: its u becomes
 * FUSE_U_NONE.  clear_u: there was no weight kernel (power 0, or an empty range), the voters' u becomes 0. */
__global__ __launch_bounds__(FUSE_THREADS) void fuse_label_kernel(const float *__restrict__ labels, long long n, int clear_u, unsigned short *__restrict__ lab,
                                                                  unsigned short *__restrict__ u)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = labels[i];
    if (isfinite(v)) {
        lab[i] = (unsigned short)label_bits(v);
        if (clear_u) u[i] = 0;
    } else {
        lab[i] = 0;
        u[i] = (unsigned short)FUSE_U_NONE;
    }
}

__device__ __forceinline__ unsigned long long fuse_weight_of(unsigned u, int power)
{
    return power == 0 ? 1ull : (power == 1 ? (unsigned long long)u : (unsigned long long)(u * u));
}

/* u, lab: K planes of n values each, plane k at k * n.  words: two per voxel. */
__global__ __launch_bounds__(FUSE_THREADS) void fuse_vote_kernel(const unsigned short *__restrict__ u, const unsigned short *__restrict__ lab, int K, long long n,
                                                                 int power, unsigned *__restrict__ words)
{
    extern __shared__ __attribute__((aligned(16))) unsigned fuse_pairs[]; /* K x 256 dwords: label | u << 16 */
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return; /* no barrier in this kernel */
    unsigned *mine = fuse_pairs + threadIdx.x;
    unsigned voters = 0, any = 0;
    for (int k = 0; k < K; k++) {
        const unsigned uk = u[(long long)k * n + i], lk = lab[(long long)k * n + i];
        mine[k * FUSE_THREADS] = lk | (uk << 16);
        if (uk != FUSE_U_NONE) {
            voters++;
            any |= uk;
        }
    }
    unsigned w0 = 0, w1 = 0;
    if (voters == 0) {
        w0 = FUSE_BIT_NONE;
    } else {
        int pw = power;
        if (power > 0 && any == 0) { /* every voter's weight is 0: every voter weighs 1 */
            pw = 0;
            w0 = FUSE_BIT_FALLBACK;
        }
        unsigned long long best = 0, total = 0;
        unsigned best_l = 0;
        for (int k = 0; k < K; k++) {
            const unsigned pk = mine[k * FUSE_THREADS], uk = pk >> 16, lk = pk & 0xffffu;
            if (uk == FUSE_U_NONE) continue;
            total += fuse_weight_of(uk, pw);
            bool first = true;
            for (int j = 0; j < k; j++) {
                const unsigned pj = mine[j * FUSE_THREADS];
                if ((pj >> 16) != FUSE_U_NONE && (pj & 0xffffu) == lk) first = false;
            }
            if (!first) continue;
            unsigned long long S = 0;
            for (int j = k; j < K; j++) {
                const unsigned pj = mine[j * FUSE_THREADS];
                if ((pj >> 16) != FUSE_U_NONE && (pj & 0xffffu) == lk) S += fuse_weight_of(pj >> 16, pw);
            }
            if (S > best || (S == best && lk < best_l)) { /* S >= 1 for a voter unless every weight is 0, which pw = 0 has replaced */
                best = S;
                best_l = lk;
            }
        }
        w0 |= best_l | (voters << 16);
        w1 = (unsigned)((best * 65535ull) / total);
    }
    words[2 * i] = w0;
    words[2 * i + 1] = w1;
}

/* qt, qw: the quantised target and warped atlas (nx ny nz int16, x fastest); u: one uint16 per voxel.  generic: 0 the form with b at
 * compile time where there is one (b = 2), anything else the form for any b.  The caller has checked 1 <= b <= 6 and the extents. */
hipError_t sift3d_launch_fuse_weight(hipStream_t s, const short *qt, const short *qw, int64_t nx, int64_t ny, int64_t nz, int b, int ncc, int generic,
                                     unsigned short *u)
{
    const brick_launch bl = brick_launch_of(nullptr, nx, ny, nz);
    const size_t lds = sizeof(unsigned) * (size_t)(BRICK_BX + 2 * b) * (BRICK_BY + 2 * b) * (BRICK_BZ + 2 * b);
    if (b < 1 || b > 6 || lds > 65536) return hipErrorInvalidValue;
    auto k = ncc ? fuse_weight_kernel<0, 1> : fuse_weight_kernel<0, 0>;
    if (generic == 0 && b == 2) k = ncc ? fuse_weight_kernel<2, 1> : fuse_weight_kernel<2, 0>;
    hipLaunchKernelGGL(k, dim3(bl.grid), dim3(FUSE_THREADS), lds, s, qt, qw, (long long)nx, (long long)ny, (long long)nz, b, u, bl.nbx, bl.nby,
                       bl.nbricks);
    return hipGetLastError();
}

hipError_t sift3d_launch_fuse_label(hipStream_t s, const float *labels, int64_t n, int clear_u, unsigned short *lab, unsigned short *u)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(fuse_label_kernel, dim3((unsigned)((n + FUSE_THREADS - 1) / FUSE_THREADS)), dim3(FUSE_THREADS), 0, s, labels, (long long)n, clear_u,
                       lab, u);
    return hipGetLastError();
}

/* the caller has checked 1 <= K <= 32, 0 <= power <= 2 and n below 2^31 * 256 */
hipError_t sift3d_launch_fuse_vote(hipStream_t s, const unsigned short *u, const unsigned short *lab, int K, int64_t n, int power, unsigned *words)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(fuse_vote_kernel, dim3((unsigned)((n + FUSE_THREADS - 1) / FUSE_THREADS)), dim3(FUSE_THREADS), sizeof(unsigned) * FUSE_THREADS * (size_t)K,
                       s, u, lab, K, (long long)n, power, words);
    return hipGetLastError();
}
