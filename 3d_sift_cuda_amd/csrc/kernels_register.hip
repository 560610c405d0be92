/*
 * kernels_register.hip -- the joint histograms of a fixed image and a moving image under K candidate maps for gfx950 (MI355X;
 * DESIGN.md section 7q; tests/register_oracle.c restates them serially).  No warped volume is written.  Everything is counts and
 * integer sums, so nothing depends on the tiling, the launch order or the order the atomics arrive in.
 *
 * reg_plane_kernel      F on the lattice of a stride, quantised (quantize.h) into an int16 plane that is contiguous at any stride:
 *                       one lattice point per thread and trip, at most REG_PLANE_MAX_BLOCKS workgroups in a grid loop.
 * warp_hist_kernel<PLANE>  one workgroup of REG_THREADS serves ONE map and walks warp_device.h's bricks of 32 x 8 x 4 LATTICE points
 *                       in a grid loop: G = min(REG_MAX_BLOCKS, the bricks rounded up to 8) workgroups per map, K G in the launch.
 *                       A thread takes four consecutive lattice points of one row: q = warp_position<0>, v = sample_volume<
 *                       WARP_LINEAR> with fill NaN, qB = quantize(v); qA from the plane (PLANE) or quantize(F[p]).
 *                       Histogram: bins^2 uint32 in LDS with LDS atomic adds; a thread merges its consecutive points of one cell
 *                       in registers first.  A workgroup counts at most 2^30 points, so a word cannot wrap.
 *                       The six sums and `outside`: 64-bit registers per thread over the whole loop, reduced across the wave, one
 *                       LDS add per wave and word.
 *                       Flush: 64-bit global atomic adds of the non-zero words into the map's result, which the call zeroed.
 *                       Order (placement, for speed only): by brick -- the launch deals block b to XCD b % 8; there block b / 8
 *                       serves map (b / 8) % K of brick slot (b / 8) / K, so the K maps of one brick run on one XCD side by side
 *                       and their nearly identical gather footprints share its L2 -- or by map: map b / G.  Either way the G slots
 *                       of a map are dealt so that each XCD walks one contiguous run of bricks, as brick_slot0 does.
 * Result words per map (uint64): bins^2 cells, the six sums, outside.
 */
#include "sift3d_internal.h"
#include "quantize.h"
#include "warp_device.h"

#define REG_THREADS 256
#define REG_MAX_BLOCKS 512         /* workgroups per map of a launch: the kernel goes round a grid loop beyond it */
#define REG_MAX_MAPS 32
#define REG_MAX_BINS 64
#define REG_WORDS 7                /* the six sums and outside */
#define REG_PLANE_MAX_BLOCKS 4096

static_assert(REG_THREADS == BRICK_TX * BRICK_BY * BRICK_BZ, "a workgroup is one brick of lattice points");
static_assert(REG_MAX_BLOCKS % 8 == 0, "the slots of a map are dealt over eight XCDs");
static_assert(REG_MAX_MAPS == SIFT3D_REGISTER_MAX_MAPS, "include/sift3d.h states the cap");

struct reg_map {
    float a[12];
};

__device__ __forceinline__ unsigned long long reg_wave_sum64(unsigned long long v)
{
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(REG_THREADS) void reg_plane_kernel(const float *__restrict__ f, long long nx, long long ny, long long lx, long long ly,
                                                                long long count, int stride, double lo, double hi, short *__restrict__ plane)
{
    for (long long i = (long long)blockIdx.x * REG_THREADS + threadIdx.x; i < count; i += (long long)gridDim.x * REG_THREADS) {
        const long long a = i % lx, t = i / lx, b = t % ly, c = t / ly;
        plane[i] = (short)quantize(f[((c * stride) * ny + b * stride) * nx + a * stride], lo, hi);
    }
}

template <bool PLANE>
__global__ __launch_bounds__(REG_THREADS) void warp_hist_kernel(const float *__restrict__ f, const short *__restrict__ plane, const float *__restrict__ mov,
                                                                const reg_map *__restrict__ maps, int n_maps, int per_map, int by_map, long long nx,
                                                                long long ny, long long lx, long long ly, long long lz, long long nbx, long long nby,
                                                                long long nbricks, int stride, long long mx, long long my, long long mz, double flo,
                                                                double fhi, double mlo, double mhi, int bins_log2, int words,
                                                                unsigned long long *__restrict__ res)
{
    __shared__ unsigned hist[REG_MAX_BINS * REG_MAX_BINS];
    __shared__ unsigned long long sums[REG_WORDS];
    /* the block's map and the first of its brick slots: scalar arithmetic */
    const unsigned b = blockIdx.x;
    int k;
    unsigned g;
    if (by_map) {
        k = (int)(b / (unsigned)per_map);
        g = b % (unsigned)per_map;
    } else {
        const unsigned i = b >> 3;
        k = (int)(i % (unsigned)n_maps);
        g = ((i / (unsigned)n_maps) << 3) | (b & 7u);
    }
    const long long slot0 = (long long)(g & 7u) * (per_map >> 3) + (g >> 3);
    if (slot0 >= nbricks) return; /* the whole workgroup: nothing to add */

    const int cells = 1 << (2 * bins_log2), shift = 10 - bins_log2;
    for (int t = threadIdx.x; t < cells; t += REG_THREADS) hist[t] = 0u;
    if (threadIdx.x < REG_WORDS) sums[threadIdx.x] = 0ull;
    __syncthreads();

    reg_map m;
#pragma unroll
    for (int r = 0; r < 12; r++) m.a[r] = maps[k].a[r];
    const float hx = (float)(mx - 1), hy = (float)(my - 1), hz = (float)(mz - 1);
    const float nanf_ = __builtin_nanf("");
    int tx, ty, tz;
    brick_lane(tx, ty, tz);
    unsigned long long s[REG_WORDS] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    for (long long L = slot0; L < nbricks; L += per_map) {
        long long i0, j, kz;
        brick_voxel(L, nbx, nby, tx, ty, tz, i0, j, kz);
        if (j >= ly || kz >= lz) continue;
        const long long frow = ((kz * stride) * ny + j * stride) * nx, prow = (kz * ly + j) * lx;
        const float py = (float)(j * stride), pz = (float)(kz * stride);
        int cell = -1;
        unsigned run = 0;
#pragma unroll
        for (int v = 0; v < BRICK_VX; v++) {
            const long long i = i0 + v;
            if (i >= lx) break;
            float q[3];
            warp_position<0>(m, nullptr, (float)(i * stride), py, pz, q);
            if (!(q[0] >= 0.0f && q[0] <= hx && q[1] >= 0.0f && q[1] <= hy && q[2] >= 0.0f && q[2] <= hz)) s[6] += 1ull;
            const float w = sample_volume<WARP_LINEAR>(mov, mx, my, mz, hx, hy, hz, q[0], q[1], q[2], nanf_);
            const int qb = quantize(w, mlo, mhi);
            const int qa = PLANE ? (int)plane[prow + i] : quantize(f[frow + i * stride], flo, fhi);
            if (qa < 0 || qb < 0) continue;
            const unsigned ua = (unsigned)qa, ub = (unsigned)qb;
            s[0] += 1ull;
            s[1] += ua;
            s[2] += ub;
            s[3] += ua * ua;
            s[4] += ub * ub;
            s[5] += ua * ub;
            const int c = (int)(((ua >> shift) << bins_log2) | (ub >> shift));
            if (c != cell) {
                if (run) atomicAdd(&hist[cell], run);
                cell = c;
                run = 0;
            }
            run++;
        }
        if (run) atomicAdd(&hist[cell], run);
    }
    for (int w = 0; w < REG_WORDS; w++) {
        const unsigned long long t = reg_wave_sum64(s[w]);
        if ((threadIdx.x & 63) == 0 && t) atomicAdd(&sums[w], t);
    }
    __syncthreads();
    unsigned long long *out = res + (long long)k * words;
    for (int t = threadIdx.x; t < cells; t += REG_THREADS)
        if (hist[t]) atomicAdd(&out[t], (unsigned long long)hist[t]);
    if (threadIdx.x < REG_WORDS && sums[threadIdx.x]) atomicAdd(&out[cells + threadIdx.x], sums[threadIdx.x]);
}

int sift3d_register_words(int bins) { return bins * bins + REG_WORDS; }

/* workgroups per map: the bricks of the lattice rounded up to a multiple of 8, at most REG_MAX_BLOCKS */
int sift3d_register_blocks(int64_t lx, int64_t ly, int64_t lz)
{
    const int64_t bricks = ((lx + BRICK_BX - 1) / BRICK_BX) * ((ly + BRICK_BY - 1) / BRICK_BY) * ((lz + BRICK_BZ - 1) / BRICK_BZ);
    const int64_t g = (bricks + 7) / 8 * 8;
    return (int)(g < REG_MAX_BLOCKS ? g : REG_MAX_BLOCKS);
}

/* F (nx x ny x .) on the lattice (lx, ly, lz) of the stride into plane (lx ly lz int16) */
hipError_t sift3d_launch_register_plane(hipStream_t s, const float *f, int64_t nx, int64_t ny, int64_t lx, int64_t ly, int64_t lz, int stride, double lo,
                                        double hi, short *plane)
{
    const int64_t count = lx * ly * lz, blocks = (count + REG_THREADS - 1) / REG_THREADS;
    if (count <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(reg_plane_kernel, dim3((unsigned)(blocks < REG_PLANE_MAX_BLOCKS ? blocks : REG_PLANE_MAX_BLOCKS)), dim3(REG_THREADS), 0, s, f,
                       (long long)nx, (long long)ny, (long long)lx, (long long)ly, (long long)count, stride, lo, hi, plane);
    return hipGetLastError();
}

/* maps: n_maps x 12 floats on the device; plane: the lattice plane, or NULL for F read per map; res: n_maps x
 * sift3d_register_words(bins) words, zeroed here */
hipError_t sift3d_launch_warp_hist(hipStream_t s, const float *f, const short *plane, const float *mov, const float *maps, int n_maps, int by_map,
                                   int64_t nx, int64_t ny, int64_t lx, int64_t ly, int64_t lz, int stride, int64_t mx, int64_t my, int64_t mz, double flo,
                                   double fhi, double mlo, double mhi, int bins, unsigned long long *res)
{
    int bins_log2 = 0;
    while ((1 << bins_log2) < bins) bins_log2++;
    if (n_maps < 1 || n_maps > REG_MAX_MAPS || (1 << bins_log2) != bins || bins < 8 || bins > REG_MAX_BINS || lx < 1 || ly < 1 || lz < 1)
        return hipErrorInvalidValue;
    const int words = sift3d_register_words(bins), per_map = sift3d_register_blocks(lx, ly, lz);
    const long long nbx = (lx + BRICK_BX - 1) / BRICK_BX, nby = (ly + BRICK_BY - 1) / BRICK_BY, nbricks = nbx * nby * ((lz + BRICK_BZ - 1) / BRICK_BZ);
    hipError_t rc = hipMemsetAsync(res, 0, sizeof(unsigned long long) * (size_t)words * (size_t)n_maps, s);
    if (rc != hipSuccess) return rc;
    const dim3 grid((unsigned)(per_map * n_maps));
    const reg_map *dm = reinterpret_cast<const reg_map *>(maps);
    if (plane)
        hipLaunchKernelGGL(warp_hist_kernel<true>, grid, dim3(REG_THREADS), 0, s, f, plane, mov, dm, n_maps, per_map, by_map, (long long)nx, (long long)ny,
                           (long long)lx, (long long)ly, (long long)lz, nbx, nby, nbricks, stride, (long long)mx, (long long)my, (long long)mz, flo, fhi, mlo,
                           mhi, bins_log2, words, res);
    else
        hipLaunchKernelGGL(warp_hist_kernel<false>, grid, dim3(REG_THREADS), 0, s, f, plane, mov, dm, n_maps, per_map, by_map, (long long)nx, (long long)ny,
                           (long long)lx, (long long)ly, (long long)lz, nbx, nby, nbricks, stride, (long long)mx, (long long)my, (long long)mz, flo, fhi, mlo,
                           mhi, bins_log2, words, res);
    return hipGetLastError();
}
