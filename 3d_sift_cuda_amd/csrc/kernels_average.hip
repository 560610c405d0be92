/*
 * kernels_average.hip -- the mean, the trimmed mean or median, the variance and the contributor mask of up to 32 warped images on
 * one output grid, in ONE launch for gfx950 (MI355X; tests/average_oracle.c restates it serially).  No warped
 * volume is written or read back: every image is sampled where the output voxel needs it.
 *
 * average_kernel<VOX>.  A workgroup of AVG_THREADS = 256 owns warp_device.h's brick of 32 x 8 x 4 output voxels, the bricks dealt over
 * the XCDs as brick_slot0 deals them, at most AVG_MAX_BLOCKS workgroups in a grid loop.  A thread owns four consecutive x voxels of
 * one row and serves them in groups of VOX: it walks the K images in image order once per group and samples the group's voxels side
 * by side, VOX independent chains of gathers in flight.  VOX is 4 up to AVG_GROUP4_MAX = 8 images, 2 up to AVG_GROUP2_MAX = 16 and 1
 * beyond, so that the workgroup's columns stay within 32 KB of LDS: it admits five workgroups per CU, the registers four (measured:
 * DESIGN.md section 7r).
 * The descriptor of image k (source pointer, extents, the 12-float map, the field's terms, nodes and grid) is read from one device
 * array under a uniform index, so its loads are scalar and the field-or-affine branch is uniform per image; q = warp_position<field>,
 * v = sample_volume<WARP_LINEAR> with fill NaN: kernels_field.hip's and kernels_resample.hip's arithmetic, from the same header.
 * A voxel's K samples sit in its lane's own LDS column (dword (k VOX + u) * 256 + lane: consecutive lanes on consecutive banks; no lane reads
 * another's column, so there is no barrier in the kernel).  K is a run-time count: in registers the samples would be an array under
 * a run-time index, which the compiler keeps in scratch.
 *   pass 1  sample, store, mask |= 1 << k and S = S + (double)v for the finite ones, from S = +0
 *   pass 2  m = S / (double)n; V = V + ((double)v - m)^2 over the contributors in image order, from the column
 *   trim > 0  the contributors are insertion-sorted in place in the column: walking k upwards, sample k moves down past the
 *           larger ones only (strictly: equal values keep their image order, -0 == 0), so position r holds the contributor of rank
 *           r as section 7r defines it.  Slot cnt <= k is written after sample k has been read, so nothing unread is overwritten.
 *           About K^2 / 4 LDS reads and as many writes for random values, none for sorted ones; no rank array, hence no scratch.
 *           Then the sum over the positions t_eff .. n - 1 - t_eff in order.
 * Every floating-point step is one IEEE double operation in the stated order: -ffp-contract=off and no -fno-honor-nans (Makefile).
 * Outputs: avg and var (float), mask (uint32), four voxels per store where the rows allow it.
 */
#include "sift3d_internal.h"
#include "warp_device.h"

#define AVG_THREADS 256
#define AVG_MAX_BLOCKS 1024 /* workgroups of a launch: the kernel goes round a grid loop beyond it */
#define AVG_MAX_IMAGES 32
#define AVG_GROUP4_MAX 8    /* up to this many images a thread walks them once for all four of its voxels */
#define AVG_GROUP2_MAX 16   /* up to this many, once per two voxels; beyond, once per voxel */

static_assert(AVG_THREADS == BRICK_TX * BRICK_BY * BRICK_BZ, "a workgroup is one brick of output voxels");
static_assert(AVG_MAX_BLOCKS % 8 == 0, "the brick slots are dealt over eight XCDs");
static_assert(AVG_MAX_IMAGES == SIFT3D_AVERAGE_MAX_IMAGES, "include/sift3d.h states the cap");

/* one image of a launch, as the kernel reads it: average_api.hip fills the array */
struct avg_image {
    const float *src;
    const float4 *nodes; /* NULL without a field */
    long long nx, ny, nz;
    warp_map m;
};

/* One voxel's results from its column (K samples, `stride` dwords apart): avg and var, which the caller has set to fill.  bits, n and S
 * are pass 1's. */
__device__ __forceinline__ void average_voxel(float *col, int stride, int K, unsigned bits, int n, double S, int trim, int min_count, float &avg, float &var)
{
    if (n < min_count) return; /* min_count >= 1: n = 0 ends here */
    const double m = S / (double)n;
    double V = 0.0;
#pragma unroll 1
    for (int k = 0; k < K; k++)
        if ((bits >> k) & 1u) {
            const double d = (double)col[k * stride] - m;
            V = V + d * d;
        }
    var = n > 1 ? (float)(V / (double)(n - 1)) : 0.0f;
    if (trim == 0) {
        avg = (float)m;
        return;
    }
    int cnt = 0;
#pragma unroll 1
    for (int k = 0; k < K; k++) {
        if (!((bits >> k) & 1u)) continue;
        const float s = col[k * stride];
        int at = cnt;
        while (at > 0) {
            const float below = col[(at - 1) * stride];
            if (!(below > s)) break;
            col[at * stride] = below;
            at--;
        }
        col[at * stride] = s;
        cnt++;
    }
    const int half = (n - 1) / 2, t = trim < half ? trim : half;
    double T = 0.0;
#pragma unroll 1
    for (int r = t; r <= n - 1 - t; r++) T = T + (double)col[r * stride];
    avg = (float)(T / (double)(n - 2 * t));
}

template <int VOX>
__global__ __launch_bounds__(AVG_THREADS) void average_kernel(const avg_image *__restrict__ images, int K, int trim, int min_count, float fill, long long ox,
                                                              long long oy, long long oz, float *__restrict__ avg, float *__restrict__ var,
                                                              unsigned *__restrict__ mask, long long nbx, long long nby, long long nbricks, int vec)
{
    static_assert(VOX == 1 || VOX == 2 || VOX == BRICK_VX, "a thread's four voxels in groups of VOX");
    extern __shared__ __attribute__((aligned(16))) float avg_column[]; /* K x VOX x 256 dwords */
    constexpr int STRIDE = VOX * AVG_THREADS;
    float *mine = avg_column + threadIdx.x;
    const float nanf_ = __builtin_nanf(""), inf = __builtin_inff();
    int tx, ty, tz;
    brick_lane(tx, ty, tz);
    for (long long L = brick_slot0(); L < nbricks; L += gridDim.x) {
        long long i0, j, kz;
        brick_voxel(L, nbx, nby, tx, ty, tz, i0, j, kz);
        if (j >= oy || kz >= oz || i0 >= ox) continue; /* no barrier in this kernel */
        const float py = (float)j, pz = (float)kz;
        float ra[BRICK_VX], rv[BRICK_VX], rm[BRICK_VX];
#pragma unroll /* fully: ra, rv and rm stay in registers */
        for (int v0 = 0; v0 < BRICK_VX; v0 += VOX) {
            unsigned bits[VOX];
            int n[VOX];
            double S[VOX];
#pragma unroll
            for (int u = 0; u < VOX; u++) {
                bits[u] = 0;
                n[u] = 0;
                S[u] = 0.0;
            }
#pragma unroll 1
            for (int k = 0; k < K; k++) {
                const avg_image &im = images[k];
                const float hx = (float)(im.nx - 1), hy = (float)(im.ny - 1), hz = (float)(im.nz - 1);
                float s[VOX];
                /* a voxel past the row's end is sampled too (the sampler reads inside its source or not at all) and never stored */
                if (im.m.has_field) {
#pragma unroll
                    for (int u = 0; u < VOX; u++) {
                        float q[3];
                        warp_position<1>(im.m, im.nodes, (float)(i0 + v0 + u), py, pz, q);
                        s[u] = sample_volume<WARP_LINEAR>(im.src, im.nx, im.ny, im.nz, hx, hy, hz, q[0], q[1], q[2], nanf_);
                    }
                } else {
#pragma unroll
                    for (int u = 0; u < VOX; u++) {
                        float q[3];
                        warp_position<0>(im.m, nullptr, (float)(i0 + v0 + u), py, pz, q);
                        s[u] = sample_volume<WARP_LINEAR>(im.src, im.nx, im.ny, im.nz, hx, hy, hz, q[0], q[1], q[2], nanf_);
                    }
                }
#pragma unroll
                for (int u = 0; u < VOX; u++) {
                    mine[(k * VOX + u) * AVG_THREADS] = s[u];
                    if (fabsf(s[u]) < inf) {
                        bits[u] |= 1u << k;
                        n[u]++;
                        S[u] = S[u] + (double)s[u];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < VOX; u++) {
                ra[v0 + u] = rv[v0 + u] = fill;
                rm[v0 + u] = __uint_as_float(bits[u]);
                average_voxel(mine + u * AVG_THREADS, STRIDE, K, bits[u], n[u], S[u], trim, min_count, ra[v0 + u], rv[v0 + u]);
            }
        }
        const long long at = (kz * oy + j) * ox + i0;
        store_row4(avg + at, ox, i0, ra, vec);
        store_row4(var + at, ox, i0, rv, vec);
        store_row4(reinterpret_cast<float *>(mask) + at, ox, i0, rm, vec);
    }
}

/* the voxels of a thread that share one walk over the images: as many as keep the workgroup's columns within 32 KB */
int sift3d_average_group(int K) { return K <= AVG_GROUP4_MAX ? 4 : (K <= AVG_GROUP2_MAX ? 2 : 1); }

/* images: K descriptors on the device (struct avg_image, which sift3d_average_fill_image fills on the host); avg, var, mask: ox oy oz
 * values each.  The caller has checked 1 <= K <= 32, 0 <= trim <= 15, 1 <= min_count <= K and the extents. */
hipError_t sift3d_launch_average(hipStream_t s, const void *images, int K, int trim, int min_count, float fill, int64_t ox, int64_t oy, int64_t oz,
                                 float *avg, float *var, unsigned *mask)
{
    if (K < 1 || K > AVG_MAX_IMAGES || trim < 0 || trim > SIFT3D_AVERAGE_MAX_TRIM || min_count < 1 || min_count > K || ox < 1 || oy < 1 || oz < 1)
        return hipErrorInvalidValue;
    brick_launch b = brick_launch_of(avg, ox, oy, oz);
    if (b.grid > AVG_MAX_BLOCKS) b.grid = AVG_MAX_BLOCKS;
    b.vec = b.vec && ((uintptr_t)var % 16) == 0 && ((uintptr_t)mask % 16) == 0;
    const int vox = sift3d_average_group(K);
    auto kernel = vox == 4 ? average_kernel<4> : (vox == 2 ? average_kernel<2> : average_kernel<1>);
    hipLaunchKernelGGL(kernel, dim3(b.grid), dim3(AVG_THREADS), sizeof(float) * AVG_THREADS * (size_t)K * (size_t)vox, s,
                       reinterpret_cast<const avg_image *>(images), K, trim, min_count, fill, (long long)ox, (long long)oy, (long long)oz, avg, var, mask, b.nbx,
                       b.nby, b.nbricks, b.vec);
    return hipGetLastError();
}

size_t sift3d_average_image_bytes(void) { return sizeof(avg_image); }

/* the descriptor at host address `at` (sift3d_average_image_bytes() bytes): a source volume on the device, its map and, with
 * has_field, the field's terms and grid with its nodes on the device */
void sift3d_average_fill_image(void *at, const float *d_src, int64_t nx, int64_t ny, int64_t nz, const float *map, const float *c, const float *k, bool has_field,
                               const float o[3], float h, const int64_t n[3], const float4 *d_nodes)
{
    avg_image *im = static_cast<avg_image *>(at);
    im->src = d_src;
    im->nodes = has_field ? d_nodes : nullptr;
    im->nx = nx;
    im->ny = ny;
    im->nz = nz;
    fill_warp_map(im->m, map, c, k, has_field, o, h, n);
}
