/*
 * kernels_normalize.hip -- the two launches of the intensity matching for gfx950 (MI355X; tests/normalize_oracle.c
 * restates them serially).  The first makes counts and integer sums only, so nothing depends on the tiling, the launch order or the
 * order the atomics arrive in; the second is one stated sequence of double operations per voxel.  No warped volume is written.
 *
 * overlap_hist_kernel<FIELD, MASK>.  A workgroup of NORM_THREADS = 256 walks warp_device.h's bricks of 32 x 8 x 4 REFERENCE voxels, the
 * bricks dealt over the XCDs as brick_slot0 deals them, at most NORM_MAX_BLOCKS workgroups in a grid loop.  A thread takes four
 * consecutive x voxels of one row: masked first (MASK: M[x] not finite or 0; nothing is sampled then), q = warp_position<FIELD>,
 * `outside` where q fails the sampler's inside test, b = sample_volume<WARP_LINEAR> with fill NaN, qa = quantize(R[x]), qb =
 * quantize(b); `excluded` where either is negative, else counted.
 *   Histograms: two of NORM_BINS = 1024 uint32 in LDS (8 KB), filled with LDS atomic adds.  A thread merges its run of equal bins in
 *   registers, per histogram; what it still holds after its four voxels goes through the wave: where every lane that holds a run holds
 *   the same bin (background, a smooth image), the runs are summed across the wave and ONE lane adds, otherwise each lane adds its
 *   own.  A workgroup counts at most 2^30 voxels, so a word cannot wrap.
 *   The six sums and the three counts: 64-bit registers per thread over the whole loop, reduced across the wave at the end, one LDS add
 *   per wave and word.
 *   Flush: 64-bit global atomic adds of the non-zero words into the result, which the caller zeroed before the launch.
 * Result words (uint64): hist_a 1024, hist_b 1024, n Sa Sb Saa Sbb Sab, masked outside excluded.
 *
 * transfer_apply_kernel.  The index is flat: a thread takes four voxels as one float4 load and store where both pointers are 16-byte
 * aligned and the stretch is whole, else voxel by voxel; at most APPLY_MAX_BLOCKS workgroups in a grid loop; 8 bytes per voxel.  The
 * knots (at most 257 x 3 doubles) are staged in LDS once per workgroup.  k = the largest index with xb[k] <= u by a bisection of
 * `steps` halvings, the same for every voxel of the launch (the host takes it from m), each one LDS read and a select; then the three
 * candidates (lower tail, segment, upper tail) and two selects.  A non-finite voxel is stored with the bits it was loaded with.
 * Every floating-point step is one IEEE double operation in the stated order: -ffp-contract=off and no -fno-honor-nans (Makefile).
 */
#include "sift3d_internal.h"
#include "quantize.h"
#include "warp_device.h"

#define NORM_THREADS 256
#define NORM_MAX_BLOCKS 1024  /* workgroups of the histogram launch: the kernel goes round a grid loop beyond it */
#define NORM_BINS 1024
#define NORM_WORDS 9          /* the six sums, masked, outside, excluded */
#define APPLY_THREADS 256
#define APPLY_VPT 4           /* consecutive voxels per thread */
#define APPLY_MAX_BLOCKS 2048 /* workgroups of the apply launch: a grid loop beyond it */
#define APPLY_MAX_KNOTS 257

static_assert(NORM_THREADS == BRICK_TX * BRICK_BY * BRICK_BZ, "a workgroup is one brick of reference voxels");
static_assert(NORM_MAX_BLOCKS % 8 == 0, "the brick slots are dealt over eight XCDs");
static_assert(NORM_BINS == QMAX + 1 && NORM_BINS == SIFT3D_NORMALIZE_BINS, "one bin per quantised value");
static_assert(APPLY_MAX_KNOTS == SIFT3D_NORMALIZE_MAX_KNOTS, "include/sift3d.h states the cap");
static_assert(NORM_WORDS == SIFT3D_SIMILARITY_SUMS + SIFT3D_NORMALIZE_COUNTS, "the sums, then the counts");

__device__ __forceinline__ unsigned norm_wave_sum(unsigned v)
{
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ unsigned long long norm_wave_sum64(unsigned long long v)
{
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

/* the run (bin, run) a lane still holds, run = 0 for none, into hist: once for the wave where all the held bins agree.  Every lane of
 * the wave calls it */
__device__ __forceinline__ void norm_add_runs(unsigned *hist, int bin, unsigned run)
{
    const unsigned long long holds = __ballot(run != 0u);
    if (!holds) return;
    const int first = __shfl(bin, __ffsll((long long)holds) - 1, 64);
    if (__ballot(run != 0u && bin != first) == 0ull) {
        const unsigned w = norm_wave_sum(run); /* the lanes without a run hold 0 */
        if ((threadIdx.x & 63) == 0) atomicAdd(&hist[first], w);
    } else if (run) {
        atomicAdd(&hist[bin], run);
    }
}

template <int FIELD, int MASK>
__global__ __launch_bounds__(NORM_THREADS) void overlap_hist_kernel(const float *__restrict__ ref, const float *__restrict__ mask, const float *__restrict__ img,
                                                                    const float4 *__restrict__ nodes, const warp_map m, long long nx, long long ny, long long nz,
                                                                    long long mx, long long my, long long mz, long long nbx, long long nby, long long nbricks,
                                                                    double alo, double ahi, double blo, double bhi, unsigned long long *__restrict__ res)
{
    __shared__ unsigned hist_a[NORM_BINS], hist_b[NORM_BINS];
    __shared__ unsigned long long sums[NORM_WORDS];
    for (int t = threadIdx.x; t < NORM_BINS; t += NORM_THREADS) hist_a[t] = hist_b[t] = 0u;
    if (threadIdx.x < NORM_WORDS) sums[threadIdx.x] = 0ull;
    __syncthreads();

    const float hx = (float)(mx - 1), hy = (float)(my - 1), hz = (float)(mz - 1);
    const float nanf_ = __builtin_nanf(""), inf = __builtin_inff();
    int tx, ty, tz;
    brick_lane(tx, ty, tz);
    unsigned long long s[NORM_WORDS] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    /* the loop's bound is the workgroup's: every lane of a wave reaches norm_add_runs */
    for (long long L = brick_slot0(); L < nbricks; L += gridDim.x) {
        long long i0, j, kz;
        brick_voxel(L, nbx, nby, tx, ty, tz, i0, j, kz);
        const bool row = j < ny && kz < nz;
        const long long at = row ? (kz * ny + j) * nx : 0;
        const float py = (float)j, pz = (float)kz;
        int bin_a = 0, bin_b = 0;
        unsigned run_a = 0, run_b = 0;
#pragma unroll
        for (int v = 0; v < BRICK_VX; v++) {
            const long long i = i0 + v;
            if (!row || i >= nx) continue;
            if (MASK) {
                const float w = mask[at + i];
                if (!(fabsf(w) < inf) || w == 0.0f) {
                    s[6] += 1ull;
                    continue;
                }
            }
            float q[3];
            warp_position<FIELD>(m, nodes, (float)i, py, pz, q);
            if (!(q[0] >= 0.0f && q[0] <= hx && q[1] >= 0.0f && q[1] <= hy && q[2] >= 0.0f && q[2] <= hz)) {
                s[7] += 1ull;
                continue;
            }
            const float b = sample_volume<WARP_LINEAR>(img, mx, my, mz, hx, hy, hz, q[0], q[1], q[2], nanf_);
            const int qa = quantize(ref[at + i], alo, ahi), qb = quantize(b, blo, bhi);
            if (qa < 0 || qb < 0) {
                s[8] += 1ull;
                continue;
            }
            const unsigned ua = (unsigned)qa, ub = (unsigned)qb;
            s[0] += 1ull;
            s[1] += ua;
            s[2] += ub;
            s[3] += ua * ua;
            s[4] += ub * ub;
            s[5] += ua * ub;
            if (qa != bin_a) {
                if (run_a) atomicAdd(&hist_a[bin_a], run_a);
                bin_a = qa;
                run_a = 0;
            }
            run_a++;
            if (qb != bin_b) {
                if (run_b) atomicAdd(&hist_b[bin_b], run_b);
                bin_b = qb;
                run_b = 0;
            }
            run_b++;
        }
        norm_add_runs(hist_a, bin_a, run_a);
        norm_add_runs(hist_b, bin_b, run_b);
    }
    for (int w = 0; w < NORM_WORDS; w++) {
        const unsigned long long t = norm_wave_sum64(s[w]);
        if ((threadIdx.x & 63) == 0 && t) atomicAdd(&sums[w], t);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < NORM_BINS; t += NORM_THREADS) {
        if (hist_a[t]) atomicAdd(&res[t], (unsigned long long)hist_a[t]);
        if (hist_b[t]) atomicAdd(&res[NORM_BINS + t], (unsigned long long)hist_b[t]);
    }
    if (threadIdx.x < NORM_WORDS && sums[threadIdx.x]) atomicAdd(&res[2 * NORM_BINS + threadIdx.x], sums[threadIdx.x]);
}

int sift3d_normalize_words(void) { return 2 * NORM_BINS + NORM_WORDS; }

/* ref, mask (or NULL), img, nodes (or NULL: no field): device pointers; m: the map and, with nodes, the field's terms and grid; res:
 * sift3d_normalize_words() words, which the caller has zeroed on the stream (the kernel adds to them).  The caller has checked the extents (1 .. 4096 each, at most 2^30 voxels a volume). */
hipError_t sift3d_launch_overlap_hist(hipStream_t s, const float *ref, const float *mask, int64_t nx, int64_t ny, int64_t nz, const float *img, int64_t mx,
                                      int64_t my, int64_t mz, const float *map, const float *c, const float *k, const float o[3], float h, const int64_t n[3],
                                      const float4 *nodes, double alo, double ahi, double blo, double bhi, unsigned long long *res)
{
    if (nx < 1 || ny < 1 || nz < 1 || mx < 1 || my < 1 || mz < 1 || nx * ny * nz > (1ll << 30)) return hipErrorInvalidValue;
    warp_map m;
    fill_warp_map(m, map, c, k, nodes != nullptr, o, h, n);
    brick_launch b = brick_launch_of(ref, nx, ny, nz);
    if (b.grid > NORM_MAX_BLOCKS) b.grid = NORM_MAX_BLOCKS;
    auto kernel = nodes ? (mask ? overlap_hist_kernel<1, 1> : overlap_hist_kernel<1, 0>) : (mask ? overlap_hist_kernel<0, 1> : overlap_hist_kernel<0, 0>);
    hipLaunchKernelGGL(kernel, dim3(b.grid), dim3(NORM_THREADS), 0, s, ref, mask, img, nodes, m, (long long)nx, (long long)ny, (long long)nz, (long long)mx,
                       (long long)my, (long long)mz, b.nbx, b.nby, b.nbricks, alo, ahi, blo, bhi, res);
    return hipGetLastError();
}

/* the table as the apply kernel reads it: transfer_api fills it on the host, the launch passes it by value */
struct apply_head {
    double blo, bhi, alo, wa, tail;
    int m, steps; /* steps: the halvings of the bisection, 2^steps >= m */
};

/* one voxel; xb, xa, slope: the staged knots */
__device__ __forceinline__ float apply_voxel(float v, const apply_head &t, const double *xb, const double *xa, const double *slope)
{
    const double u = (((double)v - t.blo) / (t.bhi - t.blo)) * (double)QMAX;
    int k = 0;
    for (int step = 1 << (t.steps - 1); step > 0; step >>= 1) { /* uniform: the same trips for every lane */
        const int c = k + step, r = c < t.m ? c : t.m - 1;
        k = ((c < t.m) & (xb[r] <= u)) ? c : k; /* & not &&: a select, no branch */
    }
    const int top = t.m - 1, ks = k < top ? k : top - 1;
    const double seg = fmin(xa[ks] + (u - xb[ks]) * slope[ks], xa[ks + 1]);
    const double low = xa[0] + (u - xb[0]) * t.tail, high = xa[top] + (u - xb[top]) * t.tail;
    const double y = u < xb[0] ? low : (u >= xb[top] ? high : seg);
    const float out = (float)(t.alo + y * t.wa);
    /* as integers: a NaN keeps its payload and its sign */
    return __uint_as_float(fabsf(v) < __builtin_inff() ? __float_as_uint(out) : __float_as_uint(v));
}

__global__ __launch_bounds__(APPLY_THREADS) void transfer_apply_kernel(const float *__restrict__ in, float *__restrict__ out, long long n, const apply_head t,
                                                                       const double *__restrict__ knots)
{
    __shared__ double xb[APPLY_MAX_KNOTS], xa[APPLY_MAX_KNOTS], slope[APPLY_MAX_KNOTS];
    for (int k = threadIdx.x; k < t.m; k += APPLY_THREADS) {
        xb[k] = knots[k];
        xa[k] = knots[APPLY_MAX_KNOTS + k];
        slope[k] = knots[2 * APPLY_MAX_KNOTS + k];
    }
    __syncthreads();
    const bool aligned = ((((size_t)in | (size_t)out)) & 15) == 0;
    const long long stretch = (long long)APPLY_THREADS * APPLY_VPT;
    for (long long base = (long long)blockIdx.x * stretch; base < n; base += (long long)gridDim.x * stretch) {
        const long long i0 = base + (long long)threadIdx.x * APPLY_VPT;
        if (aligned && i0 + APPLY_VPT <= n) {
            const float4 v = *reinterpret_cast<const float4 *>(in + i0);
            *reinterpret_cast<float4 *>(out + i0) =
                make_float4(apply_voxel(v.x, t, xb, xa, slope), apply_voxel(v.y, t, xb, xa, slope), apply_voxel(v.z, t, xb, xa, slope), apply_voxel(v.w, t, xb, xa, slope));
        } else {
            for (int e = 0; e < APPLY_VPT; e++)
                if (i0 + e < n) out[i0 + e] = apply_voxel(in[i0 + e], t, xb, xa, slope);
        }
    }
}

/* the halvings the bisection over m knots takes: the least s with 2^s >= m */
static int apply_steps(int m)
{
    int s = 1;
    while ((1 << s) < m) s++;
    return s;
}

/* in, out: n voxels on the device; knots: 3 x APPLY_MAX_KNOTS doubles on the device (xb, xa, slope, each from its own multiple of
 * APPLY_MAX_KNOTS).  The caller has checked the table (sift3d_transfer_check). */
hipError_t sift3d_launch_transfer_apply(hipStream_t s, const float *in, float *out, int64_t n, const sift3d_transfer *table, const double *knots)
{
    if (n < 1 || !table || table->m < 2 || table->m > APPLY_MAX_KNOTS) return hipErrorInvalidValue;
    apply_head t;
    t.blo = (double)table->b_lo;
    t.bhi = (double)table->b_hi;
    t.alo = (double)table->a_lo;
    t.wa = table->wa;
    t.tail = table->tail;
    t.m = table->m;
    t.steps = apply_steps(table->m);
    const int64_t stretch = (int64_t)APPLY_THREADS * APPLY_VPT, blocks = (n + stretch - 1) / stretch;
    hipLaunchKernelGGL(transfer_apply_kernel, dim3((unsigned)(blocks < APPLY_MAX_BLOCKS ? blocks : APPLY_MAX_BLOCKS)), dim3(APPLY_THREADS), 0, s, in, out,
                       (long long)n, t, knots);
    return hipGetLastError();
}
