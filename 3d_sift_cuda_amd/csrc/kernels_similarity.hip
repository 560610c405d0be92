/*
 * kernels_similarity.hip -- the joint histogram and the integer sums of two images on one grid for gfx950 (MI355X; DESIGN.md section
 * 7o; tests/similarity_oracle.c restates them serially).  Everything is counts and integer sums, so nothing depends on the tiling,
 * the launch order or the order the atomics arrive in.
 *
 * joint_hist_kernel<LABELS>  reads the two float volumes once (8 bytes per voxel; with LABELS the label volume too, 12), quantises
 *                       in registers (quantize.h's map, which bm_quantize_kernel stores as an int16 plane; none is kept here)
 *                       and counts.  The index is flat.  A thread takes SIM_VPT consecutive voxels, as one float4 per
 *                       volume where the stretch is whole and the pointers are 16-byte aligned; a workgroup of SIM_THREADS a stretch
 *                       of SIM_THREADS x SIM_VPT voxels; a launch has at most SIM_MAX_BLOCKS workgroups, which go round a grid loop.
 *                       Histogram: bins^2 uint32 in LDS (16 KiB at 64 bins), zeroed by the workgroup, filled with LDS atomic adds;
 *                       a thread merges its consecutive voxels of one cell in registers first.  A cell index is formed from q >= 0
 *                       values only, so it is below bins^2.
 *                       Six sums: 64-bit registers per thread over the whole loop, reduced across the wave at the end, one LDS
 *                       add per wave and sum.
 *                       Label sums (LABELS): SIM_MAX_LABELS x 6 uint64 in LDS.  The slot of a label is the index the host gave it
 *                       in the ascending list of the labels present (a table of 65536 bytes).  A thread gathers its voxels of one
 *                       slot in 32-bit registers (4 x 1023^2 < 2^23); a wave whose threads all hold one slot reduces them (256 x
 *                       1023^2 < 2^32) and adds once per sum, any other wave adds thread by thread.
 *                       Flush: SIM_FLUSH_SLICES: the workgroup stores its LDS words, zeros included, to its slice in global memory;
 *                       SIM_FLUSH_ATOMICS: 64-bit global atomic adds of the non-zero words to the result, which the call zeroed.
 * sum_slices_kernel     the slices into the result: a thread per word and part of the slices, one 64-bit atomic add each (the call
 *                       zeroed the result).
 * Result words (uint64): bins^2 cells, the six sums, then with LABELS SIM_MAX_LABELS x 6 label sums.
 */
#include "sift3d_internal.h"
#include "label_plane.h"
#include "quantize.h"

#define SIM_THREADS 256
#define SIM_VPT 4            /* consecutive voxels per thread */
#define SIM_MAX_BLOCKS 2048  /* of a launch: the kernel goes round a grid loop beyond it */
#define SIM_MAX_BINS 64
#define SIM_MAX_LABELS 64
#define SIM_SUMS 6
#define SIM_FLUSH_SLICES 0
#define SIM_FLUSH_ATOMICS 1
#define SIM_SLICE_PARTS 16   /* sum_slices_kernel: the slices are summed in this many parts */

__device__ __forceinline__ unsigned sim_wave_sum(unsigned v)
{
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ unsigned long long sim_wave_sum64(unsigned long long v)
{
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

/* up to SIM_VPT voxels from i0 on: one float4 where vec (whole stretch, aligned pointer), else voxel by voxel */
__device__ __forceinline__ void sim_load(const float *__restrict__ p, long long i0, int cnt, bool vec, float v[SIM_VPT])
{
    if (vec) {
        const float4 t = *reinterpret_cast<const float4 *>(p + i0);
        v[0] = t.x;
        v[1] = t.y;
        v[2] = t.z;
        v[3] = t.w;
    } else {
        for (int k = 0; k < SIM_VPT; k++) v[k] = k < cnt ? p[i0 + k] : 0.0f;
    }
}

template <bool LABELS>
__global__ __launch_bounds__(SIM_THREADS) void joint_hist_kernel(const float *__restrict__ a, const float *__restrict__ b, const float *__restrict__ lab,
                                                                 const unsigned char *__restrict__ slot_of, long long n, double alo, double ahi, double blo,
                                                                 double bhi, int bins_log2, int flush, unsigned long long *__restrict__ res,
                                                                 unsigned *__restrict__ slice_hist, unsigned long long *__restrict__ slice_sums)
{
    __shared__ unsigned hist[SIM_MAX_BINS * SIM_MAX_BINS];
    __shared__ unsigned long long sums[SIM_SUMS + (LABELS ? SIM_MAX_LABELS * SIM_SUMS : 0)];
    const int cells = 1 << (2 * bins_log2), shift = 10 - bins_log2;
    const int nsums = SIM_SUMS + (LABELS ? SIM_MAX_LABELS * SIM_SUMS : 0);
    for (int t = threadIdx.x; t < cells; t += SIM_THREADS) hist[t] = 0u;
    for (int t = threadIdx.x; t < nsums; t += SIM_THREADS) sums[t] = 0ull;
    __syncthreads();

    const bool aligned = ((((size_t)a | (size_t)b) | (LABELS ? (size_t)lab : (size_t)0)) & 15) == 0;
    unsigned long long s[SIM_SUMS] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    const long long stretch = (long long)SIM_THREADS * SIM_VPT;
    for (long long base = (long long)blockIdx.x * stretch; base < n; base += (long long)gridDim.x * stretch) {
        const long long i0 = base + (long long)threadIdx.x * SIM_VPT;
        const long long left = n - i0;
        const int cnt = left >= SIM_VPT ? SIM_VPT : (left > 0 ? (int)left : 0);
        const bool vec = aligned && cnt == SIM_VPT;
        float va[SIM_VPT], vb[SIM_VPT], vl[SIM_VPT];
        sim_load(a, i0, cnt, vec, va);
        sim_load(b, i0, cnt, vec, vb);
        if (LABELS) sim_load(lab, i0, cnt, vec, vl);
        int cell = -1, slot = -1;   /* the cell and the slot of the run the thread holds */
        unsigned run = 0;
        unsigned l[SIM_SUMS] = {0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < SIM_VPT; k++) {
            const int qa = quantize(va[k], alo, ahi), qb = quantize(vb[k], blo, bhi);
            if (k >= cnt || qa < 0 || qb < 0) continue;
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
            if (LABELS && isfinite(vl[k])) {
                const int sl = (int)(slot_of[label_bits(vl[k])] & (SIM_MAX_LABELS - 1));
                if (sl != slot) {
                    if (slot >= 0)
                        for (int j = 0; j < SIM_SUMS; j++)
                            if (l[j]) atomicAdd(&sums[SIM_SUMS + slot * SIM_SUMS + j], (unsigned long long)l[j]);
                    slot = sl;
                    for (int j = 0; j < SIM_SUMS; j++) l[j] = 0u;
                }
                l[0] += 1u;
                l[1] += ua;
                l[2] += ub;
                l[3] += ua * ua;
                l[4] += ub * ub;
                l[5] += ua * ub;
            }
        }
        if (run) atomicAdd(&hist[cell], run);
        if (LABELS) {
            /* every lane of the wave is here: the loop's bound is the workgroup's */
            const unsigned long long holds = __ballot(slot >= 0);
            if (holds) {
                const int first = __shfl(slot, __ffsll((long long)holds) - 1, 64);
                if (__ballot(slot >= 0 && slot != first) == 0ull) {
                    for (int j = 0; j < SIM_SUMS; j++) {
                        const unsigned w = sim_wave_sum(l[j]);   /* the lanes without a slot hold zeros */
                        if ((threadIdx.x & 63) == 0 && w) atomicAdd(&sums[SIM_SUMS + first * SIM_SUMS + j], (unsigned long long)w);
                    }
                } else if (slot >= 0) {
                    for (int j = 0; j < SIM_SUMS; j++)
                        if (l[j]) atomicAdd(&sums[SIM_SUMS + slot * SIM_SUMS + j], (unsigned long long)l[j]);
                }
            }
        }
    }
    for (int j = 0; j < SIM_SUMS; j++) {
        const unsigned long long w = sim_wave_sum64(s[j]);
        if ((threadIdx.x & 63) == 0 && w) atomicAdd(&sums[j], w);
    }
    __syncthreads();

    if (flush == SIM_FLUSH_SLICES) {
        for (int t = threadIdx.x; t < cells; t += SIM_THREADS) slice_hist[(long long)blockIdx.x * cells + t] = hist[t];
        for (int t = threadIdx.x; t < nsums; t += SIM_THREADS) slice_sums[(long long)blockIdx.x * nsums + t] = sums[t];
    } else {
        for (int t = threadIdx.x; t < cells; t += SIM_THREADS)
            if (hist[t]) atomicAdd(&res[t], (unsigned long long)hist[t]);
        for (int t = threadIdx.x; t < nsums; t += SIM_THREADS)
            if (sums[t]) atomicAdd(&res[cells + t], sums[t]);
    }
}

/* res[w] += the words w of the slices part, part + gridDim.y, ...: w < cells a histogram cell, else a sum */
__global__ __launch_bounds__(SIM_THREADS) void sum_slices_kernel(const unsigned *__restrict__ slice_hist, const unsigned long long *__restrict__ slice_sums,
                                                                 int slices, int cells, int nsums, unsigned long long *__restrict__ res)
{
    const int w = blockIdx.x * SIM_THREADS + threadIdx.x;
    if (w >= cells + nsums) return;
    unsigned long long t = 0ull;
    if (w < cells)
        for (int g = blockIdx.y; g < slices; g += gridDim.y) t += slice_hist[(long long)g * cells + w];
    else
        for (int g = blockIdx.y; g < slices; g += gridDim.y) t += slice_sums[(long long)g * nsums + (w - cells)];
    if (t) atomicAdd(&res[w], t);
}

int sift3d_similarity_blocks(int64_t n)
{
    const int64_t stretch = (int64_t)SIM_THREADS * SIM_VPT, blocks = (n + stretch - 1) / stretch;
    return (int)(blocks < SIM_MAX_BLOCKS ? blocks : SIM_MAX_BLOCKS);
}

int sift3d_similarity_words(int bins, bool labels) { return bins * bins + SIM_SUMS + (labels ? SIM_MAX_LABELS * SIM_SUMS : 0); }

/* lab and slot_of NULL: no label sums.  res: sift3d_similarity_words words, zeroed here.  slice_hist (blocks x bins^2 words) and
 * slice_sums (blocks x the other words), blocks = sift3d_similarity_blocks(n): read under SIM_FLUSH_SLICES only. */
hipError_t sift3d_launch_joint_hist(hipStream_t s, const float *a, const float *b, const float *lab, const unsigned char *slot_of, int64_t n, double alo,
                                    double ahi, double blo, double bhi, int bins, int flush, unsigned long long *res, unsigned *slice_hist,
                                    unsigned long long *slice_sums)
{
    int bins_log2 = 0;
    while ((1 << bins_log2) < bins) bins_log2++;
    if (n <= 0 || (1 << bins_log2) != bins || bins < 8 || bins > SIM_MAX_BINS || (flush != SIM_FLUSH_SLICES && flush != SIM_FLUSH_ATOMICS) ||
        (lab != nullptr) != (slot_of != nullptr) || (flush == SIM_FLUSH_SLICES && (!slice_hist || !slice_sums)))
        return hipErrorInvalidValue;
    const bool labels = lab != nullptr;
    const int blocks = sift3d_similarity_blocks(n), cells = bins * bins, words = sift3d_similarity_words(bins, labels);
    hipError_t rc = hipMemsetAsync(res, 0, sizeof(unsigned long long) * (size_t)words, s);
    if (rc != hipSuccess) return rc;
    if (labels)
        hipLaunchKernelGGL(joint_hist_kernel<true>, dim3((unsigned)blocks), dim3(SIM_THREADS), 0, s, a, b, lab, slot_of, (long long)n, alo, ahi, blo, bhi,
                           bins_log2, flush, res, slice_hist, slice_sums);
    else
        hipLaunchKernelGGL(joint_hist_kernel<false>, dim3((unsigned)blocks), dim3(SIM_THREADS), 0, s, a, b, lab, slot_of, (long long)n, alo, ahi, blo, bhi,
                           bins_log2, flush, res, slice_hist, slice_sums);
    rc = hipGetLastError();
    if (rc != hipSuccess || flush != SIM_FLUSH_SLICES) return rc;
    const int parts = blocks < SIM_SLICE_PARTS ? blocks : SIM_SLICE_PARTS;
    hipLaunchKernelGGL(sum_slices_kernel, dim3((unsigned)((words + SIM_THREADS - 1) / SIM_THREADS), (unsigned)parts), dim3(SIM_THREADS), 0, s, slice_hist,
                       slice_sums, blocks, cells, words - cells, res);
    return hipGetLastError();
}
