/*
 * kernels_label.hip -- the label plane of the label tools for gfx950 (MI355X; label_plane.h; DESIGN.md sections 7l, 7m): float labels
 * to a uint16 plane and one validity bit per voxel.  A wave's ballot is the 64-bit word of its 64 voxels.  The surface distances
 * (edt_api.hip) run it once per volume, the components and the cleaning (ccl_api.hip) once per labelling.
 */
#include <algorithm>

#include "sift3d_internal.h"
#include "label_plane.h"

#define LABEL_THREADS 256
#define LABEL_MAX_BLOCKS 2048 /* the kernel goes round a grid loop beyond it */

__global__ __launch_bounds__(LABEL_THREADS) void label_plane_kernel(const float *__restrict__ labels, long long n, unsigned short *__restrict__ lab,
                                                                    unsigned long long *__restrict__ valid)
{
    for (long long base = (long long)blockIdx.x * LABEL_THREADS; base < n; base += (long long)gridDim.x * LABEL_THREADS) {
        const long long i = base + threadIdx.x;
        const float v = i < n ? labels[i] : 0.0f;
        const bool ok = i < n && isfinite(v);
        /* every lane of the wave is here: the loop's bound is the workgroup's.  The lanes past n vote 0, so the last word of valid
         * is stored whole, its bits past n clear. */
        const unsigned long long m = __ballot(ok);
        if (i < n) lab[i] = ok ? (unsigned short)label_bits(v) : (unsigned short)0;
        if ((threadIdx.x & 63) == 0 && i < n) valid[i >> 6] = m;
    }
}

/* n >= 1 voxels; valid holds (n + 63) / 64 words */
hipError_t sift3d_launch_label_plane(hipStream_t s, const float *labels, int64_t n, unsigned short *lab, unsigned long long *valid)
{
    const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>((n + LABEL_THREADS - 1) / LABEL_THREADS, LABEL_MAX_BLOCKS));
    hipLaunchKernelGGL(label_plane_kernel, dim3(grid), dim3(LABEL_THREADS), 0, s, labels, (long long)n, lab, valid);
    return hipGetLastError();
}
