/*
 * kernels_resample.hip -- featResample's hot path for gfx950 (MI355X): a float32 volume resampled onto another grid through
 * a 3 x 4 map that takes an output voxel index to a source voxel position.  Beyond the reference,
 * which stops at the .trans.txt matrix.
 *
 * The arithmetic (the position, the inside test, the three interpolations) and the mapping (the brick of 32 x 8 x 4 output
 * voxels, four x voxels per thread, the XCD dealing) are warp_device.h's; its header states the contract.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "warp_device.h"

struct rs_map {
    float a[12];
};

template <int MODE>
__global__ __launch_bounds__(256) void resample_kernel(const float *__restrict__ src, long long nx, long long ny, long long nz,
                                                       float *__restrict__ dst, long long ox, long long oy, long long oz, rs_map m,
                                                       float fill, long long nbx, long long nby, long long nbricks, int vec)
{
    int tx, ty, tz;
    brick_lane(tx, ty, tz);
    const float hx = (float)(nx - 1), hy = (float)(ny - 1), hz = (float)(nz - 1);
    for (long long L = brick_slot0(); L < nbricks; L += gridDim.x) {
        long long i0, j, k;
        brick_voxel(L, nbx, nby, tx, ty, tz, i0, j, k);
        if (j >= oy || k >= oz || i0 >= ox) continue;
        float r[BRICK_VX];
#pragma unroll
        for (int v = 0; v < BRICK_VX; v++) {
            float q[3];
            warp_position<0>(m, nullptr, (float)(i0 + v), (float)j, (float)k, q);
            r[v] = sample_volume<MODE>(src, nx, ny, nz, hx, hy, hz, q[0], q[1], q[2], fill);
        }
        store_row4(dst + (k * oy + j) * ox + i0, ox, i0, r, vec);
    }
}

/* map: 12 floats, row-major 3 x 4; mode: a sift3d_interp.  The caller has checked the shapes (every extent >= 1) and the mode. */
hipError_t sift3d_launch_resample(hipStream_t s, const float *src, int64_t nx, int64_t ny, int64_t nz, float *dst, int64_t ox, int64_t oy,
                                  int64_t oz, const float *map, int mode, float fill)
{
    rs_map m;
    for (int r = 0; r < 12; r++) m.a[r] = map[r];
    const brick_launch b = brick_launch_of(dst, ox, oy, oz);
    auto kernel = mode == WARP_LABEL ? resample_kernel<WARP_LABEL> : mode == WARP_NEAREST ? resample_kernel<WARP_NEAREST> : resample_kernel<WARP_LINEAR>;
    hipLaunchKernelGGL(kernel, dim3(b.grid), dim3(256), 0, s, src, (long long)nx, (long long)ny, (long long)nz, dst, (long long)ox, (long long)oy,
                       (long long)oz, m, fill, b.nbx, b.nby, b.nbricks, b.vec);
    return hipGetLastError();
}
