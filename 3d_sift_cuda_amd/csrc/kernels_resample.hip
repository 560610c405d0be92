/*
 * kernels_resample.hip -- featResample's hot path for gfx950 (MI355X): a float32 volume resampled onto another grid through
 * a 3 x 4 map that takes an output voxel index to a source voxel position.  Beyond the reference,
 * which stops at the .trans.txt matrix.
 *
 * The arithmetic is the contract of section 7c, operation for operation (tests/resample_oracle.c restates it on the CPU):
 *   q_r = ((A[r][0] * i + A[r][1] * j) + A[r][2] * k) + A[r][3] with i, j, k converted to float; a sample only where
 *   0 <= q <= n - 1 on every axis (NaN fails), `fill` elsewhere.  Linear: f = floorf(q), w = q - f, i0 = (int64)f,
 *   i1 = min(i0 + 1, n - 1), interpolated along x, then y, then z, each step (1 - w) * a + w * b; all eight corners are
 *   read and weighed, so a NaN or infinite corner of weight 0 still reaches the result (IEEE, no -fno-honor-nans).
 *   Nearest: i = min((int64)floorf(q + 0.5f), n - 1).  No texture sampler: its filter weights are fixed-point.
 *
 * Mapping.  A workgroup of 256 threads owns a brick of 32 x 8 x 4 output voxels; a thread owns four consecutive x voxels of
 * one row (one 16-byte store when the row allows it) and evaluates the map for each of them.  The bricks are numbered x
 * fastest, then y, then z, and the launch deals block b to brick slot (b % 8) * (grid / 8) + b / 8: blocks are dealt
 * round-robin over the eight XCDs, so each XCD walks one contiguous run of bricks -- a slab of output planes whose source
 * footprint stays compact under any rotation and is shared through that XCD's L2.  The placement is for speed only.
 * Larger outputs than one grid loop over the brick slots in strides of the grid.  All voxel indices are 64-bit.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#define RS_TX 8                  /* threads along x */
#define RS_VX 4                  /* consecutive x voxels per thread */
#define RS_BX (RS_TX * RS_VX)    /* 32 */
#define RS_BY 8
#define RS_BZ 4                  /* RS_TX * RS_BY * RS_BZ = 256 threads */
#define RS_MAX_GRID (1u << 22)

struct rs_map {
    float a[12];
};

template <int NEAREST>
__global__ __launch_bounds__(256) void resample_kernel(const float *__restrict__ src, long long nx, long long ny, long long nz,
                                                       float *__restrict__ dst, long long ox, long long oy, long long oz, rs_map m,
                                                       float fill, long long nbx, long long nby, long long nbricks, int vec)
{
    const unsigned grid = gridDim.x, b = blockIdx.x;
    const long long slot0 = (long long)(b & 7u) * (grid >> 3) + (b >> 3);
    const int tx = threadIdx.x & (RS_TX - 1), ty = (threadIdx.x / RS_TX) & (RS_BY - 1), tz = threadIdx.x / (RS_TX * RS_BY);
    const float hx = (float)(nx - 1), hy = (float)(ny - 1), hz = (float)(nz - 1);
    for (long long L = slot0; L < nbricks; L += grid) {
        const long long bx = L % nbx, t = L / nbx, by = t % nby, bz = t / nby;
        const long long i0 = bx * RS_BX + tx * RS_VX, j = by * RS_BY + ty, k = bz * RS_BZ + tz;
        if (j >= oy || k >= oz || i0 >= ox) continue;
        const float py = (float)j, pz = (float)k;
        float r[RS_VX];
#pragma unroll
        for (int v = 0; v < RS_VX; v++) {
            const float px = (float)(i0 + v);
            const float qx = ((m.a[0] * px + m.a[1] * py) + m.a[2] * pz) + m.a[3];
            const float qy = ((m.a[4] * px + m.a[5] * py) + m.a[6] * pz) + m.a[7];
            const float qz = ((m.a[8] * px + m.a[9] * py) + m.a[10] * pz) + m.a[11];
            r[v] = fill;
            if (!(qx >= 0.0f && qx <= hx && qy >= 0.0f && qy <= hy && qz >= 0.0f && qz <= hz)) continue;
            if (NEAREST) {
                /* q <= n - 1 <= 2^24 - 1 here: the int conversions give the values of (int64) ones, in one instruction */
                long long ix = (int)floorf(qx + 0.5f), iy = (int)floorf(qy + 0.5f), iz = (int)floorf(qz + 0.5f);
                ix = ix < nx - 1 ? ix : nx - 1;
                iy = iy < ny - 1 ? iy : ny - 1;
                iz = iz < nz - 1 ? iz : nz - 1;
                r[v] = src[(iz * ny + iy) * nx + ix];
            } else {
                const float fx = floorf(qx), fy = floorf(qy), fz = floorf(qz);
                const float wx = qx - fx, wy = qy - fy, wz = qz - fz;
                const long long x0 = (int)fx, y0 = (int)fy, z0 = (int)fz;
                const long long x1 = x0 + 1 < nx - 1 ? x0 + 1 : nx - 1, y1 = y0 + 1 < ny - 1 ? y0 + 1 : ny - 1,
                                z1 = z0 + 1 < nz - 1 ? z0 + 1 : nz - 1;
                const float *r00 = src + (z0 * ny + y0) * nx, *r10 = src + (z0 * ny + y1) * nx, *r01 = src + (z1 * ny + y0) * nx,
                            *r11 = src + (z1 * ny + y1) * nx;
                const float ux = 1.0f - wx, uy = 1.0f - wy, uz = 1.0f - wz;
                const float c00 = ux * r00[x0] + wx * r00[x1]; /* (y0, z0) */
                const float c10 = ux * r10[x0] + wx * r10[x1]; /* (y1, z0) */
                const float c01 = ux * r01[x0] + wx * r01[x1]; /* (y0, z1) */
                const float c11 = ux * r11[x0] + wx * r11[x1]; /* (y1, z1) */
                const float c0 = uy * c00 + wy * c10, c1 = uy * c01 + wy * c11;
                r[v] = uz * c0 + wz * c1;
            }
        }
        float *o = dst + (k * oy + j) * ox + i0;
        if (vec && i0 + RS_VX <= ox) {
            *reinterpret_cast<float4 *>(o) = make_float4(r[0], r[1], r[2], r[3]);
        } else {
#pragma unroll
            for (int v = 0; v < RS_VX; v++)
                if (i0 + v < ox) o[v] = r[v];
        }
    }
}

/* map: 12 floats, row-major 3 x 4.  The caller has checked the shapes (every extent >= 1). */
hipError_t sift3d_launch_resample(hipStream_t s, const float *src, int64_t nx, int64_t ny, int64_t nz, float *dst, int64_t ox, int64_t oy,
                                  int64_t oz, const float *map, int nearest, float fill)
{
    rs_map m;
    for (int r = 0; r < 12; r++) m.a[r] = map[r];
    const long long nbx = (ox + RS_BX - 1) / RS_BX, nby = (oy + RS_BY - 1) / RS_BY, nbz = (oz + RS_BZ - 1) / RS_BZ;
    const long long nbricks = nbx * nby * nbz;
    long long g = (nbricks + 7) / 8 * 8; /* a multiple of the XCD count: grid / 8 slots per XCD */
    if (g > (long long)RS_MAX_GRID) g = RS_MAX_GRID;
    /* 16-byte stores need rows of whole float4s and an aligned base */
    const int vec = (ox % RS_VX) == 0 && ((uintptr_t)dst % 16) == 0;
    if (nearest)
        hipLaunchKernelGGL(resample_kernel<1>, dim3((unsigned)g), dim3(256), 0, s, src, (long long)nx, (long long)ny, (long long)nz, dst,
                           (long long)ox, (long long)oy, (long long)oz, m, fill, nbx, nby, nbricks, vec);
    else
        hipLaunchKernelGGL(resample_kernel<0>, dim3((unsigned)g), dim3(256), 0, s, src, (long long)nx, (long long)ny, (long long)nz, dst,
                           (long long)ox, (long long)oy, (long long)oz, m, fill, nbx, nby, nbricks, vec);
    return hipGetLastError();
}
