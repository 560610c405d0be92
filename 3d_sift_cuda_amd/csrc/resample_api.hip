/*
 * resample_api.hip -- C-ABI of featResample's resampler (include/sift3d.h, "resampling"):
 * sift3d_resample_affine on host arrays and sift3d_resample_affine_dev on device buffers, on a context's stream.  The
 * kernel is in kernels_resample.hip; the map comes from sift3d_resample_map (align_host.c).
 */
#include <cstdio>
#include <cstring>

#include "sift3d_internal.h"

#include "pipeline.h"

hipError_t sift3d_launch_resample(hipStream_t s, const float *src, int64_t nx, int64_t ny, int64_t nz, float *dst, int64_t ox, int64_t oy,
                                  int64_t oz, const float *map, int nearest, float fill);

#define RCHK(call)                                                                                       \
    do {                                                                                                 \
        hipError_t e_ = (call);                                                                          \
        if (e_ != hipSuccess) {                                                                          \
            if (err && err_len > 0) snprintf(err, (size_t)err_len, "%s failed: %s", #call, hipGetErrorString(e_)); \
            rc = SIFT3D_ERR_DEVICE;                                                                      \
            goto done;                                                                                   \
        }                                                                                                \
    } while (0)

/* NULL when the arguments are usable, else the reason.  Source extents up to 2^24, so that n - 1 is exact in float and
 * the inside test can never admit a position past the last voxel; output extents up to 2^31 each, 2^40 voxels in all. */
static const char *check_args(const float *src, int64_t nx, int64_t ny, int64_t nz, const float *dst, int64_t ox, int64_t oy, int64_t oz,
                              const float *map, int interp)
{
    if (!src || !dst || !map) return "null pointer";
    if (interp != SIFT3D_INTERP_LINEAR && interp != SIFT3D_INTERP_NEAREST) return "interp must be SIFT3D_INTERP_LINEAR or SIFT3D_INTERP_NEAREST";
    if (nx < 1 || ny < 1 || nz < 1 || nx > (1 << 24) || ny > (1 << 24) || nz > (1 << 24)) return "source extents must be 1 .. 2^24";
    if (ox < 1 || oy < 1 || oz < 1 || ox >= (1ll << 31) || oy >= (1ll << 31) || oz >= (1ll << 31)) return "output extents must be 1 .. 2^31 - 1";
    if (ox * oy > (1ll << 40) / oz) return "output larger than 2^40 voxels";
    return nullptr;
}

extern "C" int sift3d_resample_affine(int device, const float *src, int64_t nx, int64_t ny, int64_t nz, float *dst, int64_t ox, int64_t oy,
                                      int64_t oz, const float map[12], int interp, float fill, double *kernel_ms, char *err, int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (kernel_ms) *kernel_ms = 0.0;
    const char *why = check_args(src, nx, ny, nz, dst, ox, oy, oz, map, interp);
    if (why) {
        if (err && err_len > 0) snprintf(err, (size_t)err_len, "%s", why);
        return SIFT3D_ERR_ARG;
    }
    int rc = SIFT3D_OK;
    const size_t in_b = sizeof(float) * (size_t)(nx * ny * nz), out_b = sizeof(float) * (size_t)(ox * oy * oz);
    float *d_src = nullptr, *d_dst = nullptr;
    hipStream_t s = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    RCHK(hipSetDevice(device));
    RCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    RCHK(hipEventCreate(&e0));
    RCHK(hipEventCreate(&e1));
    if (hipMalloc((void **)&d_src, in_b) != hipSuccess || hipMalloc((void **)&d_dst, out_b) != hipSuccess) {
        (void)hipGetLastError();
        if (err && err_len > 0) snprintf(err, (size_t)err_len, "cannot allocate %zu + %zu bytes on device %d", in_b, out_b, device);
        rc = SIFT3D_ERR_MEMORY;
        goto done;
    }
    RCHK(hipMemcpyAsync(d_src, src, in_b, hipMemcpyHostToDevice, s));
    RCHK(hipEventRecord(e0, s));
    RCHK(sift3d_launch_resample(s, d_src, nx, ny, nz, d_dst, ox, oy, oz, map, interp == SIFT3D_INTERP_NEAREST, fill));
    RCHK(hipEventRecord(e1, s));
    RCHK(hipMemcpyAsync(dst, d_dst, out_b, hipMemcpyDeviceToHost, s));
    RCHK(hipStreamSynchronize(s));
    if (kernel_ms) {
        float ms = 0;
        RCHK(hipEventElapsedTime(&ms, e0, e1));
        *kernel_ms = ms;
    }
done:
    hipFree(d_src);
    hipFree(d_dst);
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
    if (s) hipStreamDestroy(s);
    return rc;
}

extern "C" int sift3d_resample_affine_dev(sift3d_ctx *c, const float *d_src, int64_t nx, int64_t ny, int64_t nz, float *d_dst, int64_t ox,
                                          int64_t oy, int64_t oz, const float map[12], int interp, float fill)
{
    if (!c) return SIFT3D_ERR_ARG;
    const char *why = check_args(d_src, nx, ny, nz, d_dst, ox, oy, oz, map, interp);
    if (why) return set_err(c, SIFT3D_ERR_ARG, "sift3d_resample_affine_dev: %s", why);
    HIPCHK(c, hipSetDevice(c->device));
    int rc = fence_in(c);
    if (rc) return rc;
    HIPCHK(c, sift3d_launch_resample(c->stream, d_src, nx, ny, nz, d_dst, ox, oy, oz, map, interp == SIFT3D_INTERP_NEAREST, fill));
    return fence_out(c);
}
