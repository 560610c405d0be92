/*
 * resample_api.hip -- C-ABI of featResample's resampler (include/sift3d.h, "resampling"):
 * sift3d_resample_affine on host arrays and sift3d_resample_affine_dev on device buffers, on a context's stream.  The
 * kernel is in kernels_resample.hip; the map comes from sift3d_resample_map (align_host.c).
 */
#include "field_call.h"
#include "pipeline.h"

/* NULL when the arguments are usable, else the reason */
static const char *check_args(const float *src, int64_t nx, int64_t ny, int64_t nz, const float *dst, int64_t ox, int64_t oy, int64_t oz,
                              const float *map, int interp)
{
    if (!src || !dst || !map) return "null pointer";
    if (interp != SIFT3D_INTERP_LINEAR && interp != SIFT3D_INTERP_NEAREST && interp != SIFT3D_INTERP_LABEL)
        return "interp must be SIFT3D_INTERP_LINEAR, SIFT3D_INTERP_NEAREST or SIFT3D_INTERP_LABEL";
    const char *why = check_source_extents(nx, ny, nz);
    return why ? why : check_output_extents(ox, oy, oz);
}

extern "C" int sift3d_resample_affine(int device, const float *src, int64_t nx, int64_t ny, int64_t nz, float *dst, int64_t ox, int64_t oy,
                                      int64_t oz, const float map[12], int interp, float fill, double *kernel_ms, char *err, int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (kernel_ms) *kernel_ms = 0.0;
    const char *why = check_args(src, nx, ny, nz, dst, ox, oy, oz, map, interp);
    if (why) return call_fail(err, err_len, SIFT3D_ERR_ARG, "%s", why);
    const size_t n_in = (size_t)(nx * ny * nz), n_out = (size_t)(ox * oy * oz);
    device_call dc(err, err_len);
    float *d_src, *d_dst;
    DEVCHK(dc, dc.open(device));
    if (dc.alloc(&d_src, n_in) != hipSuccess || dc.alloc(&d_dst, n_out) != hipSuccess) return dc.no_memory();
    DEVCHK(dc, dc.to_device(d_src, src, n_in));
    DEVCHK(dc, dc.mark(0));
    DEVCHK(dc, sift3d_launch_resample(dc.s, d_src, nx, ny, nz, d_dst, ox, oy, oz, map, interp, fill));
    DEVCHK(dc, dc.mark(1));
    DEVCHK(dc, dc.download(dst, d_dst, n_out));
    DEVCHK(dc, dc.sync());
    DEVCHK(dc, dc.elapsed_ms(kernel_ms));
    return SIFT3D_OK;
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
    HIPCHK(c, sift3d_launch_resample(c->stream, d_src, nx, ny, nz, d_dst, ox, oy, oz, map, interp, fill));
    return fence_out(c);
}
