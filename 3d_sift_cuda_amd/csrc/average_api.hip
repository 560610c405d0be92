/*
 * average_api.hip -- C-ABI of the template from warped images (include/sift3d.h, "a template from up to 32 warped images";
 * DESIGN.md section 7r): sift3d_average_warped.  The kernel is in kernels_average.hip; the parameters, their check, the report's
 * counts and its text are host code (average_host.c); the maps are section 7c's and 7e's (sift3d_resample_map,
 * sift3d_field_warp_terms), the checks of a field and of the extents field_call.h's.  Every image goes to the device once and
 * stays there for the one launch.
 */
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "field_call.h"

size_t sift3d_average_image_bytes(void);
void sift3d_average_fill_image(void *at, const float *d_src, int64_t nx, int64_t ny, int64_t nz, const float *map, const float *c, const float *k, bool has_field,
                               const float o[3], float h, const int64_t n[3], const float4 *d_nodes);
hipError_t sift3d_launch_average(hipStream_t s, const void *images, int K, int trim, int min_count, float fill, int64_t ox, int64_t oy, int64_t oz,
                                 float *avg, float *var, unsigned *mask);

extern "C" int sift3d_average_warped(int64_t nx, int64_t ny, int64_t nz, const float grid_vox2key[16], int32_t K, const sift3d_average_image *images,
                                     const sift3d_average_params *pp, float *avg, float *var, uint32_t *mask, sift3d_average_report *rep, char *err,
                                     int64_t err_len)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (err && err_len > 0) err[0] = 0;
    if (rep) memset(rep, 0, sizeof *rep);
    sift3d_average_params p;
    if (pp) p = *pp;
    else sift3d_average_defaults(&p);
    if (K < 1 || K > SIFT3D_AVERAGE_MAX_IMAGES) return call_fail(err, err_len, SIFT3D_ERR_ARG, "K = %d images: 1 .. %d", (int)K, SIFT3D_AVERAGE_MAX_IMAGES);
    if (!images || !avg || !var || !mask) return call_fail(err, err_len, SIFT3D_ERR_ARG, "null pointer");
    const char *why = check_source_extents(nx, ny, nz);
    if (why) return call_fail(err, err_len, SIFT3D_ERR_ARG, "grid: nx ny nz = %lld %lld %lld: extents must be 1 .. 2^24", (long long)nx, (long long)ny, (long long)nz);
    if (nx * ny > (1ll << 40) / nz) return call_fail(err, err_len, SIFT3D_ERR_ARG, "grid: more than 2^40 voxels");
    char text[256] = "";
    if (sift3d_average_check(&p, K, text, sizeof text) != 0) return call_fail(err, err_len, SIFT3D_ERR_ARG, "%s", text);
    std::vector<float> terms((size_t)K * 33); /* per image: map 12, c 12, k 9 */
    int64_t sources = 0;
    for (int k = 0; k < K; k++) {
        const sift3d_average_image &a = images[k];
        if (!a.image) return call_fail(err, err_len, SIFT3D_ERR_ARG, "image %d: null pointer", k);
        why = check_source_extents(a.nx, a.ny, a.nz);
        if (!why && a.nx * a.ny > (1ll << 38) / a.nz) why = "volume larger than 2^38 voxels";
        if (!why && a.field) why = check_field(*a.field);
        if (why) return call_fail(err, err_len, SIFT3D_ERR_ARG, "image %d: %s", k, why);
        float *t = terms.data() + (size_t)k * 33;
        if (sift3d_resample_map(a.moving_to_fixed, grid_vox2key, a.vox2key, t) != 0 || sift3d_field_warp_terms(grid_vox2key, a.vox2key, t + 12, t + 24) != 0)
            return call_fail(err, err_len, SIFT3D_ERR_ARG, "image %d: a matrix's last row is not 0 0 0 1, or a matrix is singular", k);
        sources += a.nx * a.ny * a.nz;
        if (sources > p.max_voxels)
            return call_fail(err, err_len, SIFT3D_ERR_ARG, "image %d: the source voxels up to it, %lld, exceed max_voxels = %lld", k, (long long)sources,
                             (long long)p.max_voxels);
    }
    sift3d_average_report rp;
    memset(&rp, 0, sizeof rp);
    const size_t nv = (size_t)(nx * ny * nz), desc = sift3d_average_image_bytes();
    std::vector<unsigned char> host_desc(desc * (size_t)K);
    std::vector<float4> nodes; /* send_nodes packs into it: it lives until the stream is synchronised */
    device_call dc(err, err_len);
    float *d_avg, *d_var;
    unsigned *d_mask;
    unsigned char *d_desc;
    DEVCHK(dc, dc.open(p.device));
    if (dc.alloc(&d_avg, nv) != hipSuccess || dc.alloc(&d_var, nv) != hipSuccess || dc.alloc(&d_mask, nv) != hipSuccess ||
        dc.alloc(&d_desc, host_desc.size()) != hipSuccess)
        return dc.no_memory();
    for (int k = 0; k < K; k++) {
        const sift3d_average_image &a = images[k];
        const size_t nm = (size_t)(a.nx * a.ny * a.nz);
        float *d_src;
        float4 *d_nodes = nullptr;
        if (dc.alloc(&d_src, nm) != hipSuccess || (a.field && dc.alloc(&d_nodes, (size_t)nodes_of(*a.field)) != hipSuccess))
            return dc.no_memory(": image %d of %d", k, (int)K);
        DEVCHK(dc, dc.mark(0));
        DEVCHK(dc, dc.to_device(d_src, a.image, nm));
        if (a.field) DEVCHK(dc, send_nodes(dc, *a.field, nodes, d_nodes));
        DEVCHK(dc, dc.mark(1));
        DEVCHK(dc, dc.sync());
        DEVCHK(dc, dc.elapsed_ms(&rp.image[k].upload_ms));
        const float *t = terms.data() + (size_t)k * 33;
        static const float zero3[3] = {0, 0, 0};
        static const int64_t two3[3] = {2, 2, 2};
        sift3d_average_fill_image(host_desc.data() + desc * (size_t)k, d_src, a.nx, a.ny, a.nz, t, t + 12, t + 24, a.field != nullptr,
                                  a.field ? a.field->origin : zero3, a.field ? a.field->spacing : 1.0f, a.field ? a.field->n : two3, d_nodes);
    }
    DEVCHK(dc, dc.to_device(d_desc, host_desc.data(), host_desc.size()));
    DEVCHK(dc, dc.mark(0));
    DEVCHK(dc, sift3d_launch_average(dc.s, d_desc, K, p.trim, p.min_count, p.fill, nx, ny, nz, d_avg, d_var, d_mask));
    DEVCHK(dc, dc.mark(1));
    DEVCHK(dc, dc.download(avg, d_avg, nv));
    DEVCHK(dc, dc.download(var, d_var, nv));
    DEVCHK(dc, dc.download((unsigned *)mask, d_mask, nv));
    DEVCHK(dc, dc.sync());
    DEVCHK(dc, dc.elapsed_ms(&rp.kernel_ms));
    if (sift3d_average_counts(mask, (int64_t)nv, K, p.trim, p.min_count, &rp) != 0)
        return call_fail(err, err_len, SIFT3D_ERR_DEVICE, "the mask plane holds a bit of an image that was not given");
    rp.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rep) *rep = rp;
    return SIFT3D_OK;
}
