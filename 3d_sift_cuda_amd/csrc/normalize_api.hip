/*
 * normalize_api.hip -- C-ABI of the intensity matching (include/sift3d.h, "intensity matching of a registered image"; DESIGN.md
 * section 7s): sift3d_overlap_histograms, sift3d_apply_transfer and the stage sift3d_normalize_intensity.  The kernels are in
 * kernels_normalize.hip; the parameters, the transfer table and the report's text are host code (normalize_host.c); the map is section
 * 7c's and 7e's (sift3d_resample_map, sift3d_field_warp_terms), the checks of a field field_call.h's.  Every volume goes to the device
 * once.
 */
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "field_call.h"

int sift3d_normalize_words(void);
hipError_t sift3d_launch_overlap_hist(hipStream_t s, const float *ref, const float *mask, int64_t nx, int64_t ny, int64_t nz, const float *img, int64_t mx,
                                      int64_t my, int64_t mz, const float *map, const float *c, const float *k, const float o[3], float h, const int64_t n[3],
                                      const float4 *nodes, double alo, double ahi, double blo, double bhi, unsigned long long *res);
hipError_t sift3d_launch_transfer_apply(hipStream_t s, const float *in, float *out, int64_t n, const sift3d_transfer *table, const double *knots);

namespace {

const int64_t MAX_EXTENT = 4096, MAX_VOXELS = 1ll << 30;

bool extents_ok(int64_t x, int64_t y, int64_t z) { return x >= 1 && y >= 1 && z >= 1 && x <= MAX_EXTENT && y <= MAX_EXTENT && z <= MAX_EXTENT && x * y * z <= MAX_VOXELS; }

bool range_ok(const float r[2]) { return std::isfinite(r[0]) && std::isfinite(r[1]) && r[1] > r[0]; }

/* what both the kernel's entry point and the stage refuse of the volumes and the map, and the map's terms (map 12, c 12, k 9) */
int check_pair(const float *ref, int64_t nx, int64_t ny, int64_t nz, const float *ref_vox2key, const sift3d_average_image *im, float terms[33], char *err,
               int64_t err_len)
{
    if (!ref || !im || !im->image) return call_fail(err, err_len, SIFT3D_ERR_ARG, "null pointer");
    if (!extents_ok(nx, ny, nz))
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "reference: nx ny nz = %lld %lld %lld: extents 1 .. 4096, at most 2^30 voxels", (long long)nx, (long long)ny,
                         (long long)nz);
    if (!extents_ok(im->nx, im->ny, im->nz))
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "image: nx ny nz = %lld %lld %lld: extents 1 .. 4096, at most 2^30 voxels", (long long)im->nx,
                         (long long)im->ny, (long long)im->nz);
    if (im->field) {
        const char *why = check_field(*im->field);
        if (why) return call_fail(err, err_len, SIFT3D_ERR_ARG, "image: %s", why);
    }
    if (sift3d_resample_map(im->moving_to_fixed, ref_vox2key, im->vox2key, terms) != 0 || sift3d_field_warp_terms(ref_vox2key, im->vox2key, terms + 12, terms + 24) != 0)
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "image: a matrix's last row is not 0 0 0 1, or a matrix is singular");
    return SIFT3D_OK;
}

/* the volumes of a call on the device */
struct device_pair {
    float *ref = nullptr, *mask = nullptr, *img = nullptr;
    float4 *nodes = nullptr;
    unsigned long long *res = nullptr;
    std::vector<float4> packed; /* send_nodes packs into it: it lives until the stream is synchronised */
};

/* allocate and start the copies; 0, or the call's error code */
int send_pair(device_call &dc, device_pair &d, const float *ref, const float *mask, size_t nv, const sift3d_average_image &im)
{
    const size_t nm = (size_t)(im.nx * im.ny * im.nz);
    if (dc.alloc(&d.ref, nv) != hipSuccess || (mask && dc.alloc(&d.mask, nv) != hipSuccess) || dc.alloc(&d.img, nm) != hipSuccess ||
        (im.field && dc.alloc(&d.nodes, (size_t)nodes_of(*im.field)) != hipSuccess) || dc.alloc(&d.res, (size_t)sift3d_normalize_words()) != hipSuccess)
        return dc.no_memory();
    DEVCHK(dc, dc.to_device(d.ref, ref, nv));
    if (mask) DEVCHK(dc, dc.to_device(d.mask, mask, nv));
    DEVCHK(dc, dc.to_device(d.img, im.image, nm));
    if (im.field) DEVCHK(dc, send_nodes(dc, *im.field, d.packed, d.nodes));
    return SIFT3D_OK;
}

/* the result words start at zero: before the first mark, so that the time between the marks is the launch's alone */
hipError_t zero_words(device_call &dc, const device_pair &d) { return hipMemsetAsync(d.res, 0, sizeof(unsigned long long) * (size_t)sift3d_normalize_words(), dc.s); }

int launch_hist(device_call &dc, const device_pair &d, int64_t nx, int64_t ny, int64_t nz, const sift3d_average_image &im, const float terms[33], const float ar[2],
                const float br[2])
{
    static const float zero3[3] = {0, 0, 0};
    static const int64_t two3[3] = {2, 2, 2};
    const sift3d_field *f = im.field;
    DEVCHK(dc, sift3d_launch_overlap_hist(dc.s, d.ref, d.mask, nx, ny, nz, d.img, im.nx, im.ny, im.nz, terms, terms + 12, terms + 24, f ? f->origin : zero3,
                                          f ? f->spacing : 1.0f, f ? f->n : two3, d.nodes, (double)ar[0], (double)ar[1], (double)br[0], (double)br[1], d.res));
    return SIFT3D_OK;
}

void split_words(const std::vector<unsigned long long> &w, int64_t *hist_a, int64_t *hist_b, int64_t *sums, int64_t *counts)
{
    for (int i = 0; i < SIFT3D_NORMALIZE_BINS; i++) {
        hist_a[i] = (int64_t)w[i];
        hist_b[i] = (int64_t)w[SIFT3D_NORMALIZE_BINS + i];
    }
    for (int i = 0; i < SIFT3D_SIMILARITY_SUMS; i++) sums[i] = (int64_t)w[2 * SIFT3D_NORMALIZE_BINS + i];
    for (int i = 0; i < SIFT3D_NORMALIZE_COUNTS; i++) counts[i] = (int64_t)w[2 * SIFT3D_NORMALIZE_BINS + SIFT3D_SIMILARITY_SUMS + i];
}

/* the table's knots to d_knots (3 x 257 doubles) and the launch; `knots` lives until the stream is synchronised */
int launch_apply(device_call &dc, const float *d_in, float *d_out, int64_t n, const sift3d_transfer &t, std::vector<double> &knots, double *d_knots)
{
    knots.assign(3 * SIFT3D_NORMALIZE_MAX_KNOTS, 0.0);
    for (int k = 0; k < t.m; k++) {
        knots[k] = t.xb[k];
        knots[SIFT3D_NORMALIZE_MAX_KNOTS + k] = t.xa[k];
        knots[2 * SIFT3D_NORMALIZE_MAX_KNOTS + k] = t.slope[k];
    }
    DEVCHK(dc, dc.to_device(d_knots, knots.data(), knots.size()));
    DEVCHK(dc, dc.mark(0));
    DEVCHK(dc, sift3d_launch_transfer_apply(dc.s, d_in, d_out, n, &t, d_knots));
    DEVCHK(dc, dc.mark(1));
    return SIFT3D_OK;
}

} // namespace

extern "C" int sift3d_overlap_histograms(int device, const float *ref, int64_t nx, int64_t ny, int64_t nz, const float ref_vox2key[16], const float *mask,
                                         const sift3d_average_image *image, const float ref_range[2], const float image_range[2], int64_t *hist_a,
                                         int64_t *hist_b, int64_t *sums, int64_t *counts, double *kernel_ms, char *err, int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (!ref_range || !image_range || !hist_a || !hist_b || !sums || !counts) return call_fail(err, err_len, SIFT3D_ERR_ARG, "null pointer");
    float terms[33];
    int rc = check_pair(ref, nx, ny, nz, ref_vox2key, image, terms, err, err_len);
    if (rc != SIFT3D_OK) return rc;
    if (!range_ok(ref_range)) return call_fail(err, err_len, SIFT3D_ERR_ARG, "ref_range = %g %g: finite, hi > lo", (double)ref_range[0], (double)ref_range[1]);
    if (!range_ok(image_range)) return call_fail(err, err_len, SIFT3D_ERR_ARG, "image_range = %g %g: finite, hi > lo", (double)image_range[0], (double)image_range[1]);
    device_call dc(err, err_len);
    device_pair d;
    DEVCHK(dc, dc.open(device));
    if ((rc = send_pair(dc, d, ref, mask, (size_t)(nx * ny * nz), *image)) != SIFT3D_OK) return rc;
    DEVCHK(dc, zero_words(dc, d));
    DEVCHK(dc, dc.mark(0));
    if ((rc = launch_hist(dc, d, nx, ny, nz, *image, terms, ref_range, image_range)) != SIFT3D_OK) return rc;
    DEVCHK(dc, dc.mark(1));
    std::vector<unsigned long long> words((size_t)sift3d_normalize_words());
    DEVCHK(dc, dc.download(words.data(), d.res, words.size()));
    DEVCHK(dc, dc.sync());
    DEVCHK(dc, dc.elapsed_ms(kernel_ms));
    split_words(words, hist_a, hist_b, sums, counts);
    return SIFT3D_OK;
}

extern "C" int sift3d_apply_transfer(int device, const float *image, int64_t n, const sift3d_transfer *table, float *out, double *kernel_ms, char *err,
                                     int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (!image || !table || !out) return call_fail(err, err_len, SIFT3D_ERR_ARG, "null pointer");
    if (n < 1 || n > MAX_VOXELS) return call_fail(err, err_len, SIFT3D_ERR_ARG, "n = %lld voxels: 1 .. 2^30", (long long)n);
    char text[256] = "";
    if (sift3d_transfer_check(table, text, sizeof text) != 0) return call_fail(err, err_len, SIFT3D_ERR_ARG, "%s", text);
    device_call dc(err, err_len);
    float *d_in, *d_out;
    double *d_knots;
    std::vector<double> knots;
    DEVCHK(dc, dc.open(device));
    if (dc.alloc(&d_in, (size_t)n) != hipSuccess || dc.alloc(&d_out, (size_t)n) != hipSuccess || dc.alloc(&d_knots, (size_t)3 * SIFT3D_NORMALIZE_MAX_KNOTS) != hipSuccess)
        return dc.no_memory();
    DEVCHK(dc, dc.to_device(d_in, image, (size_t)n));
    const int rc = launch_apply(dc, d_in, d_out, n, *table, knots, d_knots);
    if (rc != SIFT3D_OK) return rc;
    DEVCHK(dc, dc.download(out, d_out, (size_t)n));
    DEVCHK(dc, dc.sync());
    DEVCHK(dc, dc.elapsed_ms(kernel_ms));
    return SIFT3D_OK;
}

extern "C" int sift3d_normalize_intensity(const float *ref, int64_t nx, int64_t ny, int64_t nz, const float ref_vox2key[16], const float *mask,
                                          const sift3d_average_image *image, const sift3d_normalize_params *pp, float *out, sift3d_normalize_report *rep,
                                          char *err, int64_t err_len)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (err && err_len > 0) err[0] = 0;
    if (rep) memset(rep, 0, sizeof *rep);
    sift3d_normalize_params p;
    if (pp) p = *pp;
    else sift3d_normalize_defaults(&p);
    if (!out) return call_fail(err, err_len, SIFT3D_ERR_ARG, "null pointer");
    float terms[33];
    int rc = check_pair(ref, nx, ny, nz, ref_vox2key, image, terms, err, err_len);
    if (rc != SIFT3D_OK) return rc;
    char text[256] = "";
    if (sift3d_normalize_check(&p, text, sizeof text) != 0) return call_fail(err, err_len, SIFT3D_ERR_ARG, "%s", text);
    const int64_t nv = nx * ny * nz, nm = image->nx * image->ny * image->nz;
    float ar[2], br[2];
    if (!sift3d_blockmatch_range(ref, nv, &ar[0], &ar[1])) return call_fail(err, err_len, SIFT3D_ERR_ARG, "reference: no two distinct finite values");
    if (!sift3d_blockmatch_range(image->image, nm, &br[0], &br[1])) return call_fail(err, err_len, SIFT3D_ERR_ARG, "image: no two distinct finite values");

    sift3d_normalize_report local;
    sift3d_normalize_report &r = rep ? *rep : local;
    memset(&r, 0, sizeof r);
    r.mode = p.mode;
    r.knots = p.knots;
    r.reference_voxels = nv;
    r.image_voxels = nm;
    device_call dc(err, err_len);
    device_pair d;
    float *d_out;
    double *d_knots;
    std::vector<double> knots;
    DEVCHK(dc, dc.open(p.device));
    if ((rc = send_pair(dc, d, ref, mask, (size_t)nv, *image)) != SIFT3D_OK) return rc;
    if (dc.alloc(&d_out, (size_t)nm) != hipSuccess || dc.alloc(&d_knots, (size_t)3 * SIFT3D_NORMALIZE_MAX_KNOTS) != hipSuccess) return dc.no_memory();
    DEVCHK(dc, zero_words(dc, d));
    DEVCHK(dc, dc.mark(0));
    if ((rc = launch_hist(dc, d, nx, ny, nz, *image, terms, ar, br)) != SIFT3D_OK) return rc;
    DEVCHK(dc, dc.mark(1));
    std::vector<unsigned long long> words((size_t)sift3d_normalize_words());
    std::vector<int64_t> hist(2 * SIFT3D_NORMALIZE_BINS);
    DEVCHK(dc, dc.download(words.data(), d.res, words.size()));
    DEVCHK(dc, dc.sync());
    DEVCHK(dc, dc.elapsed_ms(&r.hist_ms));
    split_words(words, hist.data(), hist.data() + SIFT3D_NORMALIZE_BINS, r.sums, r.counts);
    if (sift3d_normalize_transfer(p.mode, p.knots, hist.data(), hist.data() + SIFT3D_NORMALIZE_BINS, r.sums, ar, br, &r.table, text, sizeof text) != 0)
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "%s", text);
    if ((rc = launch_apply(dc, d.img, d_out, nm, r.table, knots, d_knots)) != SIFT3D_OK) return rc;
    DEVCHK(dc, dc.download(out, d_out, (size_t)nm));
    DEVCHK(dc, dc.sync());
    DEVCHK(dc, dc.elapsed_ms(&r.apply_ms));
    r.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return SIFT3D_OK;
}
