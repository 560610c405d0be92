/*
 * similarity_api.hip -- C-ABI of the image similarity (include/sift3d.h, "similarity of two images on one grid"; DESIGN.md section
 * 7o): sift3d_joint_histogram and sift3d_image_similarity.  The kernels are in kernels_similarity.hip; the defaults, the check of the
 * parameters, the derived values and the report's text are host code (similarity_host.c), the check of the extents the components'
 * (ccl_host.c), the range the block search's (blockmatch_host.c), the label check the fusion's (fuse_host.c).
 */
#include <cmath>
#include <cstring>
#include <vector>

#include "device_call.h"

int sift3d_similarity_blocks(int64_t n);
int sift3d_similarity_words(int bins, bool labels);
hipError_t sift3d_launch_joint_hist(hipStream_t s, const float *a, const float *b, const float *lab, const unsigned char *slot_of, int64_t n, double alo,
                                    double ahi, double blo, double bhi, int bins, int flush, unsigned long long *res, unsigned *slice_hist,
                                    unsigned long long *slice_sums);

#define SIM_NO_SLOT 0xff

static bool bins_ok(int32_t bins) { return bins == 8 || bins == 16 || bins == 32 || bins == 64; }

/* The volumes to the device, one launch, the result's words back: res holds sift3d_similarity_words(bins, labels != NULL) words.
 * slot_of: SIFT3D_LABEL_COUNT bytes, the slot of every label present (labels given).  The arguments have been checked. */
static int run_joint_hist(int device, const float *a, const float *b, const float *labels, const unsigned char *slot_of, int64_t n, const float ar[2],
                          const float br[2], int bins, int flush, unsigned long long *res, double *kernel_ms, char *err, int64_t err_len)
{
    const size_t nv = (size_t)n;
    const int words = sift3d_similarity_words(bins, labels != nullptr), blocks = sift3d_similarity_blocks(n), cells = bins * bins;
    device_call dc(err, err_len);
    float *d_a, *d_b, *d_l = nullptr;
    unsigned char *d_slot = nullptr;
    unsigned long long *d_res, *d_ss = nullptr;
    unsigned *d_sh = nullptr;
    DEVCHK(dc, dc.open(device));
    bool ok = dc.alloc(&d_a, nv) == hipSuccess && dc.alloc(&d_b, nv) == hipSuccess && dc.alloc(&d_res, (size_t)words) == hipSuccess;
    if (ok && labels) ok = dc.alloc(&d_l, nv) == hipSuccess && dc.alloc(&d_slot, SIFT3D_LABEL_COUNT) == hipSuccess;
    if (ok && flush == 0) ok = dc.alloc(&d_sh, (size_t)blocks * cells) == hipSuccess && dc.alloc(&d_ss, (size_t)blocks * (words - cells)) == hipSuccess;
    if (!ok) return dc.no_memory();
    DEVCHK(dc, dc.to_device(d_a, a, nv));
    DEVCHK(dc, dc.to_device(d_b, b, nv));
    if (labels) {
        DEVCHK(dc, dc.to_device(d_l, labels, nv));
        DEVCHK(dc, dc.to_device(d_slot, slot_of, SIFT3D_LABEL_COUNT));
    }
    DEVCHK(dc, dc.mark(0));
    DEVCHK(dc, sift3d_launch_joint_hist(dc.s, d_a, d_b, d_l, d_slot, n, (double)ar[0], (double)ar[1], (double)br[0], (double)br[1], bins, flush, d_res, d_sh,
                                        d_ss));
    DEVCHK(dc, dc.mark(1));
    DEVCHK(dc, dc.download(res, d_res, (size_t)words));
    DEVCHK(dc, dc.sync());
    DEVCHK(dc, dc.elapsed_ms(kernel_ms));
    return SIFT3D_OK;
}

static int check_range(const char *name, const float r[2], char *err, int64_t err_len)
{
    if (std::isfinite(r[0]) && std::isfinite(r[1]) && r[1] > r[0]) return SIFT3D_OK;
    return call_fail(err, err_len, SIFT3D_ERR_ARG, "%s = %g .. %g: a range is finite with hi > lo", name, (double)r[0], (double)r[1]);
}

extern "C" int sift3d_joint_histogram(int device, const float *a, const float *b, int64_t nx, int64_t ny, int64_t nz, const float a_range[2],
                                      const float b_range[2], int32_t bins, int64_t *hist, int64_t *sums, int64_t *excluded, double *kernel_ms, char *err,
                                      int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (kernel_ms) *kernel_ms = 0.0;
    if (excluded) *excluded = 0;
    if (!a || !b || !a_range || !b_range || !hist || !sums || !excluded) return call_fail(err, err_len, SIFT3D_ERR_ARG, "null pointer");
    if (sift3d_ccl_check_extents(nx, ny, nz, err, err_len) != 0) return SIFT3D_ERR_ARG;
    if (!bins_ok(bins)) return call_fail(err, err_len, SIFT3D_ERR_ARG, "bins = %d: 8, 16, 32 or 64", (int)bins);
    if (check_range("a_range", a_range, err, err_len) != SIFT3D_OK || check_range("b_range", b_range, err, err_len) != SIFT3D_OK) return SIFT3D_ERR_ARG;
    const int64_t n = nx * ny * nz;
    sift3d_similarity_params p;
    sift3d_similarity_defaults(&p);
    std::vector<unsigned long long> res((size_t)sift3d_similarity_words(bins, false));
    const int rc = run_joint_hist(device, a, b, nullptr, nullptr, n, a_range, b_range, bins, p.flush, res.data(), kernel_ms, err, err_len);
    if (rc != SIFT3D_OK) return rc;
    const int cells = bins * bins;
    for (int c = 0; c < cells; c++) hist[c] = (int64_t)res[(size_t)c];
    for (int j = 0; j < SIFT3D_SIMILARITY_SUMS; j++) sums[j] = (int64_t)res[(size_t)(cells + j)];
    *excluded = n - sums[0];
    return SIFT3D_OK;
}

extern "C" int sift3d_image_similarity(const float *a, const float *b, const float *labels, int64_t nx, int64_t ny, int64_t nz,
                                       const sift3d_similarity_params *pp, sift3d_similarity_record *record, sift3d_similarity_label_record *label_records,
                                       int32_t *n_labels, char *err, int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (record) memset(record, 0, sizeof *record);
    if (n_labels) *n_labels = 0;
    sift3d_similarity_params p;
    if (pp) p = *pp;
    else sift3d_similarity_defaults(&p);
    if (!a || !b || !record || (labels && (!label_records || !n_labels))) return call_fail(err, err_len, SIFT3D_ERR_ARG, "null pointer");
    if (sift3d_ccl_check_extents(nx, ny, nz, err, err_len) != 0) return SIFT3D_ERR_ARG;
    if (sift3d_similarity_check(&p, err, err_len) != 0) return SIFT3D_ERR_ARG;
    const int64_t n = nx * ny * nz;
    if (labels && check_labels("", labels, n, err, err_len) != SIFT3D_OK) return SIFT3D_ERR_ARG;
    float ar[2] = {0, 0}, br[2] = {0, 0};
    int empty = sift3d_blockmatch_range(a, n, &ar[0], &ar[1]) ? 0 : 1;
    if (p.same_scale) {
        br[0] = ar[0];
        br[1] = ar[1];
    } else if (!sift3d_blockmatch_range(b, n, &br[0], &br[1])) {
        empty |= 2;
    }
    record->empty_range = empty;
    record->a_lo = ar[0];
    record->a_hi = ar[1];
    record->b_lo = br[0];
    record->b_hi = br[1];
    const int cells = p.bins * p.bins;
    if (empty) { /* no voxel counts and nothing is launched */
        record->excluded = n;
        sift3d_similarity_measures(record->hist, p.bins, record->sums, ar[0], ar[1], p.same_scale, record);
        return SIFT3D_OK;
    }
    /* the labels on counted voxels, in ascending order, and the slot of each among them */
    std::vector<unsigned char> slot_of;
    std::vector<int> present;
    if (labels) {
        std::vector<unsigned char> seen(SIFT3D_LABEL_COUNT, 0);
        for (int64_t i = 0; i < n; i++)
            if (std::isfinite(labels[i]) && std::isfinite(a[i]) && std::isfinite(b[i])) seen[(int)labels[i]] = 1;
        for (int l = 0; l < SIFT3D_LABEL_COUNT; l++)
            if (seen[l]) present.push_back(l);
        if ((int64_t)present.size() > p.max_labels)
            return call_fail(err, err_len, SIFT3D_ERR_ARG, "%lld labels on counted voxels: more than max_labels = %d (nothing is dropped)",
                             (long long)present.size(), (int)p.max_labels);
        slot_of.assign(SIFT3D_LABEL_COUNT, SIM_NO_SLOT);
        for (size_t k = 0; k < present.size(); k++) slot_of[(size_t)present[k]] = (unsigned char)k;
    }
    std::vector<unsigned long long> res((size_t)sift3d_similarity_words(p.bins, labels != nullptr));
    const int rc = run_joint_hist(p.device, a, b, labels, labels ? slot_of.data() : nullptr, n, ar, br, p.bins, p.flush, res.data(), &record->kernel_ms, err, err_len);
    if (rc != SIFT3D_OK) return rc;
    int64_t sums[SIFT3D_SIMILARITY_SUMS];
    for (int c = 0; c < cells; c++) record->hist[c] = (int64_t)res[(size_t)c];
    for (int j = 0; j < SIFT3D_SIMILARITY_SUMS; j++) sums[j] = (int64_t)res[(size_t)(cells + j)];
    record->excluded = n - sums[0];
    sift3d_similarity_measures(record->hist, p.bins, sums, ar[0], ar[1], p.same_scale, record);
    for (size_t k = 0; k < present.size(); k++) {
        int64_t ls[SIFT3D_SIMILARITY_SUMS];
        for (int j = 0; j < SIFT3D_SIMILARITY_SUMS; j++) ls[j] = (int64_t)res[(size_t)cells + SIFT3D_SIMILARITY_SUMS * (k + 1) + (size_t)j];
        sift3d_similarity_label_measures(present[k], ls, ar[0], ar[1], p.same_scale, &label_records[k]);
    }
    if (n_labels) *n_labels = (int32_t)present.size();
    return SIFT3D_OK;
}
