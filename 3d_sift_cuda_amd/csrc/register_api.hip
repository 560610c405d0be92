/*
 * register_api.hip -- C-ABI of the affine registration by mutual information (include/sift3d.h, "affine registration by mutual
 * information"): sift3d_warp_histogram and sift3d_register_affine.  The kernels are in kernels_register.hip;
 * the parameters, the transform family, the candidates and the report's text are host code (register_host.c), the scores the
 * similarity's (similarity_host.c), the check of the extents the components' (ccl_host.c), the ranges the block search's
 * (blockmatch_host.c).  One device session serves every launch of a call: the images go to the device once.
 */
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "device_call.h"

int sift3d_register_words(int bins);
hipError_t sift3d_launch_register_plane(hipStream_t s, const float *f, int64_t nx, int64_t ny, int64_t lx, int64_t ly, int64_t lz, int stride, double lo,
                                        double hi, short *plane);
hipError_t sift3d_launch_warp_hist(hipStream_t s, const float *f, const short *plane, const float *mov, const float *maps, int n_maps, int by_map,
                                   int64_t nx, int64_t ny, int64_t lx, int64_t ly, int64_t lz, int stride, int64_t mx, int64_t my, int64_t mz, double flo,
                                   double fhi, double mlo, double mhi, int bins, unsigned long long *res);

/* the form a call runs where the caller leaves it open: DESIGN.md section 7q has the times of all four */
#define REG_DEFAULT_FORM 0

static bool bins_ok(int32_t bins) { return bins == 8 || bins == 16 || bins == 32 || bins == 64; }
static bool stride_ok(int32_t s) { return s == 1 || s == 2 || s == 4 || s == 8; }

static int check_range(const char *name, const float r[2], char *err, int64_t err_len)
{
    if (std::isfinite(r[0]) && std::isfinite(r[1]) && r[1] > r[0]) return SIFT3D_OK;
    return call_fail(err, err_len, SIFT3D_ERR_ARG, "%s = %g .. %g: a range is finite with hi > lo", name, (double)r[0], (double)r[1]);
}

/* the extents of one image, with its name before sift3d_ccl_check_extents' text */
static int check_image(const char *name, int64_t nx, int64_t ny, int64_t nz, char *err, int64_t err_len)
{
    char text[256] = "";
    if (sift3d_ccl_check_extents(nx, ny, nz, text, sizeof text) == 0) return SIFT3D_OK;
    return call_fail(err, err_len, SIFT3D_ERR_ARG, "%s: %s", name, text);
}

/* what a call holds on the device: both images, the maps of a launch, the result words and, under the plane form, F's lattice plane */
struct reg_session {
    device_call dc;
    const int64_t nx, ny, nz, mx, my, mz;
    const float *fr, *mr;
    const int bins, form, words;
    float *d_f = nullptr, *d_m = nullptr, *d_maps = nullptr;
    short *d_plane = nullptr;
    unsigned long long *d_res = nullptr;
    int plane_stride = 0;

    reg_session(char *err, int64_t err_len, int64_t nx_, int64_t ny_, int64_t nz_, int64_t mx_, int64_t my_, int64_t mz_, const float *fr_, const float *mr_,
                int bins_, int form_)
        : dc(err, err_len), nx(nx_), ny(ny_), nz(nz_), mx(mx_), my(my_), mz(mz_), fr(fr_), mr(mr_), bins(bins_),
          form(form_ == SIFT3D_REGISTER_FORM_DEFAULT ? REG_DEFAULT_FORM : form_), words(sift3d_register_words(bins_))
    {
    }

    /* every buffer of the call, for lattices of min_stride and coarser, and the images */
    int open(int device, const float *f, const float *m, int min_stride)
    {
        const size_t nf = (size_t)(nx * ny * nz), nm = (size_t)(mx * my * mz);
        DEVCHK(dc, dc.open(device));
        bool ok = dc.alloc(&d_f, nf) == hipSuccess && dc.alloc(&d_m, nm) == hipSuccess && dc.alloc(&d_maps, (size_t)SIFT3D_REGISTER_MAX_MAPS * 12) == hipSuccess &&
                  dc.alloc(&d_res, (size_t)SIFT3D_REGISTER_MAX_MAPS * (size_t)words) == hipSuccess;
        if (ok && (form & SIFT3D_REGISTER_FORM_PLANE))
            ok = dc.alloc(&d_plane, (size_t)sift3d_register_lattice(nx, ny, nz, min_stride, nullptr, nullptr, nullptr, nullptr)) == hipSuccess;
        if (!ok) return dc.no_memory();
        DEVCHK(dc, dc.to_device(d_f, f, nf));
        DEVCHK(dc, dc.to_device(d_m, m, nm));
        return SIFT3D_OK;
    }

    /* one launch: K maps at a stride; res: K x words; *ms is increased by the device time of the launches */
    int run(int stride, const float *maps, int K, unsigned long long *res, double *ms)
    {
        int64_t l[3];
        sift3d_register_lattice(nx, ny, nz, stride, nullptr, l, nullptr, nullptr);
        DEVCHK(dc, dc.to_device(d_maps, maps, (size_t)K * 12));
        DEVCHK(dc, dc.mark(0));
        if (d_plane && plane_stride != stride) {
            DEVCHK(dc, sift3d_launch_register_plane(dc.s, d_f, nx, ny, l[0], l[1], l[2], stride, (double)fr[0], (double)fr[1], d_plane));
            plane_stride = stride;
        }
        DEVCHK(dc, sift3d_launch_warp_hist(dc.s, d_f, d_plane, d_m, d_maps, K, form & SIFT3D_REGISTER_FORM_BY_MAP, nx, ny, l[0], l[1], l[2], stride, mx, my, mz,
                                           (double)fr[0], (double)fr[1], (double)mr[0], (double)mr[1], bins, d_res));
        DEVCHK(dc, dc.mark(1));
        DEVCHK(dc, dc.download(res, d_res, (size_t)K * (size_t)words));
        DEVCHK(dc, dc.sync());
        double t = 0.0;
        DEVCHK(dc, dc.elapsed_ms(&t));
        if (ms) *ms += t;
        return SIFT3D_OK;
    }
};

static bool form_ok(int32_t form) { return form == SIFT3D_REGISTER_FORM_DEFAULT || (form >= 0 && form <= (SIFT3D_REGISTER_FORM_BY_MAP | SIFT3D_REGISTER_FORM_PLANE)); }

extern "C" int sift3d_warp_histogram(int device, const float *fixed, int64_t nx, int64_t ny, int64_t nz, const float *moving, int64_t mx, int64_t my,
                                     int64_t mz, const float *maps, int32_t n_maps, int32_t stride, const float fixed_range[2],
                                     const float moving_range[2], int32_t bins, int32_t form, int64_t *hist, int64_t *sums, int64_t *excluded,
                                     int64_t *outside, double *kernel_ms, char *err, int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (kernel_ms) *kernel_ms = 0.0;
    if (!fixed || !moving || !maps || !fixed_range || !moving_range || !hist || !sums || !excluded || !outside)
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "null pointer");
    if (check_image("fixed", nx, ny, nz, err, err_len) != SIFT3D_OK || check_image("moving", mx, my, mz, err, err_len) != SIFT3D_OK) return SIFT3D_ERR_ARG;
    if (!bins_ok(bins)) return call_fail(err, err_len, SIFT3D_ERR_ARG, "bins = %d: 8, 16, 32 or 64", (int)bins);
    if (!stride_ok(stride)) return call_fail(err, err_len, SIFT3D_ERR_ARG, "stride = %d: 1, 2, 4 or 8", (int)stride);
    if (n_maps < 1 || n_maps > SIFT3D_REGISTER_MAX_MAPS) return call_fail(err, err_len, SIFT3D_ERR_ARG, "n_maps = %d: 1 .. %d", (int)n_maps, SIFT3D_REGISTER_MAX_MAPS);
    if (check_range("fixed_range", fixed_range, err, err_len) != SIFT3D_OK || check_range("moving_range", moving_range, err, err_len) != SIFT3D_OK)
        return SIFT3D_ERR_ARG;
    if (!form_ok(form)) return call_fail(err, err_len, SIFT3D_ERR_ARG, "form = %d: -1 or 0 .. 3", (int)form);
    reg_session S(err, err_len, nx, ny, nz, mx, my, mz, fixed_range, moving_range, bins, form);
    int rc = S.open(device, fixed, moving, stride);
    if (rc != SIFT3D_OK) return rc;
    std::vector<unsigned long long> res((size_t)n_maps * (size_t)S.words);
    if ((rc = S.run(stride, maps, n_maps, res.data(), kernel_ms)) != SIFT3D_OK) return rc;
    const int64_t N = sift3d_register_lattice(nx, ny, nz, stride, nullptr, nullptr, nullptr, nullptr);
    const int cells = bins * bins;
    for (int k = 0; k < n_maps; k++) {
        const unsigned long long *w = res.data() + (size_t)k * (size_t)S.words;
        for (int c = 0; c < cells; c++) hist[(size_t)k * cells + c] = (int64_t)w[c];
        for (int j = 0; j < SIFT3D_SIMILARITY_SUMS; j++) sums[k * SIFT3D_SIMILARITY_SUMS + j] = (int64_t)w[cells + j];
        excluded[k] = N - (int64_t)w[cells];
        outside[k] = (int64_t)w[cells + SIFT3D_SIMILARITY_SUMS];
    }
    return SIFT3D_OK;
}

/* the score of one map's words and whether it is admissible; rec is scratch */
static double score_of(const unsigned long long *w, int bins, int metric, double min_overlap, int64_t N, sift3d_similarity_record *rec, std::vector<int64_t> &hist,
                       bool *admissible, int64_t *n)
{
    const int cells = bins * bins;
    int64_t sums[SIFT3D_SIMILARITY_SUMS];
    for (int c = 0; c < cells; c++) hist[(size_t)c] = (int64_t)w[c];
    for (int j = 0; j < SIFT3D_SIMILARITY_SUMS; j++) sums[j] = (int64_t)w[cells + j];
    sift3d_similarity_measures(hist.data(), bins, sums, 0.0f, 1.0f, 0, rec);
    const double score = metric == SIFT3D_REGISTER_METRIC_MI ? rec->mi : rec->nmi;
    *n = sums[0];
    *admissible = !std::isnan(score) && (double)sums[0] >= min_overlap * (double)N;
    return score;
}

/* a map's words as the full record of the similarity section */
static void fill_record(const unsigned long long *w, int bins, int64_t N, const float fr[2], const float mr[2], double ms, sift3d_similarity_record *rec,
                        int64_t *outside)
{
    const int cells = bins * bins;
    int64_t sums[SIFT3D_SIMILARITY_SUMS];
    memset(rec, 0, sizeof *rec);
    for (int c = 0; c < cells; c++) rec->hist[c] = (int64_t)w[c];
    for (int j = 0; j < SIFT3D_SIMILARITY_SUMS; j++) sums[j] = (int64_t)w[cells + j];
    sift3d_similarity_measures(rec->hist, bins, sums, fr[0], fr[1], 0, rec);
    rec->a_lo = fr[0];
    rec->a_hi = fr[1];
    rec->b_lo = mr[0];
    rec->b_hi = mr[1];
    rec->excluded = N - sums[0];
    rec->kernel_ms = ms;
    *outside = (int64_t)w[cells + SIFT3D_SIMILARITY_SUMS];
}

extern "C" int sift3d_register_affine(const float *fixed, int64_t nx, int64_t ny, int64_t nz, const float *moving, int64_t mx, int64_t my, int64_t mz,
                                      const float fixed_vox2key[16], const float moving_vox2key[16], const float initial[16],
                                      const sift3d_register_params *pp, sift3d_register_report *rep, char *err, int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (rep) memset(rep, 0, sizeof *rep);
    sift3d_register_params p;
    if (pp) p = *pp;
    else sift3d_register_defaults(&p);
    if (!fixed || !moving || !rep) return call_fail(err, err_len, SIFT3D_ERR_ARG, "null pointer");
    if (check_image("fixed", nx, ny, nz, err, err_len) != SIFT3D_OK || check_image("moving", mx, my, mz, err, err_len) != SIFT3D_OK) return SIFT3D_ERR_ARG;
    if (sift3d_register_check(&p, err, err_len) != 0) return SIFT3D_ERR_ARG;
    double theta[SIFT3D_REGISTER_THETA] = {0}, h = 0.0, rho = 0.0;
    float maps[SIFT3D_REGISTER_MAX_MAPS * 12];
    if (sift3d_register_lattice(nx, ny, nz, 1, fixed_vox2key, nullptr, &h, &rho) < 0 ||
        sift3d_register_map(theta, nx, ny, nz, fixed_vox2key, moving_vox2key, initial, maps) != 0)
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "a matrix is singular, not finite or its last row is not 0 0 0 1");
    float fr[2] = {0, 0}, mr[2] = {0, 0};
    if (!sift3d_blockmatch_range(fixed, nx * ny * nz, &fr[0], &fr[1]))
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "the fixed image has no two distinct finite values: there is nothing to register");
    if (!sift3d_blockmatch_range(moving, mx * my * mz, &mr[0], &mr[1]))
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "the moving image has no two distinct finite values: there is nothing to register");
    rep->dof = p.dof;
    rep->metric = p.metric;
    rep->bins = p.bins;
    rep->n_levels = p.n_levels;
    rep->h = h;
    rep->rho = rho;

    reg_session S(err, err_len, nx, ny, nz, mx, my, mz, fr, mr, p.bins, p.form);
    int rc = S.open(p.device, fixed, moving, 1);
    if (rc != SIFT3D_OK) return rc;
    std::vector<unsigned long long> res((size_t)SIFT3D_REGISTER_MAX_MAPS * (size_t)S.words);
    std::vector<int64_t> hist((size_t)(p.bins * p.bins));
    std::unique_ptr<sift3d_similarity_record> scratch(new sift3d_similarity_record);
    double cand[2 * SIFT3D_REGISTER_THETA * SIFT3D_REGISTER_THETA];

    for (int l = 0; l < p.n_levels; l++) {
        sift3d_register_level &lv = rep->level[l];
        const int stride = p.stride[l];
        const int64_t N = sift3d_register_lattice(nx, ny, nz, stride, nullptr, nullptr, nullptr, nullptr);
        lv.stride = stride;
        lv.n_lattice = N;
        /* theta on this level's lattice */
        if (sift3d_register_map(theta, nx, ny, nz, fixed_vox2key, moving_vox2key, initial, maps) != 0)
            return call_fail(err, err_len, SIFT3D_ERR_ARG, "level %d: the transform reached has no finite map", l);
        if ((rc = S.run(stride, maps, 1, res.data(), &lv.device_ms)) != SIFT3D_OK) return rc;
        lv.evaluations = 1;
        bool ok;
        int64_t n;
        double cur = score_of(res.data(), p.bins, p.metric, p.min_overlap, N, scratch.get(), hist, &ok, &n);
        if (l == 0 && !ok)
            return call_fail(err, err_len, SIFT3D_ERR_ARG, "the start is inadmissible: n = %lld of N = %lld lattice voxels count, min_overlap = %g", (long long)n,
                             (long long)N, p.min_overlap);
        if (!ok) cur = -INFINITY; /* any admissible candidate is better */
        lv.score_in = cur;
        double u = p.first_step[l] * h;
        const double last = p.last_step[l] * h;
        while (lv.iterations < p.max_iterations && !(u < last)) {
            const int K = sift3d_register_candidates(theta, p.dof, u, rho, cand);
            for (int c = 0; c < K; c++)
                if (sift3d_register_map(cand + c * SIFT3D_REGISTER_THETA, nx, ny, nz, fixed_vox2key, moving_vox2key, initial, maps + c * 12) != 0)
                    for (int e = 0; e < 12; e++) maps[c * 12 + e] = NAN; /* every voxel outside: n = 0, inadmissible */
            if ((rc = S.run(stride, maps, K, res.data(), &lv.device_ms)) != SIFT3D_OK) return rc;
            lv.iterations++;
            lv.evaluations += K;
            int best = -1;
            double best_score = 0.0;
            for (int c = 0; c < K; c++) {
                const double sc = score_of(res.data() + (size_t)c * (size_t)S.words, p.bins, p.metric, p.min_overlap, N, scratch.get(), hist, &ok, &n);
                if (ok && (best < 0 || sc > best_score)) {
                    best = c;
                    best_score = sc;
                }
            }
            if (best >= 0 && best_score > cur) {
                memcpy(theta, cand + best * SIFT3D_REGISTER_THETA, sizeof theta);
                cur = best_score;
            } else {
                u = u / 2.0;
            }
        }
        lv.stop = u < last ? 0 : 1;
        if (lv.stop) rep->stop = 1;
        lv.score_out = cur;
        lv.last_step = u;
    }
    memcpy(rep->theta, theta, sizeof theta);
    const double zero[SIFT3D_REGISTER_THETA] = {0};
    if (sift3d_register_result(theta, nx, ny, nz, fixed_vox2key, initial, rep->result) != 0 ||
        sift3d_register_map(zero, nx, ny, nz, fixed_vox2key, moving_vox2key, initial, maps) != 0 ||
        sift3d_register_map(theta, nx, ny, nz, fixed_vox2key, moving_vox2key, initial, maps + 12) != 0)
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "the transform reached has no finite matrix");
    memcpy(rep->map, maps + 12, sizeof rep->map);
    double ms = 0.0;
    if ((rc = S.run(1, maps, 2, res.data(), &ms)) != SIFT3D_OK) return rc;
    const int64_t N1 = nx * ny * nz;
    fill_record(res.data(), p.bins, N1, fr, mr, ms, &rep->before, &rep->outside_before);
    fill_record(res.data() + S.words, p.bins, N1, fr, mr, ms, &rep->after, &rep->outside_after);
    return SIFT3D_OK;
}
