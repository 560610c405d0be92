/*
 * field_api.hip -- C-ABI of the nonrigid alignment (include/sift3d.h, "nonrigid alignment"):
 * sift3d_fit_field, sift3d_refine_field and sift3d_resample_field.  The kernels are in kernels_field.hip; the grid, the
 * samples, the interpolation and the fold count are host arithmetic (field_host.c), the search is sift3d_guided_search's and
 * the accept rule the similarity loop's (guided_accept.h).
 */
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "field_call.h"
#include "guided_accept.h"

hipError_t sift3d_launch_field_fit(hipStream_t s, const float4 *ys, const float4 *vs, const int *start, const double co[3], double edge,
                                   const long long cn[3], const float o[3], float h, const int64_t n[3], float rr, double lam24, float *out);

static bool finite6(const float *y, const float *v)
{
    return std::isfinite(y[0]) && std::isfinite(y[1]) && std::isfinite(y[2]) && std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]);
}

/* NULL when every finite sample is within the bound, else the reason */
static const char *check_samples(const float *v, int64_t n)
{
    for (int64_t i = 0; i < 3 * n; i++)
        if (std::isfinite(v[i]) && !(std::fabs(v[i]) <= SIFT3D_FIELD_MAX_DISP)) return "a sample's |v| exceeds SIFT3D_FIELD_MAX_DISP (128 key units)";
    return nullptr;
}

/* One fit on the grid g (n, origin, spacing) into disp (3 N floats, host).  The finite samples (all six components) are
 * binned into a uniform grid of cells of edge R (1 + 2^-10) over their bounding box, widened until an axis has at most 2^20
 * cells and the grid at most 2^24: a passing sample is less than R from the node on every axis (plus float rounding, which
 * the margin covers), so the 27 cells around the node's cell hold it.  Shared with blockmatch_api.hip (declared in
 * field_call.h). */
int fit_on_grid(device_call &dc, const float *y, const float *v, int64_t n, const sift3d_field &g, float R, float lambda, float *disp,
                       double *kernel_ms)
{
    std::vector<int64_t> keep;
    double mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
    for (int64_t i = 0; i < n; i++) {
        if (!finite6(y + 3 * i, v + 3 * i)) continue;
        for (int k = 0; k < 3; k++) {
            const double c = y[3 * i + k];
            if (keep.empty() || c < mn[k]) mn[k] = c;
            if (keep.empty() || c > mx[k]) mx[k] = c;
        }
        keep.push_back(i);
    }
    double edge = (double)R * (1.0 + 1.0 / 1024.0), ext = 0;
    for (int k = 0; k < 3; k++) ext = std::max(ext, mx[k] - mn[k]);
    edge = std::max(edge, ext / (double)(1 << 20));
    long long cn[3];
    for (;;) {
        for (int k = 0; k < 3; k++) cn[k] = (long long)std::floor((mx[k] - mn[k]) / edge) + 1;
        if ((double)cn[0] * (double)cn[1] * (double)cn[2] <= (double)(1 << 24)) break;
        edge *= 2;
    }
    const long long nc = cn[0] * cn[1] * cn[2];
    const size_t ns = keep.size(), NS = std::max<size_t>(ns, 1);
    std::vector<long long> cell(ns);
    std::vector<int32_t> start((size_t)nc + 1, 0);
    for (size_t s = 0; s < ns; s++) {
        const float *p = y + 3 * keep[s];
        long long c[3];
        for (int k = 0; k < 3; k++) c[k] = std::min(std::max((long long)std::floor(((double)p[k] - mn[k]) / edge), 0ll), cn[k] - 1);
        cell[s] = (c[2] * cn[1] + c[1]) * cn[0] + c[0];
        start[cell[s] + 1]++;
    }
    for (long long c = 0; c < nc; c++) start[c + 1] += start[c];
    std::vector<int32_t> fill(start.begin(), start.end() - 1);
    std::vector<float4> ys(NS, make_float4(0, 0, 0, 0)), vs(NS, make_float4(0, 0, 0, 0));
    for (size_t s = 0; s < ns; s++) {
        const int32_t at = fill[cell[s]]++;
        const float *p = y + 3 * keep[s], *q = v + 3 * keep[s];
        ys[at] = make_float4(p[0], p[1], p[2], 0.0f);
        vs[at] = make_float4(q[0], q[1], q[2], 0.0f);
    }
    const int64_t N = nodes_of(g);
    float4 *d_y, *d_v;
    int *d_start;
    float *d_out;
    DEVCHK(dc, dc.upload(&d_y, ys.data(), NS));
    DEVCHK(dc, dc.upload(&d_v, vs.data(), NS));
    DEVCHK(dc, dc.upload(&d_start, start.data(), start.size()));
    if (dc.alloc(&d_out, (size_t)N * 3) != hipSuccess) return dc.no_memory();
    const double co[3] = {mn[0], mn[1], mn[2]};
    DEVCHK(dc, dc.mark(0));
    DEVCHK(dc, sift3d_launch_field_fit(dc.s, d_y, d_v, d_start, co, edge, cn, g.origin, g.spacing, g.n, R * R, (double)lambda * 16777216.0, d_out));
    DEVCHK(dc, dc.mark(1));
    DEVCHK(dc, dc.download(disp, d_out, (size_t)N * 3));
    DEVCHK(dc, dc.sync());
    DEVCHK(dc, dc.elapsed_ms(kernel_ms));
    for (void *b : {(void *)d_y, (void *)d_v, (void *)d_start, (void *)d_out}) { /* the buffers of one pass go with it */
        hipFree(b);
        dc.bufs.erase(std::find(dc.bufs.begin(), dc.bufs.end(), b));
    }
    return SIFT3D_OK;
}

static bool field_params_ok(const sift3d_field_params &p)
{
    return p.spacing > 0 && std::isfinite(p.spacing) && p.radius > 0 && std::isfinite(p.radius) && p.lambda >= 0 && std::isfinite(p.lambda) &&
           p.search_radius >= 0 && std::isfinite(p.search_radius) && p.min_tol >= 0 && std::isfinite(p.min_tol) && p.ratio_num >= 1 &&
           p.ratio_den >= 1 && p.max_nodes >= 1 && p.index_cells_max >= 1;
}

extern "C" int sift3d_fit_field(int device, const float *y, const float *v, int64_t n, const sift3d_field_params *pp, sift3d_field *f,
                                double *kernel_ms, char *err, int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (kernel_ms) *kernel_ms = 0.0;
    sift3d_field_params p;
    if (pp) p = *pp;
    else sift3d_field_defaults(&p);
    if (!f || n < 0 || n > (1ll << 31) - 4096 || (n > 0 && (!y || !v)) || !field_params_ok(p))
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "bad arguments (0 <= n <= 2^31 - 4096; spacing, radius > 0; lambda >= 0)");
    const char *why = check_samples(v, n);
    if (why) return call_fail(err, err_len, SIFT3D_ERR_ARG, "%s", why);
    if (sift3d_field_size(y, n, &p, f) != SIFT3D_OK)
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "the grid has more than max_nodes = %lld nodes or more than 2^24 along an axis",
                         (long long)p.max_nodes);
    const int64_t N = nodes_of(*f);
    if (f->capacity < 3 * N || !f->disp) return call_fail(err, err_len, SIFT3D_ERR_CAPACITY, "the field needs %lld floats", (long long)(3 * N));
    device_call dc(err, err_len);
    DEVCHK(dc, dc.open(device));
    return fit_on_grid(dc, y, v, n, *f, p.radius, p.lambda, f->disp, kernel_ms);
}

int fit_trim_refit(device_call &dc, const float *y, const float *v, int64_t n, const sift3d_field &g, float R, float lambda, float min_tol,
                   float *out_disp, int64_t *kept, double *rms_before, double *rms_after, double fit_ms[2])
{
    /* pass 1 over all samples */
    const int64_t N = nodes_of(g);
    std::vector<float> disp1((size_t)N * 3);
    sift3d_field f = g;
    f.disp = disp1.data();
    f.capacity = 3 * N;
    int rc = fit_on_grid(dc, y, v, n, f, R, lambda, disp1.data(), &fit_ms[0]);
    if (rc != SIFT3D_OK) return rc;
    /* trim: e_i <= max(min_tol, 3 x the lower median), then pass 2 over the kept samples on the same grid */
    std::vector<double> e;
    residuals(f, y, v, (size_t)n, e);
    *rms_before = rms_of(e);
    double thr = (double)min_tol;
    if (!e.empty()) {
        std::vector<double> srt(e);
        const size_t lm = (srt.size() - 1) / 2;
        std::nth_element(srt.begin(), srt.begin() + lm, srt.end());
        thr = std::max(thr, 3.0 * srt[lm]);
    }
    std::vector<float> yk, vk;
    for (int64_t k = 0; k < n; k++)
        if (e[k] <= thr) {
            yk.insert(yk.end(), y + 3 * k, y + 3 * k + 3);
            vk.insert(vk.end(), v + 3 * k, v + 3 * k + 3);
        }
    *kept = (int64_t)(yk.size() / 3);
    f.disp = out_disp;
    rc = fit_on_grid(dc, yk.data(), vk.data(), *kept, f, R, lambda, out_disp, &fit_ms[1]);
    if (rc != SIFT3D_OK) return rc;
    residuals(f, yk.data(), vk.data(), (size_t)*kept, e);
    *rms_after = rms_of(e);
    return SIFT3D_OK;
}

extern "C" int sift3d_refine_field(int device, const sift3d_feature *fixed, int64_t n_fixed, const sift3d_feature *moving, int64_t n_moving,
                                   const sift3d_similarity *t, const sift3d_field_params *pp, sift3d_field *out, sift3d_field_report *rep,
                                   char *err, int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (rep) memset(rep, 0, sizeof *rep);
    sift3d_field_params p;
    if (pp) p = *pp;
    else sift3d_field_defaults(&p);
    if (!t || !out || n_fixed < 0 || n_moving < 0 || n_fixed > (1ll << 31) - 4096 || n_moving > (1ll << 31) - 4096 || (n_fixed > 0 && !fixed) ||
        (n_moving > 0 && !moving) || !field_params_ok(p))
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "bad arguments");
    sift3d_field_report rp;
    memset(&rp, 0, sizeof rp);
    /* the search and the accept rule of sift3d_refine_similarity, at t */
    const size_t M = (size_t)n_moving;
    std::vector<int32_t> i1(std::max<size_t>(M, 1)), d1(i1.size()), i2(i1.size()), d2(i1.size()), best((size_t)n_fixed), pm, pf, pd;
    if (n_moving > 0) {
        sift3d_refine_params rprm;
        sift3d_refine_defaults(&rprm);
        rprm.index_cells_max = p.index_cells_max;
        const int rc = sift3d_guided_search_params(device, fixed, n_fixed, moving, n_moving, t, p.search_radius, &rprm, i1.data(), d1.data(),
                                                   i2.data(), d2.data(), nullptr, &rp.search_ms, err, err_len);
        if (rc != SIFT3D_OK) return rc;
        guided_accept(M, i1.data(), d1.data(), i2.data(), d2.data(), p.ratio_num, p.ratio_den, best, pm, pf, pd);
    }
    /* the samples */
    const size_t na = pm.size();
    std::vector<float> a(3 * na), b(3 * na), y(3 * na), v(3 * na);
    for (size_t k = 0; k < na; k++) {
        const sift3d_feature &F = fixed[pf[k]], &Mv = moving[pm[k]];
        b[3 * k] = F.x; b[3 * k + 1] = F.y; b[3 * k + 2] = F.z;
        a[3 * k] = Mv.x; a[3 * k + 1] = Mv.y; a[3 * k + 2] = Mv.z;
    }
    sift3d_field_samples(t, b.data(), a.data(), (int64_t)na, y.data(), v.data());
    rp.accepted = (int32_t)na;
    const char *why = check_samples(v.data(), (int64_t)na);
    if (why) return call_fail(err, err_len, SIFT3D_ERR_ARG, "%s", why);
    if (sift3d_field_size(y.data(), (int64_t)na, &p, out) != SIFT3D_OK)
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "the grid has more than max_nodes = %lld nodes or more than 2^24 along an axis",
                         (long long)p.max_nodes);
    const int64_t N = nodes_of(*out);
    if (out->capacity < 3 * N || !out->disp) {
        if (rep) *rep = rp;
        return call_fail(err, err_len, SIFT3D_ERR_CAPACITY, "the field needs %lld floats", (long long)(3 * N));
    }
    device_call dc(err, err_len);
    DEVCHK(dc, dc.open(device));
    int64_t kept;
    const int rc = fit_trim_refit(dc, y.data(), v.data(), (int64_t)na, *out, p.radius, p.lambda, p.min_tol, out->disp, &kept, &rp.rms_before,
                                  &rp.rms_after, rp.fit_ms);
    if (rc != SIFT3D_OK) return rc;
    rp.kept = (int32_t)kept;
    rp.folds = sift3d_field_folds(t, out, &rp.max_disp);
    if (rep) *rep = rp;
    return SIFT3D_OK;
}

/* NULL when the arguments are usable, else the reason: section 7c's shapes and check_field's rules */
static const char *check_warp(const float *src, int64_t nx, int64_t ny, int64_t nz, const float *dst, int64_t ox, int64_t oy, int64_t oz,
                              const float *map, int interp, const sift3d_field *f)
{
    if (!src || !dst || !map || !f) return "null pointer";
    if (interp != SIFT3D_INTERP_LINEAR && interp != SIFT3D_INTERP_NEAREST && interp != SIFT3D_INTERP_LABEL)
        return "interp must be SIFT3D_INTERP_LINEAR, SIFT3D_INTERP_NEAREST or SIFT3D_INTERP_LABEL";
    const char *why = check_source_extents(nx, ny, nz);
    if (!why) why = check_output_extents(ox, oy, oz);
    return why ? why : check_field(*f);
}

extern "C" int sift3d_resample_field(int device, const float *src, int64_t nx, int64_t ny, int64_t nz, float *dst, int64_t ox, int64_t oy,
                                     int64_t oz, const float map[12], const float fixed_vox2key[16], const float moving_vox2key[16],
                                     const sift3d_field *field, int interp, float fill, double *kernel_ms, char *err, int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (kernel_ms) *kernel_ms = 0.0;
    const char *why = check_warp(src, nx, ny, nz, dst, ox, oy, oz, map, interp, field);
    if (why) return call_fail(err, err_len, SIFT3D_ERR_ARG, "%s", why);
    float c[12], k[9];
    if (sift3d_field_warp_terms(fixed_vox2key, moving_vox2key, c, k) != 0)
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "a vox2key's last row is not 0 0 0 1, or moving_vox2key is singular");
    const int64_t N = nodes_of(*field);
    std::vector<float4> nodes; /* send_nodes packs into it: it lives until the stream is synchronised */
    const size_t n_in = (size_t)(nx * ny * nz), n_out = (size_t)(ox * oy * oz);
    device_call dc(err, err_len);
    float *d_src, *d_dst;
    float4 *d_nodes;
    DEVCHK(dc, dc.open(device));
    if (dc.alloc(&d_src, n_in) != hipSuccess || dc.alloc(&d_dst, n_out) != hipSuccess || dc.alloc(&d_nodes, (size_t)N) != hipSuccess) return dc.no_memory();
    DEVCHK(dc, dc.to_device(d_src, src, n_in));
    DEVCHK(dc, send_nodes(dc, *field, nodes, d_nodes));
    DEVCHK(dc, dc.mark(0));
    DEVCHK(dc, sift3d_launch_field_warp(dc.s, d_src, nx, ny, nz, d_dst, ox, oy, oz, map, c, k, field->origin, field->spacing, field->n, d_nodes,
                                        interp, fill));
    DEVCHK(dc, dc.mark(1));
    DEVCHK(dc, dc.download(dst, d_dst, n_out));
    DEVCHK(dc, dc.sync());
    DEVCHK(dc, dc.elapsed_ms(kernel_ms));
    return SIFT3D_OK;
}
