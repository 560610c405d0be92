/*
 * fuse_api.hip -- C-ABI of the label fusion (include/sift3d.h, "multi-atlas label fusion"):
 * sift3d_fuse_weights, sift3d_fuse_vote and sift3d_fuse_labels, and section 7k's local search: sift3d_fuse_search and
 * sift3d_fuse_labels_search.  The kernels are in kernels_fuse.hip and kernels_fuse_search.hip; the warps are section 7c's
 * and 7e's (kernels_resample.hip, kernels_field.hip), the quantisation section 7f's (kernels_blockmatch.hip); the defaults, the
 * label check, the shift codes and the reports' counts are host arithmetic (fuse_host.c and below).
 */
#include <cmath>
#include <cstring>
#include <vector>

#include "field_call.h"

hipError_t sift3d_launch_fuse_weight(hipStream_t s, const short *qt, const short *qw, int64_t nx, int64_t ny, int64_t nz, int b, int ncc, int generic,
                                     unsigned short *u);
hipError_t sift3d_launch_fuse_label(hipStream_t s, const float *labels, int64_t n, int clear_u, unsigned short *lab, unsigned short *u);
hipError_t sift3d_launch_fuse_vote(hipStream_t s, const unsigned short *u, const unsigned short *lab, int K, int64_t n, int power, unsigned *words);
hipError_t sift3d_launch_fuse_search(hipStream_t s, const short *qt, const short *qw, const float *labels, int64_t nx, int64_t ny, int64_t nz, int b, int r,
                                     int ncc, int generic, unsigned short *u, unsigned short *shift, float *picked);

/* NULL, or why the weight kernel refuses these arguments */
static const char *check_weights(int64_t nx, int64_t ny, int64_t nz, int b, int metric)
{
    const char *why = check_source_extents(nx, ny, nz);
    if (why) return "extents must be 1 .. 2^24";
    if (nx * ny > (1ll << 38) / nz) return "volume larger than 2^38 voxels";
    if (b < 1 || b > SIFT3D_BLOCKMATCH_MAX_B) return "the patch half-width must be 1 .. 6";
    if (metric != SIFT3D_BLOCKMATCH_SSD && metric != SIFT3D_BLOCKMATCH_NCC) return "unknown metric: SIFT3D_BLOCKMATCH_SSD (0) or SIFT3D_BLOCKMATCH_NCC (1)";
    return nullptr;
}

/* NULL, or why the search kernel refuses this radius with this half-width */
static const char *check_search(int b, int r)
{
    if (r < 0 || r > SIFT3D_FUSE_MAX_SEARCH) return "the search radius must be 0 .. 3";
    if (b + r > SIFT3D_BLOCKMATCH_MAX_B) return "the patch half-width plus the search radius must not exceed 6";
    return nullptr;
}

/* The range W is quantised with, into wlo and whi: w_range where it is given, under NCC W's own (w: nv values), else T's (lo, hi).
 * false: there is none -- w_range is empty or not finite, or W has no two distinct finite values */
static bool w_range_of(int metric, const float w_range[2], const float *w, size_t nv, float lo, float hi, float *wlo, float *whi)
{
    *wlo = lo;
    *whi = hi;
    if (w_range) {
        *wlo = w_range[0];
        *whi = w_range[1];
        return *whi > *wlo && std::isfinite(*wlo) && std::isfinite(*whi);
    }
    return metric != SIFT3D_BLOCKMATCH_NCC || sift3d_blockmatch_range(w, (int64_t)nv, wlo, whi) != 0;
}

extern "C" int sift3d_fuse_weights(int device, const float *t, const float *w, int64_t nx, int64_t ny, int64_t nz, int32_t b, int32_t metric,
                                   const float w_range[2], int32_t generic, uint16_t *u, double *kernel_ms, char *err, int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (kernel_ms) *kernel_ms = 0.0;
    if (!t || !w || !u) return call_fail(err, err_len, SIFT3D_ERR_ARG, "null pointer");
    const char *why = check_weights(nx, ny, nz, b, metric);
    if (why) return call_fail(err, err_len, SIFT3D_ERR_ARG, "%s", why);
    const size_t nv = (size_t)(nx * ny * nz);
    float lo, hi;
    if (!sift3d_blockmatch_range(t, (int64_t)nv, &lo, &hi))
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "the target has no two distinct finite values: nothing to quantise");
    float wlo, whi;
    if (!w_range_of(metric, w_range, w, nv, lo, hi, &wlo, &whi)) {
        memset(u, 0, sizeof(uint16_t) * nv);
        return SIFT3D_OK;
    }
    device_call dc(err, err_len);
    float *d_v;
    short *d_qt, *d_qw;
    unsigned short *d_u;
    DEVCHK(dc, dc.open(device));
    if (dc.alloc(&d_v, nv) != hipSuccess || dc.alloc(&d_qt, nv) != hipSuccess || dc.alloc(&d_qw, nv) != hipSuccess || dc.alloc(&d_u, nv) != hipSuccess)
        return dc.no_memory();
    DEVCHK(dc, send_quantised(dc, t, nv, lo, hi, d_v, d_qt));
    DEVCHK(dc, send_quantised(dc, w, nv, wlo, whi, d_v, d_qw));
    DEVCHK(dc, dc.mark(0));
    DEVCHK(dc, sift3d_launch_fuse_weight(dc.s, d_qt, d_qw, nx, ny, nz, b, metric == SIFT3D_BLOCKMATCH_NCC, generic, d_u));
    DEVCHK(dc, dc.mark(1));
    DEVCHK(dc, dc.download((unsigned short *)u, d_u, nv));
    DEVCHK(dc, dc.sync());
    DEVCHK(dc, dc.elapsed_ms(kernel_ms));
    return SIFT3D_OK;
}

/* check_labels of atlas k's labels */
static int check_atlas_labels(int k, const float *labels, int64_t n, char *err, int64_t err_len)
{
    char who[32];
    snprintf(who, sizeof who, "atlas %d: ", k);
    return check_labels(who, labels, n, err, err_len);
}

extern "C" int sift3d_fuse_search(int device, const float *t, const float *w, const float *labels, int64_t nx, int64_t ny, int64_t nz, int32_t b, int32_t r,
                                  int32_t metric, const float w_range[2], int32_t generic, uint16_t *u, uint16_t *shift, float *picked, double *kernel_ms,
                                  char *err, int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (kernel_ms) *kernel_ms = 0.0;
    if (!t || !w || !u || !shift || (labels && !picked)) return call_fail(err, err_len, SIFT3D_ERR_ARG, "null pointer");
    const char *why = check_weights(nx, ny, nz, b, metric);
    if (!why) why = check_search(b, r);
    if (why) return call_fail(err, err_len, SIFT3D_ERR_ARG, "%s", why);
    const size_t nv = (size_t)(nx * ny * nz);
    if (labels) {
        const int rc = check_atlas_labels(0, labels, (int64_t)nv, err, err_len);
        if (rc != SIFT3D_OK) return rc;
    }
    float lo, hi;
    if (!sift3d_blockmatch_range(t, (int64_t)nv, &lo, &hi))
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "the target has no two distinct finite values: nothing to quantise");
    float wlo, whi;
    const bool ranged = w_range_of(metric, w_range, w, nv, lo, hi, &wlo, &whi);
    device_call dc(err, err_len);
    float *d_v, *d_l = nullptr, *d_p = nullptr;
    short *d_qt, *d_qw;
    unsigned short *d_u, *d_s;
    DEVCHK(dc, dc.open(device));
    if (dc.alloc(&d_v, nv) != hipSuccess || dc.alloc(&d_qt, nv) != hipSuccess || dc.alloc(&d_qw, nv) != hipSuccess || dc.alloc(&d_u, nv) != hipSuccess ||
        dc.alloc(&d_s, nv) != hipSuccess || (labels && (dc.alloc(&d_l, nv) != hipSuccess || dc.alloc(&d_p, nv) != hipSuccess)))
        return dc.no_memory();
    DEVCHK(dc, send_quantised(dc, t, nv, lo, hi, d_v, d_qt));
    if (ranged) {
        DEVCHK(dc, send_quantised(dc, w, nv, wlo, whi, d_v, d_qw));
    } else {
        /* no range to quantise W with: every voxel of it is invalid, every patch is empty, u = 0 and the shift 0 wins every tie */
        DEVCHK(dc, hipMemsetAsync(d_qw, 0xff, sizeof(short) * nv, dc.s));
    }
    if (labels) DEVCHK(dc, dc.to_device(d_l, labels, nv));
    DEVCHK(dc, dc.mark(0));
    DEVCHK(dc, sift3d_launch_fuse_search(dc.s, d_qt, d_qw, d_l, nx, ny, nz, b, r, metric == SIFT3D_BLOCKMATCH_NCC, generic, d_u, d_s, d_p));
    DEVCHK(dc, dc.mark(1));
    DEVCHK(dc, dc.download((unsigned short *)u, d_u, nv));
    DEVCHK(dc, dc.download((unsigned short *)shift, d_s, nv));
    if (labels) DEVCHK(dc, dc.download(picked, d_p, nv));
    DEVCHK(dc, dc.sync());
    DEVCHK(dc, dc.elapsed_ms(kernel_ms));
    return SIFT3D_OK;
}

extern "C" int sift3d_fuse_vote(int device, int32_t K, const uint16_t *const *u, const float *const *labels, int64_t n, int32_t power, uint32_t *words,
                                double *kernel_ms, char *err, int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (kernel_ms) *kernel_ms = 0.0;
    if (K < 1 || K > SIFT3D_FUSE_MAX_ATLASES) return call_fail(err, err_len, SIFT3D_ERR_ARG, "%d atlases: 1 .. %d are taken", (int)K, SIFT3D_FUSE_MAX_ATLASES);
    if (power < 0 || power > 2) return call_fail(err, err_len, SIFT3D_ERR_ARG, "the power must be 0, 1 or 2");
    if (!u || !labels || !words || n < 1 || n > (1ll << 38)) return call_fail(err, err_len, SIFT3D_ERR_ARG, "null pointer, or n outside 1 .. 2^38");
    for (int k = 0; k < K; k++) {
        if (!u[k] || !labels[k]) return call_fail(err, err_len, SIFT3D_ERR_ARG, "atlas %d: null pointer", k);
        const int rc = check_atlas_labels(k, labels[k], n, err, err_len);
        if (rc != SIFT3D_OK) return rc;
        for (int64_t i = 0; i < n; i++)
            if (u[k][i] > SIFT3D_FUSE_U_ONE)
                return call_fail(err, err_len, SIFT3D_ERR_ARG, "atlas %d: u = %u at voxel %lld exceeds 32768", k, (unsigned)u[k][i], (long long)i);
    }
    const size_t nv = (size_t)n;
    device_call dc(err, err_len);
    float *d_l;
    unsigned short *d_u, *d_lab;
    unsigned *d_words;
    DEVCHK(dc, dc.open(device));
    if (dc.alloc(&d_l, nv) != hipSuccess || dc.alloc(&d_u, nv * K) != hipSuccess || dc.alloc(&d_lab, nv * K) != hipSuccess ||
        dc.alloc(&d_words, 2 * nv) != hipSuccess)
        return dc.no_memory();
    for (int k = 0; k < K; k++) {
        DEVCHK(dc, dc.to_device(d_u + nv * k, (const unsigned short *)u[k], nv));
        DEVCHK(dc, dc.to_device(d_l, labels[k], nv));
        DEVCHK(dc, sift3d_launch_fuse_label(dc.s, d_l, n, 0, d_lab + nv * k, d_u + nv * k));
    }
    DEVCHK(dc, dc.mark(0));
    DEVCHK(dc, sift3d_launch_fuse_vote(dc.s, d_u, d_lab, K, n, power, d_words));
    DEVCHK(dc, dc.mark(1));
    DEVCHK(dc, dc.download((unsigned *)words, d_words, 2 * nv));
    DEVCHK(dc, dc.sync());
    DEVCHK(dc, dc.elapsed_ms(kernel_ms));
    return SIFT3D_OK;
}

/* The stage.  search 0: section 7j, every atlas votes with the label and the weight it has at the voxel; 1 .. 3: section 7k, with
 * those of its best candidate within that radius, and srep (may be NULL) says how far the atlases moved. */
static int fuse_stage(int device, const float *target, int64_t nx, int64_t ny, int64_t nz, const float target_vox2key[16], int32_t K,
                      const sift3d_fuse_atlas *atlases, const sift3d_fuse_params *pp, int32_t search, uint32_t *words, sift3d_fuse_report *rep,
                      sift3d_fuse_search_report *srep, char *err, int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (rep) memset(rep, 0, sizeof *rep);
    if (srep) memset(srep, 0, sizeof *srep);
    sift3d_fuse_params p;
    if (pp) p = *pp;
    else sift3d_fuse_defaults(&p);
    if (K < 1 || K > SIFT3D_FUSE_MAX_ATLASES) return call_fail(err, err_len, SIFT3D_ERR_ARG, "%d atlases: 1 .. %d are taken", (int)K, SIFT3D_FUSE_MAX_ATLASES);
    if (!target || !atlases || !words) return call_fail(err, err_len, SIFT3D_ERR_ARG, "null pointer");
    if (p.power < 0 || p.power > 2) return call_fail(err, err_len, SIFT3D_ERR_ARG, "the power must be 0, 1 or 2");
    if (p.label_interp != SIFT3D_INTERP_NEAREST && p.label_interp != SIFT3D_INTERP_LABEL)
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "label_interp must be SIFT3D_INTERP_NEAREST (1) or SIFT3D_INTERP_LABEL (2): labels are never blended");
    const char *why = check_weights(nx, ny, nz, p.block, p.metric);
    if (!why) why = check_search(p.block, search);
    if (!why && search > 0 && p.power == 0) why = "a search needs weights to search by: the power must be 1 or 2";
    if (why) return call_fail(err, err_len, SIFT3D_ERR_ARG, "%s", why);
    const int64_t n = nx * ny * nz;
    if (p.max_voxels < 1 || n > p.max_voxels / K)
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "%lld target voxels times %d atlases exceed max_voxels = %lld", (long long)n, (int)K,
                         (long long)p.max_voxels);
    const bool ncc = p.metric == SIFT3D_BLOCKMATCH_NCC;
    size_t nm_max = 0, nodes_max = 1;
    for (int k = 0; k < K; k++) {
        const sift3d_fuse_atlas &a = atlases[k];
        if (!a.image || !a.labels || !a.moving_to_fixed) return call_fail(err, err_len, SIFT3D_ERR_ARG, "atlas %d: null pointer", k);
        why = check_source_extents(a.nx, a.ny, a.nz);
        if (!why && a.nx * a.ny > (1ll << 38) / a.nz) why = "volume larger than 2^38 voxels";
        if (!why && a.field) why = check_field(*a.field);
        if (why) return call_fail(err, err_len, SIFT3D_ERR_ARG, "atlas %d: %s", k, why);
        const int rc = check_atlas_labels(k, a.labels, a.nx * a.ny * a.nz, err, err_len);
        if (rc != SIFT3D_OK) return rc;
        nm_max = std::max(nm_max, (size_t)(a.nx * a.ny * a.nz));
        if (a.field) nodes_max = std::max(nodes_max, (size_t)nodes_of(*a.field));
    }
    sift3d_fuse_report rp;
    sift3d_fuse_search_report sp;
    memset(&rp, 0, sizeof rp);
    memset(&sp, 0, sizeof sp);
    sp.radius = search;
    if (!sift3d_blockmatch_range(target, n, &rp.lo, &rp.hi))
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "the target has no two distinct finite values: nothing to quantise");
    const size_t nv = (size_t)n;
    device_call dc(err, err_len);
    float *d_w, *d_m, *d_pick = nullptr;
    short *d_qt, *d_qw;
    unsigned short *d_u, *d_lab, *d_shift = nullptr;
    unsigned *d_words;
    float4 *d_nodes;
    std::vector<unsigned short> hs; /* one atlas' shift plane, for the search report */
    DEVCHK(dc, dc.open(device));
    if (search > 0 && (dc.alloc(&d_pick, nv) != hipSuccess || dc.alloc(&d_shift, nv) != hipSuccess)) return dc.no_memory();
    if (search > 0) hs.resize(nv);
    if (dc.alloc(&d_w, nv) != hipSuccess || dc.alloc(&d_m, nm_max) != hipSuccess || dc.alloc(&d_qt, nv) != hipSuccess || dc.alloc(&d_qw, nv) != hipSuccess ||
        dc.alloc(&d_u, nv * K) != hipSuccess || dc.alloc(&d_lab, nv * K) != hipSuccess || dc.alloc(&d_words, 2 * nv) != hipSuccess ||
        dc.alloc(&d_nodes, nodes_max) != hipSuccess)
        return dc.no_memory();
    /* T is quantised once; its float copy's buffer then holds the warped volumes */
    DEVCHK(dc, send_quantised(dc, target, nv, rp.lo, rp.hi, d_w, d_qt));
    std::vector<float4> nodes; /* send_nodes packs into it: it lives until the stream is synchronised */
    const float nanf_ = std::nanf("");
    for (int k = 0; k < K; k++) {
        const sift3d_fuse_atlas &a = atlases[k];
        sift3d_fuse_atlas_report &r = rp.atlas[k];
        const size_t nm = (size_t)(a.nx * a.ny * a.nz);
        float map[12], cterm[12], kterm[9];
        if (sift3d_resample_map(a.moving_to_fixed, target_vox2key, a.vox2key, map) != 0 ||
            sift3d_field_warp_terms(target_vox2key, a.vox2key, cterm, kterm) != 0)
            return call_fail(err, err_len, SIFT3D_ERR_ARG, "atlas %d: a matrix's last row is not 0 0 0 1, or a matrix is singular", k);
        if (a.field) DEVCHK(dc, send_nodes(dc, *a.field, nodes, d_nodes));
        /* volume `src` of the atlas through its map and field onto the target grid, into d_w */
        auto warp = [&](const float *src, int interp) -> hipError_t {
            hipError_t e = dc.to_device(d_m, src, nm);
            if (e != hipSuccess) return e;
            if (a.field)
                return sift3d_launch_field_warp(dc.s, d_m, a.nx, a.ny, a.nz, d_w, nx, ny, nz, map, cterm, kterm, a.field->origin, a.field->spacing,
                                                a.field->n, d_nodes, interp, nanf_);
            return sift3d_launch_resample(dc.s, d_m, a.nx, a.ny, a.nz, d_w, nx, ny, nz, map, interp, nanf_);
        };
        float wlo = rp.lo, whi = rp.hi;
        if (p.power > 0) r.empty_range = !w_range_of(p.metric, nullptr, a.image, nm, rp.lo, rp.hi, &wlo, &whi);
        const bool weigh = p.power > 0 && !r.empty_range;
        double ms = 0.0;
        if (weigh) {
            DEVCHK(dc, dc.mark(0));
            DEVCHK(dc, warp(a.image, SIFT3D_INTERP_LINEAR));
            DEVCHK(dc, dc.mark(1));
            DEVCHK(dc, dc.sync());
            DEVCHK(dc, dc.elapsed_ms(&ms));
            r.warp_ms += ms;
            DEVCHK(dc, dc.mark(0));
            DEVCHK(dc, sift3d_launch_bm_quantize(dc.s, d_w, n, (double)wlo, (double)whi, d_qw));
            if (search == 0) DEVCHK(dc, sift3d_launch_fuse_weight(dc.s, d_qt, d_qw, nx, ny, nz, p.block, ncc, 0, d_u + nv * k));
            DEVCHK(dc, dc.mark(1));
            DEVCHK(dc, dc.sync());
            DEVCHK(dc, dc.elapsed_ms(&r.weight_ms));
        }
        DEVCHK(dc, dc.mark(0));
        DEVCHK(dc, warp(a.labels, p.label_interp));
        DEVCHK(dc, dc.mark(1));
        if (search == 0 || !weigh) DEVCHK(dc, sift3d_launch_fuse_label(dc.s, d_w, n, !weigh, d_lab + nv * k, d_u + nv * k));
        DEVCHK(dc, dc.sync());
        DEVCHK(dc, dc.elapsed_ms(&ms));
        r.warp_ms += ms;
        if (search > 0 && weigh) {
            /* d_w holds the warped labels: the search picks among them, and the picked ones go the way the labels went.  An atlas
             * with an empty range has nothing to search by and has voted above as in section 7j: u = 0 and the shift 0. */
            sift3d_fuse_search_atlas_report &sr = sp.atlas[k];
            DEVCHK(dc, dc.mark(0));
            DEVCHK(dc, sift3d_launch_fuse_search(dc.s, d_qt, d_qw, d_w, nx, ny, nz, p.block, search, ncc, 0, d_u + nv * k, d_shift, d_pick));
            DEVCHK(dc, dc.mark(1));
            DEVCHK(dc, sift3d_launch_fuse_label(dc.s, d_pick, n, 0, d_lab + nv * k, d_u + nv * k));
            DEVCHK(dc, dc.download(hs.data(), d_shift, nv));
            DEVCHK(dc, dc.sync());
            DEVCHK(dc, dc.elapsed_ms(&sr.search_ms));
            r.weight_ms += sr.search_ms;
            sift3d_fuse_shift_stats(search, hs.data(), n, &sr.moved, &sr.dist2_sum);
        }
    }
    DEVCHK(dc, dc.mark(0));
    DEVCHK(dc, sift3d_launch_fuse_vote(dc.s, d_u, d_lab, K, n, p.power, d_words));
    DEVCHK(dc, dc.mark(1));
    DEVCHK(dc, dc.download((unsigned *)words, d_words, 2 * nv));
    std::vector<unsigned short> hu(nv * K), hl(nv * K);
    DEVCHK(dc, dc.download(hu.data(), d_u, nv * K));
    DEVCHK(dc, dc.download(hl.data(), d_lab, nv * K));
    DEVCHK(dc, dc.sync());
    DEVCHK(dc, dc.elapsed_ms(&rp.vote_ms));
    /* the report's counts from the planes and the words */
    for (size_t i = 0; i < nv; i++) {
        rp.none += (words[2 * i] & SIFT3D_FUSE_NONE) != 0;
        rp.fallback += (words[2 * i] & SIFT3D_FUSE_FALLBACK) != 0;
    }
    for (int k = 0; k < K; k++) {
        sift3d_fuse_atlas_report &r = rp.atlas[k];
        int64_t sum = 0;
        for (size_t i = 0; i < nv; i++) {
            const unsigned uk = hu[nv * k + i];
            if (uk == 0xffffu) continue;
            r.voters++;
            sum += uk;
            r.support += hl[nv * k + i] == (words[2 * i] & 0xffffu);
        }
        r.mean_u = r.voters > 0 ? (double)sum / (double)r.voters : 0.0;
    }
    if (rep) *rep = rp;
    if (srep) *srep = sp;
    return SIFT3D_OK;
}

extern "C" int sift3d_fuse_labels(int device, const float *target, int64_t nx, int64_t ny, int64_t nz, const float target_vox2key[16], int32_t K,
                                  const sift3d_fuse_atlas *atlases, const sift3d_fuse_params *pp, uint32_t *words, sift3d_fuse_report *rep, char *err,
                                  int64_t err_len)
{
    return fuse_stage(device, target, nx, ny, nz, target_vox2key, K, atlases, pp, 0, words, rep, nullptr, err, err_len);
}

extern "C" int sift3d_fuse_labels_search(int device, const float *target, int64_t nx, int64_t ny, int64_t nz, const float target_vox2key[16], int32_t K,
                                         const sift3d_fuse_atlas *atlases, const sift3d_fuse_params *pp, int32_t search, uint32_t *words,
                                         sift3d_fuse_report *rep, sift3d_fuse_search_report *srep, char *err, int64_t err_len)
{
    return fuse_stage(device, target, nx, ny, nz, target_vox2key, K, atlases, pp, search, words, rep, srep, err, err_len);
}
