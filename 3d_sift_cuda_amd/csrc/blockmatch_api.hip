/*
 * blockmatch_api.hip -- C-ABI of the intensity refinement (include/sift3d.h, "intensity refinement"; DESIGN.md sections 7f, 7g):
 * sift3d_block_match and sift3d_refine_field_intensity, and the same two under a chosen cost (sift3d_block_match_ncc,
 * sift3d_refine_field_intensity_metric).  The kernels are in kernels_blockmatch.hip; the warp and the fit are
 * section 7e's (kernels_field.hip, fit_on_grid of field_api.hip); the range, the lattice, the grid, the gates, the samples and
 * the fold count are host arithmetic (blockmatch_host.c).
 */
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "field_call.h"

hipError_t sift3d_launch_block_match(hipStream_t s, const short *qf, const short *qw, int64_t nx, int64_t ny, int64_t nz, const int64_t first[3],
                                     int64_t stride, const int64_t n[3], int b, int r, int generic, unsigned *out);
hipError_t sift3d_launch_block_match_ncc(hipStream_t s, const short *qf, const short *qw, int64_t nx, int64_t ny, int64_t nz, const int64_t first[3],
                                         int64_t stride, const int64_t n[3], int b, int r, int generic, unsigned *out);

/* the search kernel of a cost */
static hipError_t launch_search(int metric, hipStream_t s, const short *qf, const short *qw, int64_t nx, int64_t ny, int64_t nz, const int64_t first[3],
                                int64_t stride, const int64_t n[3], int b, int r, int generic, unsigned *out)
{
    const auto launch = metric == SIFT3D_BLOCKMATCH_NCC ? sift3d_launch_block_match_ncc : sift3d_launch_block_match;
    return launch(s, qf, qw, nx, ny, nz, first, stride, n, b, r, generic, out);
}

#define BM_MAX_EXTENT ((1ll << 27) - 1)
#define BM_MAX_NODES (1ll << 27)

/* NULL, or why the block search refuses these shapes */
static const char *check_search(int64_t nx, int64_t ny, int64_t nz, const int64_t first[3], int64_t stride, const int64_t count[3], int b, int r)
{
    if (nx < 1 || ny < 1 || nz < 1 || nx > BM_MAX_EXTENT || ny > BM_MAX_EXTENT || nz > BM_MAX_EXTENT) return "extents must be 1 .. 2^27 - 1";
    if (nx * ny > (1ll << 40) / nz) return "volume larger than 2^40 voxels";
    if (b < 1 || b > SIFT3D_BLOCKMATCH_MAX_B) return "the block half-width must be 1 .. 6";
    if (r < 1 || r > SIFT3D_BLOCKMATCH_MAX_R) return "the search half-width must be 1 .. 6";
    if (stride < 1 || stride > BM_MAX_EXTENT) return "the stride must be 1 .. 2^27 - 1";
    const int64_t n[3] = {nx, ny, nz};
    double total = 1;
    for (int k = 0; k < 3; k++) {
        if (count[k] < 1 || count[k] > BM_MAX_EXTENT) return "node counts must be 1 .. 2^27 - 1";
        if (first[k] < -BM_MAX_EXTENT || first[k] > BM_MAX_EXTENT) return "the first node is out of range";
        if ((double)first[k] + (double)(count[k] - 1) * (double)stride > (double)(n[k] + BM_MAX_EXTENT)) return "the lattice is out of range";
        total *= (double)count[k];
    }
    if (total > (double)BM_MAX_NODES) return "the lattice has more than 2^27 nodes";
    return nullptr;
}

/* the block search under either cost: SSD quantises W with F's range, NCC with W's own */
static int block_match(int metric, int device, const float *f, const float *w, int64_t nx, int64_t ny, int64_t nz, const int64_t first[3],
                       int64_t stride, const int64_t count[3], int32_t b, int32_t r, int32_t generic, uint32_t *out, double *kernel_ms, char *err,
                       int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (kernel_ms) *kernel_ms = 0.0;
    if (!f || !w || !first || !count || !out) return call_fail(err, err_len, SIFT3D_ERR_ARG, "null pointer");
    const char *why = check_search(nx, ny, nz, first, stride, count, b, r);
    if (why) return call_fail(err, err_len, SIFT3D_ERR_ARG, "%s", why);
    const size_t nv = (size_t)(nx * ny * nz), N = (size_t)(count[0] * count[1] * count[2]);
    float lo, hi;
    if (!sift3d_blockmatch_range(f, (int64_t)nv, &lo, &hi))
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "the fixed volume has no two distinct finite values: nothing to quantise");
    float wlo = lo, whi = hi;
    if (metric == SIFT3D_BLOCKMATCH_NCC && !sift3d_blockmatch_range(w, (int64_t)nv, &wlo, &whi))
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "the warped volume has no two distinct finite values: nothing to quantise");
    device_call dc(err, err_len);
    float *d_v;
    short *d_qf, *d_qw;
    unsigned *d_out;
    DEVCHK(dc, dc.open(device));
    if (dc.alloc(&d_v, nv) != hipSuccess || dc.alloc(&d_qf, nv) != hipSuccess || dc.alloc(&d_qw, nv) != hipSuccess ||
        dc.alloc(&d_out, N * SIFT3D_BLOCKMATCH_WORDS) != hipSuccess)
        return dc.no_memory();
    DEVCHK(dc, send_quantised(dc, f, nv, lo, hi, d_v, d_qf));
    DEVCHK(dc, send_quantised(dc, w, nv, wlo, whi, d_v, d_qw));
    DEVCHK(dc, dc.mark(0));
    DEVCHK(dc, launch_search(metric, dc.s, d_qf, d_qw, nx, ny, nz, first, stride, count, b, r, generic, d_out));
    DEVCHK(dc, dc.mark(1));
    DEVCHK(dc, dc.download((unsigned *)out, d_out, N * SIFT3D_BLOCKMATCH_WORDS));
    DEVCHK(dc, dc.sync());
    DEVCHK(dc, dc.elapsed_ms(kernel_ms));
    return SIFT3D_OK;
}

extern "C" int sift3d_block_match(int device, const float *f, const float *w, int64_t nx, int64_t ny, int64_t nz, const int64_t first[3],
                                  int64_t stride, const int64_t count[3], int32_t b, int32_t r, int32_t generic, uint32_t *out,
                                  double *kernel_ms, char *err, int64_t err_len)
{
    return block_match(SIFT3D_BLOCKMATCH_SSD, device, f, w, nx, ny, nz, first, stride, count, b, r, generic, out, kernel_ms, err, err_len);
}

extern "C" int sift3d_block_match_ncc(int device, const float *f, const float *w, int64_t nx, int64_t ny, int64_t nz, const int64_t first[3],
                                      int64_t stride, const int64_t count[3], int32_t b, int32_t r, int32_t generic, uint32_t *out,
                                      double *kernel_ms, char *err, int64_t err_len)
{
    return block_match(SIFT3D_BLOCKMATCH_NCC, device, f, w, nx, ny, nz, first, stride, count, b, r, generic, out, kernel_ms, err, err_len);
}

extern "C" int sift3d_refine_field_intensity_metric(int device, const float *fixed, int64_t fx, int64_t fy, int64_t fz, const float *moving,
                                                    int64_t mx, int64_t my, int64_t mz, const float fixed_vox2key[16],
                                                    const float moving_vox2key[16], const float moving_to_fixed[16], const sift3d_field *in,
                                                    const sift3d_blockmatch_params *pp, int32_t metric, sift3d_field *out,
                                                    sift3d_blockmatch_report *rep, float moving_range[2], char *err, int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (rep) memset(rep, 0, sizeof *rep);
    if (moving_range) moving_range[0] = moving_range[1] = 0.0f;
    if (metric != SIFT3D_BLOCKMATCH_SSD && metric != SIFT3D_BLOCKMATCH_NCC)
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "unknown metric %d: SIFT3D_BLOCKMATCH_SSD (0) or SIFT3D_BLOCKMATCH_NCC (1)", (int)metric);
    const bool ncc = metric == SIFT3D_BLOCKMATCH_NCC;
    sift3d_blockmatch_params p;
    if (pp) p = *pp;
    else sift3d_blockmatch_defaults(&p);
    if (!fixed || !moving || !moving_to_fixed || !out) return call_fail(err, err_len, SIFT3D_ERR_ARG, "null pointer");
    const char *why = check_source_extents(mx, my, mz);
    if (why) return call_fail(err, err_len, SIFT3D_ERR_ARG, "%s", why);
    if (in && check_field(*in) != nullptr) return call_fail(err, err_len, SIFT3D_ERR_ARG, "the input field needs 2 .. 2^24 nodes per axis, a positive spacing and its values");
    int64_t first[3], count[3];
    sift3d_field grid;
    memset(&grid, 0, sizeof grid);
    if (fx < 1 || fy < 1 || fz < 1 || fx > BM_MAX_EXTENT || fy > BM_MAX_EXTENT || fz > BM_MAX_EXTENT)
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "extents must be 1 .. 2^27 - 1");
    if (sift3d_blockmatch_grid(fx, fy, fz, fixed_vox2key, &p, &grid) != SIFT3D_OK)
        return call_fail(err, err_len, SIFT3D_ERR_ARG,
                         "parameters out of range (stride >= 1, block and search 1 .. 6, rounds 0 .. 8, 0 <= quantile < 1, spacing, radius > 0), "
                         "or an output grid of more than max_nodes = %lld nodes", (long long)p.max_nodes);
    if (sift3d_blockmatch_lattice(fx, fy, fz, &p, first, count) != 0)
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "the block and search window (%d voxels) is wider than the volume", 2 * (p.block + p.search) + 1);
    why = check_search(fx, fy, fz, first, p.stride, count, p.block, p.search);
    if (why) return call_fail(err, err_len, SIFT3D_ERR_ARG, "%s", why);
    const int64_t NL = count[0] * count[1] * count[2], NG = nodes_of(grid);
    if (NL > p.max_nodes) return call_fail(err, err_len, SIFT3D_ERR_ARG, "the lattice has more than max_nodes = %lld nodes", (long long)p.max_nodes);
    float map[12], cterm[12], kterm[9];
    if (sift3d_resample_map(moving_to_fixed, fixed_vox2key, moving_vox2key, map) != 0 ||
        sift3d_field_warp_terms(fixed_vox2key, moving_vox2key, cterm, kterm) != 0)
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "a matrix's last row is not 0 0 0 1, or a matrix is singular");
    const int64_t need = 3 * std::max(NG, in ? nodes_of(*in) : (int64_t)0);
    if (out->capacity < need || !out->disp) {
        for (int k = 0; k < 3; k++) {
            out->n[k] = grid.n[k];
            out->origin[k] = grid.origin[k];
        }
        out->spacing = grid.spacing;
        return call_fail(err, err_len, SIFT3D_ERR_CAPACITY, "the field needs %lld floats", (long long)need);
    }
    sift3d_blockmatch_report rp;
    memset(&rp, 0, sizeof rp);
    /* the current field: the input's grid and values, or zero on the output grid */
    sift3d_field cur = in ? *in : grid;
    std::vector<float> cur_disp((size_t)(3 * nodes_of(cur)), 0.0f);
    if (in) std::copy(in->disp, in->disp + 3 * nodes_of(cur), cur_disp.begin());
    cur.disp = cur_disp.data();
    cur.capacity = (int64_t)cur_disp.size();
    const size_t nf = (size_t)(fx * fy * fz), nm = (size_t)(mx * my * mz);
    bool ranged = sift3d_blockmatch_range(fixed, (int64_t)nf, &rp.lo, &rp.hi) != 0;
    /* W's map: F's under SSD; under NCC the moving volume's own range, which trilinear warping cannot leave */
    float wlo = rp.lo, whi = rp.hi;
    if (ncc) {
        if (!sift3d_blockmatch_range(moving, (int64_t)nm, &wlo, &whi)) ranged = false;
        if (moving_range) {
            moving_range[0] = wlo;
            moving_range[1] = whi;
        }
    }
    rp.empty_range = !ranged;
    if (ranged && p.rounds > 0) {
        device_call dc(err, err_len);
        float *d_w, *d_m;
        short *d_qf, *d_qw;
        unsigned *d_words;
        float4 *d_nodes;
        const size_t max_nodes = (size_t)std::max(NG, nodes_of(cur));
        DEVCHK(dc, dc.open(device));
        if (dc.alloc(&d_w, nf) != hipSuccess || dc.alloc(&d_m, nm) != hipSuccess || dc.alloc(&d_qf, nf) != hipSuccess ||
            dc.alloc(&d_qw, nf) != hipSuccess || dc.alloc(&d_words, (size_t)NL * SIFT3D_BLOCKMATCH_WORDS) != hipSuccess ||
            dc.alloc(&d_nodes, max_nodes) != hipSuccess)
            return dc.no_memory();
        /* F is quantised once; its float copy's buffer then holds W */
        DEVCHK(dc, send_quantised(dc, fixed, nf, rp.lo, rp.hi, d_w, d_qf));
        DEVCHK(dc, dc.to_device(d_m, moving, nm));
        std::vector<uint32_t> words((size_t)NL * SIFT3D_BLOCKMATCH_WORDS);
        std::vector<float> y((size_t)(3 * NL)), v((size_t)(3 * NL));
        std::vector<float4> nodes; /* send_nodes packs into it: it lives until the stream is synchronised */
        for (int round = 0; round < p.rounds; round++) {
            sift3d_blockmatch_round &r = rp.round[round];
            DEVCHK(dc, send_nodes(dc, cur, nodes, d_nodes));
            DEVCHK(dc, dc.mark(0));
            DEVCHK(dc, sift3d_launch_field_warp(dc.s, d_m, mx, my, mz, d_w, fx, fy, fz, map, cterm, kterm, cur.origin, cur.spacing, cur.n, d_nodes,
                                                SIFT3D_INTERP_LINEAR, std::nanf("")));
            DEVCHK(dc, dc.mark(1));
            DEVCHK(dc, dc.sync());
            DEVCHK(dc, dc.elapsed_ms(&r.warp_ms));
            DEVCHK(dc, dc.mark(0));
            DEVCHK(dc, sift3d_launch_bm_quantize(dc.s, d_w, (int64_t)nf, (double)wlo, (double)whi, d_qw));
            DEVCHK(dc, launch_search(metric, dc.s, d_qf, d_qw, fx, fy, fz, first, p.stride, count, p.block, p.search, 0, d_words));
            DEVCHK(dc, dc.mark(1));
            DEVCHK(dc, dc.download(words.data(), d_words, words.size()));
            DEVCHK(dc, dc.sync());
            DEVCHK(dc, dc.elapsed_ms(&r.match_ms));
            int64_t tally[4];
            const int64_t ns = sift3d_blockmatch_samples(words.data(), fx, fy, fz, &p, fixed_vox2key, moving_to_fixed, &cur, y.data(), v.data(), tally);
            if (ns < 0) return call_fail(err, err_len, SIFT3D_ERR_MEMORY, "out of host memory");
            r.nodes = NL;
            r.flagged = tally[0];
            r.gated_variance = tally[1];
            r.gated_border = tally[2];
            r.gated_cost = tally[3];
            r.samples = ns;
            if (ns == 0) break;
            for (int64_t i = 0; i < 3 * ns; i++)
                if (std::isfinite(v[i]) && !(std::fabs(v[i]) <= SIFT3D_FIELD_MAX_DISP))
                    return call_fail(err, err_len, SIFT3D_ERR_ARG, "a sample's |v| exceeds SIFT3D_FIELD_MAX_DISP (128 key units)");
            /* section 7e's two passes on the output grid; the current field's values are no longer needed */
            cur_disp.assign((size_t)(3 * NG), 0.0f);
            cur = grid;
            cur.disp = cur_disp.data();
            cur.capacity = 3 * NG;
            const int rc = fit_trim_refit(dc, y.data(), v.data(), ns, grid, p.radius, p.lambda, p.min_tol, cur.disp, &r.kept, &r.rms_before,
                                          &r.rms_after, r.fit_ms);
            if (rc != SIFT3D_OK) return rc;
            r.folds = sift3d_blockmatch_folds(moving_to_fixed, &cur, &r.max_disp);
            rp.rounds = round + 1;
        }
    }
    for (int k = 0; k < 3; k++) {
        out->n[k] = cur.n[k];
        out->origin[k] = cur.origin[k];
    }
    out->spacing = cur.spacing;
    std::copy(cur.disp, cur.disp + 3 * nodes_of(cur), out->disp);
    if (rep) *rep = rp;
    return SIFT3D_OK;
}

extern "C" int sift3d_refine_field_intensity(int device, const float *fixed, int64_t fx, int64_t fy, int64_t fz, const float *moving, int64_t mx,
                                             int64_t my, int64_t mz, const float fixed_vox2key[16], const float moving_vox2key[16],
                                             const float moving_to_fixed[16], const sift3d_field *in, const sift3d_blockmatch_params *pp,
                                             sift3d_field *out, sift3d_blockmatch_report *rep, char *err, int64_t err_len)
{
    return sift3d_refine_field_intensity_metric(device, fixed, fx, fy, fz, moving, mx, my, mz, fixed_vox2key, moving_vox2key, moving_to_fixed, in,
                                                pp, SIFT3D_BLOCKMATCH_SSD, out, rep, nullptr, err, err_len);
}
