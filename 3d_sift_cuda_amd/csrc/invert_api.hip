/*
 * invert_api.hip -- C-ABI of the reverse direction (include/sift3d.h, "the reverse direction"):
 * sift3d_invert_nodes, sift3d_invert_field and sift3d_jacobian_map.  The kernels are in kernels_invert.hip; the matrices, the
 * grid and the factor are host arithmetic (invert_host.c), the fold count is section 7f's (blockmatch_host.c).
 */
#include <cmath>
#include <cstring>
#include <vector>

#include "field_call.h"

hipError_t sift3d_launch_field_invert(hipStream_t s, const float4 *fwd, const float fo[3], float fh, const int64_t fn[3], const float go[3], float gh,
                                      const int64_t gn[3], const double p[12], const double q[12], const double a[9], double tol2, int max_iter,
                                      float *u, unsigned *status, double *res2);
hipError_t sift3d_launch_jacobian_map(hipStream_t s, float *dst, int64_t ox, int64_t oy, int64_t oz, const float *map, const float *c, const float *k,
                                      const float o[3], float h, const int64_t n[3], const float4 *nodes, double factor, int form);

/* the form of jacobian_map_kernel that form = -1 selects */
#define JACOBIAN_DEFAULT_FORM 1

extern "C" int sift3d_invert_nodes(int device, const float m[16], const float m_inv[16], const sift3d_field *forward, const sift3d_invert_params *pp,
                                   const sift3d_field *grid, float *u, uint32_t *status, double *res2, double *kernel_ms, char *err, int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (kernel_ms) *kernel_ms = 0.0;
    sift3d_invert_params p;
    if (pp) p = *pp;
    else sift3d_invert_defaults(&p);
    if (!m || !m_inv || !grid || !u || !status) return call_fail(err, err_len, SIFT3D_ERR_ARG, "null pointer");
    if (p.max_iter < 1 || p.max_iter > SIFT3D_INVERT_MAX_ITER || !(p.tol >= 0) || !std::isfinite(p.tol) || p.max_nodes < 1)
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "parameters out of range (max_iter 1 .. 65535, tol >= 0 and finite, max_nodes >= 1)");
    double P[16], Q[16], A[9];
    if (sift3d_affine_invert_d(m_inv, P) != 0 || sift3d_affine_invert_d(m, Q) != 0)
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "a matrix's last row is not 0 0 0 1, or a matrix is singular");
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) A[3 * r + c] = (double)m[4 * r + c];
    double total = 1;
    for (int k = 0; k < 3; k++) {
        if (grid->n[k] < 1 || grid->n[k] > (1 << 24)) return call_fail(err, err_len, SIFT3D_ERR_ARG, "the inverse grid needs 1 .. 2^24 nodes per axis");
        total *= (double)grid->n[k];
    }
    if (!(grid->spacing > 0) || !std::isfinite(grid->spacing)) return call_fail(err, err_len, SIFT3D_ERR_ARG, "the inverse grid's spacing must be positive and finite");
    if (total > (double)p.max_nodes)
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "the inverse grid has more than max_nodes = %lld nodes", (long long)p.max_nodes);
    if (forward) {
        const char *why = check_field(*forward);
        if (why) return call_fail(err, err_len, SIFT3D_ERR_ARG, "%s", why);
    }
    const size_t N = (size_t)nodes_of(*grid);
    std::vector<float4> nodes; /* send_nodes packs into it: it lives until the stream is synchronised */
    const size_t NF = forward ? (size_t)nodes_of(*forward) : 0;
    device_call dc(err, err_len);
    float4 *d_nodes = nullptr;
    float *d_u;
    unsigned *d_status;
    double *d_res;
    DEVCHK(dc, dc.open(device));
    if ((forward && dc.alloc(&d_nodes, NF) != hipSuccess) || dc.alloc(&d_u, 3 * N) != hipSuccess || dc.alloc(&d_status, N) != hipSuccess ||
        dc.alloc(&d_res, N) != hipSuccess)
        return dc.no_memory();
    if (forward) DEVCHK(dc, send_nodes(dc, *forward, nodes, d_nodes));
    DEVCHK(dc, dc.mark(0));
    DEVCHK(dc, sift3d_launch_field_invert(dc.s, d_nodes, forward ? forward->origin : nullptr, forward ? forward->spacing : 0.0f,
                                          forward ? forward->n : nullptr, grid->origin, grid->spacing, grid->n, P, Q, A, (double)p.tol * (double)p.tol,
                                          p.max_iter, d_u, d_status, d_res));
    DEVCHK(dc, dc.mark(1));
    DEVCHK(dc, dc.download(u, d_u, 3 * N));
    DEVCHK(dc, dc.download((unsigned *)status, d_status, N));
    if (res2) DEVCHK(dc, dc.download(res2, d_res, N));
    DEVCHK(dc, dc.sync());
    DEVCHK(dc, dc.elapsed_ms(kernel_ms));
    return SIFT3D_OK;
}

extern "C" int sift3d_invert_field(int device, const float m[16], const float m_inv[16], const sift3d_field *forward, const sift3d_invert_params *pp,
                                   sift3d_field *out, sift3d_invert_report *rep, char *err, int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (rep) memset(rep, 0, sizeof *rep);
    if (!out) return call_fail(err, err_len, SIFT3D_ERR_ARG, "null pointer");
    double total = 1;
    for (int k = 0; k < 3; k++) {
        if (out->n[k] < 2 || out->n[k] > (1 << 24)) return call_fail(err, err_len, SIFT3D_ERR_ARG, "the inverse grid needs 2 .. 2^24 nodes per axis");
        total *= (double)out->n[k];
    }
    if (total > (double)(1ll << 40)) return call_fail(err, err_len, SIFT3D_ERR_ARG, "the inverse grid has more than 2^40 nodes");
    const int64_t N = nodes_of(*out);
    if (out->capacity < 3 * N || !out->disp) return call_fail(err, err_len, SIFT3D_ERR_CAPACITY, "the field needs %lld floats", (long long)(3 * N));
    sift3d_invert_report rp;
    memset(&rp, 0, sizeof rp);
    std::vector<uint32_t> status((size_t)N);
    std::vector<double> res2((size_t)N);
    const int rc = sift3d_invert_nodes(device, m, m_inv, forward, pp, out, out->disp, status.data(), res2.data(), &rp.kernel_ms, err, err_len);
    if (rc != SIFT3D_OK) return rc;
    rp.nodes = N;
    double sum = 0, big = 0;
    for (int64_t i = 0; i < N; i++) {
        const uint32_t w = status[i];
        const int32_t steps = (int32_t)SIFT3D_INVERT_STEPS(w);
        if (steps > rp.max_steps) rp.max_steps = steps;
        if (SIFT3D_INVERT_STATE(w) == SIFT3D_INVERT_CONVERGED) {
            rp.converged++;
            sum += res2[i];
            if (res2[i] > big) big = res2[i];
        } else if (SIFT3D_INVERT_STATE(w) == SIFT3D_INVERT_NOT_CONVERGED) rp.not_converged++;
        else rp.diverged++;
    }
    rp.rms_residual = rp.converged ? std::sqrt(sum / (double)rp.converged) : 0.0;
    rp.max_residual = std::sqrt(big);
    rp.folds = sift3d_blockmatch_folds(m_inv, out, &rp.max_disp);
    if (rep) *rep = rp;
    return SIFT3D_OK;
}

extern "C" int sift3d_jacobian_map(int device, int64_t ox, int64_t oy, int64_t oz, const float map[12], const float out_vox2key[16],
                                   const float src_vox2key[16], const sift3d_field *field, float *out, int form, double *kernel_ms, char *err,
                                   int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (kernel_ms) *kernel_ms = 0.0;
    if (!map || !out) return call_fail(err, err_len, SIFT3D_ERR_ARG, "null pointer");
    if (form < -1 || form > 1) return call_fail(err, err_len, SIFT3D_ERR_ARG, "form must be 0 (six evaluations), 1 (through LDS) or -1 (the default)");
    const char *why = check_output_extents(ox, oy, oz);
    if (!why && field) why = check_field(*field);
    if (why) return call_fail(err, err_len, SIFT3D_ERR_ARG, "%s", why);
    float c[12], k[9];
    double factor;
    if (sift3d_field_warp_terms(out_vox2key, src_vox2key, c, k) != 0 || sift3d_jacobian_factor(out_vox2key, src_vox2key, &factor) != 0)
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "a vox2key's last row is not 0 0 0 1, or a vox2key is singular");
    std::vector<float4> nodes; /* send_nodes packs into it: it lives until the stream is synchronised */
    const size_t NF = field ? (size_t)nodes_of(*field) : 0;
    const size_t n_out = (size_t)(ox * oy * oz);
    device_call dc(err, err_len);
    float *d_dst;
    float4 *d_nodes = nullptr;
    DEVCHK(dc, dc.open(device));
    if (dc.alloc(&d_dst, n_out) != hipSuccess || (field && dc.alloc(&d_nodes, NF) != hipSuccess)) return dc.no_memory();
    if (field) DEVCHK(dc, send_nodes(dc, *field, nodes, d_nodes));
    DEVCHK(dc, dc.mark(0));
    DEVCHK(dc, sift3d_launch_jacobian_map(dc.s, d_dst, ox, oy, oz, map, c, k, field ? field->origin : nullptr, field ? field->spacing : 0.0f,
                                          field ? field->n : nullptr, d_nodes, factor, form < 0 ? JACOBIAN_DEFAULT_FORM : form));
    DEVCHK(dc, dc.mark(1));
    DEVCHK(dc, dc.download(out, d_dst, n_out));
    DEVCHK(dc, dc.sync());
    DEVCHK(dc, dc.elapsed_ms(kernel_ms));
    return SIFT3D_OK;
}
