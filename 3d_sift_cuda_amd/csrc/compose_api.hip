/*
 * compose_api.hip -- C-ABI of the composition of two alignments (include/sift3d.h, "composition"):
 * sift3d_compose_nodes and sift3d_compose_field.  The kernels are in kernels_compose.hip; the matrices, the grid and the
 * reduction of the residual are host arithmetic (compose_host.c), the fold count is section 7f's (blockmatch_host.c).
 */
#include <cmath>
#include <cstring>
#include <vector>

#include "field_call.h"

hipError_t sift3d_launch_field_compose(hipStream_t s, const float4 *f1, const float o1[3], float h1, const int64_t n1[3], const float4 *f2,
                                       const float o2[3], float h2, const int64_t n2[3], const float go[3], float gh, const int64_t gn[3],
                                       const double p1[12], const double p2[12], const double pc[12], float *w, float4 *w4, unsigned *status);
hipError_t sift3d_launch_compose_residual(hipStream_t s, const float4 *f1, const float o1[3], float h1, const int64_t n1[3], const float4 *f2,
                                          const float o2[3], float h2, const int64_t n2[3], const float go[3], float gh, const int64_t gn[3],
                                          const double p1[12], const double p2[12], const double pc[12], const float4 *w4, double *res2);

extern "C" int sift3d_compose_nodes(int device, const float m1[16], const float m2[16], const float mc[16], const sift3d_field *field1,
                                    const sift3d_field *field2, const sift3d_compose_params *pp, const sift3d_field *grid, float *w, uint32_t *status,
                                    double *res2, double kernel_ms[2], char *err, int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (kernel_ms) kernel_ms[0] = kernel_ms[1] = 0.0;
    sift3d_compose_params p;
    if (pp) p = *pp;
    else sift3d_compose_defaults(&p);
    if (!m1 || !m2 || !mc || !grid || !w || !status) return call_fail(err, err_len, SIFT3D_ERR_ARG, "null pointer");
    if (p.max_nodes < 1) return call_fail(err, err_len, SIFT3D_ERR_ARG, "parameters out of range (max_nodes >= 1)");
    double P1[16], P2[16], Pc[16];
    if (sift3d_affine_invert_d(m1, P1) != 0 || sift3d_affine_invert_d(m2, P2) != 0 || sift3d_affine_invert_d(mc, Pc) != 0)
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "a matrix's last row is not 0 0 0 1, or a matrix is singular");
    const int64_t least = res2 ? 2 : 1;
    double total = 1;
    for (int k = 0; k < 3; k++) {
        if (grid->n[k] < least || grid->n[k] > (1 << 24))
            return call_fail(err, err_len, SIFT3D_ERR_ARG, "the composite grid needs %d .. 2^24 nodes per axis", (int)least);
        total *= (double)grid->n[k];
    }
    if (!(grid->spacing > 0) || !std::isfinite(grid->spacing))
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "the composite grid's spacing must be positive and finite");
    if (total > (double)p.max_nodes)
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "the composite grid has more than max_nodes = %lld nodes", (long long)p.max_nodes);
    for (const sift3d_field *f : {field1, field2})
        if (f) {
            const char *why = check_field(*f);
            if (why) return call_fail(err, err_len, SIFT3D_ERR_ARG, "%s", why);
        }
    const size_t N = (size_t)nodes_of(*grid);
    const size_t NC = res2 ? (size_t)((grid->n[0] - 1) * (grid->n[1] - 1) * (grid->n[2] - 1)) : 0;
    const size_t N1 = field1 ? (size_t)nodes_of(*field1) : 0, N2 = field2 ? (size_t)nodes_of(*field2) : 0;
    std::vector<float4> nodes1, nodes2; /* send_nodes packs into them: they live until the stream is synchronised */
    device_call dc(err, err_len);
    stage_events<3> ev; /* around the composition and, with res2, the residual after it */
    float4 *d_f1 = nullptr, *d_f2 = nullptr, *d_w4 = nullptr;
    float *d_w;
    unsigned *d_status;
    double *d_res = nullptr;
    DEVCHK(dc, dc.open(device, false));
    DEVCHK(dc, ev.create());
    if ((field1 && dc.alloc(&d_f1, N1) != hipSuccess) || (field2 && dc.alloc(&d_f2, N2) != hipSuccess) || dc.alloc(&d_w, 3 * N) != hipSuccess ||
        dc.alloc(&d_status, N) != hipSuccess || (res2 && (dc.alloc(&d_w4, N) != hipSuccess || dc.alloc(&d_res, NC) != hipSuccess)))
        return dc.no_memory();
    if (field1) DEVCHK(dc, send_nodes(dc, *field1, nodes1, d_f1));
    if (field2) DEVCHK(dc, send_nodes(dc, *field2, nodes2, d_f2));
    const float *o1 = field1 ? field1->origin : nullptr, *o2 = field2 ? field2->origin : nullptr;
    const int64_t *n1 = field1 ? field1->n : nullptr, *n2 = field2 ? field2->n : nullptr;
    const float h1 = field1 ? field1->spacing : 0.0f, h2 = field2 ? field2->spacing : 0.0f;
    DEVCHK(dc, ev.record(0, dc.s));
    DEVCHK(dc, sift3d_launch_field_compose(dc.s, d_f1, o1, h1, n1, d_f2, o2, h2, n2, grid->origin, grid->spacing, grid->n, P1, P2, Pc, d_w, d_w4,
                                           d_status));
    DEVCHK(dc, ev.record(1, dc.s));
    if (res2) {
        DEVCHK(dc, sift3d_launch_compose_residual(dc.s, d_f1, o1, h1, n1, d_f2, o2, h2, n2, grid->origin, grid->spacing, grid->n, P1, P2, Pc, d_w4,
                                                  d_res));
        DEVCHK(dc, ev.record(2, dc.s));
        DEVCHK(dc, dc.download(res2, d_res, NC));
    }
    DEVCHK(dc, dc.download(w, d_w, 3 * N));
    DEVCHK(dc, dc.download((unsigned *)status, d_status, N));
    DEVCHK(dc, dc.sync());
    if (kernel_ms) DEVCHK(dc, ev.elapsed(0, 1, &kernel_ms[0]));
    if (res2 && kernel_ms) DEVCHK(dc, ev.elapsed(1, 2, &kernel_ms[1]));
    return SIFT3D_OK;
}

extern "C" int sift3d_compose_field(int device, const float m1[16], const float m2[16], const float mc[16], const sift3d_field *field1,
                                    const sift3d_field *field2, const sift3d_compose_params *pp, sift3d_field *out, sift3d_compose_report *rep,
                                    char *err, int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (rep) memset(rep, 0, sizeof *rep);
    if (!out) return call_fail(err, err_len, SIFT3D_ERR_ARG, "null pointer");
    sift3d_compose_params p;
    if (pp) p = *pp;
    else sift3d_compose_defaults(&p);
    if (!(p.radius >= 0) || !std::isfinite(p.radius) || p.margin < -1)
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "parameters out of range (radius >= 0 and finite, margin >= -1)");
    double total = 1;
    for (int k = 0; k < 3; k++) {
        if (out->n[k] < 2 || out->n[k] > (1 << 24)) return call_fail(err, err_len, SIFT3D_ERR_ARG, "the composite grid needs 2 .. 2^24 nodes per axis");
        total *= (double)out->n[k];
    }
    if (total > (double)(1ll << 40)) return call_fail(err, err_len, SIFT3D_ERR_ARG, "the composite grid has more than 2^40 nodes");
    if (!(out->spacing > 0) || !std::isfinite(out->spacing))
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "the composite grid's spacing must be positive and finite");
    const int64_t N = nodes_of(*out);
    if (out->capacity < 3 * N || !out->disp) return call_fail(err, err_len, SIFT3D_ERR_CAPACITY, "the field needs %lld floats", (long long)(3 * N));
    if (total > (double)p.max_nodes) /* before the host arrays below are sized by it */
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "the composite grid has more than max_nodes = %lld nodes", (long long)p.max_nodes);
    sift3d_compose_report rp;
    memset(&rp, 0, sizeof rp);
    std::vector<uint32_t> status((size_t)N);
    std::vector<double> res2((size_t)((out->n[0] - 1) * (out->n[1] - 1) * (out->n[2] - 1)));
    const int rc = sift3d_compose_nodes(device, m1, m2, mc, field1, field2, &p, out, out->disp, status.data(), res2.data(), rp.kernel_ms, err, err_len);
    if (rc != SIFT3D_OK) return rc;
    rp.nodes = N;
    for (int64_t i = 0; i < N; i++) {
        const uint32_t s = status[i];
        rp.outside1 += (s & SIFT3D_COMPOSE_OUTSIDE1) != 0;
        rp.outside2 += (s & SIFT3D_COMPOSE_OUTSIDE2) != 0;
        rp.zeroed += (s & SIFT3D_COMPOSE_ZEROED) != 0;
    }
    const double reach = std::ceil((double)p.radius / (double)out->spacing); /* past 2^24 cells no cell is left on any grid */
    const int64_t margin = p.margin >= 0 ? (int64_t)p.margin : (int64_t)(reach < 16777216.0 ? reach : 16777216.0);
    rp.residual_cells = sift3d_compose_residual(out->n, status.data(), res2.data(), margin, &rp.rms_residual, &rp.max_residual);
    rp.folds = sift3d_blockmatch_folds(mc, out, &rp.max_disp);
    if (rep) *rep = rp;
    return SIFT3D_OK;
}
