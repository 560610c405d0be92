/*
 * field_call.h -- what the entry points that take or make a displacement field share (field_api.hip, blockmatch_api.hip,
 * invert_api.hip, resample_api.hip): the checks of a field and of the volume extents with their messages, the packing of a
 * field's nodes for the device, the residuals of a fit and the two-pass fit of DESIGN.md section 7e; and what the users of the
 * quantised intensities share (blockmatch_api.hip, fuse_api.hip): a host volume to the device and through section 7f's quantiser.  Internal: nothing
 * here is part of the C-ABI.
 */
#ifndef SIFT3D_FIELD_CALL_H
#define SIFT3D_FIELD_CALL_H
#include <algorithm>
#include <cmath>
#include <vector>

#include "device_call.h"

#pragma GCC visibility push(hidden)

hipError_t sift3d_launch_field_warp(hipStream_t s, const float *src, int64_t nx, int64_t ny, int64_t nz, float *dst, int64_t ox, int64_t oy,
                                    int64_t oz, const float *map, const float *c, const float *k, const float o[3], float h, const int64_t n[3],
                                    const float4 *nodes, int mode, float fill);
hipError_t sift3d_launch_bm_quantize(hipStream_t s, const float *src, int64_t n, double lo, double hi, short *dst);

inline int64_t nodes_of(const sift3d_field &f) { return f.n[0] * f.n[1] * f.n[2]; }

/* NULL, or why a field cannot be gathered from: 2 .. 2^24 nodes per axis, a positive finite spacing and its values */
inline const char *check_field(const sift3d_field &f)
{
    for (int k = 0; k < 3; k++)
        if (f.n[k] < 2 || f.n[k] > (1 << 24)) return "the field needs 2 .. 2^24 nodes per axis";
    if (!(f.spacing > 0) || !std::isfinite(f.spacing)) return "the field's spacing must be positive and finite";
    if (f.n[0] * f.n[1] > (1ll << 40) / f.n[2]) return "the field has more than 2^40 nodes";
    if (!f.disp || f.capacity < 3 * nodes_of(f)) return "the field's disp holds fewer than 3 n0 n1 n2 floats";
    return nullptr;
}

/* NULL, or the reason.  Source extents up to 2^24, so that n - 1 is exact in float and the inside test can never admit a
 * position past the last voxel; output extents up to 2^31 each, 2^40 voxels in all. */
inline const char *check_source_extents(int64_t nx, int64_t ny, int64_t nz)
{
    if (nx < 1 || ny < 1 || nz < 1 || nx > (1 << 24) || ny > (1 << 24) || nz > (1 << 24)) return "source extents must be 1 .. 2^24";
    return nullptr;
}

inline const char *check_output_extents(int64_t ox, int64_t oy, int64_t oz)
{
    if (ox < 1 || oy < 1 || oz < 1 || ox >= (1ll << 31) || oy >= (1ll << 31) || oz >= (1ll << 31)) return "output extents must be 1 .. 2^31 - 1";
    if (ox * oy > (1ll << 40) / oz) return "output larger than 2^40 voxels";
    return nullptr;
}

/* the field's component-major values as the kernels' float4 nodes (v0, v1, v2, 0) */
inline void pack_nodes(const sift3d_field &f, std::vector<float4> &nodes)
{
    const int64_t N = nodes_of(f);
    nodes.resize((size_t)N);
    for (int64_t i = 0; i < N; i++) nodes[i] = make_float4(f.disp[i], f.disp[N + i], f.disp[2 * N + i], 0.0f);
}

/* pack f's nodes into `nodes` and start their copy to d_nodes (room for f's nodes); `nodes` lives until the stream is synchronised */
inline hipError_t send_nodes(device_call &dc, const sift3d_field &f, std::vector<float4> &nodes, float4 *d_nodes)
{
    pack_nodes(f, nodes);
    return dc.to_device(d_nodes, nodes.data(), nodes.size());
}

/* the host volume v (nv values) through d_v, quantised over [lo, hi] into d_q (quantize.h) */
inline hipError_t send_quantised(device_call &dc, const float *v, size_t nv, float lo, float hi, float *d_v, short *d_q)
{
    const hipError_t e = dc.to_device(d_v, v, nv);
    return e != hipSuccess ? e : sift3d_launch_bm_quantize(dc.s, d_v, (int64_t)nv, (double)lo, (double)hi, d_q);
}

/* e_i = |v_i - v(y_i)| in double */
inline void residuals(const sift3d_field &f, const float *y, const float *v, size_t n, std::vector<double> &e)
{
    std::vector<float> fit(3 * std::max<size_t>(n, 1));
    sift3d_field_eval(&f, y, (int64_t)n, fit.data());
    e.resize(n);
    for (size_t i = 0; i < n; i++) {
        const double dx = (double)v[3 * i] - (double)fit[3 * i], dy = (double)v[3 * i + 1] - (double)fit[3 * i + 1],
                     dz = (double)v[3 * i + 2] - (double)fit[3 * i + 2];
        e[i] = std::sqrt((dx * dx + dy * dy) + dz * dz);
    }
}

/* field_api.hip: one fit of the samples y, v (n x 3 floats, host) on the grid g into disp (3 N floats, host) */
int fit_on_grid(device_call &dc, const float *y, const float *v, int64_t n, const sift3d_field &g, float R, float lambda, float *disp,
                double *kernel_ms);

/* field_api.hip: section 7e's two passes on the grid g (its n, origin and spacing): a fit of all n samples, the trim
 * e_i <= max(min_tol, 3 x the lower median of e), and a fit of the kept samples into out_disp (3 N floats, host).  *kept: the
 * samples of the second pass; rms_before, rms_after: the RMS of e_i over all samples under the first pass and over the kept ones
 * under the second; fit_ms: the fit kernel's device time per pass */
int fit_trim_refit(device_call &dc, const float *y, const float *v, int64_t n, const sift3d_field &g, float R, float lambda, float min_tol,
                   float *out_disp, int64_t *kept, double *rms_before, double *rms_after, double fit_ms[2]);

#pragma GCC visibility pop
#endif
