/*
 * invert_host.c -- host arithmetic of the reverse direction: the default parameters, the inverse
 * grid, the inverse of an affine 4 x 4, the .trans.txt writer for a matrix and the factor of the Jacobian map.  Linked into
 * libsift3d_hip.so (invert_api.hip uses all of it) and into libsift3d_host.so (no GPU needed).
 */
#include <math.h>
#include <stdio.h>

#include "sift3d.h"

void sift3d_invert_defaults(sift3d_invert_params *p)
{
    sift3d_field_params f;
    sift3d_field_defaults(&f);
    p->spacing = f.spacing;
    p->radius = f.radius;
    p->max_iter = 30;
    p->tol = 1e-3f;
    p->max_nodes = f.max_nodes;
}

int sift3d_invert_grid(int64_t nx, int64_t ny, int64_t nz, const float moving_vox2key[16], const sift3d_invert_params *pp, sift3d_field *f)
{
    sift3d_invert_params p;
    if (pp) p = *pp;
    else sift3d_invert_defaults(&p);
    /* the corner voxels' keys, sift3d_field_size and its checks of spacing, radius and max_nodes */
    sift3d_blockmatch_params bp;
    sift3d_blockmatch_defaults(&bp);
    bp.spacing = p.spacing;
    bp.radius = p.radius;
    bp.max_nodes = p.max_nodes;
    return sift3d_blockmatch_grid(nx, ny, nz, moving_vox2key, &bp, f);
}

int sift3d_affine_invert_d(const float m[16], double o[16])
{
    double a[16];
    for (int k = 0; k < 16; k++) a[k] = (double)m[k];
    if (a[12] != 0.0 || a[13] != 0.0 || a[14] != 0.0 || a[15] != 1.0) return -1;
    const double c00 = a[5] * a[10] - a[6] * a[9], c01 = a[6] * a[8] - a[4] * a[10], c02 = a[4] * a[9] - a[5] * a[8];
    const double det = (a[0] * c00 + a[1] * c01) + a[2] * c02;
    if (!(det != 0.0) || !isfinite(det)) return -1;
    const double inv[9] = {c00, a[2] * a[9] - a[1] * a[10], a[1] * a[6] - a[2] * a[5],
                           c01, a[0] * a[10] - a[2] * a[8], a[2] * a[4] - a[0] * a[6],
                           c02, a[1] * a[8] - a[0] * a[9], a[0] * a[5] - a[1] * a[4]};
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) o[4 * r + c] = inv[3 * r + c] / det;
        o[4 * r + 3] = -((o[4 * r] * a[3] + o[4 * r + 1] * a[7]) + o[4 * r + 2] * a[11]);
        if (!isfinite(o[4 * r]) || !isfinite(o[4 * r + 1]) || !isfinite(o[4 * r + 2]) || !isfinite(o[4 * r + 3])) return -1;
    }
    o[12] = o[13] = o[14] = 0.0;
    o[15] = 1.0;
    return 0;
}

int sift3d_affine_invert(const float m[16], float out[16])
{
    double o[16];
    if (sift3d_affine_invert_d(m, o) != 0) return -1;
    for (int k = 0; k < 16; k++) out[k] = (float)o[k];
    return 0;
}

int sift3d_write_matrix(const char *path, const float m[16])
{
    FILE *f = fopen(path, "wt");
    if (!f) return -1;
    for (int r = 0; r < 3; r++) fprintf(f, "%f\t%f\t%f\t%f\n", m[4 * r], m[4 * r + 1], m[4 * r + 2], m[4 * r + 3]);
    fprintf(f, "0.0\t0.0\t0.0\t1.0\n");
    return fclose(f) == 0 ? 0 : -1;
}

static double det_linear(const float *m)
{
    if (!m) return 1.0;
    const double a0 = m[0], a1 = m[1], a2 = m[2], a3 = m[4], a4 = m[5], a5 = m[6], a6 = m[8], a7 = m[9], a8 = m[10];
    return a0 * (a4 * a8 - a5 * a7) - a1 * (a3 * a8 - a5 * a6) + a2 * (a3 * a7 - a4 * a6);
}

int sift3d_jacobian_factor(const float out_vox2key[16], const float src_vox2key[16], double *factor)
{
    const double s = det_linear(src_vox2key), o = det_linear(out_vox2key);
    if (!factor || !(s != 0.0) || !isfinite(s) || !(o != 0.0) || !isfinite(o)) return -1;
    *factor = s / o;
    return 0;
}
