/*
 * compose_host.c -- host arithmetic of the composition of two alignments: the default parameters, the
 * composite matrix, the composite grid and the reduction of the per-cell residuals.  Linked into libsift3d_hip.so
 * (compose_api.hip uses all of it) and into libsift3d_host.so (no GPU needed).
 */
#include <math.h>
#include <stddef.h>

#include "sift3d.h"

void sift3d_compose_defaults(sift3d_compose_params *p)
{
    sift3d_field_params f;
    sift3d_field_defaults(&f);
    p->spacing = 0.0f;
    p->radius = f.radius;
    p->margin = -1;
    p->max_nodes = f.max_nodes;
}

int sift3d_compose_matrix(const float m1[16], const float m2[16], float out[16])
{
    if (!m1 || !m2 || !out) return -1;
    if (m1[12] != 0.0f || m1[13] != 0.0f || m1[14] != 0.0f || m1[15] != 1.0f || m2[12] != 0.0f || m2[13] != 0.0f || m2[14] != 0.0f || m2[15] != 1.0f)
        return -1;
    float o[16];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) {
            double s = ((double)m1[4 * r] * (double)m2[c] + (double)m1[4 * r + 1] * (double)m2[4 + c]) + (double)m1[4 * r + 2] * (double)m2[8 + c];
            if (c == 3) s = s + (double)m1[4 * r + 3];
            if (!isfinite(s)) return -1;
            o[4 * r + c] = (float)s;
        }
    o[12] = o[13] = o[14] = 0.0f;
    o[15] = 1.0f;
    for (int k = 0; k < 16; k++) out[k] = o[k];
    return 0;
}

float sift3d_compose_spacing(const sift3d_compose_params *p, const sift3d_field *field1, const sift3d_field *field2)
{
    if (p && p->spacing != 0.0f) return p->spacing;
    if (field1) return field1->spacing;
    if (field2) return field2->spacing;
    sift3d_field_params f;
    sift3d_field_defaults(&f);
    return f.spacing;
}

int sift3d_compose_grid(int64_t nx, int64_t ny, int64_t nz, const float a_vox2key[16], const sift3d_compose_params *pp, const sift3d_field *field1,
                        const sift3d_field *field2, sift3d_field *f)
{
    sift3d_compose_params p;
    if (pp) p = *pp;
    else sift3d_compose_defaults(&p);
    /* the corner voxels' keys, sift3d_field_size and its checks of spacing, radius and max_nodes */
    sift3d_blockmatch_params bp;
    sift3d_blockmatch_defaults(&bp);
    bp.spacing = sift3d_compose_spacing(&p, field1, field2);
    bp.radius = p.radius;
    bp.max_nodes = p.max_nodes;
    return sift3d_blockmatch_grid(nx, ny, nz, a_vox2key, &bp, f);
}

int64_t sift3d_compose_residual(const int64_t n[3], const uint32_t *status, const double *res2, int64_t margin, double *rms, double *max)
{
    double sum = 0.0, big = 0.0;
    int64_t kept = 0;
    if (rms) *rms = 0.0;
    if (max) *max = 0.0;
    if (!n || !status || !res2 || margin < 0 || n[0] < 2 || n[1] < 2 || n[2] < 2) return 0;
    const int64_t n0 = n[0], n1 = n[1], c0 = n[0] - 1, c1 = n[1] - 1, c2 = n[2] - 1;
    for (int64_t c = margin; c < c2 - margin; c++)
        for (int64_t b = margin; b < c1 - margin; b++)
            for (int64_t a = margin; a < c0 - margin; a++) {
                uint32_t any = 0;
                for (int k = 0; k < 8; k++) any |= status[((c + (k >> 2)) * n1 + (b + ((k >> 1) & 1))) * n0 + (a + (k & 1))];
                if (any & SIFT3D_COMPOSE_ZEROED) continue;
                const double e = res2[(c * c1 + b) * c0 + a];
                kept++;
                sum += e;
                if (e > big) big = e;
            }
    if (rms) *rms = kept ? sqrt(sum / (double)kept) : 0.0;
    if (max) *max = sqrt(big);
    return kept;
}
