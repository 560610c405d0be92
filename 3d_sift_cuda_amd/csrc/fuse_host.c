/*
 * fuse_host.c -- host arithmetic of the label fusion (DESIGN.md sections 7j and 7k): the default parameters, the similarity of a patch
 * from its six sums, the check of a label volume, the overlap of two, and the code of a search shift, its way back and the counts
 * over a plane of codes.  Linked into libsift3d_hip.so (fuse_api.hip uses it) and into
 * libsift3d_host.so (no GPU needed).
 */
#include <math.h>
#include <string.h>

#include "patch_cost.h"
#include "sift3d.h"

void sift3d_fuse_defaults(sift3d_fuse_params *p)
{
    p->block = 2;
    p->metric = SIFT3D_BLOCKMATCH_SSD;
    p->power = 2;
    p->fill = 0.0f;
    p->max_voxels = (int64_t)1 << 28;
    p->label_interp = SIFT3D_INTERP_NEAREST;
}

uint32_t sift3d_fuse_similarity(int32_t metric, int64_t n, int64_t sf, int64_t sff, int64_t sw, int64_t sww, int64_t sfw)
{
    if (n <= 0) return 0;
    if (metric == SIFT3D_BLOCKMATCH_SSD) {
        const int64_t d = sff - 2 * sfw + sww;
        return (uint32_t)(((uint64_t)n << 15) / ((uint64_t)d + (uint64_t)n));
    }
    if (metric != SIFT3D_BLOCKMATCH_NCC) return 0;
    return pc_u_ncc(n, sf, sff, sw, sww, sfw);
}

static int label_ok(float v) { return !isfinite(v) || (v >= 0.0f && v <= (float)(SIFT3D_LABEL_COUNT - 1) && v == (float)(int32_t)v); }

int64_t sift3d_fuse_check_labels(const float *labels, int64_t n)
{
    for (int64_t i = 0; i < n; i++)
        if (!label_ok(labels[i])) return i;
    return -1;
}

int64_t sift3d_label_overlap(const float *a, const float *b, int64_t n, int64_t *count_a, int64_t *count_b, int64_t *count_both)
{
    if (!a || !b || !count_a || !count_b || !count_both || n < 0) return -1;
    if (sift3d_fuse_check_labels(a, n) >= 0 || sift3d_fuse_check_labels(b, n) >= 0) return -1;
    memset(count_a, 0, sizeof(int64_t) * SIFT3D_LABEL_COUNT);
    memset(count_b, 0, sizeof(int64_t) * SIFT3D_LABEL_COUNT);
    memset(count_both, 0, sizeof(int64_t) * SIFT3D_LABEL_COUNT);
    for (int64_t i = 0; i < n; i++) {
        const int fa = isfinite(a[i]), fb = isfinite(b[i]);
        if (fa) count_a[(int32_t)a[i]]++;
        if (fb) count_b[(int32_t)b[i]]++;
        if (fa && fb && a[i] == b[i]) count_both[(int32_t)a[i]]++;
    }
    int64_t present = 0;
    for (int l = 0; l < SIFT3D_LABEL_COUNT; l++) present += count_a[l] > 0 || count_b[l] > 0;
    return present;
}

uint16_t sift3d_fuse_shift_code(int32_t r, int32_t tx, int32_t ty, int32_t tz)
{
    if (r < 0 || r > SIFT3D_FUSE_MAX_SEARCH || tx < -r || tx > r || ty < -r || ty > r || tz < -r || tz > r) return SIFT3D_FUSE_NO_SHIFT;
    const int32_t s = 2 * r + 1;
    return (uint16_t)(((tz + r) * s + (ty + r)) * s + (tx + r));
}

int sift3d_fuse_shift_of(int32_t r, uint32_t code, int32_t t[3])
{
    if (!t || r < 0 || r > SIFT3D_FUSE_MAX_SEARCH) return -1;
    const uint32_t s = 2 * (uint32_t)r + 1;
    if (code >= s * s * s) return -1;
    t[0] = (int32_t)(code % s) - r;
    t[1] = (int32_t)(code / s % s) - r;
    t[2] = (int32_t)(code / (s * s)) - r;
    return 0;
}

int64_t sift3d_fuse_shift_stats(int32_t r, const uint16_t *shift, int64_t n, int64_t *moved, int64_t *dist2_sum)
{
    int64_t voters = 0, mv = 0, d2 = 0;
    if (moved) *moved = 0;
    if (dist2_sum) *dist2_sum = 0;
    if (!shift || n < 0 || r < 0 || r > SIFT3D_FUSE_MAX_SEARCH) return -1;
    for (int64_t i = 0; i < n; i++) {
        int32_t t[3];
        if (shift[i] == SIFT3D_FUSE_NO_SHIFT) continue;
        if (sift3d_fuse_shift_of(r, shift[i], t) != 0) return -1;
        const int64_t d = (int64_t)t[0] * t[0] + (int64_t)t[1] * t[1] + (int64_t)t[2] * t[2];
        voters++;
        mv += d > 0;
        d2 += d;
    }
    if (moved) *moved = mv;
    if (dist2_sum) *dist2_sum = d2;
    return voters;
}
