/*
 * fuse_host.c -- host arithmetic of the label fusion: the default parameters, the similarity of a patch from
 * its six sums, the check of a label volume and the overlap of two.  Linked into libsift3d_hip.so (fuse_api.hip uses it) and into
 * libsift3d_host.so (no GPU needed).
 */
#include <math.h>
#include <string.h>

#include "sift3d.h"

void sift3d_fuse_defaults(sift3d_fuse_params *p)
{
    p->block = 2;
    p->metric = SIFT3D_BLOCKMATCH_SSD;
    p->power = 2;
    p->fill = 0.0f;
    p->max_voxels = (int64_t)1 << 28;
}

uint32_t sift3d_fuse_similarity(int32_t metric, int64_t n, int64_t sf, int64_t sff, int64_t sw, int64_t sww, int64_t sfw)
{
    if (n <= 0) return 0;
    if (metric == SIFT3D_BLOCKMATCH_SSD) {
        const int64_t d = sff - 2 * sfw + sww;
        return (uint32_t)(((uint64_t)n << 15) / ((uint64_t)d + (uint64_t)n));
    }
    if (metric != SIFT3D_BLOCKMATCH_NCC) return 0;
    const int64_t a = n * sfw - sf * sw, vf = n * sff - sf * sf, vw = n * sww - sw * sw;
    double q = 0.0;
    if (a > 0 && vf > 0 && vw > 0) q = ((double)a * (double)a) / ((double)vf * (double)vw);
    q = q > 1.0 ? 1.0 : q;
    const uint32_t c = (uint32_t)rint((1.0 - q) * 2147483648.0);
    return (0x80000000u - c) >> 16;
}

static int label_ok(float v) { return !isfinite(v) || (v >= 0.0f && v <= 65535.0f && v == (float)(int32_t)v); }

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
    memset(count_a, 0, sizeof(int64_t) * 65536);
    memset(count_b, 0, sizeof(int64_t) * 65536);
    memset(count_both, 0, sizeof(int64_t) * 65536);
    for (int64_t i = 0; i < n; i++) {
        const int fa = isfinite(a[i]), fb = isfinite(b[i]);
        if (fa) count_a[(int32_t)a[i]]++;
        if (fb) count_b[(int32_t)b[i]]++;
        if (fa && fb && a[i] == b[i]) count_both[(int32_t)a[i]]++;
    }
    int64_t present = 0;
    for (int l = 0; l < 65536; l++) present += count_a[l] > 0 || count_b[l] > 0;
    return present;
}
