/*
 * edt_host.c -- host arithmetic of the surface distances: the default parameters, a voxel size in
 * micrometres, and the figures of one label from its two lists of squared distances.  Linked into libsift3d_hip.so (edt_api.hip
 * uses it) and into libsift3d_host.so (no GPU needed).
 */
#include <math.h>
#include <stdlib.h>

#include "sift3d.h"

void sift3d_surface_defaults(sift3d_surface_params *p)
{
    p->first_label = 1;
    p->max_labels = 64;
    p->device = 0;
    p->reserved = 0;
}

int sift3d_spacing_um(float mm, uint32_t *um)
{
    const float v = mm * 1000.0f;
    if (!um || !isfinite(v) || v < 0.0f || v > 65536.0f) return -1;
    const long r = lroundf(v);
    if (r < 1 || r > (long)SIFT3D_EDT_MAX_SPACING_UM) return -1;
    *um = (uint32_t)r;
    return 0;
}

static int by_value(const void *a, const void *b)
{
    const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b;
    return (x > y) - (x < y);
}

/* one direction: sorts the list; its last element, its 95th percentile and the sum of its roots in ascending order */
static void direction(uint64_t *list, int64_t n, uint64_t *max, uint64_t *p95, double *sum)
{
    qsort(list, (size_t)n, sizeof *list, by_value);
    double s = 0.0;
    for (int64_t i = 0; i < n; i++) s += sqrt((double)list[i]);
    *max = list[n - 1];
    *p95 = list[(95 * n + 99) / 100 - 1];
    *sum = s;
}

void sift3d_surface_stats(uint64_t *list_ab, int64_t n_a, uint64_t *list_ba, int64_t n_b, sift3d_surface_record *rec)
{
    rec->n_a = n_a;
    rec->n_b = n_b;
    if (n_a <= 0 || n_b <= 0 || !list_ab || !list_ba) {
        rec->max_ab = rec->max_ba = rec->p95_ab = rec->p95_ba = SIFT3D_EDT_NONE;
        rec->sum_ab = rec->sum_ba = rec->hausdorff_mm = rec->hd95_mm = rec->assd_mm = (double)NAN;
        return;
    }
    direction(list_ab, n_a, &rec->max_ab, &rec->p95_ab, &rec->sum_ab);
    direction(list_ba, n_b, &rec->max_ba, &rec->p95_ba, &rec->sum_ba);
    const uint64_t hd = rec->max_ab > rec->max_ba ? rec->max_ab : rec->max_ba;
    const uint64_t hd95 = rec->p95_ab > rec->p95_ba ? rec->p95_ab : rec->p95_ba;
    rec->hausdorff_mm = sqrt((double)hd) / 1000.0;
    rec->hd95_mm = sqrt((double)hd95) / 1000.0;
    rec->assd_mm = (rec->sum_ab + rec->sum_ba) / (double)(n_a + n_b) / 1000.0;
}
