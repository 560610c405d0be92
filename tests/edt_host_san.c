/*
 * edt_host_san.c -- a stand-alone program over 3d_sift_cuda_amd/csrc/edt_host.c for a build with -fsanitize=address,undefined
 * (tests/test_edt_cpu.py builds and runs it as a process of its own; nothing is loaded into Python under a sanitizer).  It drives
 * every function of the file through its edge values and prints the results, which the test compares with those of the
 * unsanitized build and with its own restatement.
 */
#include <inttypes.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sift3d.h"

static void print_record(const char *name, const sift3d_surface_record *r)
{
    uint64_t b[5];
    const double d[5] = {r->sum_ab, r->sum_ba, r->hausdorff_mm, r->hd95_mm, r->assd_mm};
    memcpy(b, d, sizeof b);
    printf("stats %s %lld %lld %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", name,
           (long long)r->n_a, (long long)r->n_b, r->max_ab, r->max_ba, r->p95_ab, r->p95_ba, b[0], b[1], b[2], b[3], b[4]);
}

int main(void)
{
    sift3d_surface_params p;
    sift3d_surface_defaults(&p);
    printf("defaults %d %d %d\n", p.first_label, p.max_labels, p.device);
    const float mm[] = {1.0f, 0.001f, 0.0004f, 0.0005f, 65.535f, 65.536f, 70.0f, 0.0f, -1.0f, 0.7f, 1e30f, -1e30f, NAN, INFINITY, -INFINITY};
    for (size_t c = 0; c < sizeof mm / sizeof mm[0]; c++) {
        uint32_t um = 0;
        const int rc = sift3d_spacing_um(mm[c], &um);
        printf("spacing %zu %d %u\n", c, rc, (unsigned)um);
    }
    printf("spacing null %d\n", sift3d_spacing_um(1.0f, NULL));
    /* lists of every length around the percentile's steps, the largest distances, equal elements, and an empty direction */
    const int64_t sizes[] = {1, 2, 19, 20, 21, 100, 101};
    sift3d_surface_record r;
    for (size_t c = 0; c < sizeof sizes / sizeof sizes[0]; c++) {
        const int64_t n = sizes[c], m = n / 2 + 1;
        uint64_t *ab = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)n), *ba = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)m);
        if (!ab || !ba) return 2;
        for (int64_t i = 0; i < n; i++) ab[i] = (uint64_t)((n - i) * (n - i)) * 1000000u; /* descending: the sort has work to do */
        for (int64_t i = 0; i < m; i++) ba[i] = i % 3 == 0 ? 216060648083791875ull : 49000000ull; /* 3 (4095 * 65535)^2 and equal elements */
        memset(&r, 0, sizeof r);
        sift3d_surface_stats(ab, n, ba, m, &r);
        char name[32];
        snprintf(name, sizeof name, "%lld", (long long)n);
        print_record(name, &r);
        for (int64_t i = 1; i < n; i++)
            if (ab[i - 1] > ab[i]) return 3; /* sorted in place */
        memset(&r, 0, sizeof r);
        sift3d_surface_stats(ab, n, NULL, 0, &r);
        print_record("absent_b", &r);
        sift3d_surface_stats(NULL, 0, ba, m, &r);
        print_record("absent_a", &r);
        free(ab);
        free(ba);
    }
    sift3d_surface_stats(NULL, 0, NULL, 0, &r);
    print_record("absent_both", &r);
    return 0;
}
