/*
 * fuse_host_san.c -- a stand-alone program over 3d_sift_cuda_amd/csrc/fuse_host.c for a build with -fsanitize=address,undefined
 * (tests/test_fuse_cpu.py builds and runs it as a process of its own; nothing is loaded into Python under a sanitizer).  It drives
 * every function of the file through its widest arguments and edge values and prints the results, which the test compares with
 * those of the unsanitized library.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "sift3d.h"

int main(void)
{
    sift3d_fuse_params p;
    sift3d_fuse_defaults(&p);
    printf("defaults %d %d %d %g %lld\n", p.block, p.metric, p.power, (double)p.fill, (long long)p.max_voxels);
    /* the widest sums: 13^3 voxels of 0 / 1023 */
    const int64_t N = 2197, q = 1023, h = N / 2;
    const int64_t cases[][6] = {
        {N, q * N, q * q * N, q * N, q * q * N, q * q * N}, /* identical, flat */
        {N, q * h, q * q * h, q * h, q * q * h, q * q * h}, /* identical, half 0 and half 1023 */
        {N, q * h, q * q * h, q * (N - h), q * q * (N - h), 0}, /* complementary: the largest D */
        {N, q * N, q * q * N, 0, 0, 0},
        {1, 5, 25, 5, 25, 25},
        {1, 0, 0, 1023, 1023 * 1023, 0},
        {2, 3, 5, 30, 500, 50},
        {0, 0, 0, 0, 0, 0},
        {-1, 0, 0, 0, 0, 0},
    };
    for (size_t c = 0; c < sizeof cases / sizeof cases[0]; c++)
        for (int metric = -1; metric <= 2; metric++)
            printf("u %zu %d %u\n", c, metric, sift3d_fuse_similarity(metric, cases[c][0], cases[c][1], cases[c][2], cases[c][3], cases[c][4], cases[c][5]));
    /* labels: every kind of voxel */
    const float good[] = {0.0f, 65535.0f, 7.0f, NAN, INFINITY, -INFINITY, 7.0f, -0.0f};
    const float other[] = {0.0f, 7.0f, 7.0f, 3.0f, NAN, 65535.0f, NAN, 0.0f};
    const float bad[][2] = {{0.5f, 0}, {-1.0f, 0}, {65536.0f, 0}, {1e30f, 0}, {-1e30f, 0}, {65534.5f, 0}};
    const int n = (int)(sizeof good / sizeof good[0]);
    printf("check %lld\n", (long long)sift3d_fuse_check_labels(good, n));
    for (size_t c = 0; c < sizeof bad / sizeof bad[0]; c++) printf("check bad %zu %lld\n", c, (long long)sift3d_fuse_check_labels(bad[c], 2));
    int64_t *cnt = (int64_t *)malloc(sizeof(int64_t) * 3 * 65536);
    if (!cnt) return 2;
    printf("overlap %lld\n", (long long)sift3d_label_overlap(good, other, n, cnt, cnt + 65536, cnt + 2 * 65536));
    for (int l = 0; l < 65536; l++)
        if (cnt[l] || cnt[65536 + l] || cnt[2 * 65536 + l])
            printf("label %d %lld %lld %lld\n", l, (long long)cnt[l], (long long)cnt[65536 + l], (long long)cnt[2 * 65536 + l]);
    printf("overlap bad %lld\n", (long long)sift3d_label_overlap(good, bad[0], 2, cnt, cnt + 65536, cnt + 2 * 65536));
    printf("overlap null %lld\n", (long long)sift3d_label_overlap(NULL, other, n, cnt, cnt + 65536, cnt + 2 * 65536));
    free(cnt);
    return 0;
}
