/*
 * fuse_search_host_san.c -- a stand-alone program over the search helpers of 3d_sift_cuda_amd/csrc/fuse_host.c
 * for a build with -fsanitize=address,undefined (tests/test_fuse_search_cpu.py builds and runs it as a process of its own; nothing is
 * loaded into Python under a sanitizer).  It drives sift3d_fuse_shift_code, sift3d_fuse_shift_of and sift3d_fuse_shift_stats through
 * every radius, every shift, the values next to their bounds and NULL, and prints the results, which the test compares with those
 * of the unsanitized build.
 */
#include <stdio.h>
#include <stdlib.h>

#include "sift3d.h"

int main(void)
{
    for (int r = -1; r <= SIFT3D_FUSE_MAX_SEARCH + 1; r++) {
        long long sum = 0, bad = 0, back = 0;
        for (int tz = -5; tz <= 5; tz++)
            for (int ty = -5; ty <= 5; ty++)
                for (int tx = -5; tx <= 5; tx++) {
                    const uint16_t c = sift3d_fuse_shift_code(r, tx, ty, tz);
                    int32_t t[3] = {99, 99, 99};
                    if (c == SIFT3D_FUSE_NO_SHIFT) {
                        bad++;
                        continue;
                    }
                    sum += c;
                    back += sift3d_fuse_shift_of(r, c, t) == 0 && t[0] == tx && t[1] == ty && t[2] == tz;
                }
        printf("radius %d codes sum %lld refused %lld back %lld\n", r, sum, bad, back);
        int32_t t[3] = {0, 0, 0};
        const uint32_t edge[] = {0u, 26u, 27u, 124u, 125u, 342u, 343u, 0xffffu, 0xffffffffu};
        for (size_t e = 0; e < sizeof edge / sizeof edge[0]; e++) {
            const int rc = sift3d_fuse_shift_of(r, edge[e], t);
            printf("of %d %u %d %d %d %d\n", r, edge[e], rc, t[0], t[1], t[2]);
        }
    }
    printf("of null %d\n", sift3d_fuse_shift_of(1, 0, NULL));
    printf("code -3 -3 -3 %u  3 3 3 %u  0 0 0 %u\n", sift3d_fuse_shift_code(3, -3, -3, -3), sift3d_fuse_shift_code(3, 3, 3, 3), sift3d_fuse_shift_code(3, 0, 0, 0));
    /* a plane of every code of radius 3, twice, and some voxels without a vote */
    const int64_t n = 2 * 343 + 5;
    uint16_t *plane = (uint16_t *)malloc(sizeof(uint16_t) * (size_t)n);
    if (!plane) return 2;
    for (int64_t i = 0; i < n; i++) plane[i] = i < 2 * 343 ? (uint16_t)(i % 343) : SIFT3D_FUSE_NO_SHIFT;
    int64_t moved = -1, d2 = -1;
    printf("stats %lld", (long long)sift3d_fuse_shift_stats(3, plane, n, &moved, &d2));
    printf(" %lld %lld\n", (long long)moved, (long long)d2);
    printf("stats under 2 %lld", (long long)sift3d_fuse_shift_stats(2, plane, n, &moved, &d2)); /* code 125 is none under r = 2 */
    printf(" %lld %lld\n", (long long)moved, (long long)d2);
    printf("stats none %lld\n", (long long)sift3d_fuse_shift_stats(3, plane + 2 * 343, 5, NULL, NULL));
    printf("stats empty %lld\n", (long long)sift3d_fuse_shift_stats(0, plane, 0, &moved, &d2));
    printf("stats null %lld radius %lld\n", (long long)sift3d_fuse_shift_stats(1, NULL, 4, &moved, &d2), (long long)sift3d_fuse_shift_stats(4, plane, 4, &moved, &d2));
    free(plane);
    return 0;
}
