/*
 * ccl_host_san.c -- a stand-alone program over 3d_sift_cuda_amd/csrc/ccl_host.c for a build with -fsanitize=address,undefined
 * (tests/test_ccl_cpu.py builds and runs it as a process of its own; nothing is loaded into Python under a sanitizer).  It drives
 * every function of the file through its edge values and prints the results, which the test compares with those of the
 * unsanitized build and with its own restatement.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sift3d.h"

static void check(const char *what, int value, const sift3d_clean_params *p)
{
    char err[128] = "";
    const int rc = sift3d_clean_check(p, err, sizeof err);
    printf("check %s %d %d %s\n", what, value, rc, err);
}

int main(void)
{
    sift3d_clean_params p;
    sift3d_clean_defaults(&p);
    printf("defaults %d %d %d %d\n", p.min_voxels, p.connectivity, p.rounds, p.device);
    char err[128] = "";
    printf("check null %d %s\n", sift3d_clean_check(NULL, err, sizeof err), err);
    const int min_voxels[] = {0, 1, 8, 16777216, 16777217, -1}, connectivity[] = {6, 26, 18, 0}, rounds[] = {0, 1, 16, 17};
    for (size_t c = 0; c < sizeof min_voxels / sizeof min_voxels[0]; c++) {
        sift3d_clean_defaults(&p);
        p.min_voxels = min_voxels[c];
        check("min_voxels", min_voxels[c], &p);
    }
    for (size_t c = 0; c < sizeof connectivity / sizeof connectivity[0]; c++) {
        sift3d_clean_defaults(&p);
        p.connectivity = connectivity[c];
        check("connectivity", connectivity[c], &p);
    }
    for (size_t c = 0; c < sizeof rounds / sizeof rounds[0]; c++) {
        sift3d_clean_defaults(&p);
        p.rounds = rounds[c];
        check("rounds", rounds[c], &p);
    }
    /* a text that does not fit is cut, and no text is wanted at all */
    sift3d_clean_defaults(&p);
    p.min_voxels = 0;
    char tiny[7];
    memset(tiny, 'x', sizeof tiny);
    printf("check short_err %d %s\n", sift3d_clean_check(&p, tiny, sizeof tiny), tiny);
    printf("check no_err %d \n", sift3d_clean_check(&p, NULL, 0));
    const long long ext[][3] = {{1, 1, 1}, {4096, 4096, 64}, {4096, 4096, 65}, {0, 1, 1}, {1, 4097, 1}, {1, 1, -5}, {4096, 1, 4096}};
    for (size_t c = 0; c < sizeof ext / sizeof ext[0]; c++) {
        err[0] = 0;
        const int rc = sift3d_ccl_check_extents(ext[c][0], ext[c][1], ext[c][2], err, sizeof err);
        printf("extents %lld %lld %lld %d %s\n", ext[c][0], ext[c][1], ext[c][2], rc, err);
    }
    printf("extents no_err %d\n", sift3d_ccl_check_extents(0, 0, 0, NULL, 0));
    /* the report: every round in use and the largest counts; buffers of every kind of length */
    sift3d_clean_report rep;
    memset(&rep, 0, sizeof rep);
    rep.rounds_run = SIFT3D_CLEAN_MAX_ROUNDS;
    for (int r = 0; r < SIFT3D_CLEAN_MAX_ROUNDS; r++) {
        int64_t *f = &rep.round[r].components;
        for (int c = 0; c < 6; c++) f[c] = ((int64_t)1 << 62) - r * 7 - c;
    }
    rep.total.components = 5;
    rep.total.resolved_voxels = (int64_t)1 << 30;
    printf("report null %lld\n", (long long)sift3d_clean_report_text(NULL, NULL, 0));
    char *text = (char *)malloc(4096);
    if (!text) return 2;
    const int64_t need = sift3d_clean_report_text(&rep, text, 4096);
    if (need < 0 || need >= 4096 || (int64_t)strlen(text) != need) return 3;
    printf("report full %lld\n%s", (long long)need, text);
    if (sift3d_clean_report_text(&rep, NULL, 0) != need) return 4;
    const int64_t rooms[] = {0, 1, 2, 100, need, need + 1};
    for (size_t c = 0; c < sizeof rooms / sizeof rooms[0]; c++) {
        char *buf = (char *)malloc((size_t)(rooms[c] > 0 ? rooms[c] : 1)); /* exactly the room: a write beyond it is the sanitizer's to find */
        if (!buf) return 2;
        const int64_t got = sift3d_clean_report_text(&rep, rooms[c] > 0 ? buf : NULL, rooms[c]);
        printf("report room %lld %lld [%s]\n", (long long)rooms[c], (long long)got, rooms[c] > 0 ? buf : "");
        free(buf);
    }
    rep.rounds_run = 1000; /* beyond the array: read as 16 */
    printf("report over %lld\n%s", (long long)sift3d_clean_report_text(&rep, text, 4096), text);
    rep.rounds_run = -3;
    if (sift3d_clean_report_text(&rep, text, 4096) <= 0 || strstr(text, "# rounds run 0\n") == NULL) return 5;
    free(text);
    return 0;
}
