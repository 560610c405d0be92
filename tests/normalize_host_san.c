/*
 * normalize_host_san.c -- a stand-alone program over 3d_sift_cuda_amd/csrc/normalize_host.c (test infrastructure): every host
 * helper of DESIGN.md section 7s on planted inputs, with its results on the standard output.  tests/test_normalize_cpu.py builds it
 * with and without -fsanitize=address,undefined and compares the two outputs (the tables are held to the oracle through the library).
 */
#include <inttypes.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sift3d.h"

static uint32_t state = 12345u;
static uint32_t next(void) { return state = state * 1664525u + 1013904223u; }

/* two histograms of n voxels each and sums that agree with them in sums[0]; kind 0: spread, 1: one dominant bin, 2: many empty bins */
static void plant(int kind, int64_t n, int64_t *ha, int64_t *hb, int64_t *sums)
{
    memset(ha, 0, sizeof(int64_t) * SIFT3D_NORMALIZE_BINS);
    memset(hb, 0, sizeof(int64_t) * SIFT3D_NORMALIZE_BINS);
    memset(sums, 0, sizeof(int64_t) * SIFT3D_SIMILARITY_SUMS);
    for (int64_t i = 0; i < n; i++) {
        int a = (int)(next() >> 22), b = (int)(next() >> 22);
        if (kind == 1 && i % 10) a = 500, b = 17;
        if (kind == 2) a = a / 64 * 64, b = b / 128 * 128 + 3;
        ha[a]++;
        hb[b]++;
        sums[0] += 1;
        sums[1] += a;
        sums[2] += b;
        sums[3] += (int64_t)a * a;
        sums[4] += (int64_t)b * b;
        sums[5] += (int64_t)a * b;
    }
}

static void show_table(const char *name, int rc, const sift3d_transfer *t, const char *err)
{
    printf("%s %d %s", name, rc, err);
    if (rc == 0) {
        printf("m %d tail %a wa %a :", (int)t->m, t->tail, t->wa);
        for (int k = 0; k < t->m; k++) printf(" %a %a %a", t->xb[k], t->xa[k], t->slope[k]);
    }
    printf("\n");
}

int main(void)
{
    sift3d_normalize_params p;
    sift3d_normalize_defaults(&p);
    printf("defaults %d %d %d\n", (int)p.mode, (int)p.knots, (int)p.device);
    char err[256], tiny[9];
    err[0] = 0;
    printf("check null %d %s\n", sift3d_normalize_check(NULL, err, sizeof err), err);
    err[0] = 0;
    printf("check defaults %d %s\n", sift3d_normalize_check(&p, err, sizeof err), err);
    for (int mode = -1; mode <= 2; mode++) {
        sift3d_normalize_defaults(&p);
        p.mode = mode;
        err[0] = 0;
        printf("check mode %d %d %s\n", mode, sift3d_normalize_check(&p, err, sizeof err), err);
    }
    const int qs[] = {1, 2, 256, 257, -5};
    for (int e = 0; e < 5; e++)
        for (int mode = 0; mode <= 1; mode++) {
            sift3d_normalize_defaults(&p);
            p.mode = mode;
            p.knots = qs[e];
            err[0] = 0;
            printf("check knots %d mode %d %d %s\n", qs[e], mode, sift3d_normalize_check(&p, err, sizeof err), err);
        }
    p.mode = 7;
    tiny[0] = 0;
    printf("check short_err %d %s\n", sift3d_normalize_check(&p, tiny, sizeof tiny), tiny);
    printf("check no_err %d\n", sift3d_normalize_check(&p, NULL, 0));

    int64_t *ha = (int64_t *)malloc(sizeof(int64_t) * SIFT3D_NORMALIZE_BINS), *hb = (int64_t *)malloc(sizeof(int64_t) * SIFT3D_NORMALIZE_BINS), sums[SIFT3D_SIMILARITY_SUMS];
    sift3d_transfer *t = (sift3d_transfer *)malloc(sizeof *t);
    sift3d_normalize_report *rep = (sift3d_normalize_report *)calloc(1, sizeof *rep);
    if (!ha || !hb || !t || !rep) return 1;
    const float ar[2] = {-100.0f, 923.0f}, br[2] = {0.5f, 2.25f}, bad[2] = {1.0f, 1.0f}, nanr[2] = {0.0f, NAN};
    const int64_t ns[] = {2, 3, 1000, 100000};
    const int Q[] = {2, 64, 256};
    for (int kind = 0; kind < 3; kind++)
        for (int e = 0; e < 4; e++) {
            plant(kind, ns[e], ha, hb, sums);
            char name[64];
            err[0] = 0;
            snprintf(name, sizeof name, "table linear kind %d n %d", kind, (int)ns[e]);
            show_table(name, sift3d_normalize_transfer(SIFT3D_NORMALIZE_LINEAR, 64, ha, hb, sums, ar, br, t, err, sizeof err), t, err);
            for (int q = 0; q < 3; q++) {
                err[0] = 0;
                snprintf(name, sizeof name, "table hist %d kind %d n %d", Q[q], kind, (int)ns[e]);
                const int rc = sift3d_normalize_transfer(SIFT3D_NORMALIZE_HIST, Q[q], ha, hb, sums, ar, br, t, err, sizeof err);
                show_table(name, rc, t, err);
                if (rc == 0) {
                    err[0] = 0;
                    printf("table check %d %s\n", sift3d_transfer_check(t, err, sizeof err), err);
                }
            }
        }
    /* the refusals */
    plant(0, 1000, ha, hb, sums);
    err[0] = 0;
    printf("transfer null %d %s\n", sift3d_normalize_transfer(0, 64, NULL, hb, sums, ar, br, t, err, sizeof err), err);
    printf("transfer mode %d %s\n", sift3d_normalize_transfer(2, 64, ha, hb, sums, ar, br, t, err, sizeof err), err);
    printf("transfer knots %d %s\n", sift3d_normalize_transfer(1, 1, ha, hb, sums, ar, br, t, err, sizeof err), err);
    printf("transfer a_range %d %s\n", sift3d_normalize_transfer(0, 64, ha, hb, sums, bad, br, t, err, sizeof err), err);
    printf("transfer b_range %d %s\n", sift3d_normalize_transfer(0, 64, ha, hb, sums, ar, nanr, t, err, sizeof err), err);
    sums[0]++;
    printf("transfer total %d %s\n", sift3d_normalize_transfer(0, 64, ha, hb, sums, ar, br, t, err, sizeof err), err);
    sums[0]--;
    ha[5] -= 1000000;
    printf("transfer negative %d %s\n", sift3d_normalize_transfer(0, 64, ha, hb, sums, ar, br, t, err, sizeof err), err);
    plant(0, 1, ha, hb, sums);
    printf("transfer one %d %s\n", sift3d_normalize_transfer(1, 64, ha, hb, sums, ar, br, t, err, sizeof err), err);
    plant(0, 0, ha, hb, sums);
    printf("transfer none %d %s\n", sift3d_normalize_transfer(0, 64, ha, hb, sums, ar, br, t, err, sizeof err), err);
    /* every voxel of the image in one bin, then of the reference: no variance for linear; hist ranks its knots inside the bin */
    plant(0, 1000, ha, hb, sums);
    memset(hb, 0, sizeof(int64_t) * SIFT3D_NORMALIZE_BINS);
    hb[1023] = 1000;
    sums[2] = 1000 * 1023;
    sums[4] = (int64_t)1000 * 1023 * 1023;
    printf("transfer flat image linear %d %s\n", sift3d_normalize_transfer(0, 64, ha, hb, sums, ar, br, t, err, sizeof err), err);
    printf("transfer flat image hist %d %s\n", sift3d_normalize_transfer(1, 64, ha, hb, sums, ar, br, t, err, sizeof err), err);
    plant(0, 1000, ha, hb, sums);
    memset(ha, 0, sizeof(int64_t) * SIFT3D_NORMALIZE_BINS);
    ha[0] = 1000;
    sums[1] = sums[3] = 0;
    printf("transfer flat reference linear %d %s\n", sift3d_normalize_transfer(0, 64, ha, hb, sums, ar, br, t, err, sizeof err), err);
    printf("transfer flat reference hist %d %s\n", sift3d_normalize_transfer(1, 2, ha, hb, sums, ar, br, t, err, sizeof err), err);
    tiny[0] = 0;
    printf("transfer short_err %d %s\n", sift3d_normalize_transfer(5, 2, ha, hb, sums, ar, br, t, tiny, sizeof tiny), tiny);

    /* a table's check */
    plant(0, 1000, ha, hb, sums);
    sift3d_normalize_transfer(1, 8, ha, hb, sums, ar, br, t, err, sizeof err);
    sift3d_transfer u = *t;
    printf("tcheck null %d %s\n", sift3d_transfer_check(NULL, err, sizeof err), err);
    u.m = 1;
    printf("tcheck m %d %s\n", sift3d_transfer_check(&u, err, sizeof err), err);
    u.m = 258;
    printf("tcheck m %d %s\n", sift3d_transfer_check(&u, err, sizeof err), err);
    u = *t;
    u.xb[3] = u.xb[2];
    printf("tcheck xb %d %s\n", sift3d_transfer_check(&u, err, sizeof err), err);
    u = *t;
    u.xa[4] = u.xa[3] - 1.0;
    printf("tcheck xa %d %s\n", sift3d_transfer_check(&u, err, sizeof err), err);
    u = *t;
    u.xa[1] = NAN;
    printf("tcheck nan %d %s\n", sift3d_transfer_check(&u, err, sizeof err), err);
    u = *t;
    u.b_hi = u.b_lo;
    printf("tcheck range %d %s\n", sift3d_transfer_check(&u, err, sizeof err), err);
    u = *t;
    u.tail = INFINITY;
    printf("tcheck tail %d %s\n", sift3d_transfer_check(&u, err, sizeof err), err);

    /* the report: the whole text at the length asked for, and every shorter buffer a prefix of it */
    rep->mode = SIFT3D_NORMALIZE_HIST;
    rep->knots = 8;
    rep->reference_voxels = 1200;
    rep->image_voxels = 999;
    rep->counts[0] = 100;
    rep->counts[1] = 60;
    rep->counts[2] = 40;
    memcpy(rep->sums, sums, sizeof sums);
    rep->hist_ms = 1.5;
    rep->apply_ms = 0.25;
    rep->wall_ms = 20.125;
    rep->table = *t;
    const int64_t need = sift3d_normalize_report_text(rep, NULL, 0);
    char *text = (char *)malloc((size_t)need + 1), *part = (char *)malloc((size_t)need + 1);
    if (!text || !part) return 1;
    const int64_t got = sift3d_normalize_report_text(rep, text, need + 1);
    printf("report %" PRId64 " %" PRId64 " %zu\n%s", need, got, strlen(text), text);
    const int64_t lens[] = {1, 2, 17, 100, need};
    for (int e = 0; e < 5; e++) {
        memset(part, 'x', (size_t)need + 1);
        const int64_t r = sift3d_normalize_report_text(rep, part, lens[e]);
        printf("report part %" PRId64 " %" PRId64 " %zu %d\n", lens[e], r, strlen(part), strncmp(part, text, strlen(part)));
    }
    rep->table.m = 1;
    printf("report refused %" PRId64 " %" PRId64 "\n", sift3d_normalize_report_text(rep, text, need + 1), sift3d_normalize_report_text(NULL, text, need + 1));
    free(part);
    free(text);
    free(rep);
    free(t);
    free(hb);
    free(ha);
    return 0;
}
