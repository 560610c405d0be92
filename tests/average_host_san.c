/*
 * average_host_san.c -- average_host.c as a stand-alone program (test infrastructure): every host helper of the template on
 * ordinary and on refused arguments, each result printed as a line.  tests/test_average_cpu.py builds it with and without
 * -fsanitize=address,undefined; both runs exit clean and print the same lines, and the test holds the lines to the oracle.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sift3d.h"

static void check(const char *name, const sift3d_average_params *p, int K, int64_t err_len)
{
    char *err = err_len > 0 ? (char *)malloc((size_t)err_len) : NULL; /* exactly err_len bytes: an overrun shows */
    const int rc = sift3d_average_check(p, K, err, err_len);
    printf("check %s %d %s\n", name, rc, err && rc != 0 ? err : "");
    free(err);
}

/* a field of n nodes per axis whose floats are on the heap, exactly 3 n0 n1 n2 of them: value = scale * index + k */
static sift3d_field make_field(int64_t n0, int64_t n1, int64_t n2, float scale, float shift)
{
    sift3d_field f;
    memset(&f, 0, sizeof f);
    f.n[0] = n0;
    f.n[1] = n1;
    f.n[2] = n2;
    f.origin[0] = -1.5f;
    f.origin[1] = 2.0f;
    f.origin[2] = 0.25f;
    f.spacing = 4.0f;
    f.capacity = 3 * n0 * n1 * n2;
    f.disp = (float *)malloc(sizeof(float) * (size_t)f.capacity);
    for (int64_t i = 0; i < f.capacity; i++) f.disp[i] = scale * (float)i / 7.0f + shift;
    return f;
}

static void mean(const char *name, int K, const sift3d_field *fields, sift3d_field *out, int print)
{
    char err[160] = "";
    const int rc = sift3d_mean_field(K, fields, out, err, sizeof err);
    printf("mean %s %d %s", name, rc, rc == 0 ? "" : err);
    if (rc == 0 && print)
        for (int64_t i = 0; i < 3 * out->n[0] * out->n[1] * out->n[2]; i++) printf(" %a", (double)out->disp[i]);
    printf("\n");
}

int main(void)
{
    sift3d_average_params p, q;
    sift3d_average_defaults(&p);
    printf("defaults %d %d %s %d %lld %d\n", p.trim, p.min_count, isnan(p.fill) ? "nan" : "number", p.device, (long long)p.max_voxels, p.form);
    check("null", NULL, 3, 64);
    check("defaults", &p, 1, 64);
    check("K 0", &p, 0, 64);
    check("K 33", &p, 33, 64);
    check("K 32", &p, 32, 64);
#define CASE(NAME, K, STMT) \
    q = p;                  \
    STMT;                   \
    check(NAME, &q, K, 96)
    CASE("trim -1", 5, q.trim = -1);
    CASE("trim 15", 5, q.trim = 15);
    CASE("trim 16", 5, q.trim = 16);
    CASE("min_count 0", 5, q.min_count = 0);
    CASE("min_count 5", 5, q.min_count = 5);
    CASE("min_count 6", 5, q.min_count = 6);
    CASE("max_voxels 0", 5, q.max_voxels = 0);
    CASE("form 0", 5, q.form = 0);
    CASE("form 1", 5, q.form = 1);
    CASE("form -2", 5, q.form = -2);
    CASE("short_err", 5, q.trim = 16);
    q = p;
    q.trim = 16;
    check("short_err 9", &q, 5, 9);
    check("no_err", &q, 5, 0);

    /* the counts: a mask plane on the heap, exactly n words */
    const int64_t n = 9;
    uint32_t *mask = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)n);
    const uint32_t words[9] = {0u, 1u, 2u, 3u, 7u, 5u, 0u, 4u, 7u};
    memcpy(mask, words, sizeof words);
    sift3d_average_report *rep = (sift3d_average_report *)malloc(sizeof *rep);
    memset(rep, 0, sizeof *rep);
    rep->kernel_ms = 1.5;
    rep->wall_ms = 20.25;
    rep->image[1].upload_ms = 0.125;
    int rc = sift3d_average_counts(mask, n, 3, 1, 2, rep);
    printf("counts %d %d %d %d %lld %lld %lld :", rc, rep->images, rep->trim, rep->min_count, (long long)rep->voxels, (long long)rep->none, (long long)rep->below);
    for (int c = 0; c <= 3; c++) printf(" %lld", (long long)rep->count[c]);
    printf(" :");
    for (int k = 0; k < 3; k++) printf(" %lld", (long long)rep->image[k].contributing);
    printf("\n");
    printf("counts stray_bit %d\n", sift3d_average_counts(mask, n, 2, 0, 1, rep));
    printf("counts refused %d %d %d %d\n", sift3d_average_counts(NULL, n, 3, 0, 1, rep), sift3d_average_counts(mask, n, 0, 0, 1, rep),
           sift3d_average_counts(mask, n, 33, 0, 1, rep), sift3d_average_counts(mask, n, 3, 0, 1, NULL));
    mask[0] = 0x80000000u;
    rc = sift3d_average_counts(mask, n, 32, 0, 1, rep);
    printf("counts K32 %d %lld\n", rc, (long long)rep->image[31].contributing);
    memcpy(mask, words, sizeof words);
    sift3d_average_counts(mask, n, 3, 1, 2, rep);

    /* the report: the whole text at the length asked for, and every shorter buffer a prefix of it */
    const int64_t need = sift3d_average_report_text(rep, NULL, 0);
    char *text = (char *)malloc((size_t)need + 1);
    const int64_t got = sift3d_average_report_text(rep, text, need + 1);
    printf("report %lld %lld %zu\n%s", (long long)need, (long long)got, strlen(text), text);
    for (int64_t len = 1; len <= need; len += 17) {
        char *part = (char *)malloc((size_t)len);
        const int64_t r = sift3d_average_report_text(rep, part, len);
        printf("report part %lld %lld %zu %d\n", (long long)len, (long long)r, strlen(part), strncmp(part, text, (size_t)len - 1));
        free(part);
    }
    rep->images = 0;
    printf("report refused %lld %lld\n", (long long)sift3d_average_report_text(NULL, text, need), (long long)sift3d_average_report_text(rep, text, need));
    free(text);
    free(rep);
    free(mask);

    /* the mean field */
    sift3d_field f[3] = {make_field(2, 3, 2, 1.0f, 0.0f), make_field(2, 3, 2, -2.5f, 1.0f), make_field(2, 3, 2, 0.3f, -4.0f)};
    sift3d_field out;
    memset(&out, 0, sizeof out);
    mean("capacity", 3, f, &out, 0);
    printf("mean grid %lld %lld %lld %a %a %a %a\n", (long long)out.n[0], (long long)out.n[1], (long long)out.n[2], (double)out.origin[0], (double)out.origin[1],
           (double)out.origin[2], (double)out.spacing);
    out.capacity = 3 * 12;
    out.disp = (float *)malloc(sizeof(float) * (size_t)out.capacity);
    mean("three", 3, f, &out, 1);
    mean("one", 1, f + 1, &out, 1);
    mean("K 0", 0, f, &out, 0);
    mean("K 33", 33, f, &out, 0);
    mean("null", 2, NULL, &out, 0);
    mean("null out", 2, f, NULL, 0);
    sift3d_field g = f[1];
    g.n[1] = 4;
    sift3d_field pair[2] = {f[0], g};
    mean("n differs", 2, pair, &out, 0);
    g = f[1];
    g.origin[2] = 0.5f;
    pair[1] = g;
    mean("origin differs", 2, pair, &out, 0);
    g = f[1];
    g.origin[0] = -0.0f;
    pair[0].origin[0] = 0.0f;
    pair[1] = g;
    mean("origin sign differs", 2, pair, &out, 0);
    pair[0] = f[0];
    g = f[1];
    g.spacing = 4.5f;
    pair[1] = g;
    mean("spacing differs", 2, pair, &out, 0);
    g = f[1];
    g.capacity = 35;
    pair[1] = g;
    mean("short disp", 2, pair, &out, 0);
    g = f[1];
    g.disp = NULL;
    pair[1] = g;
    mean("null disp", 2, pair, &out, 0);
    g = f[0];
    g.n[0] = 1;
    pair[0] = g;
    mean("one node", 2, pair, &out, 0);
    free(out.disp);
    for (int k = 0; k < 3; k++) free(f[k].disp);
    return 0;
}
