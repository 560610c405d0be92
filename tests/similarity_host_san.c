/*
 * similarity_host_san.c -- a stand-alone program over 3d_sift_cuda_amd/csrc/similarity_host.c for a build with
 * -fsanitize=address,undefined (tests/test_similarity_cpu.py builds and runs it as a process of its own; nothing is loaded into
 * Python under a sanitizer).  It drives every function of the file through its edge values and prints the results, which the test
 * compares with those of the unsanitized build and with its own restatement.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sift3d.h"

static void check(const char *what, int value, const sift3d_similarity_params *p)
{
    char err[128] = "";
    const int rc = sift3d_similarity_check(p, err, sizeof err);
    printf("check %s %d %d %s\n", what, value, rc, err);
}

static void print_measures(const char *what, const sift3d_similarity_record *r)
{
    const double v[7] = {r->mi, r->nmi, r->rho, r->rms, r->h_a, r->h_b, r->h_ab};
    printf("measures %s %d %d", what, (int)r->bins, (int)r->same_scale);
    for (int k = 0; k < 7; k++) {
        if (isnan(v[k])) printf(" nan");
        else printf(" %.17g", v[k]);
    }
    printf("\n");
}

int main(void)
{
    sift3d_similarity_params p;
    sift3d_similarity_defaults(&p);
    printf("defaults %d %d %d %d %d\n", p.bins, p.same_scale, p.max_labels, p.device, p.flush);
    char err[128] = "";
    printf("check null %d %s\n", sift3d_similarity_check(NULL, err, sizeof err), err);
    const int bins[] = {8, 16, 32, 64, 0, 7, 128, -8}, same[] = {0, 1, 2, -1}, labels[] = {0, 1, 64, 65}, flush[] = {0, 1, 2, -1};
    for (size_t c = 0; c < sizeof bins / sizeof bins[0]; c++) {
        sift3d_similarity_defaults(&p);
        p.bins = bins[c];
        check("bins", bins[c], &p);
    }
    for (size_t c = 0; c < sizeof same / sizeof same[0]; c++) {
        sift3d_similarity_defaults(&p);
        p.same_scale = same[c];
        check("same_scale", same[c], &p);
    }
    for (size_t c = 0; c < sizeof labels / sizeof labels[0]; c++) {
        sift3d_similarity_defaults(&p);
        p.max_labels = labels[c];
        check("max_labels", labels[c], &p);
    }
    for (size_t c = 0; c < sizeof flush / sizeof flush[0]; c++) {
        sift3d_similarity_defaults(&p);
        p.flush = flush[c];
        check("flush", flush[c], &p);
    }
    /* a text that does not fit is cut, and no text is wanted at all */
    sift3d_similarity_defaults(&p);
    p.bins = 7;
    char tiny[7];
    memset(tiny, 'x', sizeof tiny);
    printf("check short_err %d %s\n", sift3d_similarity_check(&p, tiny, sizeof tiny), tiny);
    printf("check no_err %d \n", sift3d_similarity_check(&p, NULL, 0));

    /* the measures: histograms of exactly bins^2 words, so that a read beyond them is the sanitizer's to find */
    sift3d_similarity_record *rec = (sift3d_similarity_record *)calloc(1, sizeof *rec);
    if (!rec) return 2;
    const int all_bins[] = {8, 16, 32, 64};
    for (int b = 0; b < 4; b++) {
        const int nb = all_bins[b];
        int64_t *h = (int64_t *)calloc((size_t)(nb * nb), sizeof(int64_t));
        if (!h) return 2;
        /* the diagonal: cell (i, i) holds i + 1 voxels of q = i (1024 / nb) on both sides */
        int64_t s[6] = {0, 0, 0, 0, 0, 0};
        for (int i = 0; i < nb; i++) {
            const int64_t c = i + 1, q = (int64_t)i * (1024 / nb);
            h[i * nb + i] = c;
            s[0] += c;
            s[1] += c * q;
            s[3] += c * q * q;
        }
        s[2] = s[1];
        s[4] = s[5] = s[3];
        if (sift3d_similarity_measures(h, nb, s, -2.0f, 3.0f, 1, rec) != 0) return 3;
        print_measures("diagonal", rec);
        /* a product: cell (i, j) holds (i + 1) (j + 2) voxels; the sums are not read for the entropies */
        memset(s, 0, sizeof s);
        for (int i = 0; i < nb; i++)
            for (int j = 0; j < nb; j++) {
                h[i * nb + j] = (int64_t)(i + 1) * (j + 2);
                s[0] += h[i * nb + j];
            }
        if (sift3d_similarity_measures(h, nb, s, 0.0f, 1.0f, 0, rec) != 0) return 3;
        print_measures("product", rec);
        /* one cell with the largest volume: n = 2^30 voxels of q = 1023 against q = 0 */
        memset(h, 0, sizeof(int64_t) * (size_t)(nb * nb));
        const int64_t n = (int64_t)1 << 30;
        h[(nb - 1) * nb] = n;
        const int64_t top[6] = {n, 1023 * n, 0, 1023 * 1023 * n, 0, 0};
        if (sift3d_similarity_measures(h, nb, top, 0.0f, 1023.0f, 1, rec) != 0) return 3;
        print_measures("one_cell", rec);
        /* no voxel at all */
        memset(h, 0, sizeof(int64_t) * (size_t)(nb * nb));
        memset(s, 0, sizeof s);
        if (sift3d_similarity_measures(h, nb, s, 0.0f, 1.0f, 1, rec) != 0) return 3;
        print_measures("empty", rec);
        free(h);
    }
    /* the widest sums: 2^30 voxels, half at (0, 1023) and half at (1023, 0): the products reach 2^80 */
    {
        int64_t *h = (int64_t *)calloc(64 * 64, sizeof(int64_t));
        if (!h) return 2;
        const int64_t half = (int64_t)1 << 29, sq = 1023 * 1023;
        h[63] = h[63 * 64] = half;
        const int64_t s[6] = {2 * half, 1023 * half, 1023 * half, sq * half, sq * half, 0};
        if (sift3d_similarity_measures(h, 64, s, -1.0e30f, 1.0e30f, 1, rec) != 0) return 3;
        print_measures("widest", rec);
        /* the histogram inside the record itself, and its own sums */
        memcpy(rec->hist, h, sizeof(int64_t) * 64 * 64);
        if (sift3d_similarity_measures(rec->hist, 64, rec->sums, -1.0e30f, 1.0e30f, 1, rec) != 0) return 3;
        print_measures("in_place", rec);
        free(h);
    }
    printf("measures refused %d %d %d\n", sift3d_similarity_measures(NULL, 8, rec->sums, 0, 1, 0, rec), sift3d_similarity_measures(rec->hist, 7, rec->sums, 0, 1, 0, rec),
           sift3d_similarity_measures(rec->hist, 8, rec->sums, 0, 1, 0, NULL));

    sift3d_similarity_label_record lr[SIFT3D_SIMILARITY_MAX_LABELS];
    const int64_t one[6] = {1, 5, 9, 25, 81, 45}, line[6] = {3, 6, 12, 14, 56, 28}, anti[6] = {2, 1023, 1023, 1023 * 1023, 1023 * 1023, 0}, none[6] = {0, 0, 0, 0, 0, 0};
    const int64_t *rows[4] = {one, line, anti, none};
    for (int k = 0; k < 4; k++)
        for (int same_scale = 0; same_scale < 2; same_scale++) {
            sift3d_similarity_label_measures(65535 - k, rows[k], -2.0f, 3.0f, same_scale, &lr[0]);
            printf("label %d %lld", (int)lr[0].label, (long long)lr[0].sums[0]);
            if (isnan(lr[0].rho)) printf(" nan");
            else printf(" %.17g", lr[0].rho);
            if (isnan(lr[0].rms)) printf(" nan\n");
            else printf(" %.17g\n", lr[0].rms);
        }

    /* the report: every label row in use and the largest counts; buffers of every kind of length */
    memset(rec, 0, sizeof *rec);
    rec->bins = 64;
    rec->same_scale = 1;
    rec->a_lo = -1.0e30f;
    rec->a_hi = 3.4028234e38f;
    rec->b_lo = -0.0f;
    rec->b_hi = 1.17549435e-38f;
    rec->excluded = ((int64_t)1 << 30) - 1;
    rec->sums[0] = (int64_t)1 << 30;
    rec->mi = 4.1588830833596715;
    rec->nmi = 2.0;
    rec->rho = -1.0;
    rec->rms = -NAN;
    rec->h_a = rec->h_b = 1.0e-300;
    rec->h_ab = NAN;
    for (int k = 0; k < SIFT3D_SIMILARITY_MAX_LABELS; k++) {
        lr[k].label = 65535 - 64 + k;
        lr[k].sums[0] = ((int64_t)1 << 30) - k;
        lr[k].rho = k % 3 == 0 ? NAN : -1.0 + k / 64.0;
        lr[k].rms = k % 5 == 0 ? -NAN : 1.0e30 / (k + 1);
    }
    printf("report null %lld\n", (long long)sift3d_similarity_report_text(NULL, NULL, 0, NULL, 0));
    char *text = (char *)malloc(8192);
    if (!text) return 2;
    const int64_t bare = sift3d_similarity_report_text(rec, NULL, 5, text, 8192);
    if (bare < 0 || bare >= 8192 || (int64_t)strlen(text) != bare) return 4;
    printf("report bare %lld\n%s", (long long)bare, text);
    const int64_t need = sift3d_similarity_report_text(rec, lr, SIFT3D_SIMILARITY_MAX_LABELS, text, 8192);
    if (need < 0 || need >= 8192 || (int64_t)strlen(text) != need) return 4;
    printf("report full %lld\n%s", (long long)need, text);
    if (sift3d_similarity_report_text(rec, lr, SIFT3D_SIMILARITY_MAX_LABELS, NULL, 0) != need) return 5;
    const int64_t rooms[] = {0, 1, 2, 100, need, need + 1};
    for (size_t c = 0; c < sizeof rooms / sizeof rooms[0]; c++) {
        char *buf = (char *)malloc((size_t)(rooms[c] > 0 ? rooms[c] : 1)); /* exactly the room: a write beyond it is the sanitizer's to find */
        if (!buf) return 2;
        const int64_t got = sift3d_similarity_report_text(rec, lr, SIFT3D_SIMILARITY_MAX_LABELS, rooms[c] > 0 ? buf : NULL, rooms[c]);
        printf("report room %lld %lld [%s]\n", (long long)rooms[c], (long long)got, rooms[c] > 0 ? buf : "");
        free(buf);
    }
    printf("report over %lld\n", (long long)sift3d_similarity_report_text(rec, lr, 1000, text, 8192)); /* beyond the array: read as 64 */
    if ((int64_t)strlen(text) != need) return 6;
    if (sift3d_similarity_report_text(rec, lr, 0, text, 8192) != bare + (int64_t)strlen("# label n rho rms\n")) return 7;
    free(text);
    free(rec);
    return 0;
}
