/*
 * register_host_san.c -- register_host.c as a stand-alone program (test infrastructure): every host helper of the registration on
 * ordinary and on refused arguments, each result printed as a line.  tests/test_register_cpu.py builds it with and without
 * -fsanitize=address,undefined; both runs exit clean and print the same lines, and the test holds the lines to the oracle.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sift3d.h"

static void print_floats(const char *name, int rc, const float *v, int n)
{
    printf("%s %d", name, rc);
    for (int k = 0; k < n; k++) printf(" %a", (double)v[k]);
    printf("\n");
}

static void check(const char *name, const sift3d_register_params *p, int64_t err_len)
{
    char *err = err_len > 0 ? (char *)malloc((size_t)err_len) : NULL; /* exactly err_len bytes: an overrun shows */
    const int rc = sift3d_register_check(p, err, err_len);
    printf("check %s %d %s\n", name, rc, err && rc != 0 ? err : "");
    free(err);
}

int main(void)
{
    sift3d_register_params p, q;
    sift3d_register_defaults(&p);
    printf("defaults %d %d %d %d %d %d %d %g", p.dof, p.metric, p.bins, p.n_levels, p.max_iterations, p.device, p.form, p.min_overlap);
    for (int l = 0; l < SIFT3D_REGISTER_MAX_LEVELS; l++) printf(" %d %g %g", p.stride[l], p.first_step[l], p.last_step[l]);
    printf("\n");
    check("null", NULL, 64);
    check("defaults", &p, 64);
    static const int dofs[] = {0, 3, 5, 6, 7, 8, 9, 12, 13};
    for (size_t k = 0; k < sizeof dofs / sizeof *dofs; k++) {
        char name[32];
        q = p;
        q.dof = dofs[k];
        snprintf(name, sizeof name, "dof %d", dofs[k]);
        check(name, &q, 64);
    }
#define CASE(NAME, STMT)  \
    q = p;                \
    STMT;                 \
    check(NAME, &q, 96)
    CASE("metric 2", q.metric = 2);
    CASE("metric 0", q.metric = 0);
    CASE("bins 48", q.bins = 48);
    CASE("bins 8", q.bins = 8);
    CASE("n_levels 0", q.n_levels = 0);
    CASE("n_levels 4", q.n_levels = 4);
    CASE("n_levels 5", q.n_levels = 5);
    CASE("stride 3", q.stride[1] = 3);
    CASE("stride 8", q.stride[0] = 8);
    CASE("stride unused", q.stride[3] = 3);
    CASE("first nan", q.first_step[0] = NAN);
    CASE("first 0", q.first_step[2] = 0.0);
    CASE("last above", q.last_step[1] = 2.0);
    CASE("last 0", q.last_step[1] = 0.0);
    CASE("max_iterations 0", q.max_iterations = 0);
    CASE("min_overlap -1", q.min_overlap = -1.0);
    CASE("min_overlap nan", q.min_overlap = NAN);
    CASE("min_overlap 1", q.min_overlap = 1.0);
    CASE("form 4", q.form = 4);
    CASE("form 3", q.form = 3);
    CASE("form -2", q.form = -2);
    q = p;
    q.dof = 5;
    check("short_err", &q, 8);
    check("no_err", &q, 0);

    /* the transform family */
    static const float fv[16] = {0.0f, -0.9f, 0.0f, 12.5f, 1.1f, 0.0f, 0.0f, -3.0f, 0.0f, 0.0f, 2.5f, 7.25f, 0, 0, 0, 1};
    static const float mv[16] = {1.2f, 0.1f, 0.0f, 1.0f, 0.0f, 0.8f, 0.05f, -2.0f, 0.0f, 0.0f, 1.5f, 0.5f, 0, 0, 0, 1};
    static const float m0[16] = {0.98f, -0.1f, 0.02f, 3.0f, 0.12f, 1.03f, 0.0f, -1.5f, -0.03f, 0.01f, 0.95f, 0.25f, 0, 0, 0, 1};
    static const float singular[16] = {1, 2, 3, 0, 2, 4, 6, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    static const float bad_row[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 1, 1};
    static const double thetas[5][12] = {{0},
                                         {1.5, -2.0, 0.25, 0, 0, 0, 0, 0, 0, 0, 0, 0},
                                         {0, 0, 0, 0.3, -0.2, 0.1, 0, 0, 0, 0, 0, 0},
                                         {0.5, 0.25, -1.0, 0.03, 0.02, -0.05, 0.1, -0.05, 0.02, 0.04, -0.02, 0.03},
                                         {0, 0, 0, 0, 0, 3.0, 2.0, -2.0, 0, 0, 5.0, 0}};
    float map[12], res[16];
    for (int k = 0; k < 5; k++) {
        char name[32];
        snprintf(name, sizeof name, "map plain %d", k);
        print_floats(name, sift3d_register_map(thetas[k], 40, 44, 48, NULL, NULL, NULL, map), map, 12);
        snprintf(name, sizeof name, "map keys %d", k);
        print_floats(name, sift3d_register_map(thetas[k], 31, 17, 13, fv, mv, m0, map), map, 12);
        snprintf(name, sizeof name, "result plain %d", k);
        print_floats(name, sift3d_register_result(thetas[k], 40, 44, 48, NULL, NULL, res), res, 16);
        snprintf(name, sizeof name, "result keys %d", k);
        print_floats(name, sift3d_register_result(thetas[k], 31, 17, 13, fv, m0, res), res, 16);
    }
    float unit[12];
    const int rm = sift3d_resample_map(m0, fv, mv, unit);
    print_floats("resample_map", rm, unit, 12);
    memset(map, 0, sizeof map);
    printf("map singular %d %d %d\n", sift3d_register_map(thetas[0], 4, 4, 4, singular, NULL, NULL, map), sift3d_register_map(thetas[0], 4, 4, 4, NULL, singular, NULL, map),
           sift3d_register_map(thetas[0], 4, 4, 4, NULL, NULL, bad_row, map));
    printf("result refused %d %d\n", sift3d_register_result(thetas[0], 4, 4, 4, NULL, bad_row, res), sift3d_register_result(NULL, 4, 4, 4, NULL, NULL, res));
    static const double inf_theta[12] = {0, 0, 0, 0, 0, 0, 800.0, 0, 0, 0, 0, 0};
    printf("map overflow %d\n", sift3d_register_map(inf_theta, 4, 4, 4, NULL, NULL, NULL, map));

    /* the candidates: exactly 2 dof x 12 doubles are written */
    for (size_t k = 0; k < sizeof dofs / sizeof *dofs; k++) {
        const int dof = dofs[k], room = dof > 0 && dof <= 12 ? 2 * dof * 12 : 1;
        double *cand = (double *)malloc(sizeof(double) * (size_t)room);
        const int n = sift3d_register_candidates(thetas[3], dof, 0.5, 20.0, cand);
        printf("candidates %d %d", dof, n);
        for (int c = 0; c < (n > 0 ? n : 0); c++)
            for (int e = 0; e < 12; e++)
                if (cand[12 * c + e] != thetas[3][e]) printf(" %d:%d:%a", c, e, cand[12 * c + e]);
        printf("\n");
        free(cand);
    }

    /* the lattice */
    static const int64_t shapes[4][3] = {{1, 1, 1}, {4, 3, 2}, {33, 9, 5}, {4096, 4096, 64}};
    static const int strides[] = {1, 2, 4, 8, 3};
    for (int s = 0; s < 4; s++)
        for (int t = 0; t < 5; t++) {
            int64_t n[3] = {-1, -1, -1};
            double h = -1, rho = -1;
            const int64_t N = sift3d_register_lattice(shapes[s][0], shapes[s][1], shapes[s][2], strides[t], s & 1 ? fv : NULL, n, &h, &rho);
            printf("lattice %lld %lld %lld stride %d: %lld %lld %lld %lld %a %a\n", (long long)shapes[s][0], (long long)shapes[s][1], (long long)shapes[s][2], strides[t],
                   (long long)N, (long long)n[0], (long long)n[1], (long long)n[2], h, rho);
        }
    printf("lattice refused %lld %lld %lld\n", (long long)sift3d_register_lattice(0, 1, 1, 1, NULL, NULL, NULL, NULL),
           (long long)sift3d_register_lattice(2, 2, 2, 1, singular + 0, NULL, NULL, NULL), (long long)sift3d_register_lattice(2, 2, 2, 1, bad_row, NULL, NULL, NULL));
    static const float zero_col[16] = {1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    printf("lattice zero column %lld\n", (long long)sift3d_register_lattice(2, 2, 2, 1, zero_col, NULL, NULL, NULL));

    /* the report: the length asked for, a buffer of exactly that size, and shorter ones */
    sift3d_register_report *rep = (sift3d_register_report *)calloc(1, sizeof *rep);
    rep->dof = 12;
    rep->metric = SIFT3D_REGISTER_METRIC_NMI;
    rep->bins = 32;
    rep->n_levels = 3;
    rep->h = 0.9;
    rep->rho = 58.75;
    for (int k = 0; k < 12; k++) rep->theta[k] = thetas[3][k];
    sift3d_register_result(thetas[3], 31, 17, 13, fv, m0, rep->result);
    for (int l = 0; l < 3; l++) {
        rep->level[l].stride = 4 >> l;
        rep->level[l].n_lattice = 100 << (3 * l);
        rep->level[l].iterations = 10 + l;
        rep->level[l].evaluations = 1 + 24 * (10 + l);
        rep->level[l].score_in = 1.25 + 0.1 * l;
        rep->level[l].score_out = l == 2 ? NAN : 1.3 + 0.1 * l;
        rep->level[l].last_step = 0.45 / (1 << (2 * l));
        rep->level[l].device_ms = 1.5 * (l + 1);
    }
    rep->before.sums[0] = 6851;
    rep->before.excluded = 12;
    rep->before.mi = 0.5;
    rep->before.nmi = 1.125;
    rep->before.rho = NAN;
    rep->after = rep->before;
    rep->after.nmi = 1.5;
    rep->outside_after = 7;
    const int64_t need = sift3d_register_report_text(rep, NULL, 0);
    char *text = (char *)malloc((size_t)need + 1);
    const int64_t wrote = sift3d_register_report_text(rep, text, need + 1);
    printf("report %lld %lld %zu\n%s", (long long)need, (long long)wrote, strlen(text), text);
    for (int64_t len = 1; len < need; len += 97) {
        char *part = (char *)malloc((size_t)len);
        const int64_t r = sift3d_register_report_text(rep, part, len);
        printf("report part %lld %lld %zu %d\n", (long long)len, (long long)r, strlen(part), strncmp(part, text, (size_t)len - 1));
        free(part);
    }
    rep->n_levels = 5;
    printf("report refused %lld %lld\n", (long long)sift3d_register_report_text(NULL, text, need), (long long)sift3d_register_report_text(rep, text, need));
    free(text);
    free(rep);
    return 0;
}
