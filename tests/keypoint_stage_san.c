/*
 * keypoint_stage_san.c -- stand-alone driver of the oracle's per-keypoint stage (o3_describe_level) for a build under
 * AddressSanitizer + UndefinedBehaviorSanitizer (oracle/Makefile, target kpstage_asan).  TEST INFRASTRUCTURE ONLY.
 *
 *   keypoint_stage_san CASE X Y Z N_CAND SIGMA_H SIGMA_C SIGMA_L OUT [EIG_THRES:DESC_MODE:SIZE_FACTOR:OCTAVE_FACTOR ...]
 *
 * CASE is raw little-endian float32: the Gaussian image (X*Y*Z), the centre DoG (X*Y*Z), then seven floats per candidate
 * (x, y, z, is_max, value, h_value, l_value) in the reference's order.  For every configuration the records are appended to OUT
 * (raw o3_record) and one line "records <n>" is printed.  A sanitizer report ends the process with a non-zero status.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sift3d_oracle.h"

int main(int argc, char **argv)
{
    if (argc < 10) {
        fprintf(stderr, "usage: %s CASE X Y Z N_CAND SIGMA_H SIGMA_C SIGMA_L OUT [EIG:MODE:SIZE:OCTAVE ...]\n", argv[0]);
        return 2;
    }
    const int64_t X = atoll(argv[2]), Y = atoll(argv[3]), Z = atoll(argv[4]), nc = atoll(argv[5]);
    const float sh = strtof(argv[6], 0), sc = strtof(argv[7], 0), sl = strtof(argv[8], 0);
    if (X < 3 || Y < 3 || Z < 3 || nc < 0) return 2;
    const size_t N = (size_t)(X * Y * Z), total = 2 * N + 7 * (size_t)nc;
    float *buf = (float *)malloc(sizeof(float) * (total ? total : 1));
    FILE *f = fopen(argv[1], "rb");
    if (!f || fread(buf, sizeof(float), total, f) != total) {
        fprintf(stderr, "%s: short or unreadable case file\n", argv[1]);
        return 2;
    }
    fclose(f);
    o3_candidate *cand = (o3_candidate *)calloc((size_t)nc + 1, sizeof(o3_candidate));
    for (int64_t i = 0; i < nc; i++) {
        const float *c = buf + 2 * N + 7 * i;
        cand[i].x = (int)c[0]; cand[i].y = (int)c[1]; cand[i].z = (int)c[2]; cand[i].is_max = (int)c[3];
        cand[i].value = c[4]; cand[i].h_value = c[5]; cand[i].l_value = c[6];
        if (cand[i].x < 1 || cand[i].x > X - 2 || cand[i].y < 1 || cand[i].y > Y - 2 || cand[i].z < 1 || cand[i].z > Z - 2) return 2;
    }
    FILE *out = fopen(argv[9], "wb");
    if (!out) return 2;
    int32_t *diag = (int32_t *)malloc(sizeof(int32_t) * O3_DIAG_WORDS * (size_t)(nc + 1));
    for (int a = 10; a < argc; a++) {
        float eig, size_factor, octave_factor;
        int mode;
        if (sscanf(argv[a], "%f:%d:%f:%f", &eig, &mode, &size_factor, &octave_factor) != 4) return 2;
        o3_record *r = 0;
        int64_t n = 0;
        if (o3_describe_level(buf, buf + N, X, Y, Z, sh, sc, sl, octave_factor, cand, nc, eig, mode, size_factor, &r, &n, diag) != 1) return 3;
        if (n && fwrite(r, sizeof(o3_record), (size_t)n, out) != (size_t)n) return 2;
        printf("records %lld\n", (long long)n);
        o3_free(r);
    }
    fclose(out);
    free(diag);
    free(cand);
    free(buf);
    return 0;
}
