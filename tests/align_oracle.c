/*
 * align_oracle.c -- independent CPU restatement of the reference's alignment path, for tests/test_align_cpu.py and
 * tests/test_gpu_align.py (compiled by them with cc -O2 -ffp-contract=off into a temporary directory and loaded with
 * ctypes).  Written from the reference's own routines, not from the product's sources (R/ = the reference tree):
 *   msComputeNearestNeighborDistanceRatioInfo   R/feat_common/featMatchUtilities.cpp:336-428, DistSqrPCs(.., 64) restored
 *   compatible_features                         :60-160 (float thresholds; log of a float is logf)
 *   determine_similarity_transform_hough        :816-1025 and its helpers :200-340, 650-800
 *   MatchKeys                                   :1028-1250
 *   similarity_transform_3point / _invert       R/src_common/MultiScale.cpp:3052-3117
 *   TransformSimilarity::Invert / WriteMatrix   R/feat_common/featMatchUtilities.h:213-290
 *   the match files of matchAllToOne            R/featMatchMultiple/featMatchMultiple.cpp:297-358
 * with the pinned choices of DESIGN.md section 8: sort by (ratio, query) with NaN last, degenerate hypotheses skipped,
 * identity where the reference has no transform, inlier flags from the counting pass, match files listing the inliers.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
    float x, y, z, scale;
    float ori[3][3];
    float eigs[3];
    uint32_t info;
    float pc[64];
} Rec;

typedef struct {
    float scale, rot[9], trans[3], c0[3], c1[3];
    int32_t n_matches, inliers, winner, capacity;
    int32_t *moving_idx, *fixed_idx, *inlier, *dist2;
} Sim;

#define INFO_FLAG_LINE 0x00000100u

static float dist_sqr_pcs(const Rec *a, const Rec *b)
{
    float s = 0;
    for (int i = 0; i < 64; i++) {
        const float d = a->pc[i] - b->pc[i];
        s += d * d;
    }
    return s;
}

static float dot3(const float *a, const float *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

/* compatible_features on the fields it reads */
static int compatible(float x1, float y1, float z1, float s1, const float *o1, uint32_t f1, float x2, float y2, float z2, float s2, const float *o2,
                      uint32_t f2, float scale_thres, float shift_thres, float cos_thres)
{
    if ((f1 & INFO_FLAG_LINE) != (f2 & INFO_FLAG_LINE)) return 0;
    if ((f1 & INFO_FLAG_LINE) == INFO_FLAG_LINE) {
        float dx = x1 - x2, dy = y1 - y2, dz = z1 - z2;
        float a = sqrtf(dx * dx + dy * dy + dz * dz);
        dx = o1[0] - o2[0]; dy = o1[1] - o2[1]; dz = o1[2] - o2[2];
        float b = sqrtf(dx * dx + dy * dy + dz * dz);
        dx = o1[0] - x1; dy = o1[1] - y1; dz = o1[2] - z1;
        float l1 = sqrtf(dx * dx + dy * dy + dz * dz);
        dx = o2[0] - x2; dy = o2[1] - y2; dz = o2[2] - z2;
        float l2 = sqrtf(dx * dx + dy * dy + dz * dz);
        return (a + b) / (l1 + l2) < shift_thres;
    }
    const float dx = x1 - x2, dy = y1 - y2, dz = z1 - z2;
    const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
    const float sd = fabsf(logf(s1 / s2));
    float mc = dot3(o1, o2);
    if (dot3(o1 + 3, o2 + 3) < mc) mc = dot3(o1 + 3, o2 + 3);
    if (dot3(o1 + 6, o2 + 6) < mc) mc = dot3(o1 + 6, o2 + 6);
    return sd < scale_thres && dist < shift_thres * s1 && cos_thres < mc;
}

static int compatible_rec(const Rec *a, const Rec *b)
{
    return compatible(a->x, a->y, a->z, a->scale, &a->ori[0][0], a->info, b->x, b->y, b->z, b->scale, &b->ori[0][0], b->info, (float)0.4054651, 0.5f,
                      -1.0f);
}

/* branches[0..3]: closer & not compatible, closer & compatible, second & not compatible, second & compatible */
int orc_ratio(const Rec *db, int64_t n_db, const Rec *q, int64_t n_q, int32_t *o_i1, int32_t *o_d1, int32_t *o_i2, int32_t *o_d2, int64_t *branches)
{
    if (n_db < 2) return -1;
    for (int64_t i = 0; i < n_q; i++) {
        float d1 = dist_sqr_pcs(&q[i], &db[0]), d2 = dist_sqr_pcs(&q[i], &db[1]);
        int i1 = 0, i2 = 1;
        if (d2 < d1) {
            const float t = d1;
            d1 = d2;
            d2 = t;
            i1 = 1;
            i2 = 0;
        }
        for (int64_t j = 2; j < n_db; j++) {
            const float d = dist_sqr_pcs(&q[i], &db[j]);
            if (d < d2) {
                const int c = compatible_rec(&db[j], &db[i1]);
                if (d < d1) {
                    if (!c) {
                        d2 = d1;
                        i2 = i1;
                    }
                    d1 = d;
                    i1 = (int)j;
                    if (branches) branches[c ? 1 : 0]++;
                } else {
                    if (!c) {
                        d2 = d;
                        i2 = (int)j;
                    }
                    if (branches) branches[c ? 3 : 2]++;
                }
            }
        }
        o_i1[i] = i1;
        o_d1[i] = (int32_t)d1;
        o_i2[i] = i2;
        o_d2[i] = (int32_t)d2;
    }
    return 0;
}

static void vdiff(const float *a, const float *b, float *o) { o[0] = b[0] - a[0]; o[1] = b[1] - a[1]; o[2] = b[2] - a[2]; }
static void vnorm(float *v)
{
    float ss = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    if (ss > 0) {
        float f = 1.0 / sqrt(ss);
        v[0] *= f; v[1] *= f; v[2] *= f;
    } else {
        v[0] = 1; v[1] = 0; v[2] = 0;
    }
}
static void vcross(const float *a, const float *b, float *c)
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = -a[0] * b[2] + a[2] * b[0];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
static float vdist(const float *a, const float *b)
{
    float dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
    return sqrtf(dx * dx + dy * dy + dz * dz);
}
static void mat_mult(float a[3][3], float b[3][3], float o[3][3])
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            o[i][j] = 0;
            for (int k = 0; k < 3; k++) o[i][j] += a[i][k] * b[k][j];
        }
}
static void mat_trans(float a[3][3], float o[3][3])
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) o[i][j] = a[j][i];
}
static void sim_transform(const float *p0, float *p1, const float *c0, const float *c1, const float *rot, float s)
{
    float d[3];
    vdiff(c0, p0, d);
    for (int i = 0; i < 3; i++) {
        p1[i] = 0;
        for (int j = 0; j < 3; j++) p1[i] += rot[3 * i + j] * d[j];
    }
    p1[0] *= s; p1[1] *= s; p1[2] *= s;
    p1[0] = c1[0] + p1[0]; p1[1] = c1[1] + p1[1]; p1[2] = c1[2] + p1[2];
}
static void rotation_3point(const float *a, const float *b, const float *c, float rot[3][3])
{
    float v12[3], v13[3], nm[3];
    vdiff(a, b, v12);
    vdiff(a, c, v13);
    vnorm(v12);
    vnorm(v13);
    vcross(v12, v13, nm);
    vnorm(nm);
    vcross(nm, v12, v13);
    vnorm(v13);
    memcpy(rot[0], v12, sizeof v12);
    memcpy(rot[1], v13, sizeof v13);
    memcpy(rot[2], nm, sizeof nm);
}
static int similarity_3point(const float *P0, const float *P1, float rot[3][3], float *s)
{
    float a = vdist(P0, P0 + 3), b = vdist(P0, P0 + 6), c = vdist(P0 + 3, P0 + 6);
    float d = vdist(P1, P1 + 3), e = vdist(P1, P1 + 6), f = vdist(P1 + 3, P1 + 6);
    if (a == 0 || b == 0 || c == 0 || d == 0 || e == 0 || f == 0) return -1;
    *s = (d + e + f) / (a + b + c);
    float r0[3][3], r1[3][3], r1t[3][3];
    rotation_3point(P0, P0 + 3, P0 + 6, r0);
    rotation_3point(P1, P1 + 3, P1 + 6, r1);
    mat_trans(r1, r1t);
    mat_mult(r1t, r0, rot);
    return 0;
}
static void three_points(const float *p, const float *o, float s, float *pts)
{
    for (int k = 0; k < 3; k++)
        for (int c = 0; c < 3; c++) pts[3 * k + c] = p[c] + s * o[3 * k + c];
}

static int hypothesis(const float *p0, const float *p1, const float *s0, const float *s1, const float *o0, const float *o1, int i, float rot[3][3], float *s)
{
    float a[9], b[9];
    three_points(p0 + 3 * i, o0 + 9 * i, s0[i], a);
    three_points(p1 + 3 * i, o1 + 9 * i, s1[i], b);
    return similarity_3point(a, b, rot, s);
}

static int inlier(const float *p0, const float *p1, const float *s0, const float *s1, const float *o0, const float *o1, int i, int j, float rot[3][3], float s)
{
    static const float zero[9] = {0};
    float t[3];
    sim_transform(p0 + 3 * j, t, p0 + 3 * i, p1 + 3 * i, &rot[0][0], s);
    const float ts = s0[j] * s;
    if (!compatible(p1[3 * j], p1[3 * j + 1], p1[3 * j + 2], s1[j], zero, 0, t[0], t[1], t[2], ts, zero, 0, 1.0f, 2.0f, -1.0f)) return 0;
    float tmp[3][3], tori[3][3];
    memcpy(tmp, o0 + 9 * j, sizeof tmp);
    mat_trans(tmp, tori);
    mat_mult(rot, tori, tmp);
    mat_trans(tmp, tori);
    return compatible(p1[3 * j], p1[3 * j + 1], p1[3 * j + 2], s1[j], o1 + 9 * j, 0, t[0], t[1], t[2], ts, &tori[0][0], 0, 1.0f, 2.0f, 0.7f);
}

int orc_hough(const float *p0, const float *p1, const float *s0, const float *s1, const float *o0, const float *o1, int M, int32_t *counts,
              int32_t *winner, float *rot_out, float *scale_out, int32_t *flags)
{
    int best = 0, w = -1;
    for (int i = 0; i < M; i++) {
        float rot[3][3], s;
        if (hypothesis(p0, p1, s0, s1, o0, o1, i, rot, &s) != 0) {
            counts[i] = -1;
            continue;
        }
        int c = 0;
        for (int j = 0; j < M; j++) c += inlier(p0, p1, s0, s1, o0, o1, i, j, rot, s);
        counts[i] = c;
        if (c > best) {
            best = c;
            w = i;
        }
    }
    *winner = w;
    for (int j = 0; j < M; j++) flags[j] = 0;
    if (w >= 0) {
        float rot[3][3], s;
        hypothesis(p0, p1, s0, s1, o0, o1, w, rot, &s);
        for (int j = 0; j < M; j++) flags[j] = inlier(p0, p1, s0, s1, o0, o1, w, j, rot, s);
        memcpy(rot_out, rot, sizeof rot);
        *scale_out = s;
    }
    return 0;
}

static const float *g_ratio;
static int cmp_match(const void *a, const void *b)
{
    const int32_t i = *(const int32_t *)a, j = *(const int32_t *)b;
    const float ri = g_ratio[i], rj = g_ratio[j];
    if (isnan(ri) != isnan(rj)) return isnan(ri) ? 1 : -1;
    if (!isnan(ri) && ri != rj) return ri < rj ? -1 : 1;
    return i < j ? -1 : (i > j);
}

/* MatchKeys from the ratio search's results i1, d1, i2, d2 of every moving record (NULL when nf < 2 or nm == 0): the centre,
 * the sort by ratio, the cut at max_matches and the Hough */
static int match_keys_from(const Rec *fixed, int64_t nf, const Rec *moving, int64_t nm, int max_matches, const int32_t *i1, const int32_t *d1,
                           const int32_t *d2, Sim *out)
{
    memset(out->c0, 0, sizeof out->c0);
    if (nm > 0) {
        float mn[3] = {moving[0].x, moving[0].y, moving[0].z}, mx[3] = {moving[0].x, moving[0].y, moving[0].z};
        for (int64_t i = 0; i < nm; i++) {
            if (moving[i].x > mx[0]) mx[0] = moving[i].x;
            if (moving[i].x < mn[0]) mn[0] = moving[i].x;
            if (moving[i].y > mx[1]) mx[1] = moving[i].y;
            if (moving[i].y < mn[1]) mn[1] = moving[i].y;
            if (moving[i].z > mx[2]) mx[2] = moving[i].z;
            if (moving[i].z < mn[2]) mn[2] = moving[i].z;
        }
        for (int k = 0; k < 3; k++) out->c0[k] = (mx[k] + mn[k]) / 2.0f;
    }
    out->scale = 1;
    for (int k = 0; k < 9; k++) out->rot[k] = (k % 4 == 0);
    for (int k = 0; k < 3; k++) {
        out->trans[k] = 0;
        out->c1[k] = out->c0[k];
    }
    out->n_matches = out->inliers = 0;
    out->winner = -1;
    if (nf < 2 || nm == 0) return 0;
    float *ratio = malloc(sizeof(float) * nm);
    int32_t *order = malloc(sizeof(int32_t) * nm);
    for (int64_t i = 0; i < nm; i++) {
        ratio[i] = (float)d1[i] / (float)d2[i];
        order[i] = (int32_t)i;
    }
    g_ratio = ratio;
    qsort(order, (size_t)nm, sizeof(int32_t), cmp_match);
    const int M = nm < max_matches ? (int)nm : max_matches;
    float *p0 = malloc(sizeof(float) * 3 * (M + 1)), *p1 = malloc(sizeof(float) * 3 * (M + 1)), *s0 = malloc(sizeof(float) * (M + 1)),
          *s1 = malloc(sizeof(float) * (M + 1)), *o0 = malloc(sizeof(float) * 9 * (M + 1)), *o1 = malloc(sizeof(float) * 9 * (M + 1));
    int32_t *counts = malloc(sizeof(int32_t) * (M + 1)), *flags = calloc((size_t)M + 1, sizeof(int32_t));
    for (int k = 0; k < M; k++) {
        const Rec *a = &moving[order[k]], *b = &fixed[i1[order[k]]];
        p0[3 * k] = a->x; p0[3 * k + 1] = a->y; p0[3 * k + 2] = a->z;
        p1[3 * k] = b->x; p1[3 * k + 1] = b->y; p1[3 * k + 2] = b->z;
        s0[k] = a->scale;
        s1[k] = b->scale;
        memcpy(o0 + 9 * k, a->ori, 36);
        memcpy(o1 + 9 * k, b->ori, 36);
    }
    out->n_matches = M;
    if (M <= 3) {
        out->inliers = M;
    } else {
        float rot[9], s;
        int32_t w;
        orc_hough(p0, p1, s0, s1, o0, o1, M, counts, &w, rot, &s, flags);
        if (w >= 0) {
            const float zero[3] = {0, 0, 0};
            out->winner = w;
            out->inliers = counts[w];
            out->scale = s;
            memcpy(out->rot, rot, sizeof rot);
            sim_transform(out->c0, out->c1, p0 + 3 * w, p1 + 3 * w, rot, s);
            sim_transform(zero, out->trans, out->c0, out->c1, rot, s);
        }
    }
    if (out->capacity >= M)
        for (int k = 0; k < M; k++) {
            out->moving_idx[k] = order[k];
            out->fixed_idx[k] = i1[order[k]];
            out->inlier[k] = flags[k];
            out->dist2[k] = d1[order[k]];
        }
    free(ratio); free(order);
    free(p0); free(p1); free(s0); free(s1); free(o0); free(o1); free(counts); free(flags);
    return 0;
}

int orc_match_keys(const Rec *fixed, int64_t nf, const Rec *moving, int64_t nm, int max_matches, Sim *out)
{
    if (nf < 2 || nm == 0) return match_keys_from(fixed, nf, moving, nm, max_matches, NULL, NULL, NULL, out);
    int32_t *i1 = malloc(sizeof(int32_t) * nm), *d1 = malloc(sizeof(int32_t) * nm), *i2 = malloc(sizeof(int32_t) * nm), *d2 = malloc(sizeof(int32_t) * nm);
    orc_ratio(fixed, nf, moving, nm, i1, d1, i2, d2, NULL);
    const int rc = match_keys_from(fixed, nf, moving, nm, max_matches, i1, d1, d2, out);
    free(i1); free(d1); free(i2); free(d2);
    return rc;
}

/* TEST ONLY: orc_match_keys with the ratio search replaced by given results (i1, d1, i2, d2 per moving record, as orc_ratio
 * writes them), for record sets whose full CPU ratio search is too slow; i2 is not read (MatchKeys does not use it).  An i1
 * outside the fixed set is refused (-1). */
int orc_match_keys_from_ratio(const Rec *fixed, int64_t nf, const Rec *moving, int64_t nm, int max_matches, const int32_t *i1, const int32_t *d1,
                              const int32_t *i2, const int32_t *d2, Sim *out)
{
    (void)i2;
    if (nf >= 2)
        for (int64_t i = 0; i < nm; i++)
            if (i1[i] < 0 || i1[i] >= nf) return -1;
    return match_keys_from(fixed, nf, moving, nm, max_matches, nf >= 2 && nm > 0 ? i1 : NULL, d1, d2, out);
}

/* TransformSimilarity::Invert */
void orc_invert(const Sim *in, Sim *out)
{
    *out = *in;
    float stuff[3] = {0, 0, 0}, trans[3], zero[3] = {0, 0, 0};
    memcpy(trans, in->trans, sizeof trans);
    /* similarity_transform_invert(stuff, trans, rot, scale): swap the centres, invert the scale, transpose the rotation */
    float tmp[3];
    memcpy(tmp, stuff, sizeof tmp);
    memcpy(stuff, trans, sizeof tmp);
    memcpy(trans, tmp, sizeof tmp);
    out->scale = 1.0f / in->scale;
    float r[3][3], rt[3][3];
    memcpy(r, in->rot, sizeof r);
    mat_trans(r, rt);
    memcpy(out->rot, rt, sizeof rt);
    sim_transform(zero, out->trans, stuff, trans, out->rot, out->scale);
}

int orc_write_matrix(const char *path, const Sim *t)
{
    FILE *f = fopen(path, "wt");
    if (!f) return -1;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) fprintf(f, "%f\t", t->scale * t->rot[3 * r + c]);
        fprintf(f, "%f\n", t->trans[r]);
    }
    fprintf(f, "0.0\t0.0\t0.0\t1.0\n");
    fclose(f);
    return 0;
}

int orc_write_matches(const char *base, const char *name1, const char *name2, const Rec *fixed, int64_t nf, const Rec *moving, const Sim *t)
{
    int32_t *model = malloc(sizeof(int32_t) * (nf + 1));
    for (int64_t g = 0; g < nf; g++) model[g] = -1;
    for (int k = 0; k < t->n_matches; k++)
        if (t->inlier[k]) model[t->fixed_idx[k]] = k;
    int matches = 0;
    for (int64_t g = 0; g < nf; g++) matches += model[g] >= 0;
    char img1[4200], img2[4200], path[4200];
    sprintf(img1, "%s", name1);
    sprintf(img2, "%s", name2);
    char *p = strrchr(img1, '.');
    sprintf(p ? p : img1 + strlen(img1), ".hdr");
    p = strrchr(img2, '.');
    sprintf(p ? p : img2 + strlen(img2), ".hdr");
    sprintf(path, "%s.matches.info.txt", base);
    FILE *info = fopen(path, "wt");
    sprintf(path, "%s.matches.img1.txt", base);
    FILE *o = fopen(path, "wt");
    fprintf(o, "# Img1: %s\n", img1);
    fprintf(o, "# Img2: %s\n", img2);
    fprintf(o, "# Matches: %d\n", matches);
    fprintf(o, "# Format: Img1 x1 y1 z1 s1 MatchIndexImg2 DistSqr\n");
    int cur = 0;
    for (int64_t g = 0; g < nf; g++) {
        if (model[g] < 0) continue;
        const Rec *f1 = &fixed[g], *f2 = &moving[t->moving_idx[model[g]]];
        float dist = (float)t->dist2[model[g]];
        fprintf(info, "%d\t%d\n", f1->info, f2->info);
        fprintf(o, "%s\t%f\t%f\t%f\t%f\timg2_match%4.4d_feat%6.6d\t%f\t%f\t%f\t%f\t%f\t%f\t%f\t%f\t%f\t%f\n", name1, f1->x, f1->y, f1->z, f1->scale, cur,
                t->moving_idx[model[g]], dist, f1->ori[0][0], f1->ori[0][1], f1->ori[0][2], f1->ori[1][0], f1->ori[1][1], f1->ori[1][2], f1->ori[2][0],
                f1->ori[2][1], f1->ori[2][2]);
        cur++;
    }
    fclose(o);
    fclose(info);
    sprintf(path, "%s.matches.img2.txt", base);
    o = fopen(path, "wt");
    fprintf(o, "# Img1: %s\n", img1);
    fprintf(o, "# Img2: %s\n", img2);
    fprintf(o, "# Matches: %d\n", matches);
    fprintf(o, "# Format: Img2 x2 y2 z2 s2 MatchIndexImg1 DistSqr\n");
    cur = 0;
    for (int64_t g = 0; g < nf; g++) {
        if (model[g] < 0) continue;
        const Rec *f2 = &moving[t->moving_idx[model[g]]];
        float dist = (float)t->dist2[model[g]];
        fprintf(o, "%s\t%f\t%f\t%f\t%f\timg2_match%4.4d_feat%6.6d\t%f\t%f\t%f\t%f\t%f\t%f\t%f\t%f\t%f\t%f\n", name2, f2->x, f2->y, f2->z, f2->scale, cur,
                (int)g, dist, f2->ori[0][0], f2->ori[0][1], f2->ori[0][2], f2->ori[1][0], f2->ori[1][1], f2->ori[1][2], f2->ori[2][0], f2->ori[2][1],
                f2->ori[2][2]);
        cur++;
    }
    fclose(o);
    free(model);
    return 0;
}

/* brute force: every float in [0.25, 4] (|log r| < 1.39 only there), the lowest and highest r with fabsf(logf(r)) < t */
int orc_interval_sweep(double t, float *lo, float *hi)
{
    const float tf = (float)t;
    float a = 0.25f, l = NAN, h = NAN;
    uint32_t b;
    memcpy(&b, &a, 4);
    for (;; b++) {
        float r;
        memcpy(&r, &b, 4);
        if (r > 4.0f) break;
        if (fabsf(logf(r)) < tf) {
            if (isnan(l)) l = r;
            h = r;
        }
    }
    *lo = l;
    *hi = h;
    return 0;
}
