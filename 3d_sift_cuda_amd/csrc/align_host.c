/*
 * align_host.c -- host side of the alignment path: the ratio interval that stands in for logf on
 * the device, the inverse of a similarity transform, and the files matchAllToOne writes per moving image
 * (R/featMatchMultiple/featMatchMultiple.cpp:297-358; TransformSimilarity, R/feat_common/featMatchUtilities.h:152-290;
 * R/ = the reference tree).  Linked into libsift3d_hip.so (the interval is computed when the library first aligns, and
 * featMatchMultiple -a writes through it) and into libsift3d_host.so.  At the end: the .trans.txt matrix, its reader and
 * the voxel-to-voxel map of featResample (section 7c).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "align_math.h"
#include "sift3d.h"

static float bits_to_float(uint32_t b)
{
    float f;
    memcpy(&f, &b, sizeof f);
    return f;
}

static uint32_t float_to_bits(float f)
{
    uint32_t b;
    memcpy(&b, &f, sizeof b);
    return b;
}

static int passes(uint32_t b, float t) { return fabsf(logf(bits_to_float(b))) < t; }

int sift3d_log_ratio_interval(double t, float *lo, float *hi)
{
    const float tf = (float)t; /* compatible_features takes its threshold as a float */
    const uint32_t one = float_to_bits(1.0f), top = 0x7f7fffffu; /* FLT_MAX */
    if (!passes(one, tf)) return -1;
    /* positive floats order like their bit patterns; logf is monotonic over them, so the set that passes is one run of
     * patterns around 1.0: binary search for its ends, then check 2^16 patterns on both sides of each end */
    uint32_t a = 1, b = one; /* lowest passing pattern in (a - 1, b] */
    while (a < b) {
        const uint32_t m = a + (b - a) / 2;
        if (passes(m, tf)) b = m;
        else a = m + 1;
    }
    const uint32_t lo_b = a;
    a = one;
    b = top; /* highest passing pattern in [a, b] */
    while (a < b) {
        const uint32_t m = a + (b - a + 1) / 2;
        if (passes(m, tf)) a = m;
        else b = m - 1;
    }
    const uint32_t hi_b = a;
    const uint32_t W = 1u << 16;
    for (uint32_t k = 1; k <= W; k++) {
        if (lo_b > k && passes(lo_b - k, tf)) return -1;
        if (lo_b + k - 1 <= one && !passes(lo_b + k - 1, tf)) return -1;
        if (hi_b + k <= top && passes(hi_b + k, tf)) return -1;
        if (hi_b >= one + k - 1 && !passes(hi_b - (k - 1), tf)) return -1;
    }
    *lo = bits_to_float(lo_b);
    *hi = bits_to_float(hi_b);
    return 0;
}

void sift3d_similarity_invert(const sift3d_similarity *in, sift3d_similarity *out)
{
    /* Invert(): similarity_transform_invert swaps the centres ({0,0,0} and trans), inverts the scale and transposes the
     * rotation; similarity_transform_3point then maps the zero vector */
    const float zero[3] = {0, 0, 0};
    float c0[3], rot[9], t[3];
    memcpy(c0, in->trans, sizeof c0);
    const float s = 1.0f / in->scale;
    am_transpose(in->rot, rot);
    am_sim_point(zero, t, c0, zero, rot, s);
    *out = *in;
    out->scale = s;
    memcpy(out->rot, rot, sizeof rot);
    memcpy(out->trans, t, sizeof t);
}

int sift3d_write_similarity(const char *path, const sift3d_similarity *t)
{
    FILE *f = fopen(path, "wt");
    if (!f) return -1;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) fprintf(f, "%f\t", t->scale * t->rot[3 * r + c]);
        fprintf(f, "%f\n", t->trans[r]);
    }
    fprintf(f, "0.0\t0.0\t0.0\t1.0\n");
    return fclose(f) == 0 ? 0 : -1;
}

/* the key file name with the extension from its last '.' replaced by .hdr (appended where there is none) */
static void hdr_name(char *out, size_t cap, const char *name)
{
    snprintf(out, cap, "%s", name);
    char *dot = strrchr(out, '.');
    const size_t at = dot ? (size_t)(dot - out) : strlen(out);
    if (at + 5 <= cap) memcpy(out + at, ".hdr", 5);
}

int sift3d_write_alignment_matches(const char *base, const char *fixed_name, const char *moving_name, const sift3d_feature *fixed,
                                   int64_t n_fixed, const sift3d_feature *moving, int64_t n_moving, const sift3d_similarity *t)
{
    int rc = -1;
    FILE *info = NULL, *f1 = NULL, *f2 = NULL;
    int32_t *model = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n_fixed > 0 ? n_fixed : 1)); /* vecModelMatches: match k, or -1 */
    const size_t cap = strlen(base) + 64;
    char *path = (char *)malloc(cap), img1[4200], img2[4200];
    if (!model || !path) goto done;
    for (int64_t g = 0; g < n_fixed; g++) model[g] = -1;
    if (t->n_matches > 0 && (!t->moving_idx || !t->fixed_idx || !t->inlier || !t->dist2 || t->capacity < t->n_matches)) goto done;
    for (int32_t k = 0; k < t->n_matches; k++) {
        const int32_t g = t->fixed_idx[k], m = t->moving_idx[k];
        if (g < 0 || g >= n_fixed || m < 0 || m >= n_moving) goto done;
        if (t->inlier[k]) model[g] = k;
    }
    int matches = 0;
    for (int64_t g = 0; g < n_fixed; g++) matches += model[g] >= 0;
    hdr_name(img1, sizeof img1, fixed_name);
    hdr_name(img2, sizeof img2, moving_name);
    snprintf(path, cap, "%s.matches.info.txt", base);
    if (!(info = fopen(path, "wt"))) goto done;
    snprintf(path, cap, "%s.matches.img1.txt", base);
    if (!(f1 = fopen(path, "wt"))) goto done;
    fprintf(f1, "# Img1: %s\n# Img2: %s\n# Matches: %d\n# Format: Img1 x1 y1 z1 s1 MatchIndexImg2 DistSqr\n", img1, img2, matches);
    int cur = 0;
    for (int64_t g = 0; g < n_fixed; g++) {
        if (model[g] < 0) continue;
        const sift3d_feature *a = &fixed[g], *b = &moving[t->moving_idx[model[g]]];
        const float dist = (float)t->dist2[model[g]];
        fprintf(info, "%d\t%d\n", (int)a->info, (int)b->info);
        fprintf(f1, "%s\t%f\t%f\t%f\t%f\timg2_match%4.4d_feat%6.6d\t%f\t%f\t%f\t%f\t%f\t%f\t%f\t%f\t%f\t%f\n", fixed_name, a->x, a->y, a->z, a->scale,
                cur, t->moving_idx[model[g]], dist, a->ori[0], a->ori[1], a->ori[2], a->ori[3], a->ori[4], a->ori[5], a->ori[6], a->ori[7],
                a->ori[8]);
        cur++;
    }
    if (fclose(f1) != 0 || fclose(info) != 0) {
        f1 = info = NULL;
        goto done;
    }
    f1 = info = NULL;
    snprintf(path, cap, "%s.matches.img2.txt", base);
    if (!(f2 = fopen(path, "wt"))) goto done;
    fprintf(f2, "# Img1: %s\n# Img2: %s\n# Matches: %d\n# Format: Img2 x2 y2 z2 s2 MatchIndexImg1 DistSqr\n", img1, img2, matches);
    cur = 0;
    for (int64_t g = 0; g < n_fixed; g++) {
        if (model[g] < 0) continue;
        const sift3d_feature *b = &moving[t->moving_idx[model[g]]];
        const float dist = (float)t->dist2[model[g]];
        /* the reference's img2 lines carry the img2_match tag too (featMatchMultiple.cpp:343) */
        fprintf(f2, "%s\t%f\t%f\t%f\t%f\timg2_match%4.4d_feat%6.6d\t%f\t%f\t%f\t%f\t%f\t%f\t%f\t%f\t%f\t%f\n", moving_name, b->x, b->y, b->z, b->scale,
                cur, (int)g, dist, b->ori[0], b->ori[1], b->ori[2], b->ori[3], b->ori[4], b->ori[5], b->ori[6], b->ori[7], b->ori[8]);
        cur++;
    }
    rc = fclose(f2) == 0 ? 0 : -1;
    f2 = NULL;
done:
    if (info) fclose(info);
    if (f1) fclose(f1);
    if (f2) fclose(f2);
    free(model);
    free(path);
    return rc;
}

/* ---- featResample ---------------------------------------------------------------------------- */

void sift3d_similarity_matrix(const sift3d_similarity *t, float m[16])
{
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) m[4 * r + c] = t->scale * t->rot[3 * r + c]; /* as WriteMatrix forms it, before %f */
        m[4 * r + 3] = t->trans[r];
    }
    m[12] = m[13] = m[14] = 0.0f;
    m[15] = 1.0f;
}

int sift3d_read_similarity(const char *path, float m[16])
{
    FILE *f = fopen(path, "rt");
    if (!f) return -1;
    double v[16];
    int n = 0;
    while (n < 16 && fscanf(f, "%lf", &v[n]) == 1) n++;
    char rest[2] = "";
    const int extra = fscanf(f, " %1s", rest); /* anything but white space after the sixteenth number is an error */
    fclose(f);
    if (n != 16 || extra == 1) return -1;
    if (v[12] != 0.0 || v[13] != 0.0 || v[14] != 0.0 || v[15] != 1.0) return -1;
    for (int k = 0; k < 16; k++) m[k] = (float)v[k];
    return 0;
}

/* the inverse of an affine 4 x 4 (last row 0 0 0 1) in double: the adjugate of the 3 x 3 part over its determinant, then
 * the translation.  -1 when the last row is not 0 0 0 1 or the 3 x 3 part is singular or not finite. */
static int affine_inverse(const double a[16], double o[16])
{
    if (a[12] != 0.0 || a[13] != 0.0 || a[14] != 0.0 || a[15] != 1.0) return -1;
    const double c00 = a[5] * a[10] - a[6] * a[9], c01 = a[6] * a[8] - a[4] * a[10], c02 = a[4] * a[9] - a[5] * a[8];
    const double det = a[0] * c00 + a[1] * c01 + a[2] * c02;
    if (!(det != 0.0) || !isfinite(det)) return -1;
    const double inv[9] = {c00, a[2] * a[9] - a[1] * a[10], a[1] * a[6] - a[2] * a[5],
                           c01, a[0] * a[10] - a[2] * a[8], a[2] * a[4] - a[0] * a[6],
                           c02, a[1] * a[8] - a[0] * a[9], a[0] * a[5] - a[1] * a[4]};
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) o[4 * r + c] = inv[3 * r + c] / det;
        o[4 * r + 3] = -(o[4 * r] * a[3] + o[4 * r + 1] * a[7] + o[4 * r + 2] * a[11]);
        if (!isfinite(o[4 * r]) || !isfinite(o[4 * r + 1]) || !isfinite(o[4 * r + 2]) || !isfinite(o[4 * r + 3])) return -1;
    }
    o[12] = o[13] = o[14] = 0.0;
    o[15] = 1.0;
    return 0;
}

static void mul44(const double a[16], const double b[16], double o[16])
{
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) o[4 * r + c] = a[4 * r] * b[c] + a[4 * r + 1] * b[4 + c] + a[4 * r + 2] * b[8 + c] + a[4 * r + 3] * b[12 + c];
}

static void load44(const float *m, double o[16])
{
    for (int k = 0; k < 16; k++) o[k] = m ? (double)m[k] : (k % 5 == 0 ? 1.0 : 0.0);
}

int sift3d_resample_map(const float moving_to_fixed[16], const float fixed_vox2key[16], const float moving_vox2key[16], float map[12])
{
    double t[16], fv[16], mv[16], ti[16], mvi[16], p[16], a[16];
    load44(moving_to_fixed, t);
    load44(fixed_vox2key, fv);
    load44(moving_vox2key, mv);
    if (affine_inverse(t, ti) != 0 || affine_inverse(mv, mvi) != 0 || affine_inverse(fv, p) != 0) return -1; /* p: scratch */
    /* A = inv(moving_vox2key) . inv(T) . fixed_vox2key: output (fixed) voxel -> fixed key -> moving key -> moving voxel */
    mul44(ti, fv, p);
    mul44(mvi, p, a);
    for (int k = 0; k < 12; k++) {
        if (!isfinite(a[k])) return -1;
        map[k] = (float)a[k];
    }
    return 0;
}

void sift3d_key_vox2key(const float voxel[3], const float world[16], float m[16])
{
    /* featExtract's records sit half a voxel past the voxel index.  Under -w the volume is first resampled to isotropic
     * voxels (world.c): isotropic voxel x' samples the original position x' * f, f = min(voxel) / voxel per axis, and the
     * matrix columns are scaled by f, so the record of original position x is world . (x + 0.5 f). */
    double v[16];
    for (int k = 0; k < 16; k++) v[k] = world ? (double)world[k] : (k % 5 == 0 ? 1.0 : 0.0);
    float f[3] = {1.0f, 1.0f, 1.0f};
    if (world) {
        float mn = voxel[0];
        if (voxel[1] < mn) mn = voxel[1];
        if (voxel[2] < mn) mn = voxel[2];
        for (int a = 0; a < 3; a++) f[a] = mn / voxel[a];
    }
    for (int r = 0; r < 4; r++) {
        for (int c = 0; c < 3; c++) m[4 * r + c] = (float)v[4 * r + c];
        m[4 * r + 3] = (float)(v[4 * r + 3] + v[4 * r] * 0.5 * f[0] + v[4 * r + 1] * 0.5 * f[1] + v[4 * r + 2] * 0.5 * f[2]);
    }
}
