/*
 * align_math.h -- the vector and similarity-transform arithmetic of the alignment path, one source
 * compiled as device code (kernels_align.hip) and as host code (align_api.hip, align_host.c), so the kernels and the host's
 * final step perform the same operations in the same order.
 *
 * Each helper restates one routine of the reference (R/ = the reference tree): vec3D_dot_3d, vec3D_cross_3d, vec3D_norm_3d,
 * vec3D_diff_3d, vec3D_summ_3d, mult_3x3, mult_3x3_matrix, transpose_3x3 (R/src_common/MultiScale.{h,cpp}),
 * vec3D_dist_3d, determine_rotation_3point, determine_similarity_transform_3point, feature_to_three_points,
 * compatible_features (R/feat_common/featMatchUtilities.cpp:60-160, 200-340, 650-800) and similarity_transform_3point
 * (MultiScale.cpp:3083-3117).  Exactness rules: only + - * /, sqrtf, and 1.0 / sqrt in double (vec3D_norm_3d); every
 * build of this file keeps -ffp-contract=off and correctly rounded fp32 divide and square root, and honours NaN.  The one
 * transcendental of the reference, fabs(log(s1 / s2)) < T, is a test of the ratio against a float interval [lo, hi]
 * computed once on the host from the host's logf (sift3d_log_ratio_interval, align_host.c).
 */
#ifndef SIFT3D_ALIGN_MATH_H
#define SIFT3D_ALIGN_MATH_H
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define AM_FN static __host__ __device__ inline
#else
#include <math.h>
#define AM_FN static inline
#endif

#define AM_INFO_LINE 0x00000100u   /* INFO_FLAG_LINE, R/src_common/MultiScale.h:34 */
#define AM_LOG_1_5 0.4054651       /* LOG_1_5: compatible_features' default scale threshold (a float parameter there) */
#define AM_HOUGH_SCALE 1.0         /* HOUGH_THRES_SCALE / _TRANS / _ORIEN, featMatchUtilities.cpp:917-919 */
#define AM_HOUGH_TRANS 2.0f
#define AM_HOUGH_ORIEN 0.7f

/* the geometry compatible_features reads */
typedef struct {
    float x, y, z, scale;
    float ori[9];
    uint32_t info;
} am_geo;

AM_FN float am_dot(const float *a, const float *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

AM_FN void am_cross(const float *a, const float *b, float *c)
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = -a[0] * b[2] + a[2] * b[0];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

/* vec3D_norm_3d: a vector whose squared length is not positive (zero or NaN) becomes (1, 0, 0) */
AM_FN void am_norm(float *v)
{
    const float ss = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    if (ss > 0) {
        const float d = (float)(1.0 / sqrt((double)ss));
        v[0] *= d;
        v[1] *= d;
        v[2] *= d;
    } else {
        v[0] = 1;
        v[1] = 0;
        v[2] = 0;
    }
}

/* vec3D_diff_3d(a, b, out): out = b - a */
AM_FN void am_diff(const float *a, const float *b, float *out)
{
    out[0] = b[0] - a[0];
    out[1] = b[1] - a[1];
    out[2] = b[2] - a[2];
}

AM_FN float am_dist(const float *a, const float *b)
{
    const float dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
    return sqrtf(dx * dx + dy * dy + dz * dz);
}

AM_FN void am_transpose(const float *m, float *t)
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) t[3 * i + j] = m[3 * j + i];
}

/* mult_3x3_matrix: every sum starts from 0 */
AM_FN void am_matmul(const float *a, const float *b, float *out)
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            float acc = 0;
            for (int k = 0; k < 3; k++) acc += a[3 * i + k] * b[3 * k + j];
            out[3 * i + j] = acc;
        }
}

/* similarity_transform_3point: out = s * rot (p - c0) + c1 */
AM_FN void am_sim_point(const float *p, float *out, const float *c0, const float *c1, const float *rot, float s)
{
    float d[3], o[3];
    am_diff(c0, p, d);
    for (int i = 0; i < 3; i++) {
        float acc = 0;
        for (int j = 0; j < 3; j++) acc += rot[3 * i + j] * d[j];
        o[i] = acc;
    }
    for (int i = 0; i < 3; i++) o[i] *= s;
    for (int i = 0; i < 3; i++) out[i] = c1[i] + o[i];
}

/* feature_to_three_points: the point plus the scaled rows of its frame */
AM_FN void am_three_points(const float *p, const float *ori, float s, float *pts)
{
    for (int k = 0; k < 3; k++)
        for (int c = 0; c < 3; c++) pts[3 * k + c] = p[c] + s * ori[3 * k + c];
}

/* determine_rotation_3point (the one-image form): rows e12, e13 (made orthogonal), normal */
AM_FN void am_rotation_3point(const float *p1, const float *p2, const float *p3, float *rot)
{
    float v12[3], v13[3], nm[3];
    am_diff(p1, p2, v12);
    am_diff(p1, p3, v13);
    am_norm(v12);
    am_norm(v13);
    am_cross(v12, v13, nm);
    am_norm(nm);
    am_cross(nm, v12, v13);
    am_norm(v13);
    for (int c = 0; c < 3; c++) {
        rot[c] = v12[c];
        rot[3 + c] = v13[c];
        rot[6 + c] = nm[c];
    }
}

/* determine_similarity_transform_3point: pts0 / pts1 three points each (moving, fixed).  Returns 0 and rot = R1^T R0,
 * *scale = ratio of the perimeters; -1 if two points of either triple coincide (the reference then leaves rot unset:
 * such a hypothesis is skipped). */
AM_FN int am_similarity_3point(const float *pts0, const float *pts1, float *rot, float *scale)
{
    const float d012 = am_dist(pts0, pts0 + 3), d013 = am_dist(pts0, pts0 + 6), d023 = am_dist(pts0 + 3, pts0 + 6);
    const float d112 = am_dist(pts1, pts1 + 3), d113 = am_dist(pts1, pts1 + 6), d123 = am_dist(pts1 + 3, pts1 + 6);
    if (d012 == 0 || d013 == 0 || d023 == 0 || d112 == 0 || d113 == 0 || d123 == 0) return -1;
    *scale = (d112 + d113 + d123) / (d012 + d013 + d023);
    float r0[9], r1[9], r1t[9];
    am_rotation_3point(pts0, pts0 + 3, pts0 + 6, r0);
    am_rotation_3point(pts1, pts1 + 3, pts1 + 6, r1);
    am_transpose(r1, r1t);
    am_matmul(r1t, r0, rot);
    return 0;
}

/* The smallest of the three row cosines, in compatible_features' order (a NaN first cosine stays; a later NaN is skipped) */
AM_FN float am_min_cosine(const float *o1, const float *o2)
{
    float m = am_dot(o1, o2);
    const float c1 = am_dot(o1 + 3, o2 + 3);
    if (c1 < m) m = c1;
    const float c2 = am_dot(o1 + 6, o2 + 6);
    if (c2 < m) m = c2;
    return m;
}

/* compatible_features(f1, f2, T, shift, cos): [lo, hi] the ratios r with fabsf(logf(r)) < (float)T */
AM_FN int am_compatible(const am_geo *f1, const am_geo *f2, float lo, float hi, float shift, float cos_thres)
{
    if ((f1->info & AM_INFO_LINE) != (f2->info & AM_INFO_LINE)) return 0;
    if (f1->info & AM_INFO_LINE) {
        float dx = f1->x - f2->x, dy = f1->y - f2->y, dz = f1->z - f2->z;
        const float d1 = sqrtf(dx * dx + dy * dy + dz * dz);
        dx = f1->ori[0] - f2->ori[0];
        dy = f1->ori[1] - f2->ori[1];
        dz = f1->ori[2] - f2->ori[2];
        const float d2 = sqrtf(dx * dx + dy * dy + dz * dz);
        dx = f1->ori[0] - f1->x;
        dy = f1->ori[1] - f1->y;
        dz = f1->ori[2] - f1->z;
        const float l1 = sqrtf(dx * dx + dy * dy + dz * dz);
        dx = f2->ori[0] - f2->x;
        dy = f2->ori[1] - f2->y;
        dz = f2->ori[2] - f2->z;
        const float l2 = sqrtf(dx * dx + dy * dy + dz * dz);
        return (d1 + d2) / (l1 + l2) < shift;
    }
    const float dx = f1->x - f2->x, dy = f1->y - f2->y, dz = f1->z - f2->z;
    const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
    const float r = f1->scale / f2->scale;
    const float mc = am_min_cosine(f1->ori, f2->ori);
    return (r >= lo && r <= hi) && dist < shift * f1->scale && cos_thres < mc;
}

/* One database record j at distance d against the state of a query, msComputeNearestNeighborDistanceRatioInfo's loop body
 * (featMatchUtilities.cpp:365-406), for d < *d2.  compat = compatible_features(db[j], db[*i1]) at its defaults. */
AM_FN void am_ratio_step(int j, int d, int compat, int *i1, int *d1, int *i2, int *d2)
{
    if (d < *d1) {
        if (!compat) {
            *d2 = *d1;
            *i2 = *i1;
        }
        *d1 = d;
        *i1 = j;
    } else if (!compat) {
        *d2 = d;
        *i2 = j;
    }
}

/* Is match j an inlier of the hypothesis (rot, s) built on match i?  determine_similarity_transform_hough's two
 * compatible_features calls (featMatchUtilities.cpp:903-934): the first with zeroed frames (cosine 0 > -1: scale and shift
 * only), the second with the same scale and shift and the frame test on rot . o0[j]^T.  p0 / s0 / o0 moving side, p1 / s1
 * / o1 fixed side; [lo, hi] the ratio interval of AM_HOUGH_SCALE. */
AM_FN int am_hough_inlier(const float *p0, const float *p1, const float *s0, const float *s1, const float *o0, const float *o1, int i, int j,
                          const float *rot, float s, float lo, float hi)
{
    float t[3];
    am_sim_point(p0 + 3 * j, t, p0 + 3 * i, p1 + 3 * i, rot, s);
    const float dx = p1[3 * j] - t[0], dy = p1[3 * j + 1] - t[1], dz = p1[3 * j + 2] - t[2];
    const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
    const float ts = s0[j] * s;
    const float r = s1[j] / ts;
    if (!((r >= lo && r <= hi) && dist < AM_HOUGH_TRANS * s1[j])) return 0;
    float ot[9], rt[9], to[9];
    am_transpose(o0 + 9 * j, ot);
    am_matmul(rot, ot, rt);
    am_transpose(rt, to);
    return AM_HOUGH_ORIEN < am_min_cosine(o1 + 9 * j, to);
}

/* The hypothesis of match i: feature_to_three_points on both sides, then am_similarity_3point.  Returns 0 or -1. */
AM_FN int am_hough_hypothesis(const float *p0, const float *p1, const float *s0, const float *s1, const float *o0, const float *o1, int i,
                              float *rot, float *s)
{
    float a[9], b[9];
    am_three_points(p0 + 3 * i, o0 + 9 * i, s0[i], a);
    am_three_points(p1 + 3 * i, o1 + 9 * i, s1[i], b);
    return am_similarity_3point(a, b, rot, s);
}
#endif
