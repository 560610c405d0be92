/*
 * keypoint_math.h -- the scalar arithmetic of the per-keypoint stage: each routine restates one scalar routine of the
 * reference (R/src_common/...), and every bit of a record's frame is decided here.  keypoint_kernel (kernels_keypoint.hip) and
 * descriptor_kernel (kernels_descriptor.hip) call them through keypoint_device.h.  Plain C++ for host and device, without a HIP
 * include: tests/keypoint_math_check.cpp runs the same functions on the CPU (tests/test_keypoint_math_cpu.py), as
 * tests/desc_bins_check.cpp does for desc_bins.h.
 *
 * Every includer is built with -ffp-contract=off: a fused multiply-add changes keypoints.
 */
#ifndef KEYPOINT_MATH_H
#define KEYPOINT_MATH_H

#include <math.h>

#include "desc_bins.h" /* interp_coord, the patch edge */

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KEYPOINT_MATH_HD __host__ __device__ inline __attribute__((always_inline)) /* as the kernels had them */
#else
#define KEYPOINT_MATH_HD inline
#endif
#define KEYPOINT_MATH_PD DESC_BINS_PD /* patch edge (SIFT3D_PATCH_DIM) */

/* interp_coord (_fioDetermineInterpCoord, R/src_common/FeatureIO.cpp:757-782) is desc_bins.h's: the descriptor's weights are
 * built from it at compile time */

/* finddet + interpolate_extremum_quadratic, R/src_common/MultiScale.cpp:2531-2534, 1641-1697 */
KEYPOINT_MATH_HD double finddet(double a1, double a2, double a3, double b1, double b2, double b3, double c1,
                                double c2, double c3)
{
    return ((a1 * b2 * c3) - (a1 * b3 * c2) - (a2 * b1 * c3) + (a3 * b1 * c2) + (a2 * b3 * c1) - (a3 * b2 * c1));
}
KEYPOINT_MATH_HD double interp_quadratic(double x0, double x1, double x2, double fx0, double fx1, double fx2)
{
    if (!(fx1 < fx0 && fx1 < fx2) && !(fx1 > fx0 && fx1 > fx2)) return x1;
    double a1 = x0 * x0, b1 = x0, c1 = 1;
    double a2 = x1 * x1, b2 = x1, c2 = 1;
    double a3 = x2 * x2, b3 = x2, c3 = 1;
    double d1 = fx0, d2 = fx1, d3 = fx2;
    double det = finddet(a1, a2, a3, b1, b2, b3, c1, c2, c3);
    double detx = finddet(d1, d2, d3, b1, b2, b3, c1, c2, c3);
    double dety = finddet(a1, a2, a3, d1, d2, d3, c1, c2, c3);
    if (d1 == 0 && d2 == 0 && d3 == 0) return x1;
    if (det != 0) {
        if (detx != 0) return dety / (-2.0 * detx);
    }
    return x1;
}

/* invert_3x3<float,double>, R/src_common/MultiScale.h:192-222 */
KEYPOINT_MATH_HD void invert3(const float *in, float *out) /* row-major 3x3 */
{
    float a11 = in[0], a21 = in[3], a31 = in[6];
    float a12 = in[1], a22 = in[4], a32 = in[7];
    float a13 = in[2], a23 = in[5], a33 = in[8];
    float det = a11 * (a33 * a22 - a32 * a23) - a21 * (a33 * a12 - a32 * a13) + a31 * (a23 * a12 - a22 * a13);
    double div = 1 / (double)det;
    out[0] = (float)((a33 * a22 - a32 * a23) * div);
    out[3] = (float)(-(a33 * a21 - a31 * a23) * div);
    out[6] = (float)((a32 * a21 - a31 * a22) * div);
    out[1] = (float)(-(a33 * a12 - a32 * a13) * div);
    out[4] = (float)((a33 * a11 - a31 * a13) * div);
    out[7] = (float)(-(a32 * a11 - a31 * a12) * div);
    out[2] = (float)((a23 * a12 - a22 * a13) * div);
    out[5] = (float)(-(a23 * a11 - a21 * a13) * div);
    out[8] = (float)((a22 * a11 - a21 * a12) * div);
}

/* vec3D_norm_3d / vec3D_mag / vec3D_dot_3d, R/src_common/MultiScale.cpp:1092-1127, 1571-1578 */
KEYPOINT_MATH_HD void v3_norm(float *p)
{
    float ss = p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
    if (ss > 0) {
        float div = (float)(1.0 / (double)sqrtf(ss));
        p[0] *= div;
        p[1] *= div;
        p[2] *= div;
    } else {
        p[0] = 1;
        p[1] = 0;
        p[2] = 0;
    }
}
KEYPOINT_MATH_HD float v3_mag(const float *p)
{
    float ss = p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
    if (ss > 0) return sqrtf(ss);
    return 0;
}
KEYPOINT_MATH_HD float v3_dot(const float *a, const float *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

/* Singular value decomposition of the 3x3 structure tensor and the sort of its result: what the reference gets from
 * SingularValueDecomp<float,3,3> + SortEigenDecomp<float,3> (R/src_common/SVD.h:15-228, the Golub-Kahan-Reinsch scheme:
 * Householder reduction to bidiagonal form, accumulation of the right- and left-hand transformations, implicit-shift QR
 * sweeps).  The eigenvectors go into the records, so this has to produce the reference's bits, and for that every
 * floating-point operation has to be the reference's, in its order and in its width: storage in float, running values in
 * double, a product of two stored floats rounded to float before it enters a double sum.  Written here for the 3x3 case
 * with 0-based indices (the sizes folded in, the branches that cannot be taken removed) and pinned three ways by the test
 * suite: its CPU restatement against the reference's own template compiled from source (bit-exact on 4 000 tensors), this
 * function compiled for the host against that restatement (tests/keypoint_math_check.cpp, bit-exact on 200 000 tensors), and
 * this function compiled for the device against that restatement through every record of the pipeline tests. */
KEYPOINT_MATH_HD double svd_with_sign(double magnitude, double sign_source) { return sign_source >= 0.0 ? fabs(magnitude) : -fabs(magnitude); }
KEYPOINT_MATH_HD double svd_hypot(double p, double q) { return sqrt(p * p + q * q); }

KEYPOINT_MATH_HD void svd3(float a[3][3], float w[3], float v[3][3])
{
    double off[3]; /* the super-diagonal of the bidiagonal form (off[0] stays 0) */
    double g = 0.0, scale = 0.0, norm = 0.0, s, f, h;
    int below = 0;

    /* ---- 1. Householder reduction: column i (left reflection), then row i (right reflection) ---- */
    for (int i = 0; i < 3; i++) {
        below = i + 1;
        off[i] = scale * g;
        g = s = scale = 0.0;
        for (int k = i; k < 3; k++) scale += fabsf(a[k][i]);
        if (scale) {
            for (int k = i; k < 3; k++) {
                a[k][i] = (float)(a[k][i] / scale);
                s += a[k][i] * a[k][i];
            }
            f = a[i][i];
            g = -svd_with_sign(sqrt(s), f);
            h = f * g - s;
            a[i][i] = (float)(f - g);
            for (int j = below; j < 3; j++) {
                s = 0.0;
                for (int k = i; k < 3; k++) s += a[k][i] * a[k][j];
                f = s / h;
                for (int k = i; k < 3; k++) a[k][j] = (float)(a[k][j] + f * a[k][i]);
            }
            for (int k = i; k < 3; k++) a[k][i] = (float)(a[k][i] * scale);
        }
        w[i] = (float)(scale * g);
        g = s = scale = 0.0;
        if (i != 2) {
            for (int k = below; k < 3; k++) scale += fabsf(a[i][k]);
            if (scale) {
                for (int k = below; k < 3; k++) {
                    a[i][k] = (float)(a[i][k] / scale);
                    s += a[i][k] * a[i][k];
                }
                f = a[i][below];
                g = -svd_with_sign(sqrt(s), f);
                h = f * g - s;
                a[i][below] = (float)(f - g);
                for (int k = below; k < 3; k++) off[k] = a[i][k] / h;
                for (int j = below; j < 3; j++) {
                    s = 0.0;
                    for (int k = below; k < 3; k++) s += a[j][k] * a[i][k];
                    for (int k = below; k < 3; k++) a[j][k] = (float)(a[j][k] + s * off[k]);
                }
                for (int k = below; k < 3; k++) a[i][k] = (float)(a[i][k] * scale);
            }
        }
        const double row_norm = fabsf(w[i]) + fabs(off[i]);
        norm = norm > row_norm ? norm : row_norm;
    }

    /* ---- 2. right-hand transformations into v, last row first (g and `below` carry over from the row above) ---- */
    for (int i = 2; i >= 0; i--) {
        if (i < 2) {
            if (g) {
                for (int j = below; j < 3; j++) v[j][i] = (float)((a[i][j] / a[i][below]) / g);
                for (int j = below; j < 3; j++) {
                    s = 0.0;
                    for (int k = below; k < 3; k++) s += a[i][k] * v[k][j];
                    for (int k = below; k < 3; k++) v[k][j] = (float)(v[k][j] + s * v[k][i]);
                }
            }
            for (int j = below; j < 3; j++) v[i][j] = v[j][i] = 0.0;
        }
        v[i][i] = 1.0;
        g = off[i];
        below = i;
    }

    /* ---- 3. left-hand transformations, in place in a ---- */
    for (int i = 2; i >= 0; i--) {
        below = i + 1;
        g = w[i];
        for (int j = below; j < 3; j++) a[i][j] = 0.0;
        if (g) {
            g = 1.0 / g;
            for (int j = below; j < 3; j++) {
                s = 0.0;
                for (int k = below; k < 3; k++) s += a[k][i] * a[k][j];
                f = (s / a[i][i]) * g;
                for (int k = i; k < 3; k++) a[k][j] = (float)(a[k][j] + f * a[k][i]);
            }
            for (int j = i; j < 3; j++) a[j][i] = (float)(a[j][i] * g);
        } else {
            for (int j = i; j < 3; j++) a[j][i] = 0.0;
        }
        a[i][i] = a[i][i] + 1;
    }

    /* ---- 4. diagonalisation: for each singular value, from the last, implicit-shift QR sweeps (at most 30) ---- */
    for (int k = 2; k >= 0; k--) {
        for (int sweep = 1; sweep <= 30; sweep++) {
            /* find the block to work on: lo = first row of it; off[0] is 0, so the search always ends by splitting */
            bool cancel = true;
            int lo = k, above = 0;
            for (; lo >= 0; lo--) {
                above = lo - 1;
                if ((double)(fabs(off[lo]) + norm) == norm) {
                    cancel = false;
                    break;
                }
                if ((double)(fabsf(w[above]) + norm) == norm) break;
            }
            double c, x, y, z;
            if (cancel) { /* w[above] is negligible: rotate off[lo] .. off[k] away */
                c = 0.0;
                s = 1.0;
                for (int i = lo; i <= k; i++) {
                    f = s * off[i];
                    off[i] = c * off[i];
                    if ((double)(fabs(f) + norm) == norm) break;
                    g = w[i];
                    h = svd_hypot(f, g);
                    w[i] = (float)h;
                    h = 1.0 / h;
                    c = g * h;
                    s = -f * h;
                    for (int j = 0; j < 3; j++) {
                        y = a[j][above];
                        z = a[j][i];
                        a[j][above] = (float)(y * c + z * s);
                        a[j][i] = (float)(z * c - y * s);
                    }
                }
            }
            z = w[k];
            if (lo == k) { /* converged: make the singular value non-negative */
                if (z < 0.0) {
                    w[k] = (float)(-z);
                    for (int j = 0; j < 3; j++) v[j][k] = -v[j][k];
                }
                break;
            }
            /* shift from the bottom 2x2 minor */
            x = w[lo];
            above = k - 1;
            y = w[above];
            g = off[above];
            h = off[k];
            f = ((y - z) * (y + z) + (g - h) * (g + h)) / (2.0 * h * y);
            g = svd_hypot(f, 1.0);
            f = ((x - z) * (x + z) + h * ((y / (f + svd_with_sign(g, f))) - h)) / x;
            /* one QR transformation: a chase of Givens rotations down the block */
            c = s = 1.0;
            for (int j = lo; j <= above; j++) {
                const int i = j + 1;
                g = off[i];
                y = w[i];
                h = s * g;
                g = c * g;
                z = svd_hypot(f, h);
                off[j] = z;
                c = f / z;
                s = h / z;
                f = x * c + g * s;
                g = g * c - x * s;
                h = y * s;
                y *= c;
                for (int r = 0; r < 3; r++) {
                    x = v[r][j];
                    z = v[r][i];
                    v[r][j] = (float)(x * c + z * s);
                    v[r][i] = (float)(z * c - x * s);
                }
                z = svd_hypot(f, h);
                w[j] = (float)z;
                if (z) {
                    z = 1.0 / z;
                    c = f * z;
                    s = h * z;
                }
                f = c * g + s * y;
                x = c * y - s * g;
                for (int r = 0; r < 3; r++) {
                    y = a[r][j];
                    z = a[r][i];
                    a[r][j] = (float)(y * c + z * s);
                    a[r][i] = (float)(z * c - y * s);
                }
            }
            off[lo] = 0.0;
            off[k] = f;
            w[k] = (float)x;
        }
    }
}
KEYPOINT_MATH_HD void sort_eig(float w[3], float v[3][3])
{
    float t;
    for (int i = 0; i < 3; i++)
        for (int j = i + 1; j < 3; j++)
            if (w[i] < w[j]) {
                t = w[j]; w[j] = w[i]; w[i] = t;
                for (int k = 0; k < 3; k++) {
                    t = v[k][j]; v[k][j] = v[k][i]; v[k][i] = t;
                }
            }
}

/* eigen test, MultiScale.cpp:1748-1769, on the sorted singular values: 1 = the extremum is kept */
KEYPOINT_MATH_HD bool eigen_test_keep(const float *w, float eig_thres)
{
    float es = w[0] + w[1] + w[2];
    float ep = w[0] * w[1] * w[2];
    float esp = es * es * es;
    return esp < eig_thres * ep || eig_thres < 0;
}

/* whether patch voxel s lies inside the orientation radius (determineOrientation3D, MultiScale.cpp:2541-2607) */
KEYPOINT_MATH_HD bool in_radius(int s)
{
    const int pd = KEYPOINT_MATH_PD;
    const int x = s % pd - pd / 2, y = (s / pd) % pd - pd / 2, z = s / (pd * pd) - pd / 2;
    const float fx = (float)x, fy = (float)y, fz = (float)z;
    return fz * fz + fy * fy + fx * fx < (float)((pd / 2) * (pd / 2));
}

/* interpolate_discrete_3D_point on an 11^3 grid, R/src_common/MultiScale.cpp:1614-1639 */
KEYPOINT_MATH_HD void interp_point_patch(const float *g, int s, float *o)
{
    const int pd = KEYPOINT_MATH_PD, ix = s % pd, iy = (s / pd) % pd, iz = s / (pd * pd);
    const float c = g[s];
    o[0] = (float)interp_quadratic(ix - 1, ix, ix + 1, g[s - 1], c, g[s + 1]);
    o[1] = (float)interp_quadratic(iy - 1, iy, iy + 1, g[s - pd], c, g[s + pd]);
    o[2] = (float)interp_quadratic(iz - 1, iz, iz + 1, g[s - pd * pd], c, g[s + pd * pd]);
}

/* Splat parameters of one in-radius voxel: the cell of corner 000, packed ix | iy<<4 | iz<<8, and
 * the three weights of _fioDetermineInterpCoord for the position (x,y,z) on the 11^3 grid. */
KEYPOINT_MATH_HD void splat_params(float x, float y, float z, short &base, float &wx, float &wy, float &wz)
{
    int ix, iy, iz;
    interp_coord(x, 0, (float)KEYPOINT_MATH_PD, ix, wx);
    interp_coord(y, 0, (float)KEYPOINT_MATH_PD, iy, wy);
    interp_coord(z, 0, (float)KEYPOINT_MATH_PD, iz, wz);
    base = (short)(ix | (iy << 4) | (iz << 8));
}

/* The orientation octant of an interior voxel's gradient e (overwritten by its direction) of magnitude mg, for the
 * descriptor's histogram (msResampleFeaturesGradientOrientationHistogram, MultiScale.cpp:583-710): the octant whose diagonal
 * has the largest dot product with the direction, the first of equals. */
KEYPOINT_MATH_HD int gradient_octant(float mg, float *e)
{
    int best = 8; /* 8 = no contribution */
    if (mg > 0) {
        v3_norm(e);
        const float oa[8][3] = {{1, 1, 1},  {1, 1, -1},  {1, -1, 1},  {1, -1, -1},
                                {-1, 1, 1}, {-1, 1, -1}, {-1, -1, 1}, {-1, -1, -1}};
        best = 0;
        float bd = v3_dot(oa[0], e);
        DESC_BINS_UNROLL
        for (int t = 1; t < 8; t++) {
            float d = v3_dot(oa[t], e);
            if (d > bd) {
                bd = d;
                best = t;
            }
        }
    }
    return best;
}

#endif
