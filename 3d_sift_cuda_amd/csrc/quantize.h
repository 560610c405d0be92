/*
 * quantize.h -- the 10-bit map of the intensities: the affine map the host fixed by its range, lo to 0 and
 * hi to QMAX, rounded to the nearest integer; -1 for a voxel that is not finite.  bm_quantize_kernel (kernels_blockmatch.hip) keeps
 * the values as an int16 plane, joint_hist_kernel (kernels_similarity.hip) in registers; tests/blockmatch_oracle.c restates the
 * map.  The constant is for the host too (similarity_host.c turns quantised differences back into intensities).
 */
#ifndef SIFT3D_QUANTIZE_H
#define SIFT3D_QUANTIZE_H

#define QMAX 1023

#ifdef __HIPCC__
__device__ __forceinline__ int quantize(float v, double lo, double hi)
{
    int q = -1;
    if (isfinite(v)) {
        const double t = (((double)v - lo) / (hi - lo)) * (double)QMAX;
        q = t <= 0.0 ? 0 : (t >= (double)QMAX ? QMAX : (int)rint(t));
    }
    return q;
}
#endif

#endif
