/*
 * patch_cost.h -- what two patches' integer sums are worth: the correlation cost of the block matcher and
 * the two similarities of the label fusion (section 7j) on top of it.  One source compiled as device code (kernels_blockmatch.hip,
 * kernels_fuse.hip, kernels_fuse_search.hip) and as host code (fuse_host.c), so every path performs the same operations in the
 * same order; the oracles under tests/ restate them independently and do not include this file.
 *
 * The sums are exact integers; the one floating-point passage is pc_ncc_cost's sequence of IEEE double operations.  It is the
 * oracles' sequence only in a translation unit built with -ffp-contract=off and without fast-math (every includer is), and fp64
 * multiply and divide are correctly rounded on the device.
 */
#ifndef SIFT3D_PATCH_COST_H
#define SIFT3D_PATCH_COST_H
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PC_FN static __host__ __device__ inline
#else
#include <math.h>
#define PC_FN static inline
#endif

/* Section 7g: cost = rint((1 - rho^2) 2^31) of the zero-mean normalised cross-correlation rho, from A = N Sfw - Sf Sw and the
 * variances Vf = N Sff - Sf^2, Vw = N Sww - Sw^2 (|A|, V <= (13^3 1023)^2 < 2^43: each converts to double exactly).  Multiply,
 * multiply, divide, clamp at 1, subtract, multiply by 2^31, rint.  A flat patch or a correlation that is not positive costs 2^31. */
PC_FN uint32_t pc_ncc_cost(int64_t A, int64_t Vf, int64_t Vw)
{
    double q = 0.0;
    if (A > 0 && Vf > 0 && Vw > 0) q = ((double)A * (double)A) / ((double)Vf * (double)Vw);
    q = q > 1.0 ? 1.0 : q;
    return (uint32_t)rint((1.0 - q) * 2147483648.0);
}

/* Section 7j, u under NCC from the six sums over the n voxels that count: section 7g's cost with n in place of N, then
 * (2^31 - cost) >> 16; an empty patch is worth 0 */
PC_FN uint32_t pc_u_ncc(int64_t n, int64_t sf, int64_t sff, int64_t sw, int64_t sww, int64_t sfw)
{
    if (n <= 0) return 0;
    return (0x80000000u - pc_ncc_cost(n * sfw - sf * sw, n * sff - sf * sf, n * sww - sw * sw)) >> 16;
}

/* Section 7j, u under SSD: (n 2^15) / (D + n), D = sum (qT - qW)^2 = Sff - 2 Sfw + Sww.  For a patch of half-width b <= 6,
 * n 2^15 <= 13^3 2^15 < 2^27 and D + n <= 13^3 1023^2 + 13^3 < 2^32: a 32-bit division with the value of the contract's 64-bit one
 * (sift3d_fuse_similarity) */
PC_FN uint32_t pc_u_ssd(uint32_t n, uint32_t d)
{
    if (n == 0) return 0;
    return (n << 15) / (d + n);
}

#endif
