/*
 * keypoint_device.h -- what the two per-keypoint kernels share, device only: keypoint_kernel (phase A, kernels_keypoint.hip)
 * and descriptor_kernel (phase B, kernels_descriptor.hip) both sample an 11^3 patch from a level, normalise it and blur an
 * 11^3 LDS volume.  The scalar arithmetic is keypoint_math.h's, the order of the samples sample_order.h's.
 *
 * Parity contract: the reference does all of this in scalar CPU code whose
 * float accumulations are order dependent (R/src_common/MultiScale.cpp).  Work is
 * spread over the lanes only where the result does not depend on the
 * order (sampling, gradients, per-voxel terms, 3/5-tap patch blurs, peak
 * tests, rank counting); every order-dependent sum is kept as ONE sequential
 * chain in the reference's raster order, with one lane per independent chain
 * (9 lanes for the structure tensor, 8 lanes for the 8 corners of a splat, 64
 * lanes for the 64 descriptor bins).  Compiled with -ffp-contract=off.
 */
#ifndef KEYPOINT_DEVICE_H
#define KEYPOINT_DEVICE_H

#include "keypoint_math.h"
#include "sample_order.h"
#include "sift3d_internal.h"

#define PD SIFT3D_PATCH_DIM
#define PV SIFT3D_PATCH_VOX
static_assert(PD == KEYPOINT_MATH_PD && PD == SAMPLE_ORDER_PD && PV == SAMPLE_ORDER_PV, "one patch edge");

#define NRAD 485 /* voxels of the 11^3 patch with dx^2+dy^2+dz^2 < 25 (all of them interior); <= 25 would be 515 */
#define NRAD_PAD 516 /* the length of the per-voxel arrays: keypoint_kernel's LDS layout is built on it */
#define NINT 729 /* interior voxels 1..9 in each axis */

/* fioGetPixelTrilinearInterp, R/src_common/FeatureIO.cpp:812-850 */
/* (x,y,z) are coordinates in the whole octave volume (Z = its slice count); img holds Zl slices
 * starting at global slice z_off, so cell and weights are those of the undivided volume and only
 * the address is shifted.  The clamp is a memory-safety net: with the 32-slice halo of Z-slab
 * mode (patch reach < 29 slices) it never binds. */
__device__ __forceinline__ float trilinear(const float *__restrict__ img, int X, int XP, int Y, int Z, int Zl, int z_off,
                                           float x, float y, float z)
{
    float wx, wy, wz;
    int ix, iy, iz;
    interp_coord(x, 0, (float)X, ix, wx);
    interp_coord(y, 0, (float)Y, iy, wy);
    interp_coord(z, 0, (float)Z, iz, wz);
    iz -= z_off;
    iz = iz < 0 ? 0 : (iz > Zl - 2 ? Zl - 2 : iz);
    const long long XY = (long long)XP * Y; /* XP: row pitch; X only bounds the coordinates */
    const float *p = img + (long long)iz * XY + (long long)iy * XP + ix;
    /* the two x-neighbours of a corner pair are adjacent in memory: four 8-byte gathers (dword aligned)
     * instead of eight 4-byte ones */
    typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));
    const f2u q00 = *reinterpret_cast<const f2u *>(p), q10 = *reinterpret_cast<const f2u *>(p + XP);
    const f2u q01 = *reinterpret_cast<const f2u *>(p + XY), q11 = *reinterpret_cast<const f2u *>(p + XY + XP);
    const float f000 = q00.x, f100 = q00.y, f010 = q10.x, f110 = q10.y;
    const float f001 = q01.x, f101 = q01.y, f011 = q11.x, f111 = q11.y;
    float fn00 = wx * f000 + (1.0f - wx) * f100;
    float fn01 = wx * f001 + (1.0f - wx) * f101;
    float fn10 = wx * f010 + (1.0f - wx) * f110;
    float fn11 = wx * f011 + (1.0f - wx) * f111;
    float fnn0 = wy * fn00 + (1.0f - wy) * fn10;
    float fnn1 = wy * fn01 + (1.0f - wy) * fn11;
    return wz * fnn0 + (1.0f - wz) * fnn1;
}

/* ---------------------------------------------------------------------- */
/* wave-cooperative building blocks (block = NT lanes)                     */
/* ---------------------------------------------------------------------- */

/* sampleImage3D, R/src_common/MultiScale.cpp:2614-2714 (bounds test done by the caller).  order: nullptr (the patch order of
 * sample_order.h), or the list wave_sort_samples left -- the j-th sample taken is patch voxel order[j] */
template <int NT>
__device__ __forceinline__ void wave_sample_patch(float *patch, const float *__restrict__ img, int X, int XP, int Y, int Z, int Zl,
                                                  int z_off, float fx, float fy, float fz, float scale, const float *ori9,
                                                  const unsigned short *order = nullptr)
{
    float inv[9];
    invert3(ori9, inv);
    const float rad = 2.0f * scale;
    const int sr = PD / 2;
    const float sc = rad / (float)(sr);
    const sample_order_strides st = sample_order_patch_strides(inv);
    /* three samples per lane per trip: the 24 gathers of a trip are issued together */
    for (int s0 = threadIdx.x; s0 < PV; s0 += 3 * NT) {
        float pix[3];
        int sidx[3];
#pragma unroll
        for (int u = 0; u < 3; u++) {
            const int t = s0 + NT * u;
            pix[u] = 0;
            sidx[u] = 0;
            if (t < PV) {
                /* the patch voxel this lane samples */
                const int s = order ? order[t] : sample_order_patch_voxel(t, st);
                sidx[u] = s;
                float o[3];
                sample_order_position(inv, sc, fx, fy, fz, s, o);
                if (o[0] < 0 || o[0] >= X) pix[u] = 0;
                else pix[u] = trilinear(img, X, XP, Y, Z, Zl, z_off, o[0], o[1], o[2]);
            }
        }
#pragma unroll
        for (int u = 0; u < 3; u++)
            if (s0 + NT * u < PV) patch[sidx[u]] = pix[u];
    }
    __syncthreads();
}

/* One sequential float sum over the 1331 patch values (optionally of their
 * squares), in raster order, by one lane; 16-byte LDS reads. d is 16-byte aligned. */
template <bool SQUARE>
__device__ __forceinline__ float serial_sum_patch(const float *d)
{
    /* 1331 = 41 blocks of 32 + 19: read a block of 32 values (eight 16-byte LDS reads) while the
     * previous block is being added, so the LDS latency stays off the add chain */
    float acc = 0;
    const v4f *d4 = reinterpret_cast<const v4f *>(d);
    /* two register buffers used alternately (the block loop unrolled by two): a single buffer pair with a copy at the end
     * of every block cost 32 register moves per 32 additions, doubling the instructions of a chain that runs on one lane */
    v4f a[8], b[8];
    auto add_block = [&](const v4f(&blk)[8]) {
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const v4f v = blk[q];
            if (SQUARE) {
                acc += v.x * v.x; acc += v.y * v.y; acc += v.z * v.z; acc += v.w * v.w;
            } else {
                acc += v.x; acc += v.y; acc += v.z; acc += v.w;
            }
        }
    };
#pragma unroll
    for (int q = 0; q < 8; q++) a[q] = d4[q];
    for (int blk = 0; blk + 1 < 41; blk += 2) { /* blocks blk (in a) and blk + 1 (into b), then blk + 2 into a */
#pragma unroll
        for (int q = 0; q < 8; q++) b[q] = d4[(blk + 1) * 8 + q];
        add_block(a);
#pragma unroll
        for (int q = 0; q < 8; q++) a[q] = d4[(blk + 2) * 8 + q]; /* blk + 2 <= 40: the last block, added after the loop */
        add_block(b);
    }
    add_block(a); /* block 40 */
    for (int i = 41 * 32; i < PV; i++) acc += SQUARE ? d[i] * d[i] : d[i];
    return acc;
}

/* Feature3D::NormalizeData, R/src_common/MultiScale.cpp:127-205: the two
 * 1331-term sums are single sequential chains (lane 0). */
template <int NT>
__device__ __forceinline__ void wave_normalize_patch(float *d, float *scratch2)
{
    if (threadIdx.x == 0) scratch2[0] = serial_sum_patch<false>(d) / (PD * PD * PD);
    __syncthreads();
    const float mean = scratch2[0];
    for (int i = threadIdx.x; i < PV; i += NT) d[i] -= mean;
    __syncthreads();
    if (threadIdx.x == 0) scratch2[1] = 1.0f / sqrtf(serial_sum_patch<true>(d));
    __syncthreads();
    const float div = scratch2[1];
    for (int i = threadIdx.x; i < PV; i += NT) d[i] *= div;
    __syncthreads();
}

/* One pass of the separable patch blur: a thread takes a whole line of the axis and slides the filter window along it,
 * one LDS read per output instead of one per tap (the per-keypoint kernels are bound by the LDS unit).  Per output the
 * same chain as before: acc = 0, then taps in ascending order, positions outside the patch skipped. */
template <int NT>
__device__ __forceinline__ void blur_pass(const float *src, float *dst, int axis, const float *taps, int ntaps)
{
    const int h = ntaps / 2;
    const int st = axis == 0 ? 1 : (axis == 1 ? PD : PD * PD);
    float tp[5], w[5];
#pragma unroll
    for (int j = 0; j < 5; j++) tp[j] = j < ntaps ? taps[j] : 0.0f;
    for (int ln = threadIdx.x; ln < PD * PD; ln += NT) {
        const int base = axis == 0 ? ln * PD : (axis == 1 ? (ln / PD) * PD * PD + ln % PD : ln);
#pragma unroll
        for (int j = 0; j < 5; j++) { /* window of output 0: positions -h .. +h */
            const int pos = j - h;
            w[j] = (j < ntaps && pos >= 0 && pos < PD) ? src[base + pos * st] : 0.0f;
        }
#pragma unroll
        for (int c = 0; c < PD; c++) {
            float acc = 0;
#pragma unroll
            for (int j = 0; j < 5; j++) {
                const int cc = c + j - h;
                if (j < ntaps && cc >= 0 && cc < PD) acc = acc + tp[j] * w[j];
            }
            dst[base + c * st] = acc;
            const int nx = c + 1 + h; /* the position entering the window */
            const float in = nx < PD ? src[base + nx * st] : 0.0f;
#pragma unroll
            for (int j = 0; j < 4; j++) w[j] = w[j + 1];
            if (ntaps >= 1) w[ntaps - 1 < 4 ? ntaps - 1 : 4] = in;
        }
    }
    __syncthreads();
}
/* 3- or 5-tap separable blur of an 11^3 LDS volume, pass order x,y,z, zero
 * borders (gb3d_blur3d on the patch: R/src_common/MultiScale.cpp:2850,2972,1032).
 * The result lands in tmp_a (in -> tmp_a -> tmp_b -> tmp_a; tmp_b may be the input buffer); taps are in LDS. */
template <int NT>
__device__ __forceinline__ void wave_blur_patch(float *in, float *tmp_a, float *tmp_b, const float *taps, int ntaps)
{
    blur_pass<NT>(in, tmp_a, 0, taps, ntaps);
    blur_pass<NT>(tmp_a, tmp_b, 1, taps, ntaps);
    blur_pass<NT>(tmp_b, tmp_a, 2, taps, ntaps);
}

#endif
