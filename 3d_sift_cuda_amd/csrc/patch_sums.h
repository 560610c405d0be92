/*
 * patch_sums.h -- the integer sums over a patch that both kernels of the label fusion keep (kernels_fuse.hip, DESIGN.md section
 * 7j; kernels_fuse_search.hip, section 7k), device code only: the sums and how a voxel enters them, and how the column sums of the
 * sliding form become a thread's window sums.  What the sums are worth is patch_cost.h's.  Each kernel stages its tiles itself: a
 * shared loader moved the search kernel's register counts.
 *
 * Under SSD only n and D = sum (qT - qW)^2 are kept (D = Sff - 2 Sfw + Sww exactly); under NCC n and the other five.  Every sum is below
 * 2^32 for a half-width b <= 6 (13^3 1023^2), and additions and subtractions are modulo 2^32, so no order of them changes a sum.
 */
#ifndef SIFT3D_PATCH_SUMS_H
#define SIFT3D_PATCH_SUMS_H
#include "patch_cost.h"
#include "warp_device.h"

struct patch_sums {
    unsigned n, sf, sff, sw, sww, sfw, d;
};

/* what a pair that counts adds under NCC, and its difference d under SSD; (0, 0) and d = 0 add nothing */
__device__ __forceinline__ void ps_moments(patch_sums &s, int f, int w)
{
    s.sf += (unsigned)f;
    s.sw += (unsigned)w;
    s.sff += (unsigned)__mul24(f, f);
    s.sww += (unsigned)__mul24(w, w);
    s.sfw += (unsigned)__mul24(f, w);
}

__device__ __forceinline__ void ps_square(patch_sums &s, int d) { s.d += (unsigned)__mul24(d, d); }

/* one pair of int16 tile values into the sums; it counts where neither is -1: the validity is the sign of f | w */
template <int NCC> __device__ __forceinline__ void ps_add(patch_sums &s, int f, int w)
{
    const int m = (f | w) >> 31; /* -1: the pair does not count */
    s.n += (unsigned)(1 + m);
    if (NCC) ps_moments(s, f & ~m, w & ~m);
    else ps_square(s, (f - w) & ~m);
}

/* one packed dword into the sums: f in bits 0 .. 15, w in bits 16 .. 30, and bit 31 says that the pair counts; one that does not
 * is staged as 0 */
template <int NCC> __device__ __forceinline__ void ps_add_packed(patch_sums &s, unsigned x)
{
    const int f = (int)(x & 0xffffu), w = (int)((x >> 16) & 0x7fffu);
    s.n += x >> 31;
    if (NCC) ps_moments(s, f, w);
    else ps_square(s, f - w);
}

/* a += b (sign > 0) or a -= b (sign < 0) */
template <int NCC> __device__ __forceinline__ void ps_merge(patch_sums &a, const patch_sums &b, int sign)
{
    const unsigned m = sign < 0 ? ~0u : 0u;
    a.n += (b.n ^ m) - m;
    if (NCC) {
        a.sf += (b.sf ^ m) - m;
        a.sff += (b.sff ^ m) - m;
        a.sw += (b.sw ^ m) - m;
        a.sww += (b.sww ^ m) - m;
        a.sfw += (b.sfw ^ m) - m;
    } else {
        a.d += (b.d ^ m) - m;
    }
}

/* section 7j's similarity u (0 .. 32768) of the two patches behind the sums */
template <int NCC> __device__ __forceinline__ unsigned ps_u(const patch_sums &s)
{
    return NCC ? pc_u_ncc(s.n, s.sf, s.sff, s.sw, s.sww, s.sfw) : pc_u_ssd(s.n, s.d);
}

/* The sliding form's last step.  col[c]: the sums over the (2B + 1)^2 rows of the patch at column c of the BRICK_VX + 2B columns
 * under a thread's BRICK_VX windows; out[v]: the sums of window v, columns v .. v + 2B.  The first window is added up, each next
 * one takes a column on and lets one go. */
template <int B, int NCC> __device__ __forceinline__ void ps_slide(const patch_sums (&col)[BRICK_VX + 2 * B], patch_sums (&out)[BRICK_VX])
{
    patch_sums win = patch_sums{0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 2 * B + 1; c++) ps_merge<NCC>(win, col[c], 1);
#pragma unroll
    for (int v = 0; v < BRICK_VX; v++) {
        out[v] = win;
        if (v + 1 < BRICK_VX) {
            ps_merge<NCC>(win, col[v + 2 * B + 1], 1);
            ps_merge<NCC>(win, col[v], -1);
        }
    }
}

#endif
