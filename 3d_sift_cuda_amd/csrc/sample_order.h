/*
 * sample_order.h -- the order in which the lanes of descriptor_kernel (kernels_descriptor.hip) take the 1331 samples of a
 * re-oriented record's patch, and the patch order wave_sample_patch (keypoint_device.h) takes them in otherwise.  Plain C++
 * for host and device, without a HIP include: tests/sample_order_check.cpp runs the same
 * functions on the CPU (tests/test_sample_order_cpu.py), as tests/desc_bins_check.cpp does for desc_bins.h.
 *
 * Which lane computes which patch value changes no value; it decides which 128-byte lines the 64 gathers of one instruction
 * touch, and the sampling phase takes its time over the count of line accesses (docs/experiments.md sections 4 and 15).  In
 * patch order neighbouring lanes sit one sample step apart along a rotated direction, so the four lanes of a quad read four
 * image rows.  Here the samples are sorted by the image row they read -- the (z, y) cell of their trilinear gather -- so that
 * neighbouring lanes read the same row, and rows that neighbour in y and z meet inside one instruction.
 *
 * The sort is a counting sort:
 *   1. sample_order_key: the bin of a sample, from the cells interp_coord gives for its position (sample_order_position, the
 *      arithmetic of sampleImage3D that wave_sample_patch uses too), taken relative to the record's centre.
 *   2. The bins are counted; a sample's rank is the count its bin had when it arrived (an atomic add's old value on the GPU).
 *   3. sample_order_chunk_total / sample_order_chunk_prefix: the counts become an exclusive prefix, every one of
 *      SAMPLE_ORDER_LANES lanes taking a run of counter words.
 *   4. sample_order_slot: prefix of the bin + rank.
 * Every sample has a key inside the bins whatever its position holds -- NaN and +-Inf are caught by comparisons before any
 * conversion to int -- and ranks within a bin are distinct, so the slots are a permutation of 0 .. 1330 for every input.
 *
 * Bins: a patch of radius rad reaches at most sqrt(3) * rad from its centre along an image axis when its frame is orthonormal,
 * so cells h below to h - 1 above the centre's, h = ceil(sqrt(3) * rad) + 1, per axis.  Anything further out (a frame that is
 * not orthonormal) is clamped to the outermost bin.  Two 16-bit counts share a word, and SAMPLE_ORDER_MAX_BINS of them fit
 * beside the list in the LDS that is dead during sampling; a larger footprint takes two (four, ...) planes, then rows, per bin.
 */
#ifndef SAMPLE_ORDER_H
#define SAMPLE_ORDER_H

#include <math.h>

#include "desc_bins.h" /* interp_coord */

#define SAMPLE_ORDER_HD DESC_BINS_HD
#define SAMPLE_ORDER_PD DESC_BINS_PD
#define SAMPLE_ORDER_PV (SAMPLE_ORDER_PD * SAMPLE_ORDER_PD * SAMPLE_ORDER_PD)
#define SAMPLE_ORDER_MAX_BINS 1224 /* 16-bit counters, two per word */
#define SAMPLE_ORDER_WORDS (SAMPLE_ORDER_MAX_BINS / 2)
#define SAMPLE_ORDER_LANES 128 /* DESC_NT: the lanes that share the prefix */
#define SAMPLE_ORDER_MAX_HALF 4096 /* cells to either side of the centre beyond which the bins no longer grow */

/* The scratch of one record's sort: the list and the counters.  It overlays LDS the descriptor kernel does not use while it
 * samples. */
struct sample_order_scratch {
    unsigned short order[SAMPLE_ORDER_PV + 1]; /* order[j]: the patch index of the j-th sample */
    unsigned count[SAMPLE_ORDER_WORDS];        /* bin b: bits 16 (b & 1) .. of word b >> 1; counts, then their exclusive prefix */
    unsigned wave_total;                       /* samples in the bins of the first wavefront's lanes */
};

/* sampleImage3D, R/src_common/MultiScale.cpp:2614-2714: where in the image patch voxel s is sampled.  inv: the inverse of the
 * frame, sc: voxels per patch step, (fx, fy, fz): the centre. */
SAMPLE_ORDER_HD inline void sample_order_position(const float *inv, float sc, float fx, float fy, float fz, int s, float *o)
{
    const int sr = SAMPLE_ORDER_PD / 2;
    const int xx = s % SAMPLE_ORDER_PD - sr, yy = (s / SAMPLE_ORDER_PD) % SAMPLE_ORDER_PD - sr, zz = s / (SAMPLE_ORDER_PD * SAMPLE_ORDER_PD) - sr;
    const float in3[3] = {(float)xx, (float)yy, (float)zz};
    DESC_BINS_UNROLL
    for (int i = 0; i < 3; i++) {
        float a = 0;
        DESC_BINS_UNROLL
        for (int j = 0; j < 3; j++) a += inv[i * 3 + j] * in3[j];
        o[i] = a;
    }
    o[0] *= sc; o[1] *= sc; o[2] *= sc;
    o[0] += fx; o[1] += fy; o[2] += fz;
}

/* The patch order, taken where there is no sorted list (the keypoint kernel's identity frame, SIFT3D_TUNE_DESC_ORDER 0, the
 * development stops).  Which sample a lane takes changes no value, only which memory lines the 64 gathers of one instruction
 * touch: the lanes walk the patch axis that runs closest to the volume's x first (then the one closest to y), so that
 * neighbouring lanes read neighbouring voxels of a row wherever the frame allows it (descriptor kernel at 512^3:
 * 4.12 -> 3.97 ms; the patch in Z-curve blocks of 4 x 4 x 4 instead of lines: no better).  inv: the inverse of the frame;
 * the strides are those of the fastest, the middle and the slowest axis in the patch. */
struct sample_order_strides {
    int fast, mid, slow;
};
SAMPLE_ORDER_HD inline sample_order_strides sample_order_patch_strides(const float *inv)
{
    const float f0 = fabsf(inv[0]), f1 = fabsf(inv[1]), f2 = fabsf(inv[2]);
    const int ax_fast = f0 >= f1 && f0 >= f2 ? 0 : (f1 >= f2 ? 1 : 2);
    const int r0 = ax_fast == 0 ? 1 : 0, r1 = ax_fast == 2 ? 1 : 2;
    const bool first = fabsf(inv[3 + r0]) >= fabsf(inv[3 + r1]);
    const int ax_mid = first ? r0 : r1, ax_slow = first ? r1 : r0, pd = SAMPLE_ORDER_PD;
    return {ax_fast == 0 ? 1 : (ax_fast == 1 ? pd : pd * pd), ax_mid == 0 ? 1 : (ax_mid == 1 ? pd : pd * pd),
            ax_slow == 0 ? 1 : (ax_slow == 1 ? pd : pd * pd)};
}
/* the patch voxel of the t-th sample in that order */
SAMPLE_ORDER_HD inline int sample_order_patch_voxel(int t, const sample_order_strides &st)
{
    const int pd = SAMPLE_ORDER_PD;
    return (t % pd) * st.fast + ((t / pd) % pd) * st.mid + (t / (pd * pd)) * st.slow;
}

/* The bins of one record. */
struct sample_order_bins {
    int half;       /* cells -half .. half - 1 relative to the centre's, per axis */
    int shy, shz;   /* rows / planes per bin: 1 << shy, 1 << shz */
    int ny, nz;     /* bins per axis; ny * nz <= SAMPLE_ORDER_MAX_BINS */
    float cy, cz;   /* floor of the centre's y and z (as floats: the centre may hold anything) */
};

SAMPLE_ORDER_HD inline sample_order_bins sample_order_bins_of(float rad, float fy, float fz)
{
    sample_order_bins b;
    const float hf = __builtin_ceilf(1.7320508f * rad) + 1.0f;
    /* the negated comparisons take a NaN radius too */
    b.half = !(hf >= 2.0f) ? 2 : (!(hf <= (float)SAMPLE_ORDER_MAX_HALF) ? SAMPLE_ORDER_MAX_HALF : (int)hf);
    b.shy = b.shz = 0;
    b.ny = b.nz = 2 * b.half;
    while (b.ny * b.nz > SAMPLE_ORDER_MAX_BINS) { /* planes are joined before rows: a bin stays a run of one row as long as it can */
        if (b.shz <= b.shy) b.shz++;
        else b.shy++;
        b.ny = ((2 * b.half - 1) >> b.shy) + 1;
        b.nz = ((2 * b.half - 1) >> b.shz) + 1;
    }
    b.cy = __builtin_floorf(fy);
    b.cz = __builtin_floorf(fz);
    return b;
}
SAMPLE_ORDER_HD inline int sample_order_nbins(const sample_order_bins &b) { return b.ny * b.nz; }

/* The cell interp_coord gives for coordinate v of an axis of n voxels; 0 for a NaN, which interp_coord would convert. */
SAMPLE_ORDER_HD inline int sample_order_cell(float v, int n)
{
    if (v != v) return 0;
    int i = 0;
    float w = 0;
    interp_coord(v, 0, (float)n, i, w); /* +-Inf and anything outside the axis leave through its first two branches */
    return i;
}

/* cell i of an axis against the centre's c: 0 .. 2 * half - 1, clamped by comparisons that a NaN or an infinite c fails */
SAMPLE_ORDER_HD inline int sample_order_rel(int i, float c, int half)
{
    const float d = (float)i - c;
    if (!(d > (float)-half)) return 0;
    if (!(d < (float)half)) return 2 * half - 1;
    return (int)d + half;
}

/* The bin of the sample at image position (., y, z) in a volume of Y rows and Z slices (those of the whole octave, as
 * trilinear takes them). */
SAMPLE_ORDER_HD inline int sample_order_key(const sample_order_bins &b, float y, float z, int Y, int Z)
{
    const int ky = sample_order_rel(sample_order_cell(y, Y), b.cy, b.half) >> b.shy;
    const int kz = sample_order_rel(sample_order_cell(z, Z), b.cz, b.half) >> b.shz;
    return kz * b.ny + ky;
}

/* A sample arrives at its bin: what to add to which counter word, and the rank in the word's old value. */
SAMPLE_ORDER_HD inline int sample_order_word(int key) { return key >> 1; }
SAMPLE_ORDER_HD inline unsigned sample_order_one(int key) { return 1u << (16 * (key & 1)); }
SAMPLE_ORDER_HD inline int sample_order_field(unsigned word, int key) { return (int)((word >> (16 * (key & 1))) & 0xffffu); }

/* Lane l of SAMPLE_ORDER_LANES turns the counter words [first, last) into prefixes. */
SAMPLE_ORDER_HD inline void sample_order_chunk(int nbins, int lane, int &first, int &last)
{
    const int nwords = (nbins + 1) / 2, per = (nwords + SAMPLE_ORDER_LANES - 1) / SAMPLE_ORDER_LANES;
    first = lane * per < nwords ? lane * per : nwords;
    last = first + per < nwords ? first + per : nwords;
}
SAMPLE_ORDER_HD inline unsigned sample_order_chunk_total(const unsigned *count, int first, int last)
{
    unsigned t = 0;
    for (int w = first; w < last; w++) t += (count[w] & 0xffffu) + (count[w] >> 16);
    return t;
}
/* base: the samples in all bins before the lane's */
SAMPLE_ORDER_HD inline void sample_order_chunk_prefix(unsigned *count, int first, int last, unsigned base)
{
    for (int w = first; w < last; w++) {
        const unsigned lo = count[w] & 0xffffu, hi = count[w] >> 16;
        count[w] = base | ((base + lo) << 16); /* at most 1331: it fits 16 bits */
        base += lo + hi;
    }
}
/* after the prefix: where the sample of this bin and rank stands in the order */
SAMPLE_ORDER_HD inline int sample_order_slot(const unsigned *count, int key, int rank) { return sample_order_field(count[sample_order_word(key)], key) + rank; }

#endif
