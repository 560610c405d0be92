/*
 * desc_bins.h -- the 64 bin sums of the SIFT-rank descriptor (msResampleFeaturesGradientOrientationHistogram,
 * R/src_common/MultiScale.cpp:583-710) as descriptor_kernel<true> (kernels_descriptor.hip) forms them: which lane holds which
 * bin, which voxels a bin's chain visits and with which weights.  Plain C++ for host and device, without a HIP include:
 * tests/desc_bins_check.cpp runs the same walk on the CPU against the oracle's o3_desc_sift (tests/test_desc_bins_cpu.py), as
 * tests/blur_plan_check.cpp does for blur_plan.h.
 *
 * The reference splats every interior voxel of the 11^3 patch (1..9 per axis; the border has zero gradient) that has a
 * non-zero gradient into a 2 x 2 x 2 x 8 histogram: orientation octant `bin`, trilinear weights over the two spatial bins of
 * each axis, all eight corners incremented, the zero-weight ones included, in raster order z, y, x.  So bin (bx, by, bz, o) is
 * ONE float chain over the voxels of octant o in raster order, with the term ((mg * wx) * wy) * wz.
 *
 * The weights do not depend on the record (desc_bins_weight, held to this table by the static_asserts below):
 *
 *     patch coordinate c     1 2 3 4    5    6 7 8 9
 *     weight of bin 0        1 1 1 1   0.5   0 0 0 0
 *     weight of bin 1        0 0 0 0   0.5   1 1 1 1
 *
 * so bin (bx, by, bz) has a non-zero weight only on its 5 x 5 x 5 box: 1..5 along an axis whose bin is 0, 5..9 along one whose
 * bin is 1.  The box walk (desc_bins_walk) visits the 125 voxels of the box in raster order and adds the term where the voxel's
 * octant is the lane's and +0.0f where it is not: a fixed trip count, addresses that are the lane's base plus a compile-time
 * offset, no lists.  It gives the bits of the chain over the whole octant because
 *   - a voxel of octant o outside the box has a weight of exactly 0 on at least one axis, and mg is finite there (below), so its
 *     term is mg * 0 = +0 (mg > 0, the weights are >= 0: no -0 arises);
 *   - acc starts at +0 and receives only terms >= +0, so it is never -0, and acc + (+0) is acc bit for bit -- whether the +0 is
 *     such a term, left out, or the walk's own for a voxel of another octant;
 *   - inside the box the terms are the same products in the same order, the multiplications by 1 included.
 * mg is finite or the voxel takes no part: a NaN anywhere in the sampled patch makes the mean and hence every value NaN, and a
 * NaN gradient has magnitude "not > 0", which is bin 8.  One case remains: a patch so faint that the sum of its squares
 * underflows to 0 is normalised by 1 / 0 to +-Inf values, and where it is normalised only once (the re-oriented records) a
 * gradient of magnitude +Inf with an octant results.  There the zero-weight terms are Inf * 0 = NaN and do count, so such a
 * record (desc_bins_needs_all; none in any volume an instrument delivers) takes the chain over all 729 voxels with all their
 * weights (desc_bins_walk_all), which is the reference's sum literally.
 */
#ifndef DESC_BINS_H
#define DESC_BINS_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DESC_BINS_HD __host__ __device__
#else
#define DESC_BINS_HD
#endif
#if defined(__clang__)
#define DESC_BINS_UNROLL _Pragma("unroll")
#define DESC_BINS_ROLLED _Pragma("nounroll")
#else
#define DESC_BINS_UNROLL
#define DESC_BINS_ROLLED
#endif

#define DESC_BINS_PD 11   /* patch edge (SIFT3D_PATCH_DIM) */
#define DESC_BINS_NI 9    /* interior voxels per axis: patch coordinates 1 .. 9 */
#define DESC_BINS_NINT 729
#define DESC_BINS_BOX 5   /* voxels per axis on which a spatial bin has a non-zero weight */
#define DESC_BINS_NONE 8  /* octant of a voxel without a gradient: it takes no part */
/* The kernel's arrays keep a plane of 81 interior voxels every 83 entries: the eight box origins of a wavefront (entries 0, 4,
 * 36, 40 and the same one plane-of-four further) then fall into eight different LDS banks instead of six. */
#define DESC_BINS_ZS 83
#define DESC_BINS_LEN (DESC_BINS_NI * DESC_BINS_ZS)

/* floorf where the compiler evaluates interp_coord itself (the static_asserts below): its floorf is no constant expression.  An
 * argument outside int's range stops the compilation there. */
DESC_BINS_HD constexpr float desc_bins_floor_ce(float x) { return (float)(int)x > x ? (float)((int)x - 1) : (float)(int)x; }

/* _fioDetermineInterpCoord, R/src_common/FeatureIO.cpp:757-782 */
DESC_BINS_HD constexpr void interp_coord(float fX, float fMin, float fMax, int &ix, float &w)
{
    if (fX < fMin + 0.5f) {
        ix = (int)fMin;
        w = 1.0f;
    } else if (fX >= fMax - 0.5f) {
        ix = (int)(fMax - 2);
        w = 0.0f;
    } else {
        float mh = fX - 0.5f;
        ix = (int)(__builtin_is_constant_evaluated() ? desc_bins_floor_ce(mh) : __builtin_floorf(mh));
        w = 1.0f - (mh - ((float)ix));
    }
}

/* spatial coordinate of patch index c in the 2-bin grid (MultiScale.cpp:641-671), then the trilinear weight of bin b along that
 * axis (fioIncPixelTrilinearInterp, FeatureIO.cpp:853-889) */
DESC_BINS_HD constexpr float desc_bins_weight(int b, int c)
{
    const float binsz = DESC_BINS_PD / (float)2;
    float v = (int)(c / binsz) + 0.5f;
    if ((int)((c + 0) / binsz) != (int)((c + 1) / binsz)) {
        float p0 = ((c + 0) / binsz);
        float p1 = ((c + 1) / binsz);
        v = (p0 + p1) / 2.0f;
    }
    float w = 0;
    int i0 = 0;
    interp_coord(v, 0, 2.0f, i0, w);
    return b ? 1.0f - w : w;
}
static_assert(desc_bins_weight(0, 1) == 1 && desc_bins_weight(0, 2) == 1 && desc_bins_weight(0, 3) == 1 && desc_bins_weight(0, 4) == 1 &&
                  desc_bins_weight(1, 1) == 0 && desc_bins_weight(1, 2) == 0 && desc_bins_weight(1, 3) == 0 && desc_bins_weight(1, 4) == 0,
              "patch coordinates 1 .. 4 belong to bin 0 alone");
static_assert(desc_bins_weight(0, 5) == 0.5f && desc_bins_weight(1, 5) == 0.5f, "the centre plane is shared in halves");
static_assert(desc_bins_weight(0, 6) == 0 && desc_bins_weight(0, 7) == 0 && desc_bins_weight(0, 8) == 0 && desc_bins_weight(0, 9) == 0 &&
                  desc_bins_weight(1, 6) == 1 && desc_bins_weight(1, 7) == 1 && desc_bins_weight(1, 8) == 1 && desc_bins_weight(1, 9) == 1,
              "patch coordinates 6 .. 9 belong to bin 1 alone");

/* lane = ((bz * 2 + by) * 2 + bx) * 8 + o, the reference's index of the bin in the descriptor */
DESC_BINS_HD constexpr int desc_bins_octant(int lane) { return lane & 7; }
DESC_BINS_HD constexpr int desc_bins_axis_bin(int lane, int axis) { return (lane >> (3 + axis)) & 1; }
/* first patch coordinate of the box of spatial bin b along an axis */
DESC_BINS_HD constexpr int desc_bins_origin(int b) { return b ? DESC_BINS_BOX : 1; }
/* entry of the interior voxel at patch coordinates (x, y, z), each 1 .. 9, in arrays of DESC_BINS_LEN */
DESC_BINS_HD constexpr int desc_bins_entry(int x, int y, int z) { return (z - 1) * DESC_BINS_ZS + (y - 1) * DESC_BINS_NI + (x - 1); }

/* does a voxel's magnitude force the chain over all voxels?  (mg > 0 there, so it has an octant) */
DESC_BINS_HD constexpr bool desc_bins_needs_all(float mg) { return mg == __builtin_huge_valf(); }

/* The five weights of the lane's box along one axis, from the arithmetic above: 1 1 1 1 0.5 for bin 0, 0.5 1 1 1 1 for bin 1. */
DESC_BINS_HD inline void desc_bins_box_weights(int b, float *w)
{
    DESC_BINS_UNROLL
    for (int d = 0; d < DESC_BINS_BOX; d++) w[d] = b ? desc_bins_weight(1, desc_bins_origin(1) + d) : desc_bins_weight(0, desc_bins_origin(0) + d);
}

/* The chain of one lane's bin over its box.  mag / bin: arrays of DESC_BINS_LEN indexed by desc_bins_entry. */
DESC_BINS_HD inline float desc_bins_walk(const float *mag, const unsigned char *bin, int lane)
{
    const int o = desc_bins_octant(lane);
    const int bx = desc_bins_axis_bin(lane, 0), by = desc_bins_axis_bin(lane, 1), bz = desc_bins_axis_bin(lane, 2);
    float wx[DESC_BINS_BOX], wy[DESC_BINS_BOX], wz[DESC_BINS_BOX];
    desc_bins_box_weights(bx, wx);
    desc_bins_box_weights(by, wy);
    desc_bins_box_weights(bz, wz);
    const int base = desc_bins_entry(desc_bins_origin(bx), desc_bins_origin(by), desc_bins_origin(bz));
    mag += base;
    bin += base;
    float acc = 0;
    DESC_BINS_UNROLL
    for (int dz = 0; dz < DESC_BINS_BOX; dz++) {
        DESC_BINS_UNROLL
        for (int dy = 0; dy < DESC_BINS_BOX; dy++) {
            DESC_BINS_UNROLL
            for (int dx = 0; dx < DESC_BINS_BOX; dx++) {
                const int e = dz * DESC_BINS_ZS + dy * DESC_BINS_NI + dx;
                const float term = ((mag[e] * wx[dx]) * wy[dy]) * wz[dz];
                acc += bin[e] == o ? term : 0.0f; /* selected, not branched: the trip is the same for all lanes */
            }
        }
    }
    return acc;
}

/* The chain of one lane's bin over all interior voxels of its octant, zero weights included: the reference's sum literally. */
DESC_BINS_HD inline float desc_bins_walk_all(const float *mag, const unsigned char *bin, int lane)
{
    const int o = desc_bins_octant(lane);
    const int bx = desc_bins_axis_bin(lane, 0), by = desc_bins_axis_bin(lane, 1), bz = desc_bins_axis_bin(lane, 2);
    float acc = 0;
    DESC_BINS_ROLLED /* never taken on real data: kept small */
    for (int z = 1; z <= DESC_BINS_NI; z++)
        DESC_BINS_ROLLED
        for (int y = 1; y <= DESC_BINS_NI; y++)
            DESC_BINS_ROLLED
            for (int x = 1; x <= DESC_BINS_NI; x++) {
                const int e = desc_bins_entry(x, y, z);
                if (bin[e] == o) acc += ((mag[e] * desc_bins_weight(bx, x)) * desc_bins_weight(by, y)) * desc_bins_weight(bz, z);
            }
    return acc;
}

#endif
