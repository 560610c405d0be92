/*
 * sift3d_internal.h -- declarations shared by the HIP translation units of libsift3d_hip.so (kernel launchers and the
 * context).  Not installed.  The launch decisions of the fused blur and of the extrema passes: blur_plan.h, extrema_plan.h.
 */
#ifndef SIFT3D_INTERNAL_H
#define SIFT3D_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "blur_plan.h"
#include "extrema_plan.h"
#include "sift3d.h"
#include "sift3d_dev.h" /* the self-test and, in DEV builds, the development hooks: declared apart from the boundary */

#define SIFT3D_MAX_TAPS 129
#define SIFT3D_FAST_MAX_R 8 /* templated kernels cover 3..17 taps (every sigma the pyramid uses) */
#define SIFT3D_PATCH_DIM 11
#define SIFT3D_PATCH_VOX 1331

struct sift3d_taps {
    float f[2 * SIFT3D_FAST_MAX_R + 1];
};

/* a row taken as 16-byte vectors (VEC = 4) or element by element (VEC = 1): the whole-volume kernels */
typedef float v4f __attribute__((ext_vector_type(4)));
template <int VEC>
struct vecT;
template <> struct vecT<4> { typedef v4f type; };
template <> struct vecT<1> { typedef float type; };
template <int VEC>
__device__ __forceinline__ typename vecT<VEC>::type vload(const float *p)
{
    return *reinterpret_cast<const typename vecT<VEC>::type *>(p);
}
template <int VEC>
__device__ __forceinline__ void vstore(float *p, typename vecT<VEC>::type v)
{
    *reinterpret_cast<typename vecT<VEC>::type *>(p) = v;
}

/* Candidates are kept as (key, value) pairs so that one device radix sort puts them in the
 * reference's order: key = level id << 40 | is_max << 39 | linear voxel index, with
 * level id = octave*3 + (DoG level - 1).  Minima sort before maxima, raster order inside. */
#define SIFT3D_KEY_LVL_SHIFT 40
#define SIFT3D_KEY_MAX_SHIFT 39
#define SIFT3D_KEY_IDX_MASK ((1ull << 39) - 1ull)
/* an own-level extremum on its way to the two-level validation */
struct sift3d_survivor {
    long long idx;
    float value;
    int is_max;
};
/* an extremum that passed the test against the level below, on its way to the test against a level above that is
 * evaluated around it instead of being stored (extrema_validate_lazy_kernel) */
struct sift3d_survivor2 {
    int x, y, z;   /* position in the (pitched) volume */
    int is_max;
    float value;
    float h;       /* the level below at the extremum */
};
struct sift3d_cval {
    float value, h, l, pad; /* DoG at the extremum, one level below (H), one level above (L) */
};

/* one detection level of one octave (table in device memory) */
struct sift3d_level {
    const float *img;  /* Gaussian level L_k the keypoints are sampled from */
    const float *dogc; /* DoG level k (centre) */
    int X, Y, Z;       /* dims of the whole octave volume (Z is the global slice count) */
    int XP;            /* row pitch of img/dogc in floats (== X for a dense volume) */
    float sigma_h, sigma_c, sigma_l;
    float octave_factor; /* 2^octave */
    int Zl;    /* slices held in img/dogc (== Z on one GPU; slab + halos in Z-slab mode) */
    int z_off; /* global z of local slice 0 */
    int pad;
};

/* ---- allocation (alloc_fill.hip): every device and pinned host block of the library comes through these, so that the fill
 * hook of sift3d_selftest_alloc_fill sees it.  Released with hipFree / hipHostFree as before. ---- */
#pragma GCC visibility push(hidden)
hipError_t sift3d_alloc_device(void **p, size_t bytes);
hipError_t sift3d_alloc_host(void **p, size_t bytes, unsigned flags);
/* a piece cut from a block the caller keeps from run to run (the slab rank's arena): filled like a new block when the hook is on */
hipError_t sift3d_alloc_reused(void *p, size_t bytes);
#pragma GCC visibility pop

/* ---- kernel launchers (kernels_volume.hip; the fused blur: kernels_blur_fused.hip) ---- */
hipError_t sift3d_launch_blur_x(hipStream_t s, const float *in, float *out, int64_t X, int64_t Y, int64_t Z,
                                const float *taps, int ntaps, const float *d_taps);
hipError_t sift3d_launch_blur_y(hipStream_t s, const float *in, float *out, int64_t X, int64_t Y, int64_t Z,
                                const float *taps, int ntaps, const float *d_taps);
/* prev/dog may be NULL (no DoG epilogue) */
hipError_t sift3d_launch_blur_z(hipStream_t s, const float *in, float *out, const float *prev, float *dog, int64_t X,
                                int64_t Y, int64_t Z, const float *taps, int ntaps, const float *d_taps);
/* all three passes and the DoG in one kernel; hipErrorNotSupported when the shape is outside it.  tune: what
 * sift3d_set_tuning forces (blur_plan.h, which decides the form of the kernel that runs) */
hipError_t sift3d_launch_blur_fused(hipStream_t s, const float *in, float *out, float *dog, int64_t X, int64_t Y, int64_t Z,
                                    const float *taps, int ntaps, const sift3d_blur_tuning &tune, int64_t zo0 = 0, int64_t zo1 = -1,
                                    float *sub = nullptr, int *sub_done = nullptr);
hipError_t sift3d_launch_dog(hipStream_t s, const float *a, const float *b, float *out, int64_t n);
hipError_t sift3d_launch_subsample(hipStream_t s, const float *in, int64_t X, int64_t Xl, int64_t Y, int64_t Z, float *out,
                                   int64_t XPout);
hipError_t sift3d_launch_zero_pad(hipStream_t s, float *a, float *b, int64_t X, int64_t Xl, int64_t rows);
/* levels 1..5 (L[4] may be NULL) and DoGs 0..4 of an octave of at most SIFT3D_TINY_VOX voxels from its level 0, rows of
 * pitch XP; hipErrorNotSupported outside that */
#define SIFT3D_TINY_VOX 4096
/* contexts of at most this many floats allocate the two pass intermediates of the three-launch blur when they are created */
#define SIFT3D_EAGER_T_FLOATS (1ll << 31)
struct sift3d_octave_out {
    float *L[5];
    float *D[5];
};
struct sift3d_octave_taps {
    float f[5][2 * SIFT3D_FAST_MAX_R + 1];
    int n[5];
};
hipError_t sift3d_launch_tiny_octave(hipStream_t s, const float *L0, const sift3d_octave_out &o, int64_t X, int64_t XP, int64_t Y,
                                     int64_t Z, const sift3d_octave_taps &t);
hipError_t sift3d_launch_double_size(hipStream_t s, const float *in, int64_t X, int64_t Y, int64_t Z, float *out);
hipError_t sift3d_launch_halve_size(hipStream_t s, const float *in, int64_t X, int64_t Y, int64_t Z, float *out);
/* ---- extrema passes (kernels_extrema.hip; every launch decision: extrema_plan.h) ---- */
/* Neighbour levels that are not stored as DoG volumes (NULL or all-zero: both neighbours are the stored dprev / dnext).
 * prev_b: the level below is dprev - prev_b, two Gaussian levels.  next_g: the level above is next_g - blur(next_g, taps),
 * and blur(next_g) is evaluated only at the 27 voxels around each extremum that passed everything else (dnext is ignored;
 * the shapes and filters this takes: lazy_shape_ok and extrema_lazy_status, extrema_plan.h). */
struct sift3d_extrema_lazy {
    const float *prev_b;
    const float *next_g;
    float taps[2 * SIFT3D_FAST_MAX_R + 1];
    int ntaps;
    sift3d_survivor2 *list2;         /* EX_SEGS segments of list2_cap / EX_SEGS entries, one per slab of z, like the own-level list */
    unsigned long long *list2_count; /* SIFT3D_LIST2_COUNTERS words, zeroed by the caller */
    int64_t list2_cap;               /* at least surv_cap of the same call */
};
static_assert(EX_LAZY_NTAPS == 2 * SIFT3D_FAST_MAX_R + 1, "the third phase is built for the widest filter of the templated kernels");
/* where validated extrema are appended: (key, value) pairs, their count on the device, the room there is */
struct cand_target {
    unsigned long long *keys;
    sift3d_cval *vals;
    unsigned long long *count; /* on the device */
    int64_t cap;
};
/* one extrema pass: a detection level, where its extrema go, and the own-level list between the first and the second phase */
struct sift3d_extrema_pass {
    const float *dprev, *dcur, *dnext; /* dnext may be NULL: no level above */
    int64_t X, Xl, Y, Z;               /* X: row pitch, Xl: logical row length (Xl == X for a dense volume) */
    int z_lo, z_hi, lvl_id;            /* planes searched: the interior ones of [z_lo, z_hi) */
    cand_target out;
    sift3d_survivor *surv;             /* NULL: no list, every voxel takes all three tests in one launch */
    unsigned long long *surv_count;    /* SIFT3D_SURV_COUNTERS words */
    unsigned long long *surv_overflow; /* raised to the length a list cut short would have needed */
    int64_t surv_cap;
    bool zero_counters;                /* clear surv_count first (the pipeline hands every level its own, already zeroed, set instead) */
    const sift3d_extrema_lazy *lazy;   /* or NULL */
    bool strict;                       /* the first phase compares element by element (sift3d_volume_needs_strict) */
};
/* hipErrorNotSupported / hipErrorInvalidValue: what the plan refuses, with nothing queued */
hipError_t sift3d_launch_extrema(hipStream_t s, const sift3d_extrema_pass &p);
/* Volumes the max / min form of the first extrema pass would get wrong: a NaN anywhere (v_max_f32 / v_min_f32 return the
 * other operand, so "c > max of 26" would hold beside a NaN neighbour where the reference's element-wise "every neighbour < c"
 * fails), an infinity, or a magnitude above FLT_MAX / 4 (the blur, DoG and subsample can overflow it to an infinity, and
 * inf - inf is NaN).  sift3d_launch_scan_strict ORs 1 into *flag when any of the n floats at v is such a value. */
hipError_t sift3d_launch_scan_strict(hipStream_t s, const float *v, int64_t n, unsigned *flag);
bool sift3d_volume_needs_strict(const float *v, int64_t n); /* the same test on host memory */
/* the three detection levels of an octave of at most SIFT3D_TINY_VOX voxels (d[0..4]: its five stored DoG levels) in one launch */
hipError_t sift3d_launch_extrema_octave_small(hipStream_t s, const float *const d[5], int64_t X, int64_t Xl, int64_t Y, int64_t Z,
                                              int lvl_id0, const cand_target &out);
#define SIFT3D_SURV_SETS 96 /* one counter set per extrema pass of a pipeline run, zeroed together */
#define SIFT3D_SURV_COUNTERS (EX_SEGS * EX_SEG_STRIDE)
#define SIFT3D_LIST2_COUNTERS EX_SEGS

/* ---- per-keypoint stage (phase A: kernels_keypoint.hip; phase B and the record bookkeeping: kernels_descriptor.hip; what
 * both share: keypoint_device.h, keypoint_math.h, sample_order.h) ---- */
/* The development stops: what sift3d_dev_set_stop (include/sift3d_dev.h) takes and debug_stop carries.  -DSIFT3D_DEV builds
 * only; a kernel returns after the stage named, so that the stages can be timed by difference. */
enum sift3d_dev_stop {
    SIFT3D_STOP_NONE = 0, /* run everything */
    /* keypoint_kernel (tools/kp_ablate.py); every extremum is reported as rejected */
    SIFT3D_STOP_A_SAMPLED = 1,     /* after the identity-frame patch is sampled */
    SIFT3D_STOP_A_NORMALIZED = 2,  /* after the patch is normalised */
    SIFT3D_STOP_A_TENSOR = 3,      /* after the gradients and the nine structure-tensor chains */
    SIFT3D_STOP_A_SPLAT = 4,       /* after the SVD + eigen test and the first orientation splat */
    SIFT3D_STOP_A_SPLAT_5 = 5, SIFT3D_STOP_A_SPLAT_6 = 6, /* the same place as 4 */
    SIFT3D_STOP_A_BLURRED = 7,     /* after the blur of the primary histogram */
    SIFT3D_STOP_A_PEAKS = 8,       /* after the peak search of the primary histogram */
    SIFT3D_STOP_A2_PREPASS = 31,   /* first primary peak: after the pre-pass of the secondary splat */
    SIFT3D_STOP_A2_SPLAT = 32,     /* first primary peak: after the secondary splat */
    SIFT3D_STOP_A2_BLURRED = 33,   /* first primary peak: after the blur of the secondary histogram */
    SIFT3D_STOP_A2_PEAKS = 34,     /* first primary peak: after the peak search of the secondary histogram */
    SIFT3D_STOP_A_SVD_FIRST = 40,  /* no stop: the SVD + eigen test before the first splat, not beside it (tools/kp_svd_first.py) */
    /* descriptor_kernel (tools/desc_ablate.py) */
    SIFT3D_STOP_B_SAMPLED = 11,    /* after the record's patch is loaded or sampled */
    SIFT3D_STOP_B_NORMALIZED = 12, /* after the patch is normalised */
    SIFT3D_STOP_B_GRADIENTS = 13,  /* SIFT-rank: after the gradient pre-pass */
    /* 21 .. 26: every record samples one cache-resident region of its level instead of its own patch, then */
    SIFT3D_STOP_B_CACHED_SAMPLED = 21,    /* stops after that sampling */
    SIFT3D_STOP_B_CACHED_ALL = 22,        /* runs to the end */
    SIFT3D_STOP_B_CACHED_NORMALIZED = 23, /* stops where 12 does */
    SIFT3D_STOP_B_CACHED_GRADIENTS = 24,  /* stops where 13 does */
    SIFT3D_STOP_B_CACHED_25 = 25,         /* no stage of its own: runs to the end as 22 does */
    SIFT3D_STOP_B_CACHED_BINS = 26,       /* SIFT-rank: stops after the bin chains */
};
struct sift3d_kp_params {
    const sift3d_level *levels; /* device table indexed by level id */
    float eig_thres;
    float size_factor;
    int desc_mode;
    int debug_stop; /* a sift3d_dev_stop; -DSIFT3D_DEV builds only (timing ablation, tools/kp_ablate.py); 0 = run everything */
    float *patch0;  /* per extremum: the identity-frame patch (1331 floats, normalised once) that phase A sampled anyway;
                     * phase B reads it for the un-reoriented record instead of sampling it again */
    int *sampler_tokens; /* phase B: per-CU count of workgroups in their sampling phase (SIFT3D_CU_SLOTS ints, zero between runs) */
    int sampler_cap;     /* at most this many per CU sample at a time (0: no limit) */
    int desc_seg;        /* descriptor kernel: records per segment of the XCD-contiguous order (a multiple of 8; 0: the whole list is one) */
    int desc_order;      /* descriptor kernel: 1 = the lanes take a re-oriented record's samples in image-row order (sample_order.h), 0 = in patch order */
    const int *rec_shift; /* descriptor kernel: NULL, or SIFT3D_GROUPS ints -- record r of group g is stored at slot r + rec_shift[g] (several
                           * contexts writing one merged list: the slab driver) */
};
/* SIFT3D_GROUPS (include/sift3d.h, 193): level id * 2 + is_max for up to 96 levels, and one slot for anything beyond */
hipError_t sift3d_launch_group_counts(hipStream_t s, const unsigned long long *keys, const int *nrec, int64_t ncand, int *counts);
#define SIFT3D_CU_SLOTS 2048
#define SIFT3D_MAX_FRAMES 11 /* determineCanonicalOrientation3D stops at FEATURE_3D_DIM frames */
/* phase A result per extremum */
struct sift3d_dkp {
    float x, y, z, scale; /* octave coordinates, +0.5 applied */
    float eigs[3];
    float ori0[9]; /* sorted eigenvectors (record 0) */
    int nframes;
    float frames[SIFT3D_MAX_FRAMES * 9];
    int lvl;
    unsigned info;
};
/* nrec[k] = 0 (rejected) or 1 + number of canonical frames */
hipError_t sift3d_launch_keypointsA(hipStream_t s, const sift3d_kp_params &p, const unsigned long long *keys,
                                    const sift3d_cval *vals, int64_t ncand, sift3d_dkp *kps, int *nrec, const float *taps3);
/* nrec / offs: one chunk of the candidate list starting at candidate cand_off; rec_base[0] = its first record (in), rec_base[1] =
 * the first record of the next chunk (out) */
hipError_t sift3d_launch_recmap(hipStream_t s, const int *nrec, const int *offs, int64_t ncand, int cand_off, int *rec_base,
                                int *rec_kp, int *rec_frame, unsigned long long *kp_count);
hipError_t sift3d_launch_descriptors(hipStream_t s, const sift3d_kp_params &p, const sift3d_dkp *kps, const int *rec_kp,
                                     const int *rec_frame, int64_t nrec, sift3d_feature *recs, int *rec_group,
                                     const float *taps5);
/* device sort / scan (sort_scan.hip, rocPRIM) */
size_t sift3d_sort_temp_bytes(int64_t n);
hipError_t sift3d_sort_candidates(hipStream_t s, void *temp, size_t temp_bytes, const unsigned long long *keys_in,
                                  unsigned long long *keys_out, const sift3d_cval *vals_in, sift3d_cval *vals_out, int64_t n);
size_t sift3d_scan_temp_bytes(int64_t n);
hipError_t sift3d_scan_counts(hipStream_t s, void *temp, size_t temp_bytes, const int *in, int *out, int64_t n);

/* ---- matcher (kernels_match.hip) ---- */
/* stats: three words the caller has preset to {~0, ~0, 0} */
hipError_t sift3d_launch_knn_norms(hipStream_t s, const signed char *v, int64_t n, int *norms, unsigned long long *stats);
hipError_t sift3d_launch_knn(hipStream_t s, const signed char *db, const int *db_norm, int64_t n_db, const signed char *q, const int *q_norm,
                             int64_t n_q, int k, int const_norm, int groups, int segments, int *part_d, int *part_i, int *out_i, int *out_d);
int sift3d_knn_list_length(int k);
void sift3d_knn_plan(int64_t n_db, int64_t n_q, int k, int *groups, int *segments);

/* ---- alignment (kernels_align.hip), resampling (kernels_resample.hip), guided re-matching (kernels_refine.hip) ---- */
hipError_t sift3d_launch_ratio(hipStream_t s, const signed char *db, const int *db_norm, int64_t n_db, const signed char *q, const int *q_norm,
                               int64_t n_q, const float *geo, const unsigned *info, float lo, float hi, int *i1, int *d1, int *i2, int *d2);
hipError_t sift3d_launch_hough(hipStream_t s, const float *p0, const float *p1, const float *s0, const float *s1, const float *o0, const float *o1,
                               int M, float lo, float hi, int one, int *counts, int *flags, float *hyp);
hipError_t sift3d_launch_resample(hipStream_t s, const float *src, int64_t nx, int64_t ny, int64_t nz, float *dst, int64_t ox, int64_t oy,
                                  int64_t oz, const float *map, int mode, float fill);
hipError_t sift3d_launch_guided(hipStream_t s, const void *f_rows, const int *f_norm, const float *f_pos, const unsigned *f_info, const int *f_idx,
                                int n_f, const int *cell_start, const long long *keys, const double grid_o[3], double edge, const long long grid_n[3],
                                int dense, const void *m_rows, const float *m_pos, const unsigned *m_info, const int *order, int n_m,
                                const float c0[3], const float c1[3], const float rot[9], float scale, float radius, float lo, float hi, int *i1,
                                int *d1, int *i2, int *d2, int *visited);

/* ---- host code the alignment and the guided re-matching share (align_api.hip) ---- */
#pragma GCC visibility push(hidden)
/* the ratio intervals of the two scale thresholds, computed once from the host's logf: [0] LOG_1_5 (ratio and guided
 * search), [1] HOUGH_THRES_SCALE; ok[k] == 0 where that logf is not monotonic near threshold k */
struct sift3d_scale_intervals {
    float lo[2], hi[2];
    int ok[2];
};
const sift3d_scale_intervals &sift3d_scale_ivs();
/* The capacity rule of sift3d_similarity: with room for the n pairs, the arrays out names get them (moving, fixed, inlier, dist2)
 * and SIFT3D_OK; else "<n> <what>, arrays for <capacity>" in err and SIFT3D_ERR_CAPACITY, or SIFT3D_OK where out has no arrays. */
int sift3d_put_pairs(sift3d_similarity *out, int32_t n, const int32_t *moving, const int32_t *fixed, const int32_t *inlier, const int32_t *dist2,
                     const char *what, char *err, int64_t err_len);
#pragma GCC visibility pop

#endif
