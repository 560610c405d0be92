/*
 * kernels_descriptor.hip -- phase B of the per-keypoint stage for gfx950: patch re-sampling + 64-value descriptor + rank
 * transform, one output record per workgroup, and the record bookkeeping between the phases (records per group, the map from
 * records to keypoints and frames).  The patch and every histogram live in LDS.  Phase A (extremum -> keypoint and its
 * frames) is kernels_keypoint.hip; what the two share, and the parity contract, keypoint_device.h; the scalar arithmetic,
 * keypoint_math.h; the bin chains, desc_bins.h; the order of the samples, sample_order.h.
 */
#include <cstddef>
#include <type_traits>

#include "keypoint_device.h"

#define DESC_NT 128  /* phase B: one record per workgroup of two wavefronts (15 independent records per CU beat 8 four-wave workgroups) */

/* The development stops (sift3d_dev_stop, sift3d_internal.h) */
#ifdef SIFT3D_DEV
#define DESC_DEV_STOP(cond) if (cond) return;
#else
#define DESC_DEV_STOP(cond)
#endif

/* The order in which wave_sample_patch is to take the samples of a re-oriented record: by the image row they read
 * (sample_order.h), a counting sort by the NT lanes of the workgroup.  tmp: PV words that are dead until the sampling (the patch
 * itself).  Which sample of a bin gets which rank is the arrival order of the LDS atomics and varies from run to run; the list
 * is a permutation of the patch voxels either way, and a patch value is the same whichever lane computes it, so no result
 * depends on it. */
template <int NT>
__device__ __forceinline__ void wave_sort_samples(sample_order_scratch &so, unsigned *tmp, int Y, int Z, float fx, float fy, float fz,
                                                  float scale, const float *ori9)
{
    static_assert(NT == SAMPLE_ORDER_LANES && NT == 128, "the prefix is shared by two wavefronts");
    float inv[9];
    invert3(ori9, inv);
    const float rad = 2.0f * scale;
    const float sc = rad / (float)(PD / 2);
    const sample_order_bins b = sample_order_bins_of(rad, fy, fz);
    const int nbins = sample_order_nbins(b), lane = threadIdx.x;
    for (int w = lane; w < (nbins + 1) / 2; w += NT) so.count[w] = 0;
    __syncthreads();
    for (int s = lane; s < PV; s += NT) {
        float o[3];
        sample_order_position(inv, sc, fx, fy, fz, s, o);
        const int key = sample_order_key(b, o[1], o[2], Y, Z);
        const unsigned old = atomicAdd(&so.count[sample_order_word(key)], sample_order_one(key));
        tmp[s] = ((unsigned)key << 16) | (unsigned)sample_order_field(old, key); /* bin and rank in it */
    }
    __syncthreads();
    int first, last;
    sample_order_chunk(nbins, lane, first, last);
    const unsigned mine = sample_order_chunk_total(so.count, first, last);
    unsigned incl = mine; /* inclusive scan over the wavefront's 64 lanes */
#pragma unroll
    for (int d = 1; d < 64; d *= 2) {
        const unsigned up = __shfl_up(incl, d, 64);
        if ((lane & 63) >= d) incl += up;
    }
    if (lane == 63) so.wave_total = incl;
    __syncthreads();
    sample_order_chunk_prefix(so.count, first, last, incl - mine + (lane >= 64 ? so.wave_total : 0u));
    __syncthreads();
    for (int s = lane; s < PV; s += NT) {
        const unsigned kr = tmp[s];
        so.order[sample_order_slot(so.count, (int)(kr >> 16), (int)(kr & 0xffffu))] = (unsigned short)s;
    }
    __syncthreads();
}

/* Workgroups are dealt round-robin over the 8 XCDs (b and b+8 share one, with its private L2), and the
 * work items arrive sorted by (level, raster index), so neighbours in the list sample neighbouring
 * image regions: an XCD takes RUNS of consecutive items instead of every eighth item, and the trilinear
 * gathers of neighbouring keypoints / of the frames of one keypoint meet in one L2.
 * Round 4: the runs are short -- the list is cut into segments of seg items (256 by default) and each
 * segment is dealt to the XCDs in contiguous eighths -- so that all eight XCDs are in the same part of the
 * list at the same time.  With one eighth of the WHOLE list per XCD (rounds 2 - 3) the eighths took
 * different times (the records of the first detection levels sample compact footprints, the later ones
 * sparse ones) and the kernel ended with some XCDs idle for a tenth of its time: 9.60 -> 9.23 ms per 512^3
 * extraction (profiles/r04_desc_segment.txt).  Placement only changes speed, never results. */
__device__ __forceinline__ long long xcd_contiguous_item(long long n, int seg)
{
    const long long b = blockIdx.x;
    if (seg <= 0) {
        const long long per = (n + 7) / 8;
        return (b % 8) * per + b / 8;
    }
    /* the list in segments of seg items (a multiple of 8), each dealt to the XCDs in contiguous eighths: every XCD still walks
     * neighbouring items, and all eight are in the same part of the list at the same time */
    const long long s0 = b / seg * seg, local = b - s0;
    return s0 + (local % 8) * (seg / 8) + local / 8;
}

/* ---------------------------------------------------------------------- */
/* Phase B: one output record per workgroup: re-sample, normalise, describe */
/* ---------------------------------------------------------------------- */
/* value of lane i (compile-time i) of a wavefront-wide float: v_readlane_b32 */
__device__ __forceinline__ float lane_value(float x, int i)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), i));
}

/* pair tables of msGenerateBRIEFindex method 2 (data, R/src_common/MultiScale.cpp:805-807) */
__constant__ unsigned char c_brief_x[192] = {
    5,4,4,4,4,2,6,5,5,4,4,4,3,8,5,5,6,3,5,5,5,5,6,5,4,6,6,6,3,4,4,4,5,3,4,5,4,5,5,4,2,7,7,5,3,5,4,5,3,5,7,3,5,5,2,3,5,5,6,6,4,6,5,4,
    4,6,5,3,5,6,4,3,6,4,4,5,3,3,3,6,6,5,2,4,4,6,3,6,3,2,3,5,4,5,3,4,3,6,5,4,3,6,4,5,2,4,3,7,2,3,6,5,2,6,3,3,5,6,3,6,3,5,3,6,5,7,4,2,
    5,5,5,2,5,7,4,2,5,3,4,3,3,7,4,4,7,6,4,4,2,8,7,6,5,4,7,3,6,6,5,2,4,5,3,2,5,5,1,6,3,6,3,6,2,5,4,4,7,2,6,3,2,2,4,3,3,2,3,4,2,5,6,7};
__constant__ unsigned char c_brief_y[192] = {
    6,5,3,4,5,3,7,4,6,4,3,2,4,7,5,3,5,1,5,4,7,6,8,4,4,5,6,5,2,5,4,6,4,0,4,3,3,4,4,2,1,7,8,6,4,4,1,6,1,3,7,2,3,3,1,3,6,1,6,6,4,7,6,4,
    3,5,4,2,3,6,4,5,6,3,3,5,1,3,1,6,7,4,1,4,3,5,2,4,2,1,2,5,4,5,2,3,3,3,3,4,2,6,3,4,3,3,3,6,1,2,5,4,2,4,1,4,6,7,3,6,2,4,3,6,5,6,4,0,
    6,6,5,1,4,7,2,1,5,3,4,2,2,7,3,3,6,4,2,4,1,9,7,7,5,2,7,1,7,5,5,1,5,4,1,3,3,4,0,5,1,6,3,5,3,2,3,3,7,2,5,1,1,0,4,1,3,1,0,3,1,6,5,9};

struct kpB_sift { /* SIFT-rank: per interior voxel gradient magnitude + orientation octant, laid out by desc_bins_entry */
    float mag[DESC_BINS_LEN];
    unsigned char bin[DESC_BINS_LEN + 1];
    /* Not used.  It keeps a record's LDS where the octant lists had it, so that 15 workgroups share a CU and not the 17 the two
     * arrays above would admit: with 17 waiting for the sampling tokens the sampling phase is 0.14 ms slower at 512^3 and the
     * whole step 0.23 ms (docs/experiments.md section 13) */
    int hold[379];
    int all; /* a magnitude of +Inf: the chains take all 729 voxels (desc_bins.h) */
};
struct kpB_brief { /* BRIEF family: blur output (the middle pass goes back into the patch) */
    float t1[PV + 1];
};
/* LDS of one record: 10.6 KB for both instantiations */
template <bool SIFT>
struct kpB_smem {
    float patch[PV + 1];
    union {
        typename std::conditional<SIFT, kpB_sift, kpB_brief>::type v;
        sample_order_scratch order; /* the sampling order of a re-oriented record: dead once the patch is sampled, before v is first written */
    } u;
    float sc[16];
    float taps[8];
};

static_assert(sizeof(kpB_smem<true>) > 160 * 1024 / 16 && sizeof(kpB_smem<true>) <= 160 * 1024 / 15 && sizeof(kpB_smem<false>) > 160 * 1024 / 16 &&
                  sizeof(kpB_smem<false>) <= 160 * 1024 / 15,
              "15 records per CU by LDS (160 KB)");
/* kpB_sift::all is set before the sort and first read long after it */
static_assert(sizeof(sample_order_scratch) <= offsetof(kpB_sift, all) && sizeof(sample_order_scratch) <= sizeof(kpB_brief),
              "the sampling order overlays only what is dead while a patch is sampled");

template <bool SIFT>
__global__ __launch_bounds__(DESC_NT) void descriptor_kernel(sift3d_kp_params p, const sift3d_dkp *__restrict__ kps,
                                                        const int *__restrict__ rec_kp, const int *__restrict__ rec_frame,
                                                        long long nrec, sift3d_feature *__restrict__ recs,
                                                        int *__restrict__ rec_group, sift3d_taps taps5)
{
    __shared__ __attribute__((aligned(16))) kpB_smem<SIFT> sm;
    const long long r = xcd_contiguous_item(nrec, p.desc_seg);
    if (r >= nrec) return;
    const int lane = threadIdx.x;
    if (lane < 5) sm.taps[lane] = taps5.f[lane];
    if constexpr (SIFT) {
        if (lane == 5) sm.u.v.all = 0; /* raised by the gradient pre-pass, behind the barriers of the normalisation */
    }
    const sift3d_dkp *kp = kps + rec_kp[r];
    const int fr = rec_frame[r]; /* -1: the un-reoriented record */
    float ori[9];
    if (fr < 0) {
        ori[0] = 1; ori[1] = 0; ori[2] = 0; ori[3] = 0; ori[4] = 1; ori[5] = 0; ori[6] = 0; ori[7] = 0; ori[8] = 1;
    } else {
        for (int i = 0; i < 9; i++) ori[i] = kp->frames[fr * 9 + i];
    }
    const sift3d_level lv = p.levels[kp->lvl];
#ifdef SIFT3D_DEV /* timing ablation (tools/desc_ablate.py): every record samples one cache-resident region */
    if (p.debug_stop >= SIFT3D_STOP_B_CACHED_SAMPLED && p.debug_stop <= SIFT3D_STOP_B_CACHED_BINS) {
        wave_sample_patch<DESC_NT>(sm.patch, lv.img, lv.X, lv.XP, lv.Y, lv.Z, lv.Zl, lv.z_off, 20.0f, 20.0f, 20.0f, 3.0f, ori);
        if (p.debug_stop == SIFT3D_STOP_B_CACHED_SAMPLED) return;
    } else
#endif
    if (fr < 0) {
        /* record 0 is sampled with the identity frame and normalised once inside generateFeature3D
         * (MultiScale.cpp:1742): phase A did exactly that and left the result in patch0 */
        const float *src = p.patch0 + (long long)rec_kp[r] * PV;
        for (int s = lane; s < PV; s += DESC_NT) sm.patch[s] = src[s];
        __syncthreads();
    } else {
        /* The gathers of this phase are paced by the L1's miss handling, and the fewer footprints (a patch's is the size of
         * the whole L1) share a CU's L1 at a time the better it hits -- while the chains of the later phases want every
         * resident workgroup they can hide under.  So at most sampler_cap workgroups per CU sample at once: one takes a
         * token of its CU (a counter in memory, indexed by the hardware's XCC / SE / SH / CU numbers) before the phase and
         * gives it back after it; the others wait asleep and cost no issue slots.  Which CU a counter really belongs to
         * only affects speed. */
        /* the order of the samples is worked out first: a workgroup that waits for a token has it ready */
        if (p.desc_order) wave_sort_samples<DESC_NT>(sm.u.order, reinterpret_cast<unsigned *>(sm.patch), lv.Y, lv.Z, kp->x, kp->y, kp->z, kp->scale, ori);
        int *tok = nullptr;
        if (p.sampler_cap > 0) {
            unsigned hw, xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            tok = p.sampler_tokens + ((((xcc & 7u) * 8u + ((hw >> 13) & 7u)) * 2u + ((hw >> 12) & 1u)) * 16u + ((hw >> 8) & 15u));
            if (lane == 0) {
                /* (bounded: a counter that was left high -- it cannot be, every taker gives back -- must not hold the kernel
                 * for ever; after ~0.1 s of waiting the workgroup samples without a token of its own) */
                for (int tries = 0;; tries++) {
                    if (atomicAdd(tok, 1) < p.sampler_cap || tries > 50000) break;
                    atomicSub(tok, 1);
                    __builtin_amdgcn_s_sleep(64);
                }
            }
            __syncthreads();
        }
        if (p.desc_order)
            wave_sample_patch<DESC_NT>(sm.patch, lv.img, lv.X, lv.XP, lv.Y, lv.Z, lv.Zl, lv.z_off, kp->x, kp->y, kp->z, kp->scale, ori, sm.u.order.order);
        else
            wave_sample_patch<DESC_NT>(sm.patch, lv.img, lv.X, lv.XP, lv.Y, lv.Z, lv.Zl, lv.z_off, kp->x, kp->y, kp->z, kp->scale, ori);
        if (tok && lane == 0) atomicSub(tok, 1);
    }
    /* ... and every record is normalised once more in main (featExtract.cpp:480) */
    DESC_DEV_STOP(p.debug_stop == SIFT3D_STOP_B_SAMPLED);
    wave_normalize_patch<DESC_NT>(sm.patch, sm.sc);
    DESC_DEV_STOP(p.debug_stop == SIFT3D_STOP_B_NORMALIZED || p.debug_stop == SIFT3D_STOP_B_CACHED_NORMALIZED);

    const bool w0 = lane < 64; /* wavefront 0: lane = descriptor bin for everything that follows the parallel pre-pass */
    float myval = 0.0f;
    if constexpr (SIFT) {
        /* msResampleFeaturesGradientOrientationHistogram, MultiScale.cpp:583-710.  Border voxels
         * have zero gradient (FeatureIO.cpp:2307-2312) and are skipped there, so only the 9^3
         * interior takes part. */
        for (int q = lane; q < NINT; q += DESC_NT) {
            const int x = q % 9 + 1, y = (q / 9) % 9 + 1, z = q / 81 + 1;
            const int s = (z * PD + y) * PD + x;
            float e[3] = {sm.patch[s + 1] - sm.patch[s - 1], sm.patch[s + PD] - sm.patch[s - PD],
                          sm.patch[s + PD * PD] - sm.patch[s - PD * PD]};
            float mg = v3_mag(e);
            const int best = gradient_octant(mg, e);
            const int en = desc_bins_entry(x, y, z);
            sm.u.v.mag[en] = mg;
            sm.u.v.bin[en] = (unsigned char)best;
            if (desc_bins_needs_all(mg)) sm.u.v.all = 1;
        }
        __syncthreads();
        DESC_DEV_STOP(p.debug_stop == SIFT3D_STOP_B_GRADIENTS || p.debug_stop == SIFT3D_STOP_B_CACHED_GRADIENTS);
        if (w0) {
            /* lane = ((z*2+y)*2+x)*8 + orientation: one sequential chain per bin, over the 5^3 box on which the bin's weights are
             * not zero (desc_bins.h says why that is the reference's sum over the whole octant, bit for bit) */
            const float acc = sm.u.v.all ? desc_bins_walk_all(sm.u.v.mag, sm.u.v.bin, lane) : desc_bins_walk(sm.u.v.mag, sm.u.v.bin, lane);
            DESC_DEV_STOP(p.debug_stop == SIFT3D_STOP_B_CACHED_BINS);
            /* msNormalizeDataPositive, MultiScale.cpp:1580-1611 (lane i's value through v_readlane_b32: a scalar
             * broadcast instead of an LDS permute per term) */
            float mn = 100000;
#pragma unroll
            for (int i = 0; i < 64; i++) {
                float vi = lane_value(acc, i);
                if (vi < mn) mn = vi;
            }
            float v = acc - mn;
            float ss = 0;
#pragma unroll
            for (int i = 0; i < 64; i++) {
                float vi = lane_value(v, i);
                ss += vi * vi;
            }
            float div = 1.0f / sqrtf(ss);
            myval = v * div;
        }
    } else {
        /* msResampleFeaturesBRIEF, MultiScale.cpp:989-1049 */
        wave_blur_patch<DESC_NT>(sm.patch, sm.u.v.t1, sm.patch, sm.taps, 5);
        if (w0) {
            const float *bl = sm.u.v.t1;
            const int x1 = c_brief_x[3 * lane], y1 = c_brief_x[3 * lane + 1], z1 = c_brief_x[3 * lane + 2];
            const int x2 = c_brief_y[3 * lane], y2 = c_brief_y[3 * lane + 1], z2 = c_brief_y[3 * lane + 2];
            float d = bl[x1 + y1 * PD + z1 * PD * PD] - bl[x2 + y2 * PD + z2 * PD * PD];
            if (p.desc_mode == SIFT3D_DESC_BRIEF) {
                myval = (d < 0) ? 1.0f : 0.0f;
            } else if (p.desc_mode == SIFT3D_DESC_RRIEF) {
                myval = d;
            } else {
                float fdx = x1 - x2, fdy = y1 - y2, fdz = z1 - z2;
                int dist = (int)sqrtf(fdx * fdx + fdy * fdy + fdz * fdz);
                myval = d / dist;
            }
        }
    }
    if (!w0) return;
    /* NormalizeDataRankedPCs, MultiScale.cpp:207-233, order of :3148-3176 */
    int rank = 0;
    const unsigned long long nans = __ballot(myval != myval);
    if (nans == 0) {
#pragma unroll
        for (int j = 0; j < 64; j++) {
            float vj = lane_value(myval, j);
            rank += (vj < myval || (vj == myval && j < lane)) ? 1 : 0;
        }
    } else {
        /* NaN values (a patch that reached a NaN region of the volume): the reference's stable insertion sort moves a value
         * left only past values that compare greater, and nothing compares greater than or less than a NaN -- so every NaN
         * keeps its own index and the values between two NaNs are sorted among themselves (o3_rank) */
        const unsigned long long below = nans & ((1ull << lane) - 1ull), above = lane == 63 ? 0ull : nans & ~((2ull << lane) - 1ull);
        const int lo = below ? 64 - __clzll((long long)below) : 0; /* first index of this lane's run of non-NaN values */
        const int hi = above ? __ffsll((long long)above) - 1 : 64;  /* one past its last */
        rank = lo;
        for (int j = 0; j < 64; j++) {
            float vj = lane_value(myval, j);
            rank += (j >= lo && j < hi && (vj < myval || (vj == myval && j < lane))) ? 1 : 0;
        }
        if (myval != myval) rank = lane;
    }
    /* where the record goes: slot r of this launch's records -- or, when several contexts write ONE merged list (the slab
     * driver), shifted by a per-group offset: a rank's records are sorted by group already, so the merged position of its
     * record r is r + rec_shift[group] (group = level id * 2 + is_max) */
    const int grp = kp->lvl * 2 + ((kp->info & SIFT3D_INFO_MIN0MAX1) ? 1 : 0);
    sift3d_feature *out = recs + r + (p.rec_shift ? (long long)p.rec_shift[grp] : 0ll);
    out->desc[lane] = (float)rank;
    /* The seventeen words in front of the descriptor, one lane each: one 68-byte store instead of seventeen 4-byte ones by
     * lane 0 (the records may lie in host memory, where every store is a transaction on the bus). */
    static_assert(offsetof(sift3d_feature, desc) == 17 * 4 && offsetof(sift3d_feature, ori) == 16 && offsetof(sift3d_feature, eigs) == 52 &&
                      offsetof(sift3d_feature, info) == 64, "record layout: x y z scale ori[9] eigs[3] info desc[64]");
    if (lane < 17) {
        /* octave -> image space (MultiScale.cpp:531-543), then fSizeFactor (featExtract.cpp:502-505) */
        const float fac = lv.octave_factor, add = 0;
        unsigned word;
        if (lane < 4) {
            float v = lane == 0 ? kp->x : (lane == 1 ? kp->y : (lane == 2 ? kp->z : kp->scale));
            if (lane == 3) v *= fac;
            else v = v * fac + add;
            v *= p.size_factor;
            word = __builtin_bit_cast(unsigned, v);
        } else if (lane < 13) {
            word = __builtin_bit_cast(unsigned, fr < 0 ? kp->ori0[lane - 4] : kp->frames[fr * 9 + lane - 4]);
        } else if (lane < 16) {
            word = __builtin_bit_cast(unsigned, kp->eigs[lane - 13]);
        } else {
            word = kp->info | (fr < 0 ? 0u : SIFT3D_INFO_REORIENT);
        }
        reinterpret_cast<unsigned *>(out)[lane] = word;
        if (lane == 0) rec_group[r] = grp;
    }
}

/* Records per group (level id * 2 + is_max; SIFT3D_GROUPS - 1 takes anything beyond) of a sorted candidate list: what a driver
 * with several contexts needs to place every context's records in one merged list before the descriptor launches run. */
__global__ void group_count_kernel(const unsigned long long *__restrict__ keys, const int *__restrict__ nrec, long long ncand, int *__restrict__ counts)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= ncand) return;
    const int n = nrec[k];
    if (n <= 0) return;
    int g = (int)(keys[k] >> SIFT3D_KEY_LVL_SHIFT) * 2 + (int)((keys[k] >> SIFT3D_KEY_MAX_SHIFT) & 1ull);
    if (g < 0 || g >= SIFT3D_GROUPS - 1) g = SIFT3D_GROUPS - 1;
    atomicAdd(counts + g, n);
}

hipError_t sift3d_launch_group_counts(hipStream_t s, const unsigned long long *keys, const int *nrec, int64_t ncand, int *counts)
{
    if (ncand <= 0) return hipSuccess;
    hipLaunchKernelGGL(group_count_kernel, dim3((unsigned)((ncand + 255) / 256)), dim3(256), 0, s, keys, nrec, (long long)ncand, counts);
    return hipGetLastError();
}

/* Record r of candidate k: rec_kp = k (counted over the whole sorted list), rec_frame = -1 (un-reoriented) or the frame
 * index.  The per-keypoint stage runs over the list in chunks: nrec / offs belong to one chunk (offs = exclusive prefix of
 * nrec inside the chunk), its first candidate is cand_off, its first record rec_base[0]; the kernel leaves the first record
 * of the next chunk in rec_base[1]. */
__global__ void recmap_kernel(const int *__restrict__ nrec, const int *__restrict__ offs, long long ncand, int cand_off,
                              int *rec_base, int *__restrict__ rec_kp, int *__restrict__ rec_frame, unsigned long long *kp_count)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= ncand) return;
    const int n = nrec[k], o = rec_base[0] + offs[k];
    if (k == ncand - 1) rec_base[1] = o + n;
    if (n > 0) atomicAdd(kp_count, 1ull); /* keypoints that survived the bounds and eigenvalue tests (statistics) */
    for (int f = 0; f < n; f++) {
        rec_kp[o + f] = cand_off + (int)k;
        rec_frame[o + f] = f - 1;
    }
}

hipError_t sift3d_launch_recmap(hipStream_t s, const int *nrec, const int *offs, int64_t ncand, int cand_off, int *rec_base,
                                int *rec_kp, int *rec_frame, unsigned long long *kp_count)
{
    if (ncand <= 0) return hipSuccess;
    hipLaunchKernelGGL(recmap_kernel, dim3((unsigned)((ncand + 255) / 256)), dim3(256), 0, s, nrec, offs, (long long)ncand,
                       cand_off, rec_base, rec_kp, rec_frame, kp_count);
    return hipGetLastError();
}

hipError_t sift3d_launch_descriptors(hipStream_t s, const sift3d_kp_params &p, const sift3d_dkp *kps, const int *rec_kp,
                                     const int *rec_frame, int64_t nrec, sift3d_feature *recs, int *rec_group,
                                     const float *taps5)
{
    if (nrec <= 0) return hipSuccess;
    sift3d_taps t;
    for (int i = 0; i < 17; i++) t.f[i] = i < 5 ? taps5[i] : 0.0f;
    const int seg = p.desc_seg;
    const dim3 grid((unsigned)(seg > 0 ? (nrec + seg - 1) / seg * seg : ((nrec + 7) / 8) * 8));
    if (p.desc_mode == SIFT3D_DESC_SIFT)
        hipLaunchKernelGGL(descriptor_kernel<true>, grid, dim3(DESC_NT), 0, s, p, kps, rec_kp, rec_frame, (long long)nrec, recs,
                           rec_group, t);
    else
        hipLaunchKernelGGL(descriptor_kernel<false>, grid, dim3(DESC_NT), 0, s, p, kps, rec_kp, rec_frame, (long long)nrec, recs,
                           rec_group, t);
    return hipGetLastError();
}
