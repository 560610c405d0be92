/*
 * kernels_keypoint.hip -- phase A of the per-keypoint stage for gfx950: sub-voxel refinement, 11^3 patch sampling,
 * structure-tensor eigen test, canonical orientation frames; one workgroup of four wavefronts per extremum.  The patch and
 * every histogram live in LDS.  Phase B (patch re-sampling + 64-value descriptor + rank transform, one output record per
 * workgroup) is kernels_descriptor.hip; what the two share, and the parity contract, keypoint_device.h; the scalar
 * arithmetic, keypoint_math.h.
 */
#include <cstddef>

#include "keypoint_device.h"

/* One workgroup of KP_NT threads (4 wavefronts) per keypoint.  The LDS footprint is per
 * workgroup, so four wavefronts share what one used to hold alone: four times the wavefronts per CU for
 * the order-independent phases (gathers, gradients, pre-passes, patch blurs, peak tests), while the
 * sequential chains run on wavefront 0 and the others wait at the barrier. */
#define KP_NT 256   /* phase A: four wavefronts per keypoint */

/* The development stops (sift3d_dev_stop, sift3d_internal.h): the extremum counts as rejected */
#ifdef SIFT3D_DEV
#define KP_DEV_STOP(cond) if (cond) { if (lane == 0) nrec_out[k] = 0; return; }
#else
#define KP_DEV_STOP(cond)
#endif

/* Raster-ordered list of the in-radius voxels (ballot compaction by wavefront 0); returns the count (NRAD). */
__device__ __forceinline__ int wave_build_radius_list(unsigned short *rlist, int *n_lds)
{
    if (threadIdx.x < 64) {
        int n = 0;
        for (int base = 0; base < PV; base += 64) {
            const int s = base + threadIdx.x;
            const bool in = s < PV && in_radius(s);
            const unsigned long long m = __ballot(in);
            if (in) rlist[n + __popcll(m & ((1ull << threadIdx.x) - 1ull))] = (unsigned short)s;
            n += __popcll(m);
        }
        if (threadIdx.x == 0) *n_lds = n;
    }
    __syncthreads();
    return *n_lds;
}

/* regFindFEATUREIOPeaks without callback (R/src_common/MultiScale.cpp:1987-2121)
 * + lvSortHighLow (R/src_common/LocationValue.cpp:28-56, stable): every thread tests its voxels
 * and leaves a flag, wavefront 0 compacts the flags in raster order (ballot), then a stable
 * descending rank by counting.  Returns the count; pk_idx/pk_val hold the sorted list.
 * flags: PV bytes of scratch LDS; n_lds: one LDS int. */
template <int NT>
__device__ __forceinline__ int wave_peaks_sorted(const float *g, unsigned char *flags, int *n_lds, short *raw_idx, float *raw_val,
                                                 short *pk_idx, float *pk_val)
{
    /* One thread per interior row (y, z in 1..9) slides a 3-column window of the nine neighbouring rows along x: nine
     * LDS reads per voxel instead of twenty-seven (the kernel is bound by its LDS unit); the comparisons are the same. */
    static_assert(NT >= 81 + PD * PD, "one thread per interior row plus one per row for the border flags");
    const int t = threadIdx.x;
    if (t < 81) {
        const int y = t % 9 + 1, z = t / 9 + 1;
        const int rb = (z * PD + y) * PD; /* the row's first voxel */
        float a[9], b[9];
#pragma unroll
        for (int k = 0; k < 9; k++) {
            const int off = rb + ((k / 3 - 1) * PD + (k % 3 - 1)) * PD;
            a[k] = g[off];
            b[k] = g[off + 1];
        }
        flags[rb] = 0;
#pragma unroll
        for (int x = 1; x < PD - 1; x++) {
            float n[9];
#pragma unroll
            for (int k = 0; k < 9; k++) n[k] = g[rb + ((k / 3 - 1) * PD + (k % 3 - 1)) * PD + x + 1];
            const float c = b[4];
            bool pk = true;
#pragma unroll
            for (int k = 0; k < 9; k++) {
                pk = pk && (a[k] < c) && (n[k] < c);
                if (k != 4) pk = pk && (b[k] < c);
            }
            flags[rb + x] = pk ? 1 : 0;
#pragma unroll
            for (int k = 0; k < 9; k++) {
                a[k] = b[k];
                b[k] = n[k];
            }
        }
        flags[rb + PD - 1] = 0;
    } else if (t < 81 + PD * PD) { /* rows on a face of the patch hold no peaks */
        const int q = t - 81, y = q % PD, z = q / PD;
        if (y == 0 || y == PD - 1 || z == 0 || z == PD - 1) {
#pragma unroll
            for (int x = 0; x < PD; x++) flags[(z * PD + y) * PD + x] = 0;
        }
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        int n = 0;
        for (int base = 0; base < PV; base += 64) {
            const int s = base + threadIdx.x;
            const bool pk = s < PV && flags[s] != 0;
            const unsigned long long m = __ballot(pk);
            if (pk) {
                const int pos = n + __popcll(m & ((1ull << threadIdx.x) - 1ull));
                raw_idx[pos] = (short)s;
                raw_val[pos] = g[s];
            }
            n += __popcll(m);
        }
        if (threadIdx.x == 0) *n_lds = n;
    }
    __syncthreads();
    const int n = *n_lds;
    for (int i = threadIdx.x; i < n; i += NT) {
        const float vi = raw_val[i];
        int rank = 0;
        for (int j = 0; j < n; j++) {
            const float vj = raw_val[j];
            rank += (vj > vi || (vj == vi && j < i)) ? 1 : 0;
        }
        pk_idx[rank] = raw_idx[i];
        pk_val[rank] = vi;
    }
    __syncthreads();
    return n;
}

/* Sequential trilinear splat of the in-radius voxels into an 11^3 grid
 * (fioIncPixelTrilinearInterp, R/src_common/FeatureIO.cpp:853-889), voxels in
 * raster order.  64 lanes = 8 consecutive voxels x 8 corners: cell index and
 * contribution value*wx'*wy'*wz' are computed for eight voxels at once (order
 * independent), then the eight voxels are applied one after the other, each
 * as one 8-lane read-modify-write of eight different cells.  LDS operations
 * of a wavefront execute in issue order, so every cell sees its updates in
 * voxel order, which is the reference's.  A voxel the reference skips has
 * mag == 0 and adds +0, which leaves a cell unchanged. */
__device__ __forceinline__ void wave_splat_sequence(float *grid, int n, const short *sp_base, const v4f *sp4)
{
    const int lane = threadIdx.x;
    const int slot = lane >> 3;
    const int a = lane & 1, b = (lane >> 1) & 1, c = (lane >> 2) & 1;
    float *g = grid; /* plain LDS accesses: a volatile generic pointer would turn them into system-scope flat ops */
    if (lane < 64) { /* wavefront 0 carries the chain */
        /* parameters of the group after the current one are read while the current one is being applied */
        int packed = 0;
        float wx = 0, wy = 0, wz = 0, v = 0;
        if (slot < n) { /* (wx, wy, wz, magnitude) of a voxel in one 16-byte read */
            packed = sp_base[slot];
            const v4f q = sp4[slot];
            wx = q.x; wy = q.y; wz = q.z; v = q.w;
        }
        for (int g0 = 0; g0 < n; g0 += 8) {
            const int i = g0 + slot;
            const bool ok = i < n;
            const int ix = packed & 15, iy = (packed >> 4) & 15, iz = packed >> 8;
            const int cell = ((iz + c) * PD + (iy + b)) * PD + (ix + a);
            const float ux = a ? (1.0f - wx) : wx;
            const float uy = b ? (1.0f - wy) : wy;
            const float uz = c ? (1.0f - wz) : wz;
            const float contrib = v * ux * uy * uz;
            const int in = i + 8;
            if (in < n) {
                packed = sp_base[in];
                const v4f q = sp4[in];
                wx = q.x; wy = q.y; wz = q.z; v = q.w;
            }
            /* ds_add_f32 without return: the LDS unit performs the IEEE single-precision add (round to nearest
             * even, denormals kept: the same operation as v_add_f32, checked by sift3d_selftest_lds_add) in the
             * order the instructions were issued, and the wavefront does not wait for any of them */
#pragma unroll
            for (int j = 0; j < 8; j++) {
                if (slot == j && ok) __hip_atomic_fetch_add(&g[cell], contrib, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
    __syncthreads();
}

/* ---------------------------------------------------------------------- */
/* Phase A: extremum -> keypoint (geometry, eigen test, orientation frames) */
/* ---------------------------------------------------------------------- */
/* 23 032 bytes: seven workgroups per CU (the kernel is latency-bound; its throughput follows the number of resident
 * workgroups).  Buffers are shared between phases that never overlap:
 *   A   patch -> blurred grid                            B   splat grid t0 / middle pass of the blur
 *   A+C (contiguous) splat parameters (wx, wy, wz, magnitude) of the in-radius voxels, one 16-byte vector each
 *   C   scratch of the peak search                       r   in-radius list -> splat base cells */
struct kpA_smem {
    float A[PV + 1];
    union { /* directly behind A */
        float sp_tail[2 * NRAD_PAD]; /* the splat parameters run from A into here: live from the pre-pass to the end of the splat */
        struct {                    /* live from the peak search to the end of the frame loop body */
            unsigned char flags[PV + 13];
            short raw_idx[128], pk2_idx[128];
            float raw_val[128], pk2_val[128];
        } pk;
    } C;
    float B[PV + 1];
    float gx[NRAD_PAD], gy[NRAD_PAD], gz[NRAD_PAD]; /* gradients of the in-radius voxels */
    union {
        unsigned short rlist[NRAD_PAD]; /* until the gradients are taken */
        short sp_base[NRAD_PAD];        /* from the first splat pre-pass on */
    } r;
    short pk_idx[128];
    float pk_val[128];
    float ori_data[PD * 3 + 3];
    float sc[16];
    float taps[8];
    int cnt[4];
};
static_assert(sizeof(kpA_smem) * 7 <= 160 * 1024, "seven workgroups per CU");
static_assert(offsetof(kpA_smem, C) == sizeof(float) * (PV + 1) && sizeof(float) * (PV + 1) + sizeof(float) * 2 * NRAD_PAD >= 16 * NRAD_PAD,
              "the splat parameters span A and C");

__global__ __launch_bounds__(KP_NT, 7) void keypoint_kernel(sift3d_kp_params p, const unsigned long long *__restrict__ keys,
                                                      const sift3d_cval *__restrict__ vals, long long ncand,
                                                      sift3d_dkp *__restrict__ kps, int *__restrict__ nrec_out,
                                                      sift3d_taps taps3)
{
    __shared__ __attribute__((aligned(16))) kpA_smem sm;
    const long long k = blockIdx.x;
    if (k >= ncand) return;
    const int lane = threadIdx.x;
    if (lane < 3) sm.taps[lane] = taps3.f[lane];
    const unsigned long long key = keys[k];
    const sift3d_cval cvl = vals[k];
    const int lvl = (int)(key >> SIFT3D_KEY_LVL_SHIFT);
    const int is_max = (int)((key >> SIFT3D_KEY_MAX_SHIFT) & 1ull);
    const long long cidx = (long long)(key & SIFT3D_KEY_IDX_MASK);
    const sift3d_level lv = p.levels[lvl];
    sift3d_dkp *kp = kps + k;
    const int X = lv.X, Y = lv.Y, Z = lv.Z, XP = lv.XP;
    const long long XY = (long long)XP * Y;
    /* cidx indexes the local buffer; refinement and all geometry use the global slice number */
    const int ix = (int)(cidx % XP), iy = (int)((cidx / XP) % Y), iz = (int)(cidx / XY) + lv.z_off;

    /* generateFeatures3D_efficient, R/src_common/MultiScale.cpp:1361-1421 (every lane, identical) */
    const float *C = lv.dogc;
    const float cv = C[cidx];
    float fx = (float)interp_quadratic(ix - 1, ix, ix + 1, C[cidx - 1], cv, C[cidx + 1]);
    float fy = (float)interp_quadratic(iy - 1, iy, iy + 1, C[cidx - XP], cv, C[cidx + XP]);
    float fz = (float)interp_quadratic(iz - 1, iz, iz + 1, C[cidx - XY], cv, C[cidx + XY]);
    float scale = (float)(2 * interp_quadratic(lv.sigma_h, lv.sigma_c, lv.sigma_l, cvl.h, cv, cvl.l));
    fx += 0.5f; fy += 0.5f; fz += 0.5f;

    /* sampleImage3D bounds test, MultiScale.cpp:2630-2643 */
    const float rad = 2.0f * scale;
    const int rmax = (int)(rad + 2);
    if (fx - rmax < 0 || fy - rmax < 0 || fz - rmax < 0 || fx + rmax >= X || fy + rmax >= Y || fz + rmax >= Z) {
        if (lane == 0) nrec_out[k] = 0;
        return;
    }
    float *patch = sm.A;
    const float ident[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    wave_sample_patch<KP_NT>(patch, lv.img, X, lv.XP, Y, Z, lv.Zl, lv.z_off, fx, fy, fz, scale, ident);
    KP_DEV_STOP(p.debug_stop == SIFT3D_STOP_A_SAMPLED);
    wave_normalize_patch<KP_NT>(patch, sm.sc);
    KP_DEV_STOP(p.debug_stop == SIFT3D_STOP_A_NORMALIZED);
    const int nrad = wave_build_radius_list(sm.r.rlist, &sm.cnt[0]);

    /* determineOrientation3D, MultiScale.cpp:2541-2607: gradients (fioGenerateEdgeImages3D,
     * FeatureIO.cpp:2284-2326) are only ever used inside the radius */
    for (int i = lane; i < NRAD_PAD; i += KP_NT) {
        float a = 0, b = 0, c = 0;
        if (i < nrad) {
            const int s = sm.r.rlist[i];
            a = patch[s + 1] - patch[s - 1];
            b = patch[s + PD] - patch[s - PD];
            c = patch[s + PD * PD] - patch[s - PD * PD];
        }
        sm.gx[i] = a; sm.gy[i] = b; sm.gz[i] = c;
    }
    __syncthreads();
    if (lane < 9) {
        const float *ei = lane / 3 == 0 ? sm.gx : (lane / 3 == 1 ? sm.gy : sm.gz);
        const float *ej = lane % 3 == 0 ? sm.gx : (lane % 3 == 1 ? sm.gy : sm.gz);
        /* one sequential chain per matrix entry; the LDS reads of a block of 16 terms are issued together so
         * that their latency stays off the add chain */
        float acc = 0;
        int i = 0;
        for (; i + 16 <= nrad; i += 16) { /* 16-byte LDS reads: the kernel is bound by its LDS unit */
            v4f a[4], b[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                a[q] = *reinterpret_cast<const v4f *>(ei + i + 4 * q);
                b[q] = *reinterpret_cast<const v4f *>(ej + i + 4 * q);
            }
#pragma unroll
            for (int q = 0; q < 4; q++) {
                acc += a[q].x * b[q].x; acc += a[q].y * b[q].y; acc += a[q].z * b[q].z; acc += a[q].w * b[q].w;
            }
        }
        for (; i < nrad; i++) acc += ei[i] * ej[i];
        sm.sc[lane] = acc;
    }
    __syncthreads();
    KP_DEV_STOP(p.debug_stop == SIFT3D_STOP_A_TENSOR);
    /* The SVD + eigen test (one lane, double-precision internals) and the first orientation-histogram splat (one
     * wavefront, a chain of LDS atomics) do not depend on each other: the splat runs on wavefront 0 while lane 0 of
     * the last wavefront does the SVD.  For the ~15 % of the extrema the eigen test rejects the splat was wasted. */
    auto svd_and_eigen_test = [&]() {
        float mat[3][3], w[3], v[3][3];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                mat[i][j] = sm.sc[i * 3 + j];
                v[i][j] = 0;
            }
        w[0] = w[1] = w[2] = 0;
        svd3(mat, w, v);
        sort_eig(w, v);
        int keep = eigen_test_keep(w, p.eig_thres) ? 1 : 0;
        sm.sc[15] = keep ? 1.0f : 0.0f;
        if (keep) {
            kp->x = fx; kp->y = fy; kp->z = fz; kp->scale = scale;
            kp->eigs[0] = w[0]; kp->eigs[1] = w[1]; kp->eigs[2] = w[2];
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) kp->ori0[i * 3 + j] = v[i][j];
            kp->info = is_max ? SIFT3D_INFO_MIN0MAX1 : 0u;
            kp->lvl = lvl;
        } else {
            nrec_out[k] = 0;
        }
    };
#ifdef SIFT3D_DEV
    /* development build, SIFT3D_STOP_A_SVD_FIRST (round-4 review item 5b): the SVD and the eigen test BEFORE the first splat instead of
     * beside it -- the 16 % of the extrema the test rejects then skip the patch hand-over, the splat pre-pass and the splat;
     * the others lose the overlap of the SVD (one lane, ~0.7 us of double-precision chain) with the splat */
    const bool svd_first = p.debug_stop == SIFT3D_STOP_A_SVD_FIRST;
    if (svd_first) {
        if (lane == KP_NT - 64) svd_and_eigen_test();
        __syncthreads();
        if (sm.sc[15] == 0.0f) return;
    }
#else
    constexpr bool svd_first = false;
#endif
    /* the un-reoriented record is described from exactly this patch (identity frame, normalised once): hand it to
     * phase B instead of having it gathered from the image a second time (unused if the eigen test rejects) */
    for (int s = lane; s < PV; s += KP_NT) p.patch0[(long long)k * PV + s] = patch[s];
    __syncthreads(); /* the splat parameters below overwrite the patch */

    /* determineCanonicalOrientation3D, MultiScale.cpp:2722-3037.  The patch (A) is dead from here on. */
    float *t0 = sm.B;
    float *ta = sm.A;                        /* blur: t0 -> ta -> t0 -> ta */
    v4f *sp4 = reinterpret_cast<v4f *>(sm.A); /* live only between the pre-pass and the end of the splat */
    const float radius = (float)(PD / 2);
    for (int s = lane; s < PV; s += KP_NT) t0[s] = 0;
    for (int i = lane; i < nrad; i += KP_NT) {
        float e[3] = {sm.gx[i], sm.gy[i], sm.gz[i]};
        float m2 = e[0] * e[0] + e[1] * e[1] + e[2] * e[2];
        float mg = 0, wx = 0, wy = 0, wz = 0;
        short base = 0;
        if (m2 != 0) {
            mg = sqrtf(m2);
            float u[3];
            for (int q = 0; q < 3; q++) u[q] = e[q] * radius / mg;
            for (int q = 0; q < 3; q++) u[q] += radius;
            splat_params((float)(u[0] + 0.5), (float)(u[1] + 0.5), (float)(u[2] + 0.5), base, wx, wy, wz);
        }
        sm.r.sp_base[i] = base;
        v4f q; q.x = wx; q.y = wy; q.z = wz; q.w = mg;
        sp4[i] = q;
    }
    __syncthreads();
    if (!svd_first && lane == KP_NT - 64) svd_and_eigen_test();
    wave_splat_sequence(t0, nrad, sm.r.sp_base, sp4); /* wavefront 0; ends with a barrier */
    if (sm.sc[15] == 0.0f) return;
    KP_DEV_STOP(p.debug_stop == SIFT3D_STOP_A_SPLAT || p.debug_stop == SIFT3D_STOP_A_SPLAT_5);
    KP_DEV_STOP(p.debug_stop == SIFT3D_STOP_A_SPLAT_6); /* its own line: one test for all three gives the development build other code */
    wave_blur_patch<KP_NT>(t0, ta, t0, sm.taps, 3);
    KP_DEV_STOP(p.debug_stop == SIFT3D_STOP_A_BLURRED);
    const int npk = wave_peaks_sorted<KP_NT>(ta, sm.C.pk.flags, &sm.cnt[1], sm.C.pk.raw_idx, sm.C.pk.raw_val, sm.pk_idx, sm.pk_val);
    KP_DEV_STOP(p.debug_stop == SIFT3D_STOP_A_PEAKS);

    if (lane < npk && lane < PD && lane < 30) {
        float o[3];
        interp_point_patch(ta, sm.pk_idx[lane], o);
        o[0] -= radius; o[1] -= radius; o[2] -= radius;
        v3_norm(o);
        sm.ori_data[lane * 3 + 0] = o[0];
        sm.ori_data[lane * 3 + 1] = o[1];
        sm.ori_data[lane * 3 + 2] = o[2];
    }
    __syncthreads();

    int nret = 0;
    const float pk0 = npk > 0 ? sm.pk_val[0] : 0.0f;
    for (int i = 0; i < npk && i < PD && nret < 30; i++) {
        if ((double)sm.pk_val[i] < 0.8 * (double)pk0) break;
        const float p1[3] = {sm.ori_data[i * 3], sm.ori_data[i * 3 + 1], sm.ori_data[i * 3 + 2]};
        __syncthreads();
        for (int s = lane; s < PV; s += KP_NT) t0[s] = 0;
        for (int q = lane; q < nrad; q += KP_NT) {
            float e[3] = {sm.gx[q], sm.gy[q], sm.gz[q]};
            float mg = v3_mag(e);
            float wx = 0, wy = 0, wz = 0;
            short base = 0;
            if (mg != 0) {
                float u[3] = {e[0], e[1], e[2]};
                v3_norm(u);
                float par = v3_dot(p1, u);
                float pp[3];
                pp[0] = u[0] - par * p1[0];
                pp[1] = u[1] - par * p1[1];
                pp[2] = u[2] - par * p1[2];
                v3_norm(pp);
                for (int r = 0; r < 3; r++) {
                    pp[r] *= radius;
                    pp[r] += radius;
                }
                splat_params((float)(pp[0] + 0.5), (float)(pp[1] + 0.5), (float)(pp[2] + 0.5), base, wx, wy, wz);
            }
            sm.r.sp_base[q] = base;
            v4f pq; pq.x = wx; pq.y = wy; pq.z = wz; pq.w = mg;
            sp4[q] = pq;
        }
        __syncthreads();
        KP_DEV_STOP(p.debug_stop == SIFT3D_STOP_A2_PREPASS);
        wave_splat_sequence(t0, nrad, sm.r.sp_base, sp4);
        KP_DEV_STOP(p.debug_stop == SIFT3D_STOP_A2_SPLAT);
        wave_blur_patch<KP_NT>(t0, ta, t0, sm.taps, 3);
        KP_DEV_STOP(p.debug_stop == SIFT3D_STOP_A2_BLURRED);
        const int npk2 = wave_peaks_sorted<KP_NT>(ta, sm.C.pk.flags, &sm.cnt[2], sm.C.pk.raw_idx, sm.C.pk.raw_val, sm.C.pk.pk2_idx, sm.C.pk.pk2_val);
        KP_DEV_STOP(p.debug_stop == SIFT3D_STOP_A2_PEAKS);
        const float pk20 = npk2 > 0 ? sm.C.pk.pk2_val[0] : 0.0f;
        for (int j = 0; j < npk2 && nret < PD && nret < 30; j++) {
            if (sm.C.pk.pk2_val[j] < 0.5f * pk20) break;
            if (lane == 0) {
                float p2[3], p3[3];
                interp_point_patch(ta, sm.C.pk.pk2_idx[j], p2);
                p2[0] -= radius; p2[1] -= radius; p2[2] -= radius;
                v3_norm(p2);
                float par = v3_dot(p1, p2);
                p2[0] = p2[0] - par * p1[0];
                p2[1] = p2[1] - par * p1[1];
                p2[2] = p2[2] - par * p1[2];
                v3_norm(p2);
                p3[0] = p1[1] * p2[2] - p1[2] * p2[1];
                p3[1] = -p1[0] * p2[2] + p1[2] * p2[0];
                p3[2] = p1[0] * p2[1] - p1[1] * p2[0];
                float *m = kp->frames + 9 * nret;
                for (int iv = 0; iv < 3; iv++) {
                    m[0 * 3 + iv] = p1[iv];
                    m[1 * 3 + iv] = p2[iv];
                    m[2 * 3 + iv] = p3[iv];
                }
            }
            nret++;
        }
    }
    if (lane == 0) {
        kp->nframes = nret;
        nrec_out[k] = 1 + nret;
    }
}

hipError_t sift3d_launch_keypointsA(hipStream_t s, const sift3d_kp_params &p, const unsigned long long *keys,
                                    const sift3d_cval *vals, int64_t ncand, sift3d_dkp *kps, int *nrec, const float *taps3)
{
    if (ncand <= 0) return hipSuccess;
    sift3d_taps t;
    for (int i = 0; i < 17; i++) t.f[i] = i < 3 ? taps3[i] : 0.0f;
    hipLaunchKernelGGL(keypoint_kernel, dim3((unsigned)ncand), dim3(KP_NT), 0, s, p, keys, vals, (long long)ncand, kps, nrec, t);
    return hipGetLastError();
}
