/*
 * kernels_align.hip -- the alignment path of the matcher for gfx950 (MI355X): the ratio search of
 * msComputeNearestNeighborDistanceRatioInfo and the one-match Hough of determine_similarity_transform_hough
 * (R/feat_common/featMatchUtilities.cpp:336-428, 816-1025; R/ = the reference tree).
 *
 * ratio_kernel.  The reference visits the database in index order and keeps, per query, a best and a second-best record
 * whose update depends on the geometry of the records seen so far: a closer record that is compatible with the current
 * best replaces it and keeps the old second distance.  The final state therefore depends on the order of the visit, and
 * the database cannot be cut into segments whose results are merged afterwards (as knn_merge_kernel does).  Each
 * workgroup owns 128 queries and walks the WHOLE database in order.  The distances come from the Gram-tile pipeline of
 * knn_search_kernel (kernels_match.hip): int8 rows staged through LDS in tiles of 256 with the XOR chunk swizzle,
 * v_mfma_i32_32x32x32_i8 with the database rows as the A operand, d = |q|^2 + |b|^2 - 2 q.b exactly in integers.  A lane
 * holds sixteen of the 32 rows of a subtile for its query; the lane 32 apart holds the other sixteen.
 *   Common path: the sixteen distances against the query's current second distance d2.  If no lane of the wavefront has
 *   one below, the subtile changes nothing (every branch of the reference needs d < d2) and the next one is looked at.
 *   Rare path: the two lanes of a query swap their distances (sixteen shuffles), so each holds all 32 in row order, and
 *   both run the reference's state machine over the rows below d2, reading the geometry of db[j] and db[i1] from global
 *   memory.  Both lanes do the same arithmetic on the same values, so they finish with the same state.
 * Rows past the end of the database get a squared norm above every real distance and never pass.  Parallelism is over
 * queries only: n_q / 128 workgroups, so small query sets leave most of the chip idle.
 *
 * hough_kernel.  One workgroup per hypothesis (match i): every lane builds the hypothesis transform (align_math.h), the
 * lanes take the matches j, and the inlier count is reduced to one integer.  With `one` >= 0 a single workgroup evaluates
 * hypothesis `one` only and writes its inlier flags and its rotation and scale, which the host compares bit for bit with
 * its own computation of the same hypothesis.
 *
 * Exactness: this file honours NaN (no -fno-honor-nans, unlike kernels_match.o) and uses only + - * /, sqrtf and a
 * double 1 / sqrt; the scale test against logf is the ratio interval [lo, hi] the host computed.
 */
#include "align_math.h"
#include "sift3d_internal.h"

typedef int a_v4i __attribute__((ext_vector_type(4)));
typedef int a_v16i __attribute__((ext_vector_type(16)));

#define AL_DIM 64
#define AL_TILE 256
#define AL_QW 32
#define AL_PAD_NORM (1 << 21) /* squared norm of the rows past the end: above every real distance (at most 64 * 127^2 < 2^20) */

/* record j of the SoA geometry: geo[k * n + j], k = x, y, z, scale, ori[0..8] */
__device__ __forceinline__ am_geo al_load_geo(const float *__restrict__ geo, const unsigned *__restrict__ info, long long n, int j)
{
    am_geo g;
    g.x = geo[j];
    g.y = geo[n + j];
    g.z = geo[2 * n + j];
    g.scale = geo[3 * n + j];
#pragma unroll
    for (int k = 0; k < 9; k++) g.ori[k] = geo[(4 + k) * n + j];
    g.info = info[j];
    return g;
}

__device__ __forceinline__ int al_dot_rows(const signed char *__restrict__ a, const signed char *__restrict__ b)
{
    int s = 0;
    for (int c = 0; c < AL_DIM; c += 16) {
        const a_v4i x = *reinterpret_cast<const a_v4i *>(a + c), y = *reinterpret_cast<const a_v4i *>(b + c);
        const int xs[4] = {x.x, x.y, x.z, x.w}, ys[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
        for (int e = 0; e < 4; e++)
#pragma unroll
            for (int k = 0; k < 4; k++) s += (int)(signed char)((xs[e] >> (8 * k)) & 0xff) * (int)(signed char)((ys[e] >> (8 * k)) & 0xff);
    }
    return s;
}

/* n_db >= 2 (the host checks).  Outputs per query: i1, d1, i2, d2. */
__global__ __launch_bounds__(256, 2) void ratio_kernel(const signed char *__restrict__ db, const int *__restrict__ db_norm, long long n_db,
                                                       const signed char *__restrict__ q, const int *__restrict__ q_norm, long long n_q,
                                                       const float *__restrict__ geo, const unsigned *__restrict__ info, float lo, float hi,
                                                       int *__restrict__ o_i1, int *__restrict__ o_d1, int *__restrict__ o_i2,
                                                       int *__restrict__ o_d2)
{
    __shared__ __attribute__((aligned(256))) signed char tile[2][AL_TILE * AL_DIM];
    __shared__ __attribute__((aligned(16))) int tnorm[2][AL_TILE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const long long qi = ((long long)blockIdx.x * 4 + wave) * AL_QW + r;
    const bool qok = qi < n_q;
    a_v4i bq[2];
#pragma unroll
    for (int s = 0; s < 2; s++) bq[s] = qok ? *reinterpret_cast<const a_v4i *>(q + qi * AL_DIM + 32 * s + 16 * h) : a_v4i(0);
    const int qn = qok ? q_norm[qi] : 0;
    /* the state starts from rows 0 and 1, swapped only if d(1) < d(0); a query past the end has d2 = -1 and never moves */
    int i1 = 0, i2 = 1, d1 = -1, d2 = -1;
    if (qok) {
        const int e0 = qn + db_norm[0] - 2 * al_dot_rows(q + qi * AL_DIM, db);
        const int e1 = qn + db_norm[1] - 2 * al_dot_rows(q + qi * AL_DIM, db + AL_DIM);
        d1 = e0;
        d2 = e1;
        if (e1 < e0) {
            d1 = e1;
            d2 = e0;
            i1 = 1;
            i2 = 0;
        }
    }
    const long long ntiles = (n_db + AL_TILE - 1) / AL_TILE;
    const int sc = tid & 3, srow = tid >> 2;
    a_v4i st[4];
    int stn = 0;
    auto fetch = [&](long long t) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const long long v = t * AL_TILE + srow + 64 * j;
            st[j] = v < n_db ? *reinterpret_cast<const a_v4i *>(db + v * AL_DIM + 16 * sc) : a_v4i(0);
        }
        const long long v = t * AL_TILE + tid;
        stn = v < n_db ? db_norm[v] : AL_PAD_NORM;
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int row = srow + 64 * j;
            *reinterpret_cast<a_v4i *>(&tile[buf][row * AL_DIM + 16 * (sc ^ ((row >> 2) & 3))]) = st[j];
        }
        tnorm[buf][tid] = stn;
    };
    const int sw = (r >> 2) & 3;
    const int a_off0 = r * AL_DIM + 16 * (h ^ sw), a_off1 = r * AL_DIM + 16 * ((2 + h) ^ sw);
    auto compat = [&](int j, int k) __attribute__((always_inline)) -> int {
        const am_geo a = al_load_geo(geo, info, n_db, j), b = al_load_geo(geo, info, n_db, k);
        return am_compatible(&a, &b, lo, hi, 0.5f, -1.0f);
    };
    /* accumulator register e holds row (e & 3) + 8 (e >> 2) + 4 h of the subtile */
    auto take = [&](const a_v16i &acc, int buf, int sub, long long t) __attribute__((always_inline)) {
        int dv[16], m = 0x7fffffff;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const a_v4i nn = *reinterpret_cast<const a_v4i *>(&tnorm[buf][sub * 32 + 8 * u + 4 * h]);
            const int nv[4] = {nn.x, nn.y, nn.z, nn.w};
#pragma unroll
            for (int e = 0; e < 4; e++) {
                dv[4 * u + e] = qn + nv[e] - 2 * acc[4 * u + e];
                m = min(m, dv[4 * u + e]);
            }
        }
        if (__builtin_expect(__ballot(m < d2) != 0, 0)) {
            int pd[16];
#pragma unroll
            for (int e = 0; e < 16; e++) pd[e] = __shfl_xor(dv[e], 32);
            const long long base = t * AL_TILE + sub * 32;
#pragma unroll
            for (int rr = 0; rr < 32; rr++) {
                const int e = (rr & 3) + 4 * (rr >> 3);
                const int d = ((rr >> 2) & 1) == h ? dv[e] : pd[e];
                const long long row = base + rr;
                if (d < d2 && row >= 2 && row < n_db) {
                    const int c = compat((int)row, i1);
                    am_ratio_step((int)row, d, c, &i1, &d1, &i2, &d2);
                }
            }
        }
    };
    auto gram = [&](const a_v4i &a0, const a_v4i &a1) __attribute__((always_inline)) -> a_v16i {
        a_v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, bq[0], acc, 0, 0, 0);
        return __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, bq[1], acc, 0, 0, 0);
    };
    fetch(0);
    stash(0);
    __syncthreads();
    for (long long t = 0; t < ntiles; t++) {
        const int buf = (int)(t & 1);
        if (t + 1 < ntiles) fetch(t + 1);
        const signed char *tb = &tile[buf][0];
        const signed char *p0 = tb + a_off0, *p1 = tb + a_off1;
        a_v16i acc_a, acc_b;
        acc_a = gram(*reinterpret_cast<const a_v4i *>(p0), *reinterpret_cast<const a_v4i *>(p1));
#pragma unroll 1
        for (int sub = 0; sub < AL_TILE / 32; sub += 2) {
            acc_b = gram(*reinterpret_cast<const a_v4i *>(p0 + 32 * AL_DIM), *reinterpret_cast<const a_v4i *>(p1 + 32 * AL_DIM));
            take(acc_a, buf, sub, t);
            if (sub + 2 < AL_TILE / 32) acc_a = gram(*reinterpret_cast<const a_v4i *>(p0 + 64 * AL_DIM), *reinterpret_cast<const a_v4i *>(p1 + 64 * AL_DIM));
            take(acc_b, buf, sub + 1, t);
            p0 += 64 * AL_DIM;
            p1 += 64 * AL_DIM;
        }
        if (t + 1 < ntiles) stash(buf ^ 1);
        __syncthreads();
    }
    if (qok && h == 0) {
        o_i1[qi] = i1;
        o_d1[qi] = d1;
        o_i2[qi] = i2;
        o_d2[qi] = d2;
    }
}

/* p0 / s0 / o0: moving side of the M matches (3, 1, 9 floats each); p1 / s1 / o1 fixed side.  one < 0: grid of M
 * workgroups, counts[i] = inliers of hypothesis i (-1: degenerate).  one >= 0: one workgroup, flags[j] for hypothesis one,
 * counts[one], and hyp[0..9] = its rotation and scale. */
__global__ __launch_bounds__(256) void hough_kernel(const float *__restrict__ p0, const float *__restrict__ p1, const float *__restrict__ s0,
                                                    const float *__restrict__ s1, const float *__restrict__ o0, const float *__restrict__ o1, int M,
                                                    float lo, float hi, int one, int *__restrict__ counts, int *__restrict__ flags,
                                                    float *__restrict__ hyp)
{
    __shared__ int part[4];
    const int i = one >= 0 ? one : (int)blockIdx.x;
    const int tid = threadIdx.x;
    float rot[9], s = 0;
    if (am_hough_hypothesis(p0, p1, s0, s1, o0, o1, i, rot, &s) != 0) { /* the same for every lane: the whole workgroup leaves */
        if (tid == 0) counts[i] = -1;
        if (one >= 0)
            for (int j = tid; j < M; j += blockDim.x) flags[j] = 0;
        return;
    }
    int c = 0;
    for (int j = tid; j < M; j += blockDim.x) {
        const int in = am_hough_inlier(p0, p1, s0, s1, o0, o1, i, j, rot, s, lo, hi);
        if (one >= 0) flags[j] = in;
        c += in;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
    if ((tid & 63) == 0) part[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        counts[i] = part[0] + part[1] + part[2] + part[3];
        if (one >= 0) {
#pragma unroll
            for (int k = 0; k < 9; k++) hyp[k] = rot[k];
            hyp[9] = s;
        }
    }
}

hipError_t sift3d_launch_ratio(hipStream_t s, const signed char *db, const int *db_norm, int64_t n_db, const signed char *q, const int *q_norm,
                               int64_t n_q, const float *geo, const unsigned *info, float lo, float hi, int *i1, int *d1, int *i2, int *d2)
{
    if (n_q <= 0) return hipSuccess;
    if (n_db < 2) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ratio_kernel, dim3((unsigned)((n_q + 127) / 128)), dim3(256), 0, s, db, db_norm, (long long)n_db, q, q_norm, (long long)n_q,
                       geo, info, lo, hi, i1, d1, i2, d2);
    return hipGetLastError();
}

hipError_t sift3d_launch_hough(hipStream_t s, const float *p0, const float *p1, const float *s0, const float *s1, const float *o0, const float *o1,
                               int M, float lo, float hi, int one, int *counts, int *flags, float *hyp)
{
    if (M <= 0) return hipSuccess;
    if (one >= M) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hough_kernel, dim3(one >= 0 ? 1u : (unsigned)M), dim3(256), 0, s, p0, p1, s0, s1, o0, o1, M, lo, hi, one, counts, flags, hyp);
    return hipGetLastError();
}
