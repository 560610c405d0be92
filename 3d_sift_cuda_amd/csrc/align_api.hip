/*
 * align_api.hip -- C-ABI of the alignment path (include/sift3d.h, "matcher, alignment path"):
 * sift3d_match_ratio, sift3d_hough_similarity and sift3d_match_keys, which restates MatchKeys
 * (R/feat_common/featMatchUtilities.cpp:1028-1250; R/ = the reference tree).  The kernels are in kernels_align.hip; the
 * sort of the matches, the bounding-box centre and the final transform are host arithmetic, as in the reference, done
 * with the same helpers (align_math.h) the kernels use.
 */
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "align_math.h"
#include "match.h"
#include "sift3d_internal.h"

hipError_t sift3d_launch_knn_norms(hipStream_t s, const signed char *v, int64_t n, int *norms, unsigned long long *stats);
hipError_t sift3d_launch_ratio(hipStream_t s, const signed char *db, const int *db_norm, int64_t n_db, const signed char *q, const int *q_norm,
                               int64_t n_q, const float *geo, const unsigned *info, float lo, float hi, int *i1, int *d1, int *i2, int *d2);
hipError_t sift3d_launch_hough(hipStream_t s, const float *p0, const float *p1, const float *s0, const float *s1, const float *o0, const float *o1,
                               int M, float lo, float hi, int one, int *counts, int *flags, float *hyp);

#define ACHK(call)                                                                                       \
    do {                                                                                                 \
        hipError_t e_ = (call);                                                                          \
        if (e_ != hipSuccess) {                                                                          \
            if (err && err_len > 0) snprintf(err, (size_t)err_len, "%s failed: %s", #call, hipGetErrorString(e_)); \
            rc = SIFT3D_ERR_DEVICE;                                                                      \
            goto done;                                                                                   \
        }                                                                                                \
    } while (0)

/* the ratio intervals of the two scale thresholds, computed once from the host's logf */
static std::once_flag g_iv_once;
static int g_iv_ok = 0;
static float g_iv_lo[2], g_iv_hi[2]; /* [0]: LOG_1_5 (ratio search), [1]: HOUGH_THRES_SCALE */

static int intervals(char *err, int64_t err_len)
{
    std::call_once(g_iv_once, [] {
        g_iv_ok = sift3d_log_ratio_interval(AM_LOG_1_5, &g_iv_lo[0], &g_iv_hi[0]) == 0 &&
                  sift3d_log_ratio_interval(AM_HOUGH_SCALE, &g_iv_lo[1], &g_iv_hi[1]) == 0;
    });
    if (!g_iv_ok && err && err_len > 0) snprintf(err, (size_t)err_len, "this host's logf is not monotonic near the scale thresholds");
    return g_iv_ok ? SIFT3D_OK : SIFT3D_ERR_DEVICE;
}

static int bad_arg(char *err, int64_t err_len, const char *what)
{
    if (err && err_len > 0) snprintf(err, (size_t)err_len, "%s", what);
    return SIFT3D_ERR_ARG;
}

/* the ratio search into host arrays (n_db >= 2, n_q >= 1) */
static int ratio_search(int device, const sift3d_feature *db, int64_t n_db, const sift3d_feature *q, int64_t n_q, int32_t *i1, int32_t *d1,
                        int32_t *i2, int32_t *d2, double *kernel_ms, char *err, int64_t err_len)
{
    int rc = intervals(err, err_len);
    if (rc != SIFT3D_OK) return rc;
    std::vector<int8_t> bdb((size_t)n_db * SIFT3D_DESC_LEN), bq((size_t)n_q * SIFT3D_DESC_LEN);
    if (sift3d_match_descriptors(db, n_db, bdb.data()) != 0) return bad_arg(err, err_len, "a database descriptor value is outside 0..127");
    if (sift3d_match_descriptors(q, n_q, bq.data()) != 0) return bad_arg(err, err_len, "a query descriptor value is outside 0..127");
    std::vector<float> geo((size_t)n_db * 13);
    std::vector<unsigned> info((size_t)n_db);
    for (int64_t j = 0; j < n_db; j++) {
        geo[j] = db[j].x;
        geo[n_db + j] = db[j].y;
        geo[2 * n_db + j] = db[j].z;
        geo[3 * n_db + j] = db[j].scale;
        for (int k = 0; k < 9; k++) geo[(4 + k) * n_db + j] = db[j].ori[k];
        info[j] = db[j].info;
    }
    signed char *d_db = nullptr, *d_q = nullptr;
    int *d_dbn = nullptr, *d_qn = nullptr, *d_out = nullptr;
    float *d_geo = nullptr;
    unsigned *d_info = nullptr;
    unsigned long long *d_stats = nullptr, stats[6];
    hipStream_t s = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ACHK(hipSetDevice(device));
    ACHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    ACHK(hipEventCreate(&e0));
    ACHK(hipEventCreate(&e1));
    ACHK(hipMalloc((void **)&d_db, (size_t)n_db * 64));
    ACHK(hipMalloc((void **)&d_q, (size_t)n_q * 64));
    ACHK(hipMalloc((void **)&d_dbn, sizeof(int) * (size_t)n_db));
    ACHK(hipMalloc((void **)&d_qn, sizeof(int) * (size_t)n_q));
    ACHK(hipMalloc((void **)&d_out, sizeof(int) * (size_t)n_q * 4));
    ACHK(hipMalloc((void **)&d_geo, sizeof(float) * geo.size()));
    ACHK(hipMalloc((void **)&d_info, sizeof(unsigned) * info.size()));
    ACHK(hipMalloc((void **)&d_stats, sizeof(stats)));
    ACHK(hipMemcpyAsync(d_db, bdb.data(), bdb.size(), hipMemcpyHostToDevice, s));
    ACHK(hipMemcpyAsync(d_q, bq.data(), bq.size(), hipMemcpyHostToDevice, s));
    ACHK(hipMemcpyAsync(d_geo, geo.data(), sizeof(float) * geo.size(), hipMemcpyHostToDevice, s));
    ACHK(hipMemcpyAsync(d_info, info.data(), sizeof(unsigned) * info.size(), hipMemcpyHostToDevice, s));
    stats[0] = stats[1] = stats[3] = stats[4] = ~0ull;
    stats[2] = stats[5] = 0;
    ACHK(hipMemcpyAsync(d_stats, stats, sizeof(stats), hipMemcpyHostToDevice, s));
    ACHK(sift3d_launch_knn_norms(s, d_db, n_db, d_dbn, d_stats));
    ACHK(sift3d_launch_knn_norms(s, d_q, n_q, d_qn, d_stats + 3));
    ACHK(hipEventRecord(e0, s));
    ACHK(sift3d_launch_ratio(s, d_db, d_dbn, n_db, d_q, d_qn, n_q, d_geo, d_info, g_iv_lo[0], g_iv_hi[0], d_out, d_out + n_q, d_out + 2 * n_q,
                             d_out + 3 * n_q));
    ACHK(hipEventRecord(e1, s));
    ACHK(hipMemcpyAsync(i1, d_out, sizeof(int) * (size_t)n_q, hipMemcpyDeviceToHost, s));
    ACHK(hipMemcpyAsync(d1, d_out + n_q, sizeof(int) * (size_t)n_q, hipMemcpyDeviceToHost, s));
    ACHK(hipMemcpyAsync(i2, d_out + 2 * n_q, sizeof(int) * (size_t)n_q, hipMemcpyDeviceToHost, s));
    ACHK(hipMemcpyAsync(d2, d_out + 3 * n_q, sizeof(int) * (size_t)n_q, hipMemcpyDeviceToHost, s));
    ACHK(hipStreamSynchronize(s));
    if (kernel_ms) {
        float ms = 0;
        ACHK(hipEventElapsedTime(&ms, e0, e1));
        *kernel_ms = ms;
    }
done:
    hipFree(d_db); hipFree(d_q); hipFree(d_dbn); hipFree(d_qn); hipFree(d_out); hipFree(d_geo); hipFree(d_info); hipFree(d_stats);
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
    if (s) hipStreamDestroy(s);
    return rc;
}

extern "C" int sift3d_match_ratio(int device, const sift3d_feature *db, int64_t n_db, const sift3d_feature *q, int64_t n_q, int32_t *i1,
                                  int32_t *d1, int32_t *i2, int32_t *d2, double *kernel_ms, char *err, int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (kernel_ms) *kernel_ms = 0.0;
    /* 32-bit row indices, the last tile padded to a whole one (as sift3d_knn64) */
    if (!db || !q || !i1 || !d1 || !i2 || !d2 || n_db < 2 || n_q < 1 || n_db > (1ll << 31) - 4096 || n_q > (1ll << 31) - 4096)
        return bad_arg(err, err_len, "bad arguments (2 <= n_db, 1 <= n_q, both at most 2^31 - 4096)");
    return ratio_search(device, db, n_db, q, n_q, i1, d1, i2, d2, kernel_ms, err, err_len);
}

/* the Hough on device copies of the match arrays; counts_h: M entries */
static int hough(int device, const float *p0, const float *p1, const float *s0, const float *s1, const float *o0, const float *o1, int M,
                 int32_t *counts_h, int32_t *winner, float *rot, float *scale, int32_t *flags, char *err, int64_t err_len)
{
    int rc = intervals(err, err_len);
    if (rc != SIFT3D_OK) return rc;
    float *d_in = nullptr, *d_hyp = nullptr;
    int *d_counts = nullptr, *d_flags = nullptr;
    hipStream_t s = nullptr;
    const float *src[6] = {p0, p1, s0, s1, o0, o1};
    const size_t width[6] = {3, 3, 1, 1, 9, 9};
    float *dev[6];
    size_t off = 0;
    float hyp[10];
    int w = -1, best = 0;
    *winner = -1;
    ACHK(hipSetDevice(device));
    ACHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    ACHK(hipMalloc((void **)&d_in, sizeof(float) * (size_t)M * 26));
    ACHK(hipMalloc((void **)&d_counts, sizeof(int) * (size_t)M));
    ACHK(hipMalloc((void **)&d_flags, sizeof(int) * (size_t)M));
    ACHK(hipMalloc((void **)&d_hyp, sizeof(float) * 10));
    for (int a = 0; a < 6; a++) {
        dev[a] = d_in + off;
        ACHK(hipMemcpyAsync(dev[a], src[a], sizeof(float) * width[a] * (size_t)M, hipMemcpyHostToDevice, s));
        off += width[a] * (size_t)M;
    }
    ACHK(sift3d_launch_hough(s, dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], M, g_iv_lo[1], g_iv_hi[1], -1, d_counts, nullptr, nullptr));
    ACHK(hipMemcpyAsync(counts_h, d_counts, sizeof(int) * (size_t)M, hipMemcpyDeviceToHost, s));
    ACHK(hipStreamSynchronize(s));
    for (int i = 0; i < M; i++) /* fInlierProb > fMaxInlierProb: the first of the most, at least one */
        if (counts_h[i] > best) {
            best = counts_h[i];
            w = i;
        }
    if (w < 0) {
        if (flags)
            for (int j = 0; j < M; j++) flags[j] = 0;
        goto done;
    }
    ACHK(sift3d_launch_hough(s, dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], M, g_iv_lo[1], g_iv_hi[1], w, d_counts, d_flags, d_hyp));
    if (flags) ACHK(hipMemcpyAsync(flags, d_flags, sizeof(int) * (size_t)M, hipMemcpyDeviceToHost, s));
    ACHK(hipMemcpyAsync(hyp, d_hyp, sizeof hyp, hipMemcpyDeviceToHost, s));
    ACHK(hipStreamSynchronize(s));
    {
        float hrot[9], hs = 0;
        if (am_hough_hypothesis(p0, p1, s0, s1, o0, o1, w, hrot, &hs) != 0 || memcmp(hrot, hyp, sizeof hrot) != 0 || memcmp(&hs, hyp + 9, sizeof hs) != 0) {
            if (err && err_len > 0) snprintf(err, (size_t)err_len, "the device's transform of hypothesis %d differs from the host's", w);
            rc = SIFT3D_ERR_DEVICE;
            goto done;
        }
        memcpy(rot, hrot, sizeof hrot);
        *scale = hs;
        *winner = w;
    }
done:
    hipFree(d_in); hipFree(d_counts); hipFree(d_flags); hipFree(d_hyp);
    if (s) hipStreamDestroy(s);
    return rc;
}

extern "C" int sift3d_hough_similarity(int device, const float *p0, const float *p1, const float *s0, const float *s1, const float *o0,
                                       const float *o1, int32_t m, int32_t *counts, int32_t *winner, float *rot, float *scale, int32_t *flags,
                                       char *err, int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (!p0 || !p1 || !s0 || !s1 || !o0 || !o1 || !winner || !rot || !scale || m < 1 || m > (1 << 24))
        return bad_arg(err, err_len, "bad arguments (1 <= m <= 2^24)");
    std::vector<int32_t> c((size_t)m);
    const int rc = hough(device, p0, p1, s0, s1, o0, o1, m, c.data(), winner, rot, scale, flags, err, err_len);
    if (rc == SIFT3D_OK && counts) memcpy(counts, c.data(), sizeof(int32_t) * (size_t)m);
    return rc;
}

static void set_identity(sift3d_similarity *out)
{
    out->scale = 1;
    for (int k = 0; k < 9; k++) out->rot[k] = k % 4 == 0 ? 1.0f : 0.0f;
    for (int k = 0; k < 3; k++) {
        out->trans[k] = 0;
        out->center1[k] = out->center0[k];
    }
    out->winner = -1;
}

extern "C" int sift3d_match_keys(int device, const sift3d_feature *fixed, int64_t n_fixed, const sift3d_feature *moving, int64_t n_moving,
                                 int32_t max_matches, sift3d_similarity *out, char *err, int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (!out || (n_fixed > 0 && !fixed) || (n_moving > 0 && !moving) || n_fixed < 0 || n_moving < 0 || max_matches < 0 ||
        n_fixed > (1ll << 31) - 4096 || n_moving > (1ll << 31) - 4096)
        return bad_arg(err, err_len, "bad arguments");
    /* getMinMaxDim over the moving records: comparisons from record 0 on (a NaN coordinate never replaces an extreme) */
    for (int k = 0; k < 3; k++) out->center0[k] = 0;
    if (n_moving > 0) {
        float mn[3] = {moving[0].x, moving[0].y, moving[0].z}, mx[3] = {moving[0].x, moving[0].y, moving[0].z};
        for (int64_t i = 0; i < n_moving; i++) {
            const float v[3] = {moving[i].x, moving[i].y, moving[i].z};
            for (int k = 0; k < 3; k++) {
                if (v[k] > mx[k]) mx[k] = v[k];
                if (v[k] < mn[k]) mn[k] = v[k];
            }
        }
        for (int k = 0; k < 3; k++) out->center0[k] = (mx[k] + mn[k]) / 2.0f;
    }
    set_identity(out);
    out->n_matches = 0;
    out->inliers = 0;
    if (n_fixed < 2 || n_moving == 0) return SIFT3D_OK;
    std::vector<int32_t> i1((size_t)n_moving), d1((size_t)n_moving), i2((size_t)n_moving), d2((size_t)n_moving);
    int rc = ratio_search(device, fixed, n_fixed, moving, n_moving, i1.data(), d1.data(), i2.data(), d2.data(), nullptr, err, err_len);
    if (rc != SIFT3D_OK) return rc;
    /* sort by ratio ascending, ties by query index, NaN (0 / 0) after every number; keep the first max_matches */
    std::vector<float> ratio((size_t)n_moving);
    std::vector<int32_t> order((size_t)n_moving);
    for (int64_t i = 0; i < n_moving; i++) {
        ratio[i] = (float)d1[i] / (float)d2[i];
        order[i] = (int32_t)i;
    }
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
        const float ra = ratio[a], rb = ratio[b];
        const bool na = std::isnan(ra), nb = std::isnan(rb);
        if (na != nb) return nb;
        if (!na && ra != rb) return ra < rb;
        return a < b;
    });
    const int M = (int)std::min<int64_t>(n_moving, max_matches);
    out->n_matches = M;
    std::vector<float> p0((size_t)M * 3), p1((size_t)M * 3), s0((size_t)M), s1((size_t)M), o0((size_t)M * 9), o1((size_t)M * 9);
    std::vector<int32_t> flags((size_t)M, 0);
    for (int k = 0; k < M; k++) {
        const sift3d_feature &a = moving[order[k]], &b = fixed[i1[order[k]]];
        p0[3 * k] = a.x; p0[3 * k + 1] = a.y; p0[3 * k + 2] = a.z;
        p1[3 * k] = b.x; p1[3 * k + 1] = b.y; p1[3 * k + 2] = b.z;
        s0[k] = a.scale;
        s1[k] = b.scale;
        memcpy(&o0[9 * (size_t)k], a.ori, sizeof a.ori);
        memcpy(&o1[9 * (size_t)k], b.ori, sizeof b.ori);
    }
    if (M <= 3) {
        out->inliers = M; /* "not enough matches to determine a solution": MatchKeys returns the match count */
    } else {
        std::vector<int32_t> counts((size_t)M);
        float rot[9], s = 1;
        int32_t w = -1;
        rc = hough(device, p0.data(), p1.data(), s0.data(), s1.data(), o0.data(), o1.data(), M, counts.data(), &w, rot, &s, flags.data(), err, err_len);
        if (rc != SIFT3D_OK) return rc;
        if (w >= 0) {
            const float zero[3] = {0, 0, 0};
            out->winner = w;
            out->inliers = counts[w];
            out->scale = s;
            memcpy(out->rot, rot, sizeof rot);
            am_sim_point(out->center0, out->center1, &p0[3 * (size_t)w], &p1[3 * (size_t)w], rot, s);
            am_sim_point(zero, out->trans, out->center0, out->center1, rot, s);
        }
    }
    if (out->capacity < M) {
        if (err && err_len > 0) snprintf(err, (size_t)err_len, "%d matches, arrays for %d", M, out->capacity);
        return out->capacity > 0 || out->moving_idx ? SIFT3D_ERR_CAPACITY : SIFT3D_OK;
    }
    for (int k = 0; k < M; k++) {
        if (out->moving_idx) out->moving_idx[k] = order[k];
        if (out->fixed_idx) out->fixed_idx[k] = i1[order[k]];
        if (out->inlier) out->inlier[k] = flags[k];
        if (out->dist2) out->dist2[k] = d1[order[k]];
    }
    return SIFT3D_OK;
}
