/*
 * align_api.hip -- C-ABI of the alignment path (include/sift3d.h, "matcher, alignment path"):
 * sift3d_match_ratio, sift3d_hough_similarity and sift3d_match_keys, which restates MatchKeys
 * (R/feat_common/featMatchUtilities.cpp:1028-1250; R/ = the reference tree).  The kernels are in kernels_align.hip; the
 * sort of the matches, the bounding-box centre and the final transform are host arithmetic, as in the reference, done
 * with the same helpers (align_math.h) the kernels use.
 */
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "align_math.h"
#include "device_call.h"
#include "match.h"

static std::once_flag g_iv_once;
static sift3d_scale_intervals g_iv;

const sift3d_scale_intervals &sift3d_scale_ivs()
{
    std::call_once(g_iv_once, [] {
        g_iv.ok[0] = sift3d_log_ratio_interval(AM_LOG_1_5, &g_iv.lo[0], &g_iv.hi[0]) == 0;
        g_iv.ok[1] = sift3d_log_ratio_interval(AM_HOUGH_SCALE, &g_iv.lo[1], &g_iv.hi[1]) == 0;
    });
    return g_iv;
}

int sift3d_put_pairs(sift3d_similarity *out, int32_t n, const int32_t *moving, const int32_t *fixed, const int32_t *inlier, const int32_t *dist2,
                     const char *what, char *err, int64_t err_len)
{
    if (out->capacity < n)
        return call_fail(err, err_len, out->capacity > 0 || out->moving_idx ? SIFT3D_ERR_CAPACITY : SIFT3D_OK, "%d %s, arrays for %d", n, what,
                         out->capacity);
    for (int32_t k = 0; k < n; k++) {
        if (out->moving_idx) out->moving_idx[k] = moving[k];
        if (out->fixed_idx) out->fixed_idx[k] = fixed[k];
        if (out->inlier) out->inlier[k] = inlier[k];
        if (out->dist2) out->dist2[k] = dist2[k];
    }
    return SIFT3D_OK;
}

/* both scale intervals, or SIFT3D_ERR_DEVICE */
static int intervals(char *err, int64_t err_len)
{
    const sift3d_scale_intervals &iv = sift3d_scale_ivs();
    if (iv.ok[0] && iv.ok[1]) return SIFT3D_OK;
    return call_fail(err, err_len, SIFT3D_ERR_DEVICE, "this host's logf is not monotonic near the scale thresholds");
}

/* the ratio search into host arrays (n_db >= 2, n_q >= 1) */
static int ratio_search(int device, const sift3d_feature *db, int64_t n_db, const sift3d_feature *q, int64_t n_q, int32_t *i1, int32_t *d1,
                        int32_t *i2, int32_t *d2, double *kernel_ms, char *err, int64_t err_len)
{
    int rc = intervals(err, err_len);
    if (rc != SIFT3D_OK) return rc;
    std::vector<int8_t> bdb((size_t)n_db * SIFT3D_DESC_LEN), bq((size_t)n_q * SIFT3D_DESC_LEN);
    if (sift3d_match_descriptors(db, n_db, bdb.data()) != 0) return call_fail(err, err_len, SIFT3D_ERR_ARG, "a database descriptor value is outside 0..127");
    if (sift3d_match_descriptors(q, n_q, bq.data()) != 0) return call_fail(err, err_len, SIFT3D_ERR_ARG, "a query descriptor value is outside 0..127");
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
    device_call dc(err, err_len);
    signed char *d_db, *d_q;
    int *d_dbn, *d_qn, *d_out;
    float *d_geo;
    unsigned *d_info;
    unsigned long long *d_stats, stats[6];
    DEVCHK(dc, dc.open(device));
    DEVCHK(dc, dc.upload(&d_db, bdb.data(), bdb.size()));
    DEVCHK(dc, dc.upload(&d_q, bq.data(), bq.size()));
    DEVCHK(dc, dc.alloc(&d_dbn, (size_t)n_db));
    DEVCHK(dc, dc.alloc(&d_qn, (size_t)n_q));
    DEVCHK(dc, dc.alloc(&d_out, (size_t)n_q * 4));
    DEVCHK(dc, dc.upload(&d_geo, geo.data(), geo.size()));
    DEVCHK(dc, dc.upload(&d_info, info.data(), info.size()));
    /* the norms kernel writes its verdict on the bytes into stats; nothing reads it here (sift3d_match_descriptors checked them) */
    stats[0] = stats[1] = stats[3] = stats[4] = ~0ull;
    stats[2] = stats[5] = 0;
    DEVCHK(dc, dc.upload(&d_stats, stats, 6));
    DEVCHK(dc, sift3d_launch_knn_norms(dc.s, d_db, n_db, d_dbn, d_stats));
    DEVCHK(dc, sift3d_launch_knn_norms(dc.s, d_q, n_q, d_qn, d_stats + 3));
    DEVCHK(dc, dc.mark(0));
    const sift3d_scale_intervals &iv = sift3d_scale_ivs();
    DEVCHK(dc, sift3d_launch_ratio(dc.s, d_db, d_dbn, n_db, d_q, d_qn, n_q, d_geo, d_info, iv.lo[0], iv.hi[0], d_out, d_out + n_q, d_out + 2 * n_q,
                                   d_out + 3 * n_q));
    DEVCHK(dc, dc.mark(1));
    DEVCHK(dc, dc.download(i1, d_out, (size_t)n_q));
    DEVCHK(dc, dc.download(d1, d_out + n_q, (size_t)n_q));
    DEVCHK(dc, dc.download(i2, d_out + 2 * n_q, (size_t)n_q));
    DEVCHK(dc, dc.download(d2, d_out + 3 * n_q, (size_t)n_q));
    DEVCHK(dc, dc.sync());
    DEVCHK(dc, dc.elapsed_ms(kernel_ms));
    return SIFT3D_OK;
}

extern "C" int sift3d_match_ratio(int device, const sift3d_feature *db, int64_t n_db, const sift3d_feature *q, int64_t n_q, int32_t *i1,
                                  int32_t *d1, int32_t *i2, int32_t *d2, double *kernel_ms, char *err, int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (kernel_ms) *kernel_ms = 0.0;
    /* 32-bit row indices, the last tile padded to a whole one (as sift3d_knn64) */
    if (!db || !q || !i1 || !d1 || !i2 || !d2 || n_db < 2 || n_q < 1 || n_db > (1ll << 31) - 4096 || n_q > (1ll << 31) - 4096)
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "bad arguments (2 <= n_db, 1 <= n_q, both at most 2^31 - 4096)");
    return ratio_search(device, db, n_db, q, n_q, i1, d1, i2, d2, kernel_ms, err, err_len);
}

/* the Hough on device copies of the match arrays; counts_h: M entries */
static int hough(int device, const float *p0, const float *p1, const float *s0, const float *s1, const float *o0, const float *o1, int M,
                 int32_t *counts_h, int32_t *winner, float *rot, float *scale, int32_t *flags, char *err, int64_t err_len)
{
    int rc = intervals(err, err_len);
    if (rc != SIFT3D_OK) return rc;
    const float lo = sift3d_scale_ivs().lo[1], hi = sift3d_scale_ivs().hi[1];
    const float *src[6] = {p0, p1, s0, s1, o0, o1};
    const size_t width[6] = {3, 3, 1, 1, 9, 9};
    device_call dc(err, err_len);
    float *d_in, *d_hyp, *dev[6], hyp[10];
    int *d_counts, *d_flags;
    size_t off = 0;
    int w = -1, best = 0;
    *winner = -1;
    DEVCHK(dc, dc.open(device, false));
    DEVCHK(dc, dc.alloc(&d_in, (size_t)M * 26));
    DEVCHK(dc, dc.alloc(&d_counts, (size_t)M));
    DEVCHK(dc, dc.alloc(&d_flags, (size_t)M));
    DEVCHK(dc, dc.alloc(&d_hyp, 10));
    for (int a = 0; a < 6; a++) {
        dev[a] = d_in + off;
        DEVCHK(dc, dc.to_device(dev[a], src[a], width[a] * (size_t)M));
        off += width[a] * (size_t)M;
    }
    DEVCHK(dc, sift3d_launch_hough(dc.s, dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], M, lo, hi, -1, d_counts, nullptr, nullptr));
    DEVCHK(dc, dc.download(counts_h, d_counts, (size_t)M));
    DEVCHK(dc, dc.sync());
    for (int i = 0; i < M; i++) /* fInlierProb > fMaxInlierProb: the first of the most, at least one */
        if (counts_h[i] > best) {
            best = counts_h[i];
            w = i;
        }
    if (w < 0) {
        if (flags)
            for (int j = 0; j < M; j++) flags[j] = 0;
        return SIFT3D_OK;
    }
    DEVCHK(dc, sift3d_launch_hough(dc.s, dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], M, lo, hi, w, d_counts, d_flags, d_hyp));
    if (flags) DEVCHK(dc, dc.download(flags, d_flags, (size_t)M));
    DEVCHK(dc, dc.download(hyp, d_hyp, 10));
    DEVCHK(dc, dc.sync());
    float hrot[9], hs = 0;
    if (am_hough_hypothesis(p0, p1, s0, s1, o0, o1, w, hrot, &hs) != 0 || memcmp(hrot, hyp, sizeof hrot) != 0 || memcmp(&hs, hyp + 9, sizeof hs) != 0)
        return call_fail(err, err_len, SIFT3D_ERR_DEVICE, "the device's transform of hypothesis %d differs from the host's", w);
    memcpy(rot, hrot, sizeof hrot);
    *scale = hs;
    *winner = w;
    return SIFT3D_OK;
}

extern "C" int sift3d_hough_similarity(int device, const float *p0, const float *p1, const float *s0, const float *s1, const float *o0,
                                       const float *o1, int32_t m, int32_t *counts, int32_t *winner, float *rot, float *scale, int32_t *flags,
                                       char *err, int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (!p0 || !p1 || !s0 || !s1 || !o0 || !o1 || !winner || !rot || !scale || m < 1 || m > (1 << 24))
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "bad arguments (1 <= m <= 2^24)");
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
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "bad arguments");
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
    std::vector<int32_t> flags((size_t)M, 0), fixed_idx((size_t)M), dist2((size_t)M);
    for (int k = 0; k < M; k++) {
        fixed_idx[k] = i1[order[k]];
        dist2[k] = d1[order[k]];
        const sift3d_feature &a = moving[order[k]], &b = fixed[fixed_idx[k]];
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
    return sift3d_put_pairs(out, M, order.data(), fixed_idx.data(), flags.data(), dist2.data(), "matches", err, err_len);
}
