/*
 * match_api.hip -- C-ABI of the exact nearest-neighbour search (include/sift3d.h, "matcher").  The kernels are in
 * kernels_match.hip; the vote accumulation of the reference's matcher, which consumes these lists, is host code
 * (csrc/match_votes.c), as it is in the reference (R/feat_common/featMatchUtilities.cpp:1584-1819).
 */
#include "device_call.h"

extern "C" int sift3d_knn64(int device, const int8_t *db, int64_t n_db, const int8_t *queries, int64_t n_q, int k, int32_t *idx,
                            int32_t *dist2, int repeats, double *kernel_ms, char *err, int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (kernel_ms) *kernel_ms = 0.0;
    const int KK = sift3d_knn_list_length(k);
    int groups = 1, segments = 1, const_norm = -1;
    /* row indices are 32-bit in the kernels, and the last tile is padded to a whole one: n_db + a tile must stay below 2^31,
     * or a pad row's index wraps and no longer compares >= n_db in the merge (advisor, round 3) */
    if (!db || !queries || !idx || !dist2 || n_db <= 0 || n_q <= 0 || k < 1 || KK == 0 || n_db > (1ll << 31) - 4096 || n_q > (1ll << 31) - 4096)
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "bad arguments (1 <= k <= 32, 0 < n_db, n_q <= 2^31 - 4096)");
    if (repeats < 1) repeats = 1;
    sift3d_knn_plan(n_db, n_q, k, &groups, &segments);
    device_call dc(err, err_len);
    signed char *d_db, *d_q;
    int *d_dbn, *d_qn, *d_pd, *d_pi, *d_oi, *d_od;
    unsigned long long *d_stats, stats[6];
    const size_t parts = (size_t)n_q * 2 * segments * KK;
    DEVCHK(dc, dc.open(device));
    DEVCHK(dc, dc.upload(&d_db, db, (size_t)n_db * 64));
    DEVCHK(dc, dc.upload(&d_q, queries, (size_t)n_q * 64));
    DEVCHK(dc, dc.alloc(&d_dbn, (size_t)n_db));
    DEVCHK(dc, dc.alloc(&d_qn, (size_t)n_q));
    DEVCHK(dc, dc.alloc(&d_pd, parts));
    DEVCHK(dc, dc.alloc(&d_pi, parts));
    DEVCHK(dc, dc.alloc(&d_oi, (size_t)n_q * k));
    DEVCHK(dc, dc.alloc(&d_od, (size_t)n_q * k));
    /* The matrix cores take signed bytes: components must be 0..127 (rank descriptors are 0..63).  The norms kernel looks at
     * every byte anyway and reports the first offender -- and whether all database vectors have one squared norm: rank
     * descriptors do (every one a permutation of 0..63), and the search then needs no arithmetic on its candidates in the
     * common case (knn_search_kernel<KK, true>). */
    DEVCHK(dc, dc.alloc(&d_stats, 6));
    for (int it = 0; it < repeats; it++) { /* repeats > 1: timing (the first run is a warm-up; the last run's results are returned) */
        /* timing starts behind the warm-up run; with repeats == 1 there is none, and the one run's verdict on the bytes (a
         * device-to-host copy the host waits for) sits inside the interval: kernel_ms is then end to end, not kernel time */
        if (it == 0 || (it == 1 && repeats > 1)) DEVCHK(dc, dc.mark(0));
        stats[0] = stats[1] = stats[3] = stats[4] = ~0ull;
        stats[2] = stats[5] = 0;
        DEVCHK(dc, dc.to_device(d_stats, stats, 6));
        DEVCHK(dc, sift3d_launch_knn_norms(dc.s, d_db, n_db, d_dbn, d_stats));
        DEVCHK(dc, sift3d_launch_knn_norms(dc.s, d_q, n_q, d_qn, d_stats + 3));
        if (it == 0) { /* the verdict on the bytes: once (the timed repeats run the kernels again but do not wait for it) */
            DEVCHK(dc, dc.download(stats, d_stats, 6));
            DEVCHK(dc, dc.sync());
            if (stats[0] != ~0ull || stats[3] != ~0ull)
                return call_fail(err, err_len, SIFT3D_ERR_ARG, "%s component %llu is outside 0..127", stats[0] != ~0ull ? "database" : "query",
                                 stats[0] != ~0ull ? stats[0] : stats[3]);
            const_norm = stats[1] == stats[2] ? (int)stats[1] : -1;
        }
        DEVCHK(dc, sift3d_launch_knn(dc.s, d_db, d_dbn, n_db, d_q, d_qn, n_q, k, const_norm, groups, segments, d_pd, d_pi, d_oi, d_od));
    }
    DEVCHK(dc, dc.mark(1));
    DEVCHK(dc, dc.download(idx, d_oi, (size_t)n_q * k));
    DEVCHK(dc, dc.download(dist2, d_od, (size_t)n_q * k));
    DEVCHK(dc, dc.sync());
    DEVCHK(dc, dc.elapsed_ms(kernel_ms, repeats > 1 ? repeats - 1 : 1));
    return SIFT3D_OK;
}
