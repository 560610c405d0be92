/*
 * refine_api.hip -- C-ABI of the guided re-matching (include/sift3d.h, "guided re-matching"):
 * sift3d_guided_search and sift3d_refine_similarity.  The search kernel is in kernels_refine.hip; the spatial index, the
 * acceptance, the fits (refine_host.c) and every choice of the loop are host arithmetic in double.
 */
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "align_math.h"
#include "device_call.h"
#include "guided_accept.h"

/* What the index and the loop read of a record set, compact: one pass over the 332-byte records converts the descriptors
 * (sift3d_match_descriptors' accepted set -- whole numbers 0..127 -- without its early exit, so the inner loop vectorises; NaN
 * clamps to 0 and then differs from its conversion) and copies the positions, scales and info words.  Every later pass works
 * on these arrays. */
struct RecordSet {
    int64_t n = 0;
    std::vector<int8_t> rows;
    std::vector<int32_t> norm; /* squared length of each row */
    std::vector<float> pos;    /* x[n], y[n], z[n], scale[n] */
    std::vector<unsigned> info;

    int load(const sift3d_feature *f, int64_t count)
    {
        n = count;
        const size_t N = (size_t)std::max<int64_t>(n, 1);
        rows.resize(N * SIFT3D_DESC_LEN);
        norm.resize(N);
        pos.resize(N * 4);
        info.resize(N);
        int bad = 0;
        for (int64_t i = 0; i < n; i++) {
            const float *d = f[i].desc;
            int8_t *o = &rows[(size_t)i * SIFT3D_DESC_LEN];
            int nn = 0;
            for (int j = 0; j < SIFT3D_DESC_LEN; j++) {
                const int k = (int)fminf(fmaxf(d[j], 0.0f), 127.0f);
                bad |= d[j] != (float)k;
                o[j] = (int8_t)k;
                nn += k * k;
            }
            norm[i] = nn;
            pos[i] = f[i].x;
            pos[N + i] = f[i].y;
            pos[2 * N + i] = f[i].z;
            pos[3 * N + i] = f[i].scale;
            info[i] = f[i].info;
        }
        return bad ? -1 : 0;
    }
    size_t stride() const { return (size_t)std::max<int64_t>(n, 1); }
    float x(int64_t i) const { return pos[i]; }
    float y(int64_t i) const { return pos[stride() + i]; }
    float z(int64_t i) const { return pos[2 * stride() + i]; }
    bool finite(int64_t i) const { return std::isfinite(x(i)) && std::isfinite(y(i)) && std::isfinite(z(i)); }
};

/* the bounding box of a record set's finite records; false (and 0 .. 0) where there is none */
static bool finite_box(const RecordSet &r, double mn[3], double mx[3])
{
    bool any = false;
    for (int k = 0; k < 3; k++) mn[k] = mx[k] = 0;
    for (int64_t i = 0; i < r.n; i++) {
        if (!r.finite(i)) continue;
        const double v[3] = {r.x(i), r.y(i), r.z(i)};
        for (int k = 0; k < 3; k++) {
            if (!any || v[k] < mn[k]) mn[k] = v[k];
            if (!any || v[k] > mx[k]) mx[k] = v[k];
        }
        any = true;
    }
    return any;
}

/* A uniform grid over the finite bounding box of a record set: edge = radius (1 + 2^-10), widened to min_edge and where an
 * axis would get more than 2^20 cells (a wider cell only makes a query visit more records). */
struct Grid {
    double o[3] = {0, 0, 0}, edge = 1;
    long long n[3] = {1, 1, 1};

    void fit(const RecordSet &r, float radius, double min_edge)
    {
        double mn[3], mx[3];
        finite_box(r, mn, mx);
        edge = (double)radius * (1.0 + 1.0 / 1024.0);
        double ext = 0;
        for (int k = 0; k < 3; k++) ext = std::max(ext, mx[k] - mn[k]);
        if (!(edge > 0) || !std::isfinite(edge)) edge = 1.0;
        edge = std::max(std::max(edge, min_edge), ext / (double)(1 << 20));
        for (int k = 0; k < 3; k++) {
            o[k] = mn[k];
            n[k] = (long long)std::floor((mx[k] - mn[k]) / edge) + 1;
        }
    }
    /* the cell of a finite record */
    long long cell(const RecordSet &r, int64_t i) const
    {
        const double v[3] = {r.x(i), r.y(i), r.z(i)};
        long long c[3];
        for (int k = 0; k < 3; k++) c[k] = std::min(std::max((long long)std::floor((v[k] - o[k]) / edge), 0ll), n[k] - 1);
        return (c[2] * n[1] + c[1]) * n[0] + c[0];
    }
    long long cells() const { return n[0] * n[1] * n[2]; }
};

/* the fixed set on the device in cell order (rows in the callers' order, read through the original index), and the moving set
 * with its query order: built once per call */
struct GuidedIndex {
    device_call dc{nullptr, 0}; /* the stream, the events and the buffers, kept across the rounds of the loop; each call reports into its own err */
    Grid g;
    int dense = 1, n_f = 0, n_m = 0;
    int8_t *d_frows = nullptr, *d_mrows = nullptr;
    int *d_fnorm = nullptr, *d_fidx = nullptr, *d_cell = nullptr, *d_order = nullptr, *d_out = nullptr;
    float *d_fpos = nullptr, *d_mpos = nullptr;
    unsigned *d_finfo = nullptr, *d_minfo = nullptr;
    long long *d_keys = nullptr;

    RecordSet F, M; /* host copies in the callers' index order: the loop fits and measures residuals on them */

    int build(int device, const sift3d_feature *fixed, int64_t n_fixed, const sift3d_feature *moving, int64_t n_moving, float max_radius,
              int64_t cells_max, char *err, int64_t err_len)
    {
        dc.err = err;
        dc.err_len = err_len;
        if (!sift3d_scale_ivs().ok[0]) return call_fail(err, err_len, SIFT3D_ERR_DEVICE, "this host's logf is not monotonic near the scale threshold");
        if (F.load(fixed, n_fixed) != 0) return call_fail(err, err_len, SIFT3D_ERR_ARG, "a fixed descriptor value is outside 0..127");
        if (M.load(moving, n_moving) != 0) return call_fail(err, err_len, SIFT3D_ERR_ARG, "a moving descriptor value is outside 0..127");
        /* fixed: counting sort of the finite records by cell (dense) or a sort by cell key (sorted form); ties keep index order */
        g.fit(F, max_radius, 0);
        const long long nc = g.cells();
        dense = nc <= cells_max ? 1 : 0;
        std::vector<int32_t> perm;
        std::vector<long long> key((size_t)n_fixed);
        for (int64_t i = 0; i < n_fixed; i++) key[i] = F.finite(i) ? g.cell(F, i) : -1;
        std::vector<int32_t> start;
        if (dense) {
            start.assign((size_t)nc + 1, 0);
            for (int64_t i = 0; i < n_fixed; i++)
                if (key[i] >= 0) start[key[i] + 1]++;
            for (long long c = 0; c < nc; c++) start[c + 1] += start[c];
            perm.resize((size_t)start[nc]);
            std::vector<int32_t> fill(start.begin(), start.end() - 1);
            for (int64_t i = 0; i < n_fixed; i++)
                if (key[i] >= 0) perm[fill[key[i]]++] = (int32_t)i;
        } else {
            for (int64_t i = 0; i < n_fixed; i++)
                if (key[i] >= 0) perm.push_back((int32_t)i);
            std::stable_sort(perm.begin(), perm.end(), [&](int32_t a, int32_t b) { return key[a] < key[b]; });
        }
        n_f = (int)perm.size();
        const size_t FS = (size_t)std::max(n_f, 1), fs = F.stride();
        std::vector<int32_t> norm(FS), idx(FS);
        std::vector<float> pos(FS * 4);
        std::vector<unsigned> info(FS);
        std::vector<long long> skey(dense ? 0 : FS);
        for (int j = 0; j < n_f; j++) {
            const int64_t i = perm[j];
            norm[j] = F.norm[i];
            idx[j] = (int32_t)i;
            for (int k = 0; k < 4; k++) pos[k * FS + j] = F.pos[k * fs + i];
            info[j] = F.info[i];
            if (!dense) skey[j] = key[i];
        }
        /* moving: queries dealt in the cell order of their own position on a grid of the same edge (at most 2^22 cells) */
        n_m = (int)n_moving;
        Grid gm;
        gm.fit(M, max_radius, 0);
        while (gm.cells() > (1ll << 22)) gm.fit(M, max_radius, gm.edge * 2);
        const long long mc = gm.cells();
        std::vector<int32_t> mstart((size_t)mc + 2, 0), order((size_t)std::max(n_m, 1));
        std::vector<long long> mkey((size_t)n_m);
        for (int i = 0; i < n_m; i++) {
            mkey[i] = M.finite(i) ? gm.cell(M, i) : mc; /* non-finite last */
            mstart[mkey[i] + 1]++;
        }
        for (long long c = 0; c <= mc; c++) mstart[c + 1] += mstart[c];
        for (int i = 0; i < n_m; i++) order[mstart[mkey[i]]++] = i;
        const size_t MS = M.stride();
        DEVCHK(dc, dc.open(device));
        DEVCHK(dc, dc.upload(&d_frows, F.rows.data(), fs * 64));
        DEVCHK(dc, dc.upload(&d_fnorm, norm.data(), FS));
        DEVCHK(dc, dc.upload(&d_fidx, idx.data(), FS));
        DEVCHK(dc, dc.upload(&d_fpos, pos.data(), FS * 4));
        DEVCHK(dc, dc.upload(&d_finfo, info.data(), FS));
        DEVCHK(dc, dc.upload(&d_mrows, M.rows.data(), MS * 64));
        DEVCHK(dc, dc.upload(&d_mpos, M.pos.data(), MS * 4));
        DEVCHK(dc, dc.upload(&d_minfo, M.info.data(), MS));
        DEVCHK(dc, dc.upload(&d_order, order.data(), MS));
        DEVCHK(dc, dc.alloc(&d_out, MS * 5));
        if (dense) DEVCHK(dc, dc.upload(&d_cell, start.data(), start.size()));
        else DEVCHK(dc, dc.upload(&d_keys, skey.data(), FS));
        DEVCHK(dc, dc.sync()); /* the host vectors go out of scope */
        return SIFT3D_OK;
    }

    /* one search of every moving record under t at `radius` (at most the build radius) into host arrays */
    int search(const sift3d_similarity *t, float radius, int32_t *i1, int32_t *d1, int32_t *i2, int32_t *d2, int32_t *visited, double *kernel_ms,
               char *err, int64_t err_len)
    {
        if (n_m == 0) return SIFT3D_OK;
        dc.err = err;
        dc.err_len = err_len;
        const size_t nq = (size_t)n_m;
        int *o = d_out;
        const long long gn[3] = {g.n[0], g.n[1], g.n[2]};
        const float lo = sift3d_scale_ivs().lo[0], hi = sift3d_scale_ivs().hi[0];
        DEVCHK(dc, hipSetDevice(dc.device));
        DEVCHK(dc, dc.mark(0));
        DEVCHK(dc, sift3d_launch_guided(dc.s, d_frows, d_fnorm, d_fpos, d_finfo, d_fidx, n_f, d_cell, d_keys, g.o, g.edge, gn, dense, d_mrows, d_mpos,
                                        d_minfo, d_order, n_m, t->center0, t->center1, t->rot, t->scale, radius, lo, hi, o, o + nq, o + 2 * nq,
                                        o + 3 * nq, visited ? o + 4 * nq : nullptr));
        DEVCHK(dc, dc.mark(1));
        DEVCHK(dc, dc.download(i1, o, nq));
        DEVCHK(dc, dc.download(d1, o + nq, nq));
        DEVCHK(dc, dc.download(i2, o + 2 * nq, nq));
        DEVCHK(dc, dc.download(d2, o + 3 * nq, nq));
        if (visited) DEVCHK(dc, dc.download(visited, o + 4 * nq, nq));
        DEVCHK(dc, dc.sync());
        DEVCHK(dc, dc.elapsed_ms(kernel_ms));
        return SIFT3D_OK;
    }
};

static bool sizes_ok(int64_t n_fixed, int64_t n_moving)
{
    return n_fixed >= 0 && n_moving >= 0 && n_fixed <= (1ll << 31) - 4096 && n_moving <= (1ll << 31) - 4096;
}

extern "C" int sift3d_guided_search_params(int device, const sift3d_feature *fixed, int64_t n_fixed, const sift3d_feature *moving,
                                           int64_t n_moving, const sift3d_similarity *t, float radius, const sift3d_refine_params *p, int32_t *i1,
                                           int32_t *d1, int32_t *i2, int32_t *d2, int32_t *visited, double *kernel_ms, char *err, int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    if (kernel_ms) *kernel_ms = 0.0;
    sift3d_refine_params dp;
    sift3d_refine_defaults(&dp);
    const int64_t cells_max = p ? p->index_cells_max : dp.index_cells_max;
    if (!t || !sizes_ok(n_fixed, n_moving) || (n_fixed > 0 && !fixed) || (n_moving > 0 && (!moving || !i1 || !d1 || !i2 || !d2)) ||
        !(radius >= 0) || !std::isfinite(radius) || cells_max < 1)
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "bad arguments (0 <= n <= 2^31 - 4096, a finite radius >= 0)");
    GuidedIndex ix;
    const int rc = ix.build(device, fixed, n_fixed, moving, n_moving, radius, cells_max, err, err_len);
    return rc == SIFT3D_OK ? ix.search(t, radius, i1, d1, i2, d2, visited, kernel_ms, err, err_len) : rc;
}

extern "C" int sift3d_guided_search(int device, const sift3d_feature *fixed, int64_t n_fixed, const sift3d_feature *moving, int64_t n_moving,
                                    const sift3d_similarity *t, float radius, int32_t *i1, int32_t *d1, int32_t *i2, int32_t *d2, int32_t *visited,
                                    double *kernel_ms, char *err, int64_t err_len)
{
    return sift3d_guided_search_params(device, fixed, n_fixed, moving, n_moving, t, radius, nullptr, i1, d1, i2, d2, visited, kernel_ms, err, err_len);
}

/* ---- the loop ----------------------------------------------------------------------------------------------------- */

/* x_fixed = s rot (p - c0) + c1 in double, the sums in similarity_transform_3point's order */
static void apply_d(const sift3d_similarity *t, const double p[3], double q[3])
{
    double d[3];
    for (int k = 0; k < 3; k++) d[k] = p[k] - (double)t->center0[k];
    for (int r = 0; r < 3; r++)
        q[r] = (double)t->center1[r] + (double)t->scale * (((double)t->rot[3 * r] * d[0] + (double)t->rot[3 * r + 1] * d[1]) + (double)t->rot[3 * r + 2] * d[2]);
}

static double residual(const sift3d_similarity *t, const double p[3], float fx, float fy, float fz)
{
    double q[3];
    apply_d(t, p, q);
    const double dx = q[0] - (double)fx, dy = q[1] - (double)fy, dz = q[2] - (double)fz;
    return std::sqrt((dx * dx + dy * dy) + dz * dz);
}

static double residual(const sift3d_similarity *t, const RecordSet &M, int32_t m, const RecordSet &F, int32_t f)
{
    const double p[3] = {M.x(m), M.y(m), M.z(m)};
    return residual(t, p, F.x(f), F.y(f), F.z(f));
}

/* the fit over pairs (moving index, fixed index) */
static int fit_pairs(const RecordSet &F, const RecordSet &M, const std::vector<int32_t> &pm, const std::vector<int32_t> &pf, sift3d_similarity *t)
{
    std::vector<float> a(pm.size() * 3), b(pm.size() * 3);
    for (size_t k = 0; k < pm.size(); k++) {
        a[3 * k] = M.x(pm[k]); a[3 * k + 1] = M.y(pm[k]); a[3 * k + 2] = M.z(pm[k]);
        b[3 * k] = F.x(pf[k]); b[3 * k + 1] = F.y(pf[k]); b[3 * k + 2] = F.z(pf[k]);
    }
    return sift3d_fit_similarity(a.data(), b.data(), (int64_t)pm.size(), t);
}

extern "C" int sift3d_refine_similarity(int device, const sift3d_feature *fixed, int64_t n_fixed, const sift3d_feature *moving, int64_t n_moving,
                                        const sift3d_similarity *init, const sift3d_refine_params *pp, sift3d_similarity *out,
                                        sift3d_refine_report *rep, char *err, int64_t err_len)
{
    if (err && err_len > 0) err[0] = 0;
    sift3d_refine_params p;
    if (pp) p = *pp;
    else sift3d_refine_defaults(&p);
    if (!init || !out || !sizes_ok(n_fixed, n_moving) || (n_fixed > 0 && !fixed) || (n_moving > 0 && !moving) || p.max_rounds < 1 ||
        p.max_rounds > SIFT3D_REFINE_MAX_ROUNDS || !(p.min_radius > 0) || !(p.max_radius >= p.min_radius) || !std::isfinite(p.max_radius) ||
        p.ratio_num < 1 || p.ratio_den < 1 || !(p.stop_shift >= 0) || p.index_cells_max < 1 ||
        (init->n_matches > 0 && (init->capacity < init->n_matches || !init->moving_idx || !init->fixed_idx || !init->inlier || !init->dist2)))
        return call_fail(err, err_len, SIFT3D_ERR_ARG, "bad arguments");
    for (int32_t k = 0; k < init->n_matches; k++)
        if (init->moving_idx[k] < 0 || init->moving_idx[k] >= n_moving || init->fixed_idx[k] < 0 || init->fixed_idx[k] >= n_fixed)
            return call_fail(err, err_len, SIFT3D_ERR_ARG, "init's match arrays index outside the record sets");
    /* init's matches, read before anything of *out is written (out may share them) */
    const int32_t n0 = init->n_matches;
    std::vector<int32_t> im(init->moving_idx, init->moving_idx + n0), ifx(init->fixed_idx, init->fixed_idx + n0), iin(init->inlier, init->inlier + n0),
        idd(init->dist2, init->dist2 + n0);
    sift3d_similarity cur = *init;
    if (rep) memset(rep, 0, sizeof *rep);
    sift3d_refine_report rp;
    memset(&rp, 0, sizeof rp);
    /* round 0's radius: 3 x the RMS residual of the Hough inliers under init, clamped */
    double radius;
    {
        std::vector<double> r;
        for (int32_t k = 0; k < n0; k++)
            if (iin[k]) {
                const sift3d_feature &a = moving[im[k]], &b = fixed[ifx[k]];
                const double pt[3] = {a.x, a.y, a.z};
                r.push_back(residual(&cur, pt, b.x, b.y, b.z));
            }
        const double rms = rms_of(r);
        radius = (r.empty() || !std::isfinite(rms)) ? (double)p.max_radius : std::min(std::max(3.0 * rms, (double)p.min_radius), (double)p.max_radius);
    }
    std::vector<int32_t> keep_m, keep_f, keep_d; /* the pairs of the last round that was not refused */
    bool refined = false;
    if (n_fixed == 0 || n_moving == 0) {
        rp.stop = SIFT3D_REFINE_STOP_NONE;
    } else {
        GuidedIndex ix;
        int rc = ix.build(device, fixed, n_fixed, moving, n_moving, (float)radius, p.index_cells_max, err, err_len);
        if (rc != SIFT3D_OK) return rc;
        const RecordSet &FS = ix.F, &MS = ix.M;
        /* the moving records' finite bounding box: its eight corners measure how far a round moves the map */
        double bmn[3], bmx[3];
        const bool bany = finite_box(MS, bmn, bmx);
        const size_t M = (size_t)n_moving;
        std::vector<int32_t> i1(M), d1(M), i2(M), d2(M), vis(M), best((size_t)n_fixed);
        rp.stop = SIFT3D_REFINE_STOP_ROUNDS;
        for (int round = 0; round < p.max_rounds; round++) {
            sift3d_refine_round &R = rp.round[round];
            const float rad = (float)radius;
            R.radius = rad;
            rp.rounds = round + 1;
            rc = ix.search(&cur, rad, i1.data(), d1.data(), i2.data(), d2.data(), vis.data(), &R.kernel_ms, err, err_len);
            if (rc != SIFT3D_OK) return rc;
            for (size_t m = 0; m < M; m++) R.visited += vis[m];
            /* accept by the ratio test; one pair per fixed record: the least (d1, moving index) */
            std::vector<int32_t> pm, pf, pd;
            guided_accept(M, i1.data(), d1.data(), i2.data(), d2.data(), p.ratio_num, p.ratio_den, best, pm, pf, pd);
            R.accepted = (int32_t)pm.size();
            sift3d_similarity t1 = cur;
            if (fit_pairs(FS, MS, pm, pf, &t1) != 0) {
                rp.stop = SIFT3D_REFINE_STOP_FIT;
                break;
            }
            /* trim: residuals at most 3 x the lower median, then refit */
            std::vector<double> res(pm.size());
            for (size_t k = 0; k < pm.size(); k++) res[k] = residual(&t1, MS, pm[k], FS, pf[k]);
            std::vector<double> srt(res);
            const size_t lm = (srt.size() - 1) / 2; /* the lower median: element lm of the ascending order */
            std::nth_element(srt.begin(), srt.begin() + lm, srt.end());
            const double thr = 3.0 * srt[lm];
            std::vector<int32_t> km, kf, kd;
            for (size_t k = 0; k < pm.size(); k++)
                if (res[k] <= thr) {
                    km.push_back(pm[k]);
                    kf.push_back(pf[k]);
                    kd.push_back(pd[k]);
                }
            sift3d_similarity t2 = cur;
            if (fit_pairs(FS, MS, km, kf, &t2) != 0) {
                rp.stop = SIFT3D_REFINE_STOP_FIT;
                break;
            }
            std::vector<double> kr(km.size());
            for (size_t k = 0; k < km.size(); k++) kr[k] = residual(&t2, MS, km[k], FS, kf[k]);
            R.kept = (int32_t)km.size();
            R.rms = rms_of(kr);
            double shift = 0;
            if (bany)
                for (int c = 0; c < 8; c++) {
                    const double v[3] = {c & 1 ? bmx[0] : bmn[0], c & 2 ? bmx[1] : bmn[1], c & 4 ? bmx[2] : bmn[2]};
                    double a[3], b[3];
                    apply_d(&cur, v, a);
                    apply_d(&t2, v, b);
                    shift = std::max(shift, std::sqrt(((b[0] - a[0]) * (b[0] - a[0]) + (b[1] - a[1]) * (b[1] - a[1])) + (b[2] - a[2]) * (b[2] - a[2])));
                }
            R.shift = shift;
            cur = t2;
            refined = true;
            keep_m.swap(km);
            keep_f.swap(kf);
            keep_d.swap(kd);
            radius = std::min((double)rad, std::max((double)p.min_radius, 3.0 * R.rms));
            if (shift < (double)p.stop_shift) {
                rp.stop = SIFT3D_REFINE_STOP_CONVERGED;
                break;
            }
        }
    }
    if (rep) *rep = rp;
    /* the transform, then the pairs that made it (init's matches where no round was kept) */
    out->scale = cur.scale;
    memcpy(out->rot, cur.rot, sizeof out->rot);
    memcpy(out->trans, cur.trans, sizeof out->trans);
    memcpy(out->center0, cur.center0, sizeof out->center0);
    memcpy(out->center1, cur.center1, sizeof out->center1);
    if (!refined) {
        out->n_matches = n0;
        out->inliers = init->inliers;
        out->winner = init->winner;
        keep_m = im;
        keep_f = ifx;
        keep_d = idd;
    } else {
        out->n_matches = out->inliers = (int32_t)keep_m.size();
        out->winner = -1;
        iin.assign(keep_m.size(), 1);
    }
    return sift3d_put_pairs(out, (int32_t)keep_m.size(), keep_m.data(), keep_f.data(), iin.data(), keep_d.data(), "pairs", err, err_len);
}
