/*
 * register_oracle.c -- CPU restatement of the affine registration by mutual information of DESIGN.md section 7q (test
 * infrastructure; written from that text, it includes none of the product's headers).  Built with cc -O2 -ffp-contract=off by
 * tests/register_cases.py.  The quantiser, the range and the derived values are tests/similarity_oracle.c's, compiled beside it
 * unchanged.
 *
 * oreg_warp_hist: every lattice voxel in index order, every map, serially: q by section 7c's order, the linear sample with all
 *   eight corners and NaN outside, both quantised, counted when both are >= 0.
 * oreg_map, oreg_result, oreg_candidates, oreg_lattice: section 7q's double sequence, the same libm calls in the same order.
 * oreg_register: the compass search over oreg_warp_hist, one map at a time.
 */
#include "similarity_oracle.c"

static float lerp(float a, float b, float w) { return (1.0f - w) * a + w * b; }

/* the sample of M at the image of the fixed voxel (i, j, k); *out_of_bounds where q fails 0 <= q <= n - 1 */
static float warped(const float *M, int64_t mx, int64_t my, int64_t mz, const float *A, int64_t i, int64_t j, int64_t k, int *out_of_bounds)
{
    const float p[3] = {(float)i, (float)j, (float)k};
    const int64_t n[3] = {mx, my, mz};
    float q[3];
    for (int r = 0; r < 3; r++) {
        float s = A[4 * r] * p[0];
        s = s + A[4 * r + 1] * p[1];
        s = s + A[4 * r + 2] * p[2];
        q[r] = s + A[4 * r + 3];
    }
    *out_of_bounds = 0;
    for (int r = 0; r < 3; r++)
        if (!(q[r] >= 0.0f) || !(q[r] <= (float)(n[r] - 1))) *out_of_bounds = 1;
    if (*out_of_bounds) return NAN;
    int64_t lo[3], hi[3];
    float w[3];
    for (int r = 0; r < 3; r++) {
        const float f = floorf(q[r]);
        w[r] = q[r] - f;
        lo[r] = (int64_t)f;
        hi[r] = lo[r] + 1 <= n[r] - 1 ? lo[r] + 1 : n[r] - 1;
    }
#define AT(x, y, z) M[((z) * my + (y)) * mx + (x)]
    const float e00 = lerp(AT(lo[0], lo[1], lo[2]), AT(hi[0], lo[1], lo[2]), w[0]);
    const float e10 = lerp(AT(lo[0], hi[1], lo[2]), AT(hi[0], hi[1], lo[2]), w[0]);
    const float e01 = lerp(AT(lo[0], lo[1], hi[2]), AT(hi[0], lo[1], hi[2]), w[0]);
    const float e11 = lerp(AT(lo[0], hi[1], hi[2]), AT(hi[0], hi[1], hi[2]), w[0]);
#undef AT
    return lerp(lerp(e00, e10, w[1]), lerp(e01, e11, w[1]), w[2]);
}

/* hist K bins^2, sums K 6, excluded K, outside K; returns N */
int64_t oreg_warp_hist(const float *F, int64_t nx, int64_t ny, int64_t nz, const float *M, int64_t mx, int64_t my, int64_t mz, const float *maps, int K,
                       int stride, float flo, float fhi, float mlo, float mhi, int bins, int64_t *hist, int64_t *sums, int64_t *excluded, int64_t *outside)
{
    int s = 10;
    for (int b = bins; b > 1; b >>= 1) s--;
    memset(hist, 0, sizeof(int64_t) * (size_t)(K * bins * bins));
    memset(sums, 0, sizeof(int64_t) * 6 * (size_t)K);
    int64_t N = 0;
    for (int m = 0; m < K; m++) {
        excluded[m] = outside[m] = 0;
        N = 0;
        for (int64_t k = 0; k < nz; k += stride)
            for (int64_t j = 0; j < ny; j += stride)
                for (int64_t i = 0; i < nx; i += stride) {
                    int oob;
                    const float v = warped(M, mx, my, mz, maps + 12 * m, i, j, k, &oob);
                    const int64_t qa = osim_q(F[(k * ny + j) * nx + i], flo, fhi), qb = osim_q(v, mlo, mhi);
                    N++;
                    outside[m] += oob;
                    if (qa < 0 || qb < 0) {
                        excluded[m]++;
                        continue;
                    }
                    const int64_t term[6] = {1, qa, qb, qa * qa, qb * qb, qa * qb};
                    hist[(int64_t)m * bins * bins + (qa >> s) * bins + (qb >> s)]++;
                    for (int t = 0; t < 6; t++) sums[6 * m + t] += term[t];
                }
    }
    return N;
}

/* ---- theta -> matrices ---- */
static int inverse(const double a[16], double o[16])
{
    if (a[12] != 0.0 || a[13] != 0.0 || a[14] != 0.0 || a[15] != 1.0) return -1;
    const double c00 = a[5] * a[10] - a[6] * a[9], c01 = a[6] * a[8] - a[4] * a[10], c02 = a[4] * a[9] - a[5] * a[8];
    const double det = a[0] * c00 + a[1] * c01 + a[2] * c02;
    if (!(det != 0.0) || !isfinite(det)) return -1;
    const double inv[9] = {c00, a[2] * a[9] - a[1] * a[10], a[1] * a[6] - a[2] * a[5],
                           c01, a[0] * a[10] - a[2] * a[8], a[2] * a[4] - a[0] * a[6],
                           c02, a[1] * a[8] - a[0] * a[9], a[0] * a[5] - a[1] * a[4]};
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) o[4 * r + c] = inv[3 * r + c] / det;
        o[4 * r + 3] = -(o[4 * r] * a[3] + o[4 * r + 1] * a[7] + o[4 * r + 2] * a[11]);
        for (int c = 0; c < 4; c++)
            if (!isfinite(o[4 * r + c])) return -1;
    }
    o[12] = o[13] = o[14] = 0.0;
    o[15] = 1.0;
    return 0;
}

static void mul4(const double a[16], const double b[16], double o[16])
{
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) o[4 * r + c] = a[4 * r] * b[c] + a[4 * r + 1] * b[4 + c] + a[4 * r + 2] * b[8 + c] + a[4 * r + 3] * b[12 + c];
}

static void mul3(const double a[9], const double b[9], double o[9])
{
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) o[3 * r + c] = (a[3 * r] * b[c] + a[3 * r + 1] * b[3 + c]) + a[3 * r + 2] * b[6 + c];
}

static void widen(const float *m, double o[16])
{
    for (int k = 0; k < 16; k++) o[k] = m ? (double)m[k] : (k % 5 == 0 ? 1.0 : 0.0);
}

static void d_of_theta(const double *th, int64_t nx, int64_t ny, int64_t nz, const double fv[16], double d[16])
{
    const double ctr[3] = {(double)(nx - 1) / 2.0, (double)(ny - 1) / 2.0, (double)(nz - 1) / 2.0};
    double c[3], R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, RG[9];
    for (int i = 0; i < 3; i++) c[i] = ((fv[4 * i] * ctr[0] + fv[4 * i + 1] * ctr[1]) + fv[4 * i + 2] * ctr[2]) + fv[4 * i + 3];
    const double rx = th[3], ry = th[4], rz = th[5];
    const double a = sqrt((rx * rx + ry * ry) + rz * rz);
    if (a > 0.0) {
        const double K[9] = {0.0, -rz, ry, rz, 0.0, -rx, -ry, rx, 0.0};
        double KK[9];
        mul3(K, K, KK);
        const double A = sin(a) / a, B = (1.0 - cos(a)) / (a * a);
        for (int k = 0; k < 9; k++) R[k] = (R[k] + A * K[k]) + B * KK[k];
    }
    const double G[9] = {1.0, th[9], th[10], 0.0, 1.0, th[11], 0.0, 0.0, 1.0};
    const double e[3] = {exp(th[6]), exp(th[7]), exp(th[8])};
    mul3(R, G, RG);
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) d[4 * i + j] = RG[3 * i + j] * e[j];
        d[4 * i + 3] = (c[i] - ((d[4 * i] * c[0] + d[4 * i + 1] * c[1]) + d[4 * i + 2] * c[2])) + th[i];
    }
    d[12] = d[13] = d[14] = 0.0;
    d[15] = 1.0;
}

int oreg_map(const double *th, int64_t nx, int64_t ny, int64_t nz, const float *fixed_vox2key, const float *moving_vox2key, const float *initial, float *map)
{
    double t[16], fv[16], mv[16], ti[16], mvi[16], fvi[16], d[16], e[16], p[16], a[16];
    widen(initial, t);
    widen(fixed_vox2key, fv);
    widen(moving_vox2key, mv);
    if (inverse(t, ti) != 0 || inverse(mv, mvi) != 0 || inverse(fv, fvi) != 0) return -1;
    d_of_theta(th, nx, ny, nz, fv, d);
    mul4(d, fv, e);
    mul4(ti, e, p);
    mul4(mvi, p, a);
    for (int k = 0; k < 12; k++) {
        if (!isfinite(a[k])) return -1;
        map[k] = (float)a[k];
    }
    return 0;
}

int oreg_result(const double *th, int64_t nx, int64_t ny, int64_t nz, const float *fixed_vox2key, const float *initial, float *result)
{
    double t[16], fv[16], d[16], di[16], m[16];
    widen(initial, t);
    widen(fixed_vox2key, fv);
    if (t[12] != 0.0 || t[13] != 0.0 || t[14] != 0.0 || t[15] != 1.0) return -1;
    d_of_theta(th, nx, ny, nz, fv, d);
    if (inverse(d, di) != 0) return -1;
    mul4(di, t, m);
    for (int k = 0; k < 12; k++)
        if (!isfinite(m[k])) return -1;
    for (int k = 0; k < 16; k++) result[k] = (float)m[k];
    return 0;
}

/* the active parameters of a dof in order; under 7 the index 6 is the shared scale */
static int active(int dof)
{
    return dof == 3 || dof == 6 || dof == 7 || dof == 9 || dof == 12 ? dof : 0;
}

int oreg_candidates(const double *th, int dof, double u, double rho, double *cand)
{
    const int n = active(dof);
    if (!n) return -1;
    for (int k = 0; k < n; k++)
        for (int sign = 0; sign < 2; sign++) {
            double *c = cand + 12 * (2 * k + sign);
            memcpy(c, th, sizeof(double) * 12);
            const double step = k < 3 ? u : u / rho;
            c[k] = sign ? th[k] - step : th[k] + step;
            if (dof == 7 && k == 6) c[7] = c[8] = c[6];
        }
    return 2 * n;
}

int64_t oreg_lattice(int64_t nx, int64_t ny, int64_t nz, int stride, const float *fixed_vox2key, int64_t *n, double *h, double *rho)
{
    const int64_t ext[3] = {nx, ny, nz};
    double fv[16], least = 0.0, edge = 0.0;
    int64_t N = 1;
    widen(fixed_vox2key, fv);
    for (int a = 0; a < 3; a++) {
        n[a] = (ext[a] - 1) / stride + 1;
        N *= n[a];
        const double col = sqrt((fv[a] * fv[a] + fv[4 + a] * fv[4 + a]) + fv[8 + a] * fv[8 + a]);
        if (a == 0 || col < least) least = col;
        if ((double)(ext[a] - 1) * col > edge) edge = (double)(ext[a] - 1) * col;
    }
    *h = least;
    *rho = edge > 0.0 ? edge / 2.0 : least / 2.0;
    return N;
}

/* ---- the search ---- */
typedef struct {
    const float *F, *M, *fv, *mv, *m0;
    int64_t nx, ny, nz, mx, my, mz;
    float flo, fhi, mlo, mhi;
    int bins, metric;
    double min_overlap;
} oreg_pair;

/* the score of theta at a stride and whether it is admissible (a theta without a finite map: no voxel counts) */
static double score(const oreg_pair *P, const double *th, int stride, int *admissible)
{
    static int64_t hist[64 * 64];
    int64_t sums[6], excluded, outside;
    float map[12];
    double out[7];
    if (oreg_map(th, P->nx, P->ny, P->nz, P->fv, P->mv, P->m0, map) != 0)
        for (int k = 0; k < 12; k++) map[k] = NAN;
    const int64_t N = oreg_warp_hist(P->F, P->nx, P->ny, P->nz, P->M, P->mx, P->my, P->mz, map, 1, stride, P->flo, P->fhi, P->mlo, P->mhi, P->bins, hist, sums,
                                     &excluded, &outside);
    osim_measures(hist, P->bins, sums, 0.0f, 1.0f, 0, out);
    const double sc = P->metric == 0 ? out[0] : out[1];
    *admissible = !isnan(sc) && (double)sums[0] >= P->min_overlap * (double)N;
    return sc;
}

/* 0; -1: a matrix or an image without a range; -2: the start is inadmissible.  Per level l < n_levels: iterations, evaluations, stop,
 * score_in, score_out, last_step.  theta 12, result 16. */
int oreg_register(const float *F, int64_t nx, int64_t ny, int64_t nz, const float *M, int64_t mx, int64_t my, int64_t mz, const float *fv, const float *mv,
                  const float *m0, int dof, int metric, int bins, int n_levels, const int *strides, const double *first, const double *last, int max_iterations,
                  double min_overlap, double *theta, float *result, int *iterations, int *evaluations, int *stop, double *score_in, double *score_out,
                  double *last_step)
{
    oreg_pair P = {F, M, fv, mv, m0, nx, ny, nz, mx, my, mz, 0, 0, 0, 0, bins, metric, min_overlap};
    int64_t n3[3];
    double h, rho, cand[24 * 12];
    float map[12];
    memset(theta, 0, sizeof(double) * 12);
    if (!osim_range(F, nx * ny * nz, &P.flo, &P.fhi) || !osim_range(M, mx * my * mz, &P.mlo, &P.mhi)) return -1;
    if (oreg_map(theta, nx, ny, nz, fv, mv, m0, map) != 0) return -1;
    oreg_lattice(nx, ny, nz, 1, fv, n3, &h, &rho);
    for (int l = 0; l < n_levels; l++) {
        int ok;
        double cur = score(&P, theta, strides[l], &ok);
        if (l == 0 && !ok) return -2;
        if (!ok) cur = -INFINITY;
        score_in[l] = cur;
        iterations[l] = 0;
        evaluations[l] = 1;
        double u = first[l] * h;
        const double end = last[l] * h;
        while (iterations[l] < max_iterations && !(u < end)) {
            const int K = oreg_candidates(theta, dof, u, rho, cand);
            int best = -1;
            double best_score = 0.0;
            for (int c = 0; c < K; c++) {
                const double sc = score(&P, cand + 12 * c, strides[l], &ok);
                if (ok && (best < 0 || sc > best_score)) {
                    best = c;
                    best_score = sc;
                }
            }
            iterations[l]++;
            evaluations[l] += K;
            if (best >= 0 && best_score > cur) {
                memcpy(theta, cand + 12 * best, sizeof(double) * 12);
                cur = best_score;
            } else {
                u = u / 2.0;
            }
        }
        stop[l] = u < end ? 0 : 1;
        score_out[l] = cur;
        last_step[l] = u;
    }
    return oreg_result(theta, nx, ny, nz, fv, m0, result);
}
