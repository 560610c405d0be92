/*
 * average_oracle.c -- CPU restatement of the template from warped images of DESIGN.md section 7r (test infrastructure; written from
 * that text, it includes none of the product's headers).  Built with cc -O2 -ffp-contract=off by tests/average_cases.py.  The
 * sampler is the resampling oracle's and the field oracle's, compiled beside it (their file-local helpers renamed apart).
 *
 * oav_warp: one image on the output grid, linear, fill NaN: ofd_warp with a field, orc_resample without one.
 * oav_average: the contract on K warped planes, voxel by voxel and serially.  The rank of a contributor is counted as the text
 * defines it, #{j : v_j < v_k, or v_j == v_k and j < k}; the trimmed sum then looks up the contributor of each rank in turn.
 * oav_counts, oav_mean_field: the report's counts and the node-wise mean of K fields.
 */
#define at orc_at
#define lerp orc_lerp
#define one_voxel orc_one_voxel
#include "resample_oracle.c"
#undef at
#undef lerp
#undef one_voxel
#define at ofd_at
#define lerp ofd_lerp
#define one_voxel ofd_one_voxel
#include "field_oracle.c"
#undef at
#undef lerp
#undef one_voxel

int oav_warp(const float *src, int64_t nx, int64_t ny, int64_t nz, float *dst, int64_t ox, int64_t oy, int64_t oz, const float *A, const float *C,
             const float *K, const float *disp, const int64_t *nn, const float *o, float h)
{
    if (disp) return ofd_warp(src, nx, ny, nz, dst, ox, oy, oz, A, C, K, disp, nn, o, h, 0, NAN, 0, oz);
    return orc_resample(src, nx, ny, nz, dst, ox, oy, oz, A, 0, NAN, 0, oz);
}

/* planes: K x n warped values, plane k at k * n */
int oav_average(int K, const float *planes, int64_t n, int trim, int min_count, float fill, float *avg, float *var, uint32_t *mask)
{
    if (K < 1 || K > 32 || trim < 0 || trim > 15 || min_count < 1 || min_count > K || n < 0) return -1;
    for (int64_t i = 0; i < n; i++) {
        float v[32];
        int in[32], rank[32], c = 0;
        uint32_t bits = 0;
        for (int k = 0; k < K; k++) {
            v[k] = planes[(int64_t)k * n + i];
            in[k] = isfinite(v[k]) ? 1 : 0;
            if (in[k]) {
                bits |= (uint32_t)1 << k;
                c++;
            }
        }
        mask[i] = bits;
        if (c < min_count) {
            avg[i] = var[i] = fill;
            continue;
        }
        double S = 0.0;
        for (int k = 0; k < K; k++)
            if (in[k]) S = S + (double)v[k];
        const double m = S / (double)c;
        double V = 0.0;
        for (int k = 0; k < K; k++)
            if (in[k]) {
                const double d = (double)v[k] - m;
                V = V + d * d;
            }
        var[i] = c > 1 ? (float)(V / (double)(c - 1)) : 0.0f;
        if (trim == 0) {
            avg[i] = (float)m;
            continue;
        }
        for (int k = 0; k < K; k++) {
            rank[k] = -1;
            if (!in[k]) continue;
            rank[k] = 0;
            for (int j = 0; j < K; j++)
                if (in[j] && (v[j] < v[k] || (v[j] == v[k] && j < k))) rank[k]++;
        }
        const int half = (c - 1) / 2, t = trim < half ? trim : half;
        double T = 0.0;
        for (int r = t; r <= c - 1 - t; r++)
            for (int k = 0; k < K; k++)
                if (rank[k] == r) T = T + (double)v[k];
        avg[i] = (float)(T / (double)(c - 2 * t));
    }
    return 0;
}

/* out: none, below, count[0 .. 32], contributing[0 .. 31] */
void oav_counts(const uint32_t *mask, int64_t n, int K, int min_count, int64_t *out)
{
    for (int e = 0; e < 2 + 33 + 32; e++) out[e] = 0;
    for (int64_t i = 0; i < n; i++) {
        int c = 0;
        for (int k = 0; k < K; k++)
            if ((mask[i] >> k) & 1u) {
                c++;
                out[35 + k]++;
            }
        out[2 + c]++;
        if (c == 0) out[0]++;
        if (c < min_count) out[1]++;
    }
}

/* disps: K x count floats, field k at k * count */
void oav_mean_field(int K, const float *disps, int64_t count, float *out)
{
    for (int64_t i = 0; i < count; i++) {
        double s = 0.0;
        for (int k = 0; k < K; k++) s = s + (double)disps[(int64_t)k * count + i];
        out[i] = (float)(s / (double)K);
    }
}
