/*
 * fuse_oracle.c -- multi-atlas label fusion by locally weighted voting as a serial brute force, written
 * from the contract and not from the kernels.  Built by the tests with cc -O2 -ffp-contract=off and bound with ctypes.
 *
 * The contract.  A target T and K warped atlases (W_k intensities, M_k labels) on T's grid, nx ny nz, x fastest.
 *   Quantisation (section 7f): q(v) = -1 where v is not finite, else t = (((double)v - lo) / (hi - lo)) * 1023 in double, q = 0 for
 *   t <= 0, 1023 for t >= 1023, else rint(t).
 *   Patch sums at voxel x, half-width b: over u in [-b, b]^3 with x + u inside the volume, qT(x + u) >= 0 and qW(x + u) >= 0:
 *   n, Sf = sum qT, Sff = sum qT^2, Sw = sum qW, Sww = sum qW^2, Sfw = sum qT qW.
 *   Similarity u in 0 .. 32768, 0 where n = 0.  SSD: D = Sff - 2 Sfw + Sww, u = (n 2^15) / (D + n) in unsigned 64-bit division.
 *   NCC: A = n Sfw - Sf Sw, Vf = n Sff - Sf^2, Vw = n Sww - Sw^2; rho2 = A > 0 and Vf > 0 and Vw > 0 ? (A * A) / (Vf * Vw) : 0 in
 *   double, one operation at a time; c = (uint32) rint((1 - min(rho2, 1)) * 2^31); u = (2^31 - c) >> 16.
 *   Weight: 1 (power 0), u (power 1), u u (power 2).
 *   Vote: atlas k votes at x iff M_k(x) is finite.  S(l) = sum of the weights of the voters with label l.  Power > 0 and every
 *   voter's weight 0: every voter weighs 1, FALLBACK (bit 30).  Winner: the largest S(l), ties to the smallest l.
 *   conf = (S(win) * 65535) / sum of all S, integer division.  No voter: label 0, conf 0, NONE (bit 31).
 *   Words: [0] = label | voters << 16 | flags, [1] = conf.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

int ofu_range(const float *f, int64_t n, float *lo, float *hi)
{
    int any = 0;
    float a = 0, b = 0;
    for (int64_t i = 0; i < n; i++) {
        if (!isfinite(f[i])) continue;
        if (!any) a = b = f[i];
        if (f[i] < a) a = f[i];
        if (f[i] > b) b = f[i];
        any = 1;
    }
    *lo = a;
    *hi = b;
    return any && b > a;
}

void ofu_quantize(const float *f, int64_t n, float lo, float hi, int16_t *q)
{
    for (int64_t i = 0; i < n; i++) {
        if (!isfinite(f[i])) {
            q[i] = -1;
            continue;
        }
        const double t = (((double)f[i] - (double)lo) / ((double)hi - (double)lo)) * 1023.0;
        q[i] = t <= 0.0 ? 0 : (t >= 1023.0 ? 1023 : (int16_t)rint(t));
    }
}

/* metric 0: SSD, 1: NCC */
uint32_t ofu_similarity(int metric, int64_t n, int64_t Sf, int64_t Sff, int64_t Sw, int64_t Sww, int64_t Sfw)
{
    if (n <= 0) return 0;
    if (metric == 0) {
        const int64_t D = Sff - 2 * Sfw + Sww;
        const uint64_t num = (uint64_t)n * 32768u, den = (uint64_t)D + (uint64_t)n;
        return (uint32_t)(num / den);
    }
    const int64_t A = n * Sfw - Sf * Sw, Vf = n * Sff - Sf * Sf, Vw = n * Sww - Sw * Sw;
    double rho2 = 0.0;
    if (A > 0 && Vf > 0 && Vw > 0) {
        const double aa = (double)A * (double)A;
        const double vv = (double)Vf * (double)Vw;
        rho2 = aa / vv;
    }
    if (rho2 > 1.0) rho2 = 1.0;
    const double c = rint((1.0 - rho2) * 2147483648.0);
    return (uint32_t)((2147483648u - (uint32_t)c) >> 16);
}

/* the six sums of every voxel; sums: 6 int64 per voxel (n, Sf, Sff, Sw, Sww, Sfw), may be NULL; u: one uint16 per voxel */
int ofu_weights(const int16_t *qt, const int16_t *qw, int64_t nx, int64_t ny, int64_t nz, int b, int metric, uint16_t *u, int64_t *sums)
{
    if (b < 1 || b > 6 || (metric != 0 && metric != 1)) return -1;
    for (int64_t z = 0; z < nz; z++)
        for (int64_t y = 0; y < ny; y++)
            for (int64_t x = 0; x < nx; x++) {
                int64_t s[6] = {0, 0, 0, 0, 0, 0};
                for (int64_t dz = -b; dz <= b; dz++)
                    for (int64_t dy = -b; dy <= b; dy++)
                        for (int64_t dx = -b; dx <= b; dx++) {
                            const int64_t X = x + dx, Y = y + dy, Z = z + dz;
                            if (X < 0 || X >= nx || Y < 0 || Y >= ny || Z < 0 || Z >= nz) continue;
                            const int64_t f = qt[(Z * ny + Y) * nx + X], w = qw[(Z * ny + Y) * nx + X];
                            if (f < 0 || w < 0) continue;
                            s[0] += 1;
                            s[1] += f;
                            s[2] += f * f;
                            s[3] += w;
                            s[4] += w * w;
                            s[5] += f * w;
                        }
                const int64_t i = (z * ny + y) * nx + x;
                u[i] = (uint16_t)ofu_similarity(metric, s[0], s[1], s[2], s[3], s[4], s[5]);
                if (sums) memcpy(sums + 6 * i, s, sizeof s);
            }
    return 0;
}

/* u, labels: K planes of n values each, plane k at k * n; words: 2 per voxel.  -1 for arguments outside the contract. */
int ofu_vote(int K, const uint16_t *u, const float *labels, int64_t n, int power, uint32_t *words)
{
    if (K < 1 || K > 32 || power < 0 || power > 2) return -1;
    for (int64_t i = 0; i < n; i++) {
        uint64_t w[32];
        int64_t lab[32];
        int voters = 0;
        for (int k = 0; k < K; k++) {
            const float l = labels[(int64_t)k * n + i];
            if (!isfinite(l)) continue;
            if (l < 0 || l > 65535 || l != floorf(l)) return -1;
            const uint64_t uk = u[(int64_t)k * n + i];
            if (uk > 32768) return -1;
            lab[voters] = (int64_t)l;
            w[voters] = power == 0 ? 1 : (power == 1 ? uk : uk * uk);
            voters++;
        }
        if (voters == 0) {
            words[2 * i] = 0x80000000u;
            words[2 * i + 1] = 0;
            continue;
        }
        uint32_t flags = 0;
        uint64_t total = 0;
        for (int v = 0; v < voters; v++) total += w[v];
        if (power > 0 && total == 0) {
            flags = 0x40000000u;
            for (int v = 0; v < voters; v++) w[v] = 1;
            total = (uint64_t)voters;
        }
        /* every voter's label as a candidate: the largest sum wins, and of equal sums the smallest label */
        uint64_t best = 0;
        int64_t win = -1;
        for (int c = 0; c < voters; c++) {
            uint64_t S = 0;
            for (int v = 0; v < voters; v++)
                if (lab[v] == lab[c]) S += w[v];
            if (win < 0 || S > best || (S == best && lab[c] < win)) {
                best = S;
                win = lab[c];
            }
        }
        words[2 * i] = (uint32_t)win | ((uint32_t)voters << 16) | flags;
        words[2 * i + 1] = (uint32_t)((best * 65535u) / total);
    }
    return 0;
}

/* per label 0 .. 65535: voxels of a, of b, of both; -1 where a voxel is finite and no such integer */
int ofu_overlap(const float *a, const float *b, int64_t n, int64_t *ca, int64_t *cb, int64_t *cboth)
{
    memset(ca, 0, 65536 * sizeof(int64_t));
    memset(cb, 0, 65536 * sizeof(int64_t));
    memset(cboth, 0, 65536 * sizeof(int64_t));
    for (int64_t i = 0; i < n; i++) {
        const float v[2] = {a[i], b[i]};
        int64_t l[2] = {-1, -1};
        for (int s = 0; s < 2; s++) {
            if (!isfinite(v[s])) continue;
            if (v[s] < 0 || v[s] > 65535 || v[s] != floorf(v[s])) return -1;
            l[s] = (int64_t)v[s];
        }
        if (l[0] >= 0) ca[l[0]]++;
        if (l[1] >= 0) cb[l[1]]++;
        if (l[0] >= 0 && l[0] == l[1]) cboth[l[0]]++;
    }
    return 0;
}
