/*
 * blockmatch_oracle.c -- CPU restatement of the block search of DESIGN.md section 7f (test infrastructure; written from that
 * text, it includes none of the product's headers).  Built with cc -O2 -ffp-contract=off by tests/blockmatch_cases.py.
 *
 * obm_range: lo, hi = the least and the largest finite value of F; 1 where hi > lo, else 0.
 * obm_quantize: q = -1 where v is not finite, else t = (((double)v - lo) / (hi - lo)) * 1023; 0 for t <= 0, 1023 for t >= 1023,
 *   else rint(t).
 * obm_match: every node, every shift (z, then y, then x, ascending), every voxel of the block, serially:
 *   cost(s) = sum (qF(p + u) - qW(p + u + s))^2 in uint64 (it stays below 2^32); the argmin is the least
 *   (cost, |s|^2, s_z, s_y, s_x); flagged where a voxel of the F block or of the W window is outside the volume or -1, and
 *   then every other word is 0.  16 words per node: shift x, y, z; flag; cost(argmin); cost(0); cost at argmin -x, +x, -y, +y,
 *   -z, +z (0xffffffff outside the search cube); sum qF; sum qF^2; 0; 0.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

int obm_range(const float *f, int64_t n, float *lo, float *hi)
{
    int any = 0;
    float a = 0, b = 0;
    for (int64_t i = 0; i < n; i++) {
        if (!isfinite(f[i])) continue;
        if (!any || f[i] < a) a = f[i];
        if (!any || f[i] > b) b = f[i];
        any = 1;
    }
    *lo = a;
    *hi = b;
    return any && b > a;
}

void obm_quantize(const float *src, int64_t n, float lo, float hi, int16_t *dst)
{
    for (int64_t i = 0; i < n; i++) {
        if (!isfinite(src[i])) {
            dst[i] = -1;
            continue;
        }
        const double t = (((double)src[i] - (double)lo) / ((double)hi - (double)lo)) * 1023.0;
        dst[i] = t <= 0.0 ? 0 : (t >= 1023.0 ? 1023 : (int16_t)rint(t));
    }
}

static uint64_t cost_at(const int16_t *qf, const int16_t *qw, int64_t nx, int64_t ny, const int64_t p[3], int b, int sx, int sy, int sz)
{
    uint64_t c = 0;
    for (int uz = -b; uz <= b; uz++)
        for (int uy = -b; uy <= b; uy++)
            for (int ux = -b; ux <= b; ux++) {
                const int64_t d = (int64_t)qf[((p[2] + uz) * ny + (p[1] + uy)) * nx + (p[0] + ux)] -
                                  (int64_t)qw[((p[2] + uz + sz) * ny + (p[1] + uy + sy)) * nx + (p[0] + ux + sx)];
                c += (uint64_t)(d * d);
            }
    return c;
}

int obm_match(const int16_t *qf, const int16_t *qw, int64_t nx, int64_t ny, int64_t nz, const int64_t *first, int64_t stride, const int64_t *cnt,
              int b, int r, uint32_t *out)
{
    if (b < 1 || r < 1 || stride < 1) return -1;
    const int64_t n[3] = {nx, ny, nz};
    for (int64_t c = 0; c < cnt[2]; c++)
        for (int64_t bb = 0; bb < cnt[1]; bb++)
            for (int64_t a = 0; a < cnt[0]; a++) {
                uint32_t *o = out + 16 * ((c * cnt[1] + bb) * cnt[0] + a);
                memset(o, 0, 16 * sizeof(uint32_t));
                const int64_t p[3] = {first[0] + a * stride, first[1] + bb * stride, first[2] + c * stride};
                int flag = 0;
                for (int k = 0; k < 3; k++) flag |= p[k] - b - r < 0 || p[k] + b + r > n[k] - 1;
                if (!flag) {
                    for (int uz = -b - r; uz <= b + r && !flag; uz++)
                        for (int uy = -b - r; uy <= b + r && !flag; uy++)
                            for (int ux = -b - r; ux <= b + r; ux++) {
                                const int64_t at = ((p[2] + uz) * ny + (p[1] + uy)) * nx + (p[0] + ux);
                                const int in_block = abs(ux) <= b && abs(uy) <= b && abs(uz) <= b;
                                if (qw[at] < 0 || (in_block && qf[at] < 0)) {
                                    flag = 1;
                                    break;
                                }
                            }
                }
                if (flag) {
                    o[3] = 1;
                    continue;
                }
                uint64_t best = 0, c0 = 0;
                int bs[3] = {0, 0, 0}, have = 0;
                for (int sz = -r; sz <= r; sz++)
                    for (int sy = -r; sy <= r; sy++)
                        for (int sx = -r; sx <= r; sx++) {
                            const uint64_t cs = cost_at(qf, qw, nx, ny, p, b, sx, sy, sz);
                            if (!sx && !sy && !sz) c0 = cs;
                            const int m2 = sx * sx + sy * sy + sz * sz, b2 = bs[0] * bs[0] + bs[1] * bs[1] + bs[2] * bs[2];
                            /* the shifts come in (z, y, x) order, so among equal (cost, |s|^2) the first one stays */
                            if (!have || cs < best || (cs == best && m2 < b2)) {
                                best = cs;
                                bs[0] = sx;
                                bs[1] = sy;
                                bs[2] = sz;
                                have = 1;
                            }
                        }
                o[0] = (uint32_t)bs[0];
                o[1] = (uint32_t)bs[1];
                o[2] = (uint32_t)bs[2];
                o[4] = (uint32_t)best;
                o[5] = (uint32_t)c0;
                for (int k = 0; k < 3; k++)
                    for (int up = 0; up < 2; up++) {
                        int s[3] = {bs[0], bs[1], bs[2]};
                        s[k] += up ? 1 : -1;
                        o[6 + 2 * k + up] = abs(s[k]) > r ? 0xffffffffu : (uint32_t)cost_at(qf, qw, nx, ny, p, b, s[0], s[1], s[2]);
                    }
                uint64_t s1 = 0, s2 = 0;
                for (int uz = -b; uz <= b; uz++)
                    for (int uy = -b; uy <= b; uy++)
                        for (int ux = -b; ux <= b; ux++) {
                            const uint64_t q = (uint64_t)qf[((p[2] + uz) * ny + (p[1] + uy)) * nx + (p[0] + ux)];
                            s1 += q;
                            s2 += q * q;
                        }
                o[12] = (uint32_t)s1;
                o[13] = (uint32_t)s2;
            }
    return 0;
}
