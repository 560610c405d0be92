/*
 * blockmatch_ncc_oracle.c -- CPU restatement of the block search under the correlation cost of DESIGN.md section 7g (test
 * infrastructure; written from that text, it includes none of the product's headers).  Built with cc -O2 -ffp-contract=off by
 * tests/blockmatch_ncc_cases.py.  The quantised volumes come from blockmatch_oracle.c's obm_quantize (the 10-bit map is section
 * 7f's; what section 7g changes is the range W is quantised with, which is the caller's business).
 *
 * oncc_cost: the cost from the five sums and N, every integer in int64:
 *   A = N Sfw - Sf Sw, Vf = N Sff - Sf^2, Vw = N Sww - Sw^2;
 *   rho2 = A > 0 and Vf > 0 and Vw > 0 ? ((double)A * (double)A) / ((double)Vf * (double)Vw) : 0;
 *   cost = (uint32) rint((1 - (rho2 > 1 ? 1 : rho2)) * 2^31).
 * oncc_match: every node, every shift (z, then y, then x, ascending), every voxel of the block, serially; the argmin is the
 *   least (cost, |s|^2, s_z, s_y, s_x); flagged where a voxel of the F block or of the W window is outside the volume or -1, and
 *   then every other word is 0.  16 words per node: shift x, y, z; flag; cost(argmin); cost(0); cost at argmin -x, +x, -y, +y,
 *   -z, +z (0xffffffff outside the search cube); sum qF; sum qF^2; 0; 0.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

uint32_t oncc_cost(int64_t N, int64_t Sf, int64_t Sff, int64_t Sw, int64_t Sww, int64_t Sfw)
{
    const int64_t A = N * Sfw - Sf * Sw, Vf = N * Sff - Sf * Sf, Vw = N * Sww - Sw * Sw;
    double rho2 = 0.0;
    if (A > 0 && Vf > 0 && Vw > 0) {
        const double num = (double)A * (double)A;
        const double den = (double)Vf * (double)Vw;
        rho2 = num / den;
    }
    if (rho2 > 1.0) rho2 = 1.0;
    const double scaled = (1.0 - rho2) * 2147483648.0;
    return (uint32_t)rint(scaled);
}

static uint32_t cost_at(const int16_t *qf, const int16_t *qw, int64_t nx, int64_t ny, const int64_t p[3], int b, int sx, int sy, int sz,
                        int64_t Sf, int64_t Sff)
{
    int64_t Sw = 0, Sww = 0, Sfw = 0, N = 0;
    for (int uz = -b; uz <= b; uz++)
        for (int uy = -b; uy <= b; uy++)
            for (int ux = -b; ux <= b; ux++) {
                const int64_t f = qf[((p[2] + uz) * ny + (p[1] + uy)) * nx + (p[0] + ux)];
                const int64_t w = qw[((p[2] + uz + sz) * ny + (p[1] + uy + sy)) * nx + (p[0] + ux + sx)];
                Sw += w;
                Sww += w * w;
                Sfw += f * w;
                N++;
            }
    return oncc_cost(N, Sf, Sff, Sw, Sww, Sfw);
}

int oncc_match(const int16_t *qf, const int16_t *qw, int64_t nx, int64_t ny, int64_t nz, const int64_t *first, int64_t stride, const int64_t *cnt,
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
                for (int uz = -b - r; uz <= b + r && !flag; uz++)
                    for (int uy = -b - r; uy <= b + r && !flag; uy++)
                        for (int ux = -b - r; ux <= b + r && !flag; ux++) {
                            const int64_t at = ((p[2] + uz) * ny + (p[1] + uy)) * nx + (p[0] + ux);
                            if (qw[at] < 0) flag = 1;
                            if (abs(ux) <= b && abs(uy) <= b && abs(uz) <= b && qf[at] < 0) flag = 1;
                        }
                if (flag) {
                    o[3] = 1;
                    continue;
                }
                int64_t Sf = 0, Sff = 0;
                for (int uz = -b; uz <= b; uz++)
                    for (int uy = -b; uy <= b; uy++)
                        for (int ux = -b; ux <= b; ux++) {
                            const int64_t q = qf[((p[2] + uz) * ny + (p[1] + uy)) * nx + (p[0] + ux)];
                            Sf += q;
                            Sff += q * q;
                        }
                uint32_t best = 0, c0 = 0;
                int bs[3] = {0, 0, 0}, have = 0;
                for (int sz = -r; sz <= r; sz++)
                    for (int sy = -r; sy <= r; sy++)
                        for (int sx = -r; sx <= r; sx++) {
                            const uint32_t cs = cost_at(qf, qw, nx, ny, p, b, sx, sy, sz, Sf, Sff);
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
                o[4] = best;
                o[5] = c0;
                for (int k = 0; k < 3; k++)
                    for (int up = 0; up < 2; up++) {
                        int s[3] = {bs[0], bs[1], bs[2]};
                        s[k] += up ? 1 : -1;
                        o[6 + 2 * k + up] = abs(s[k]) > r ? 0xffffffffu : cost_at(qf, qw, nx, ny, p, b, s[0], s[1], s[2], Sf, Sff);
                    }
                o[12] = (uint32_t)Sf;
                o[13] = (uint32_t)Sff;
            }
    return 0;
}
