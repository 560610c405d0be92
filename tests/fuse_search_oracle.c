/*
 * fuse_search_oracle.c -- the local search of the label fusion as a serial program, written from the contract
 * and not from the kernel.  Built by the tests with cc -O2 -ffp-contract=off and bound with ctypes.  It includes fuse_oracle.c: the
 * quantisation, the similarity and the vote are section 7j's, unchanged.
 *
 * The contract.  qT and qW on the target grid (int16, -1: not finite), M the warped labels (or none), half-width b, radius r
 * (0 .. 3, b + r <= 6).
 *   Candidates at x: the shifts t in [-r, r]^3 with x + t inside the volume and M(x + t) finite (no labels: every shift inside).
 *   Sums per candidate: over v in [-b, b]^3 with x + v and x + t + v inside the volume, qT(x + v) >= 0 and qW(x + t + v) >= 0:
 *   n, Sf = sum qT(x + v), Sff, Sw = sum qW(x + t + v), Sww, Sfw.
 *   u(x, t) = ofu_similarity(metric, sums).  t* = the candidate of the largest u; ties to the smallest |t|^2, then tz, ty, tx.
 *   Result: u* = u(x, t*), picked = M(x + t*), code = ((tz + r)(2r + 1) + (ty + r))(2r + 1) + (tx + r).  No candidate: u = 0xffff,
 *   picked NaN, code 0xffff.
 * ofs_search is the brute force.  ofs_search_sat states the same sums through summed-area tables, one per shift (the sums are
 * integers, so any order of the additions gives the same words); the tests hold it to the brute force and use it where the brute
 * force would take minutes.
 */
#include "fuse_oracle.c"

int ofs_shift_code(int r, int tx, int ty, int tz)
{
    const int s = 2 * r + 1;
    return ((tz + r) * s + (ty + r)) * s + (tx + r);
}

/* 1 where (u, t) is a better choice than (bu, bt), both candidates */
static int ofs_better(uint32_t u, const int t[3], uint32_t bu, const int bt[3])
{
    if (u != bu) return u > bu;
    const int d = t[0] * t[0] + t[1] * t[1] + t[2] * t[2], bd = bt[0] * bt[0] + bt[1] * bt[1] + bt[2] * bt[2];
    if (d != bd) return d < bd;
    if (t[2] != bt[2]) return t[2] < bt[2];
    if (t[1] != bt[1]) return t[1] < bt[1];
    return t[0] < bt[0];
}

static int ofs_args_ok(int b, int r, int metric) { return b >= 1 && r >= 0 && r <= 3 && b + r <= 6 && (metric == 0 || metric == 1); }

static void ofs_result(int have, uint32_t u, const int t[3], int r, const float *labels, int64_t at, int64_t nx, int64_t ny, uint16_t *uo, uint16_t *so,
                       float *po)
{
    if (!have) {
        *uo = 0xffff;
        *so = 0xffff;
        if (po) *po = NAN;
        return;
    }
    *uo = (uint16_t)u;
    *so = (uint16_t)ofs_shift_code(r, t[0], t[1], t[2]);
    if (po) *po = labels ? labels[at + ((int64_t)t[2] * ny + t[1]) * nx + t[0]] : NAN;
}

/* labels, picked: may be NULL; sums: 6 int64 per voxel, those of the chosen candidate (0 where there is none), may be NULL */
int ofs_search(const int16_t *qt, const int16_t *qw, const float *labels, int64_t nx, int64_t ny, int64_t nz, int b, int r, int metric, uint16_t *u,
               uint16_t *shift, float *picked, int64_t *sums)
{
    if (!ofs_args_ok(b, r, metric)) return -1;
    for (int64_t z = 0; z < nz; z++)
        for (int64_t y = 0; y < ny; y++)
            for (int64_t x = 0; x < nx; x++) {
                const int64_t at = (z * ny + y) * nx + x;
                int have = 0, bt[3] = {0, 0, 0};
                uint32_t bu = 0;
                int64_t bs[6] = {0, 0, 0, 0, 0, 0};
                for (int tz = -r; tz <= r; tz++)
                    for (int ty = -r; ty <= r; ty++)
                        for (int tx = -r; tx <= r; tx++) {
                            const int64_t cx = x + tx, cy = y + ty, cz = z + tz;
                            if (cx < 0 || cx >= nx || cy < 0 || cy >= ny || cz < 0 || cz >= nz) continue;
                            if (labels && !isfinite(labels[(cz * ny + cy) * nx + cx])) continue;
                            int64_t s[6] = {0, 0, 0, 0, 0, 0};
                            for (int64_t dz = -b; dz <= b; dz++)
                                for (int64_t dy = -b; dy <= b; dy++)
                                    for (int64_t dx = -b; dx <= b; dx++) {
                                        const int64_t X = x + dx, Y = y + dy, Z = z + dz, XW = X + tx, YW = Y + ty, ZW = Z + tz;
                                        if (X < 0 || X >= nx || Y < 0 || Y >= ny || Z < 0 || Z >= nz) continue;
                                        if (XW < 0 || XW >= nx || YW < 0 || YW >= ny || ZW < 0 || ZW >= nz) continue;
                                        const int64_t f = qt[(Z * ny + Y) * nx + X], w = qw[(ZW * ny + YW) * nx + XW];
                                        if (f < 0 || w < 0) continue;
                                        s[0] += 1;
                                        s[1] += f;
                                        s[2] += f * f;
                                        s[3] += w;
                                        s[4] += w * w;
                                        s[5] += f * w;
                                    }
                            const uint32_t uu = ofu_similarity(metric, s[0], s[1], s[2], s[3], s[4], s[5]);
                            const int t[3] = {tx, ty, tz};
                            if (!have || ofs_better(uu, t, bu, bt)) {
                                have = 1;
                                bu = uu;
                                memcpy(bt, t, sizeof bt);
                                memcpy(bs, s, sizeof bs);
                            }
                        }
                ofs_result(have, bu, bt, r, labels, at, nx, ny, &u[at], &shift[at], picked ? &picked[at] : NULL);
                if (sums) memcpy(sums + 6 * at, bs, sizeof bs);
            }
    return 0;
}

/* the same words through one summed-area table of the six pointwise terms per shift */
int ofs_search_sat(const int16_t *qt, const int16_t *qw, const float *labels, int64_t nx, int64_t ny, int64_t nz, int b, int r, int metric, uint16_t *u,
                   uint16_t *shift, float *picked)
{
    if (!ofs_args_ok(b, r, metric)) return -1;
    const int64_t n = nx * ny * nz, px = nx + 1, py = ny + 1, pn = px * py * (nz + 1);
    int64_t *sat = (int64_t *)malloc(sizeof(int64_t) * 6 * (size_t)pn);
    uint32_t *bu = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)n);
    int *bt = (int *)malloc(sizeof(int) * 3 * (size_t)n);
    char *have = (char *)calloc((size_t)n, 1);
    if (!sat || !bu || !bt || !have) return -2;
    for (int tz = -r; tz <= r; tz++)
        for (int ty = -r; ty <= r; ty++)
            for (int tx = -r; tx <= r; tx++) {
                /* sat[c][(z, y, x)] = the sum of term c over the voxels below (z, y, x) on every axis */
                memset(sat, 0, sizeof(int64_t) * 6 * (size_t)pn);
                for (int64_t z = 0; z < nz; z++)
                    for (int64_t y = 0; y < ny; y++)
                        for (int64_t x = 0; x < nx; x++) {
                            int64_t term[6] = {0, 0, 0, 0, 0, 0};
                            const int64_t XW = x + tx, YW = y + ty, ZW = z + tz;
                            if (XW >= 0 && XW < nx && YW >= 0 && YW < ny && ZW >= 0 && ZW < nz) {
                                const int64_t f = qt[(z * ny + y) * nx + x], w = qw[(ZW * ny + YW) * nx + XW];
                                if (f >= 0 && w >= 0) {
                                    term[0] = 1;
                                    term[1] = f;
                                    term[2] = f * f;
                                    term[3] = w;
                                    term[4] = w * w;
                                    term[5] = f * w;
                                }
                            }
                            const int64_t i = ((z + 1) * py + (y + 1)) * px + (x + 1);
                            for (int c = 0; c < 6; c++) {
                                const int64_t *S = sat + c * pn;
                                sat[c * pn + i] = term[c] + S[i - 1] + S[i - px] + S[i - px * py] - S[i - px - 1] - S[i - px * py - 1] - S[i - px * py - px] +
                                                  S[i - px * py - px - 1];
                            }
                        }
                for (int64_t z = 0; z < nz; z++)
                    for (int64_t y = 0; y < ny; y++)
                        for (int64_t x = 0; x < nx; x++) {
                            const int64_t cx = x + tx, cy = y + ty, cz = z + tz, at = (z * ny + y) * nx + x;
                            if (cx < 0 || cx >= nx || cy < 0 || cy >= ny || cz < 0 || cz >= nz) continue;
                            if (labels && !isfinite(labels[(cz * ny + cy) * nx + cx])) continue;
                            const int64_t x0 = x - b < 0 ? 0 : x - b, x1 = x + b + 1 > nx ? nx : x + b + 1;
                            const int64_t y0 = y - b < 0 ? 0 : y - b, y1 = y + b + 1 > ny ? ny : y + b + 1;
                            const int64_t z0 = z - b < 0 ? 0 : z - b, z1 = z + b + 1 > nz ? nz : z + b + 1;
                            int64_t s[6];
                            for (int c = 0; c < 6; c++) {
                                const int64_t *S = sat + c * pn;
#define AT(Z, Y, X) S[((Z) * py + (Y)) * px + (X)]
                                s[c] = AT(z1, y1, x1) - AT(z1, y1, x0) - AT(z1, y0, x1) - AT(z0, y1, x1) + AT(z1, y0, x0) + AT(z0, y1, x0) + AT(z0, y0, x1) -
                                       AT(z0, y0, x0);
#undef AT
                            }
                            const uint32_t uu = ofu_similarity(metric, s[0], s[1], s[2], s[3], s[4], s[5]);
                            const int t[3] = {tx, ty, tz};
                            if (!have[at] || ofs_better(uu, t, bu[at], bt + 3 * at)) {
                                have[at] = 1;
                                bu[at] = uu;
                                memcpy(bt + 3 * at, t, sizeof t);
                            }
                        }
            }
    for (int64_t at = 0; at < n; at++) ofs_result(have[at], bu[at], bt + 3 * at, r, labels, at, nx, ny, &u[at], &shift[at], picked ? &picked[at] : NULL);
    free(sat);
    free(bu);
    free(bt);
    free(have);
    return 0;
}
