/*
 * kernels_fuse_search.hip -- the local search of the label fusion for gfx950 (MI355X; tests/fuse_search_oracle.c
 * restates it as a serial brute force).  fuse_search_kernel<B, R, NCC> lets one warped atlas compare the target patch at every voxel
 * x with its own patches at x + t, t in [-r, r]^3, and keeps per voxel the similarity u, the shift code and the label of the best
 * candidate.  The sums and the similarity are section 7j's (patch_sums.h, patch_cost.h), so no result depends on the tiling, the
 * order of the additions or the wave layout.
 *
 * The workgroup and its brick are fuse_weight_kernel's (kernels_fuse.hip).  It stages three tiles in LDS once per brick: qT with a
 * halo of b and qW with a halo of b + r as int16 (-1: outside the volume or not finite), and one byte per voxel with a halo of r
 * that says whether the voxel may be picked (inside the volume, and its label finite where there are labels).  Whether a patch
 * voxel counts depends on the shift -- qT at x + v and qW at x + t + v must both be valid -- so the validity is tested per pair;
 * the weight kernel's trick of staging the joint validity does not carry over.
 *   The loop over the shifts is outermost, z then y then x.  The running best of each of a thread's four voxels is one dword,
 *   u << 14 | (0x3fff - rank), rank = |t|^2 << 9 | (tz + r) << 6 | (ty + r) << 3 | (tx + r): the unsigned maximum is the contract's
 *   choice (largest u, then smallest |t|^2, tz, ty, tx), and 0 says that no shift was a candidate.
 *   B > 0 (b and r at compile time; instantiated for b = 2, r = 1, 2, 3): the weight kernel's sliding form per shift, a row of qT
 *   and a row of qW in place of its row of dwords.
 *   B = 0 (any b, r with b + r <= 6): every patch voxel straight from the tiles, per output voxel and shift.
 * The picked label is gathered from the warped labels at x + t* by the same thread; no scratch, no LDS atomics, no float sums.
 */
#include "sift3d_internal.h"
#include "patch_sums.h"

#define FS_THREADS 256
#define FS_NONE 0xffffu /* in the u and the shift plane: the atlas does not vote here */

/* labels: the warped labels (float, not finite: may not be picked) or nullptr (every voxel inside the volume may be picked, and
 * picked is not written).  u, shift: one uint16 per voxel. */
template <int B, int R, int NCC>
__global__ __launch_bounds__(FS_THREADS) void fuse_search_kernel(const short *__restrict__ qt, const short *__restrict__ qw, const float *__restrict__ labels,
                                                                 long long nx, long long ny, long long nz, int b_any, int r_any,
                                                                 unsigned short *__restrict__ u, unsigned short *__restrict__ shift,
                                                                 float *__restrict__ picked, long long nbx, long long nby, long long nbricks)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char fs_lds[];
    const int b = B > 0 ? B : b_any, r = B > 0 ? R : r_any, h = b + r, side = 2 * b + 1, span = 2 * r + 1;
    const int tex = BRICK_BX + 2 * b, tey = BRICK_BY + 2 * b, tez = BRICK_BZ + 2 * b, texy = tex * tey, tvol = texy * tez;
    const int wex = BRICK_BX + 2 * h, wey = BRICK_BY + 2 * h, wez = BRICK_BZ + 2 * h, wexy = wex * wey, wvol = wexy * wez;
    const int mex = BRICK_BX + 2 * r, mey = BRICK_BY + 2 * r, mez = BRICK_BZ + 2 * r, mexy = mex * mey, mvol = mexy * mez;
    short *tile_t = reinterpret_cast<short *>(fs_lds);
    short *tile_w = tile_t + ((tvol + 1) & ~1);
    unsigned char *tile_m = reinterpret_cast<unsigned char *>(tile_w + ((wvol + 1) & ~1));
    int tx, ty, tz;
    brick_lane(tx, ty, tz);
    for (long long L = brick_slot0(); L < nbricks; L += gridDim.x) {
        long long x0, y0, z0;
        brick_origin(L, nbx, nby, x0, y0, z0);
        __syncthreads(); /* the tiles of the brick before are no longer read */
        for (int i = threadIdx.x; i < tvol; i += FS_THREADS) {
            const int x = i % tex, t = i / tex, y = t % tey, z = t / tey;
            const long long gx = x0 - b + x, gy = y0 - b + y, gz = z0 - b + z;
            short v = -1;
            if (gx >= 0 && gx < nx && gy >= 0 && gy < ny && gz >= 0 && gz < nz) v = qt[(gz * ny + gy) * nx + gx];
            tile_t[i] = v;
        }
        for (int i = threadIdx.x; i < wvol; i += FS_THREADS) {
            const int x = i % wex, t = i / wex, y = t % wey, z = t / wey;
            const long long gx = x0 - h + x, gy = y0 - h + y, gz = z0 - h + z;
            short v = -1;
            if (gx >= 0 && gx < nx && gy >= 0 && gy < ny && gz >= 0 && gz < nz) v = qw[(gz * ny + gy) * nx + gx];
            tile_w[i] = v;
        }
        for (int i = threadIdx.x; i < mvol; i += FS_THREADS) {
            const int x = i % mex, t = i / mex, y = t % mey, z = t / mey;
            const long long gx = x0 - r + x, gy = y0 - r + y, gz = z0 - r + z;
            unsigned char v = 0;
            if (gx >= 0 && gx < nx && gy >= 0 && gy < ny && gz >= 0 && gz < nz) v = labels ? (isfinite(labels[(gz * ny + gy) * nx + gx]) ? 1 : 0) : 1;
            tile_m[i] = v;
        }
        __syncthreads();
        const long long i0 = x0 + tx * BRICK_VX, j = y0 + ty, k = z0 + tz;
        if (j >= ny || k >= nz || i0 >= nx) continue; /* no barrier below this line */
        const int lx = tx * BRICK_VX;
        const short *t0 = tile_t + tz * texy + ty * tex + lx;              /* qT at the patch's first voxel of output voxel 0 */
        const short *w0 = tile_w + (tz + r) * wexy + (ty + r) * wex + lx + r; /* qW there under the shift 0 */
        const unsigned char *m0 = tile_m + (tz + r) * mexy + (ty + r) * mex + lx + r;
        unsigned best[BRICK_VX];
#pragma unroll
        for (int v = 0; v < BRICK_VX; v++) best[v] = 0;
#pragma unroll 1
        for (int sz = -r; sz <= r; sz++)
#pragma unroll 1
            for (int sy = -r; sy <= r; sy++)
#pragma unroll 1
                for (int sx = -r; sx <= r; sx++) {
                    const unsigned rank = ((unsigned)(sz * sz + sy * sy + sx * sx) << 9) | ((unsigned)(sz + r) << 6) | ((unsigned)(sy + r) << 3) | (unsigned)(sx + r);
                    const short *ws = w0 + sz * wexy + sy * wex + sx;
                    const unsigned char *ms = m0 + sz * mexy + sy * mex + sx;
                    patch_sums out[BRICK_VX];
                    if constexpr (B > 0) {
                        constexpr int COLS = BRICK_VX + 2 * B;
                        patch_sums col[COLS];
#pragma unroll
                        for (int c = 0; c < COLS; c++) col[c] = patch_sums{0, 0, 0, 0, 0, 0, 0};
#pragma unroll 1
                        for (int dz = 0; dz < 2 * B + 1; dz++)
#pragma unroll 1
                            for (int dy = 0; dy < 2 * B + 1; dy++) {
                                const short *rt = t0 + dz * texy + dy * tex, *rw = ws + dz * wexy + dy * wex;
                                int f[COLS], w[COLS];
#pragma unroll
                                for (int c = 0; c < COLS; c++) {
                                    f[c] = rt[c];
                                    w[c] = rw[c];
                                }
#pragma unroll
                                for (int c = 0; c < COLS; c++) ps_add<NCC>(col[c], f[c], w[c]);
                            }
                        ps_slide<B, NCC>(col, out);
                    } else {
#pragma unroll
                        for (int v = 0; v < BRICK_VX; v++) {
                            patch_sums s = patch_sums{0, 0, 0, 0, 0, 0, 0};
#pragma unroll 1
                            for (int dz = 0; dz < side; dz++)
#pragma unroll 1
                                for (int dy = 0; dy < side; dy++) {
                                    const short *rt = t0 + dz * texy + dy * tex + v, *rw = ws + dz * wexy + dy * wex + v;
                                    for (int dx = 0; dx < side; dx++) ps_add<NCC>(s, rt[dx], rw[dx]);
                                }
                            out[v] = s;
                        }
                    }
#pragma unroll
                    for (int v = 0; v < BRICK_VX; v++) {
                        const unsigned uv = ps_u<NCC>(out[v]);
                        const unsigned key = ms[v] ? ((uv << 14) | (0x3fffu - rank)) : 0u;
                        best[v] = key > best[v] ? key : best[v];
                    }
                }
        const long long at = (k * ny + j) * nx + i0;
#pragma unroll
        for (int v = 0; v < BRICK_VX; v++) {
            if (i0 + v >= nx) continue;
            unsigned uv = FS_NONE, code = FS_NONE;
            float lab = __builtin_nanf("");
            if (best[v] != 0) {
                const unsigned rank = 0x3fffu - (best[v] & 0x3fffu);
                const int cz = (int)((rank >> 6) & 7u), cy = (int)((rank >> 3) & 7u), cx = (int)(rank & 7u);
                uv = best[v] >> 14;
                code = (unsigned)((cz * span + cy) * span + cx);
                if (labels) lab = labels[at + v + ((long long)(cz - r) * ny + (cy - r)) * nx + (cx - r)];
            }
            u[at + v] = (unsigned short)uv;
            shift[at + v] = (unsigned short)code;
            if (labels) picked[at + v] = lab;
        }
    }
}

/* the bytes of LDS a workgroup takes at (b, r): the two int16 tiles and the byte tile */
static size_t fuse_search_lds(int b, int r)
{
    const int h = b + r;
    const size_t tvol = (size_t)(BRICK_BX + 2 * b) * (BRICK_BY + 2 * b) * (BRICK_BZ + 2 * b);
    const size_t wvol = (size_t)(BRICK_BX + 2 * h) * (BRICK_BY + 2 * h) * (BRICK_BZ + 2 * h);
    const size_t mvol = (size_t)(BRICK_BX + 2 * r) * (BRICK_BY + 2 * r) * (BRICK_BZ + 2 * r);
    return 2 * ((tvol + 1) & ~(size_t)1) + 2 * ((wvol + 1) & ~(size_t)1) + mvol;
}

/* qt, qw: the quantised target and warped atlas (nx ny nz int16, x fastest); labels: the warped labels or nullptr (then picked is
 * not written and may be nullptr); u, shift: one uint16 per voxel.  generic: 0 the form with b and r at compile time where there is
 * one (b = 2, r = 1 .. 3), anything else the form for any b, r.  The caller has checked the extents. */
hipError_t sift3d_launch_fuse_search(hipStream_t s, const short *qt, const short *qw, const float *labels, int64_t nx, int64_t ny, int64_t nz, int b, int r,
                                     int ncc, int generic, unsigned short *u, unsigned short *shift, float *picked)
{
    const brick_launch bl = brick_launch_of(nullptr, nx, ny, nz);
    if (b < 1 || r < 0 || r > 3 || b + r > 6 || (labels && !picked)) return hipErrorInvalidValue;
    const size_t lds = fuse_search_lds(b, r);
    if (lds > 65536) return hipErrorInvalidValue;
    auto k = ncc ? fuse_search_kernel<0, 0, 1> : fuse_search_kernel<0, 0, 0>;
    if (generic == 0 && b == 2) {
        if (r == 1) k = ncc ? fuse_search_kernel<2, 1, 1> : fuse_search_kernel<2, 1, 0>;
        if (r == 2) k = ncc ? fuse_search_kernel<2, 2, 1> : fuse_search_kernel<2, 2, 0>;
        if (r == 3) k = ncc ? fuse_search_kernel<2, 3, 1> : fuse_search_kernel<2, 3, 0>;
    }
    hipLaunchKernelGGL(k, dim3(bl.grid), dim3(FS_THREADS), lds, s, qt, qw, labels, (long long)nx, (long long)ny, (long long)nz, b, r, u, shift, picked, bl.nbx,
                       bl.nby, bl.nbricks);
    return hipGetLastError();
}
