/*
 * kernels_extrema.hip -- extrema detection on the DoG levels for gfx950 (MI355X): the first phase in its four forms (march,
 * plane per block, element-wise "strict", generic), the second phase against the neighbour levels, the third phase of a level
 * whose upper neighbour is not stored, and their launchers.  Which form runs, on which grid, with which segments of the
 * own-level list, is decided in extrema_plan.h; sift3d_launch_extrema makes the plan and launches what it says.
 * R/ = the reference's source tree; -ffp-contract=off as everywhere (the third phase repeats the blur's arithmetic).
 */
#include <type_traits>

#include "sift3d_internal.h"

/* ------------------------------------------------------------------------ */
/* Extrema: strict max/min of d_cur over its 26 neighbours, then centre + 26 */
/* of d_prev and (when present) of d_next: the decision of regFindFEATUREIO  */
/* + peak/valleyFunction4D (R/src_common/MultiScale.cpp:2260-2524) followed  */
/* by validateDifferencePeak/Valley3D (:1135-1318).                          */
/*                                                                          */
/* "c > every one of 26 neighbours" == "c > max of the 26" when none is NaN  */
/* (volumes that may hold one take extrema_strict_kernel: sift3d_volume_needs_strict), */
/* and max/min are exact, so the own-level test is done separably: a workgroup owns 64 x by  */
/* EX_ROWS y and marches along z; each wavefront owns one row (two extra     */
/* wavefronts carry the halo rows), gets its x-neighbours with wave-wide DPP */
/* shifts, publishes the row's 3-max / 3-min through LDS, and keeps the 3x3  */
/* plane max/min of planes z-1 and z+1 in registers.  Every voxel of d_cur   */
/* is loaded once; d_prev / d_next are touched only around the rare          */
/* survivors.  Survivors are appended with a wave-aggregated atomic; the     */
/* radix sort restores raster order.                                         */
/* ------------------------------------------------------------------------ */
#define EX_LOAD (EX_ROWS + 2) /* rows loaded per plane (one halo row on each side) */
#define EX_RSRC_FLAGS 0x00020000 /* buffer descriptors: raw buffer, 32-bit data format */

__device__ __forceinline__ float dpp_from_lower(float v) /* lane l gets lane l-1 (lane 0 keeps its own) */
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, v), __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float dpp_from_upper(float v) /* lane l gets lane l+1 (lane 63 keeps its own) */
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, v), __builtin_bit_cast(int, v), 0x130, 0xf, 0xf, false));
}

/* The hardware's own max / min (IEEE mode: a NaN operand yields the other one, as fmaxf / fminf do).  Written as
 * instructions because fmaxf / fminf on values that come straight from memory make the compiler quiet possible signalling
 * NaNs first -- one v_max_f32 v, v, v per loaded element, 12 % of the march loop's vector instructions -- which the
 * instruction does itself. */
__device__ __forceinline__ float ex_max(float a, float b)
{
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float ex_min(float a, float b)
{
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float ex_max3(float a, float b, float c)
{
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ float ex_min3(float a, float b, float c)
{
    float r;
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

/* the same shifts with a value of the lane's own for the lane that has no neighbour in the wavefront (lane 0 / lane 63) */
__device__ __forceinline__ float dpp_from_lower_or(float v, float edge)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, edge), __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float dpp_from_upper_or(float v, float edge)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, edge), __builtin_bit_cast(int, v), 0x130, 0xf, 0xf, false));
}

/* max / min over the x-triple of every element of a row: rmax/rmin include the element, l2max/l2min do not */
__device__ __forceinline__ void row_extrema_v(const float (&v)[6], float (&rmax)[4], float (&rmin)[4], float (&l2max)[4], float (&l2min)[4])
{
#pragma unroll
    for (int e = 0; e < 4; e++) {
        l2max[e] = ex_max(v[e], v[e + 2]);
        l2min[e] = ex_min(v[e], v[e + 2]);
        rmax[e] = ex_max3(v[e], v[e + 2], v[e + 1]);
        rmin[e] = ex_min3(v[e], v[e + 2], v[e + 1]);
    }
}
/* a wavefront covers all of its 256 x: the left neighbour of lane 0 and the right neighbour of lane 63 are `edge` */
__device__ __forceinline__ void row_extrema_edge(v4f a, float edge, float (&rmax)[4], float (&rmin)[4], float (&l2max)[4], float (&l2min)[4])
{
    const float v[6] = {dpp_from_lower_or(a.w, edge), a.x, a.y, a.z, a.w, dpp_from_upper_or(a.x, edge)};
    row_extrema_v(v, rmax, rmin, l2max, l2min);
}
__device__ __forceinline__ void row_extrema(v4f a, float (&rmax)[4], float (&rmin)[4], float (&l2max)[4], float (&l2min)[4])
{
    const float v[6] = {dpp_from_lower(a.w), a.x, a.y, a.z, a.w, dpp_from_upper(a.x)};
    row_extrema_v(v, rmax, rmin, l2max, l2min);
}

/* the segment of the own-level list this workgroup appends to: blockIdx.y counts the first phase's z blocks (extrema_plan.h) */
__device__ __forceinline__ int ex_my_segment() { return ex_segment_of_z_block(blockIdx.y, gridDim.y); }

/* An own-level extremum goes to the second phase: one returning atomic on its segment's counter (surv_cap: entries per segment). */
__device__ __forceinline__ void ex_append_own(sift3d_survivor *__restrict__ surv, unsigned long long *surv_count, long long surv_cap, int seg,
                                              long long idx, float c, bool mx)
{
    const unsigned long long slot = atomicAdd(surv_count + seg * EX_SEG_STRIDE, 1ull);
    if ((long long)slot < surv_cap) {
        sift3d_survivor sv;
        sv.idx = idx;
        sv.value = c;
        sv.is_max = mx ? 1 : 0;
        surv[(long long)seg * surv_cap + (long long)slot] = sv;
    }
}

/* A validated extremum goes to the (key, value) list: h / l are the levels below / above at the voxel. */
__device__ __forceinline__ void ex_emit(unsigned long long *__restrict__ keys, sift3d_cval *__restrict__ vals, unsigned long long *count,
                                        long long cap, int lvl_id, bool mx, long long idx, float c, float h, float l)
{
    const unsigned long long slot = atomicAdd(count, 1ull);
    if ((long long)slot < cap) {
        sift3d_cval r;
        r.value = c;
        r.h = h;
        r.l = l;
        r.pad = 0.0f;
        keys[slot] = ((unsigned long long)lvl_id << SIFT3D_KEY_LVL_SHIFT) | ((unsigned long long)(mx ? 1 : 0) << SIFT3D_KEY_MAX_SHIFT) |
                     (unsigned long long)idx;
        vals[slot] = r;
    }
}

/* First phase.  One wavefront = 248 output voxels along x (64 lanes x float4; the first and last lane
 * only supply x-neighbours) by EX_ROWS rows of ONE plane: it loads EX_ROWS+2 rows of the three planes
 * z-1, z, z+1 as twelve independent 16-byte loads per lane (all in flight together, re-reads are L1/L2
 * hits), reduces them in registers and hands the own-level extrema to the second phase. */
__global__ __launch_bounds__(256) void extrema_kernel(const float *__restrict__ dcur, int X, int Xl, int Y, int Z, int z_first, int z_last, int zchunk,
                                                      int xtiles, sift3d_survivor *__restrict__ surv, unsigned long long *surv_count, long long surv_cap)
{
    const int lane = threadIdx.x & 63;
    const int wv = blockIdx.x * 4 + (threadIdx.x >> 6); /* wavefront index over (x tile, y tile) */
    const int xt = wv % xtiles, yt = wv / xtiles;
    const int y0 = 1 + yt * EX_ROWS;                 /* first output row */
    if (y0 >= Y - 1) return;
    const int z = z_first + blockIdx.y;
    if (z >= z_last) return;
    const int xv = xt * EX_XOUT - 4 + lane * 4;      /* x of this lane's first element (may be -4 or >= X: clamped loads) */
    const int xld = xv < 0 ? 0 : (xv > X - 4 ? X - 4 : xv);
    const long long XY = (long long)X * Y;
    v4f pl[3][EX_LOAD];
#pragma unroll
    for (int r = 0; r < EX_LOAD; r++) {
        int yy = y0 - 1 + r;
        yy = yy < Y ? yy : Y - 1;
        const long long off = (long long)yy * X + xld;
#pragma unroll
        for (int k = 0; k < 3; k++) pl[k][r] = vload<4>(dcur + (long long)(z - 1 + k) * XY + off);
    }
    float p9max[EX_ROWS][4], p9min[EX_ROWS][4]; /* over the 3x3 of planes z-1 and z+1 together */
    float e8max[EX_ROWS][4], e8min[EX_ROWS][4]; /* over the 8 in-plane neighbours */
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float rmax[EX_LOAD][4], rmin[EX_LOAD][4], l2max[EX_LOAD][4], l2min[EX_LOAD][4];
#pragma unroll
        for (int r = 0; r < EX_LOAD; r++) row_extrema(pl[k][r], rmax[r], rmin[r], l2max[r], l2min[r]);
#pragma unroll
        for (int r = 0; r < EX_ROWS; r++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                if (k == 1) {
                    e8max[r][e] = fmaxf(fmaxf(rmax[r][e], rmax[r + 2][e]), l2max[r + 1][e]);
                    e8min[r][e] = fminf(fminf(rmin[r][e], rmin[r + 2][e]), l2min[r + 1][e]);
                } else {
                    const float m = fmaxf(fmaxf(rmax[r][e], rmax[r + 1][e]), rmax[r + 2][e]);
                    const float n = fminf(fminf(rmin[r][e], rmin[r + 1][e]), rmin[r + 2][e]);
                    p9max[r][e] = k == 0 ? m : fmaxf(p9max[r][e], m);
                    p9min[r][e] = k == 0 ? n : fminf(p9min[r][e], n);
                }
            }
    }
#pragma unroll
    for (int r = 0; r < EX_ROWS; r++) {
        const int y = y0 + r;
        const v4f cv = pl[1][r + 1];
        const float cc[4] = {cv.x, cv.y, cv.z, cv.w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const float c = cc[e];
            const bool mx = c > fmaxf(e8max[r][e], p9max[r][e]);
            const bool mn = c < fminf(e8min[r][e], p9min[r][e]);
            const int x = xv + e;
            if ((mx || mn) && lane >= 1 && lane <= 62 && x >= 1 && x < Xl - 1 && y < Y - 1)
                ex_append_own(surv, surv_count, surv_cap, ex_my_segment(), (long long)z * XY + (long long)y * X + x, c, mx);
        }
    }
}

/* First phase, marching form (used when the volume has enough planes).  A wavefront owns 256 x (64 lanes x float4) by EXM_ROWS rows and walks a chunk of planes; every plane is loaded and
 * reduced once.  Round 3 form.  What a lane carries from plane to plane is, per voxel, four floats:
 *   pm, pn    the 3x3 max / min (centre included) of the plane just below: the "26 neighbours" of the next plane's voxel
 *             that lie in that plane;
 *   cmx, cmn  the voxel's own value if it beat its 8 in-plane neighbours and the plane below (-inf / +inf otherwise): a
 *             candidate waiting for the plane above.
 * A step on plane p computes the 3x3 max m / min n and the 8-neighbour max / min of p, FINISHES plane p-1 (cmx > m: a
 * maximum; cmn < n: a minimum -- a comparison with -inf / +inf is false, so non-candidates need no flag), and restarts the
 * candidates from p.  The decisions are the max / min / compare operations of extrema_kernel on the same values --
 * "c > every one of 26" == "c > max of 8" and "c > max of 9 below" and "c > max of 9 above" (NaN-free levels; see
 * extrema_strict_kernel) -- so the lists are the same.
 * The round-2 form kept the five reduced arrays of three planes (195 registers for two rows); this one keeps four arrays of
 * one plane, which pays for four rows per wavefront (six rows loaded for four instead of four for two: 1.5 instead of 2
 * requests per voxel to L1/L2), two planes of prefetch in registers, and buffer loads (row offset in a VGPR, plane offset in
 * an SGPR: no 64-bit address arithmetic in the loop).  The four wavefronts of a workgroup are neighbours in y, so the halo
 * rows they share are L1 hits. */
#define EXM_LOAD (EXM_ROWS + 2)
#define EXM_STAGE (64 + 4 * 64) /* a wavefront's staging buffer: flushed at 64 after every row, a row adds at most 4 per lane */

__global__ __launch_bounds__(256) void extrema_march_kernel(const float *__restrict__ dcur, int X, int Xl, int Y, int Z, int z_first, int z_last,
                                                            int zchunk, int xtiles, int ygroups, sift3d_survivor *__restrict__ surv,
                                                            unsigned long long *surv_count, long long surv_cap)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); /* wave-uniform by construction: say so, or every buffer descriptor below lands in vector registers */
    /* consecutive workgroups land on consecutive XCDs: XCD x takes the x-th eighth of the (x tile, y group) list, so that the
     * two halo rows a y group shares with each neighbour are fetched into ONE L2 (SIFT3D_MARCH_ORDER 0: the round-3 order) */
#ifndef SIFT3D_MARCH_ORDER
#define SIFT3D_MARCH_ORDER 1
#endif
    const unsigned gx = gridDim.x;
    const unsigned bx = (SIFT3D_MARCH_ORDER && (gx & 7u) == 0) ? (blockIdx.x & 7u) * (gx >> 3) + (blockIdx.x >> 3) : blockIdx.x;
    const int xt = (int)(bx % (unsigned)xtiles), yg = (int)(bx / (unsigned)xtiles);
    const int y0 = 1 + (yg * 4 + wave) * EXM_ROWS;   /* first output row of this wavefront */
    const int za = z_first + blockIdx.y * zchunk;
    const int zb = za + zchunk < z_last ? za + zchunk : z_last; /* output planes za .. zb-1; plane zb <= Z-1 exists */
    const bool idle = y0 >= Y - 1 || za >= z_last;             /* wave-uniform */
    /* all 64 lanes produce outputs: x = xv .. xv + 3.  The left neighbour of lane 0's first element and the right
     * neighbour of lane 63's last one come from one extra 4-byte load per row in which only those two lanes carry an
     * address inside the buffer (the others, and positions outside the row, are answered with zeros by the bounds check
     * and cost no memory access).  The round-2 form gave up the outer two lanes instead (248 outputs per wavefront): three
     * wavefronts for a 512-voxel row, i.e. 46 % more loads and arithmetic than the row has voxels. */
    const int xv = xt * EXM_XOUT + lane * 4;
    const long long XY = (long long)X * Y;
    unsigned roff[EXM_LOAD], eoff[EXM_LOAD];
    const int xe = lane == 0 ? xv - 1 : (lane == 63 ? xv + 4 : -1);
#pragma unroll
    for (int r = 0; r < EXM_LOAD; r++) {
        int yy = y0 - 1 + r;
        yy = yy < Y ? yy : Y - 1;
        roff[r] = xv < X ? (unsigned)(yy * X + xv) * 4u : 0xFFFFFFFFu; /* X * Y < 2^29: a plane is below 2 GiB; X % 4 == 0 */
        eoff[r] = (xe >= 0 && xe < X) ? (unsigned)(yy * X + xe) * 4u : 0xFFFFFFFFu;
    }
    const int seg = ex_my_segment();
    /* the chunk's planes za-1 .. zb through one descriptor: (zchunk + 2) planes stay below 4 GiB (the launcher sees to it) */
    const float *const chunk_base = dcur + (long long)(idle ? 0 : za - 1) * XY;
    const int chunk_bytes = idle ? 0 : (int)(unsigned)((long long)(zb - za + 2) * XY * 4);
    const unsigned plane_bytes = (unsigned)(XY * 4);
    /* za-1 <= z.  The plane offset travels in an SGPR, which the hardware's bounds check does not see: a plane past zb
     * (the prefetch runs two planes ahead; its data is never used) goes through a descriptor of no records instead */
    auto load_plane = [&](v4f(&raw)[EXM_LOAD], float(&edge)[EXM_LOAD], int z) {
        const bool ok = z <= zb; /* wave-uniform */
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)chunk_base, 0, ok ? chunk_bytes : 0, EX_RSRC_FLAGS);
        const int so = ok ? (int)((unsigned)(z - (za - 1)) * plane_bytes) : 0;
#pragma unroll
        for (int r = 0; r < EXM_LOAD; r++) raw[r] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)roff[r], so, 0));
#pragma unroll
        for (int r = 0; r < EXM_LOAD; r++) edge[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, (int)eoff[r], so, 0));
    };
    /* Own-level extrema go to a staging buffer of the wavefront in LDS (compacted with a ballot and a prefix count) and
     * from there to the list in batches: ONE returning atomic and a coalesced store per 64 or more of them (a returning
     * atomic per extremum needs s_waitcnt vmcnt(0), which also drains the next plane's loads: 0.33 ms per 512^3 level in
     * round 1).  The order inside the list does not matter: the validated extrema are sorted by key. */
    __shared__ sift3d_survivor stage_all[4][EXM_STAGE];
    sift3d_survivor *const stage = stage_all[wave];
    if (idle) return;
    int pending = 0; /* wave-uniform */
    auto flush = [&]() {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(surv_count + seg * EX_SEG_STRIDE, (unsigned long long)pending);
        base = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(base >> 32)) << 32) |
               (unsigned)__builtin_amdgcn_readfirstlane((int)(base & 0xffffffffull));
        __builtin_amdgcn_wave_barrier(); /* LDS operations of a wavefront execute in issue order: the entries are written */
        for (int i = lane; i < pending; i += 64)
            if ((long long)(base + i) < surv_cap) surv[(long long)seg * surv_cap + (long long)(base + i)] = stage[i];
        __builtin_amdgcn_wave_barrier();
        pending = 0;
    };
    auto stage_hits = [&](bool hit, float c, int is_max, int z, int y, int x) {
        const unsigned long long m = __ballot(hit);
        if (m) { /* wave-uniform */
            if (hit) {
                const int pos = pending + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                sift3d_survivor sv;
                sv.idx = (long long)z * XY + (long long)y * X + x;
                sv.value = c;
                sv.is_max = is_max;
                stage[pos] = sv;
            }
            pending += __popcll(m);
        }
    };
    const float NEG = -__builtin_inff(), POS = __builtin_inff();
    float pm[EXM_ROWS][4], pn[EXM_ROWS][4], cmx[EXM_ROWS][4], cmn[EXM_ROWS][4];
#pragma unroll
    for (int r = 0; r < EXM_ROWS; r++)
#pragma unroll
        for (int e = 0; e < 4; e++) {
            pm[r][e] = pn[r][e] = 0.0f;
            cmx[r][e] = NEG; /* plane za-1 has no candidates here: it is the chunk below's, or the volume's face */
            cmn[r][e] = POS;
        }
    /* One plane: reduce it, finish the candidates of the plane below (plane z-1), start this plane's.  FIRST: plane za-1,
     * of which only the 3x3 max / min are wanted. */
    auto step = [&](const v4f(&raw)[EXM_LOAD], const float(&edge)[EXM_LOAD], int z, auto first_tag) {
        constexpr bool FIRST = decltype(first_tag)::value;
        /* a window of three reduced rows (slot = row % 3) and the in-row pair max / min of two (slot = row & 1) */
        float rmax[3][4], rmin[3][4], l2max[2][4], l2min[2][4];
        row_extrema_edge(raw[0], edge[0], rmax[0], rmin[0], l2max[0], l2min[0]);
        row_extrema_edge(raw[1], edge[1], rmax[1], rmin[1], l2max[1], l2min[1]);
#pragma unroll
        for (int r = 0; r < EXM_ROWS; r++) {
            const int a = r % 3, b = (r + 1) % 3, c2 = (r + 2) % 3; /* window slots of rows r, r+1 (the output row), r+2 */
            row_extrema_edge(raw[r + 2], edge[r + 2], rmax[c2], rmin[c2], l2max[r & 1], l2min[r & 1]);
            const v4f cv = raw[r + 1];
            const float cc[4] = {cv.x, cv.y, cv.z, cv.w};
            float oldx[4], oldn[4];
            bool hx[4], hn[4], rowhit = false;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const float m = ex_max3(rmax[a][e], rmax[b][e], rmax[c2][e]);
                const float n = ex_min3(rmin[a][e], rmin[b][e], rmin[c2][e]);
                if constexpr (!FIRST) {
                    const float e8x = ex_max3(rmax[a][e], rmax[c2][e], l2max[(r + 1) & 1][e]);
                    const float e8n = ex_min3(rmin[a][e], rmin[c2][e], l2min[(r + 1) & 1][e]);
                    oldx[e] = cmx[r][e];
                    oldn[e] = cmn[r][e];
                    hx[e] = oldx[e] > m; /* the candidate of plane z-1 also beats the nine voxels above it */
                    hn[e] = oldn[e] < n;
                    rowhit = rowhit || hx[e] || hn[e];
                    const float c = cc[e];
                    cmx[r][e] = c > ex_max(e8x, pm[r][e]) ? c : NEG;
                    cmn[r][e] = c < ex_min(e8n, pn[r][e]) ? c : POS;
                }
                pm[r][e] = m;
                pn[r][e] = n;
            }
            if constexpr (!FIRST) {
                /* the rare part: extrema of plane z-1 in row y0 + r, inside the searched x and y range */
                const int y = y0 + r;
                const bool rowok = y < Y - 1;
                if (__ballot(rowhit && rowok)) {
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const int x = xv + e;
                        const bool inx = rowok && x >= 1 && x < Xl - 1;
                        /* a voxel is never both: one append serves the maximum and the minimum test */
                        stage_hits((hx[e] || hn[e]) && inx, hx[e] ? oldx[e] : oldn[e], hx[e] ? 1 : 0, z - 1, y, x);
                    }
                    if (pending >= 64) flush();
                }
            }
        }
    };
    using T = std::true_type;
    using F = std::false_type;
    v4f w0[EXM_LOAD], w1[EXM_LOAD], w2[EXM_LOAD];
    float g0[EXM_LOAD], g1[EXM_LOAD], g2[EXM_LOAD];
    load_plane(w0, g0, za - 1);
    load_plane(w1, g1, za);
    load_plane(w2, g2, za + 1);
    step(w0, g0, za - 1, T{});
    /* planes za .. zb (zb only finishes zb-1).  Invariant at the top: w1 holds plane z, w2 plane z+1 (in flight), w0 is free;
     * the three register windows rotate without copies, two planes are always in flight */
    for (int z = za;;) {
        load_plane(w0, g0, z + 2);
        step(w1, g1, z, F{});
        if (++z > zb) break;
        load_plane(w1, g1, z + 2);
        step(w2, g2, z, F{});
        if (++z > zb) break;
        load_plane(w2, g2, z + 2);
        step(w0, g0, z, F{});
        if (++z > zb) break;
    }
    if (pending > 0) flush();
}

/* Second phase: one thread per own-level extremum checks centre + 26 of d_prev and of d_next and
 * appends the survivors as (key, value) pairs.  The list length lives in device memory, so the grid
 * is sized for the capacity and surplus threads leave at once (no host round trip).
 *
 * PAIR: the level below is not stored as a DoG volume; its value at a voxel is gprev_a[i] - gprev_b[i], the two
 * Gaussian levels it is the difference of -- which is how the reference itself validates against a DoG level it never
 * materialises (validateDifferencePeak3D, R/src_common/MultiScale.cpp:1135-1223: fG1 - fG2 at the 27 positions).
 * DEFER: the level above is not stored either, nor is the Gaussian level it would be made from: what passes the test
 * against the level below goes to a second list, and extrema_validate_lazy_kernel evaluates that Gaussian level at the
 * 27 positions around each entry. */
template <bool PAIR, bool DEFER>
__global__ __launch_bounds__(256) void extrema_validate_kernel(const float *__restrict__ dprev, const float *__restrict__ gprev_b,
                                                               const float *__restrict__ dnext, int X, int Y, const sift3d_survivor *__restrict__ surv,
                                                               const unsigned long long *__restrict__ surv_count, long long surv_cap,
                                                               unsigned long long *surv_overflow, int lvl_id, unsigned long long *__restrict__ keys,
                                                               sift3d_cval *__restrict__ vals, unsigned long long *count, long long cap,
                                                               sift3d_survivor2 *__restrict__ list2, unsigned long long *list2_count, long long list2_cap)
{
    const int seg = blockIdx.y; /* surv_cap is the capacity of one segment */
    long long n = (long long)surv_count[seg * EX_SEG_STRIDE];
    if (n > surv_cap) { /* the segment was cut short: tell the host how much room a replay needs */
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicMax(surv_overflow, (unsigned long long)n * gridDim.y); /* gridDim.y = segments in use */
        n = surv_cap;
    }
    /* The grid normally covers the list's capacity (surplus workgroups leave at once); a shorter grid walks the list in
     * strides.  The bound is the same for every thread of the workgroup (the DEFER form votes).  (Round 3 tried a grid sized
     * for 1/256 of the voxels with the strides doing the rest: own-level extrema are 0.4 - 0.5 % of a blob field, so the
     * strides were the common case and every form got slower: 40 -> 65, 24 -> 46, 86 -> 93 us at 512^3.) */
    for (long long i0 = (long long)blockIdx.x * blockDim.x; i0 < n; i0 += (long long)gridDim.x * blockDim.x) {
    const long long i = i0 + threadIdx.x;
    bool ok = i < n;
    if (!DEFER && !ok) continue;
    sift3d_survivor sv;
    sv.idx = 0; sv.value = 0.0f; sv.is_max = 0;
    if (ok) sv = surv[(long long)seg * surv_cap + i];
    const long long XY = (long long)X * Y;
    const float c = sv.value;
    const bool mx = sv.is_max != 0;
    float hval = 0.0f, lval = 0.0f;
    auto prev_at = [&](long long j) -> float { return PAIR ? dprev[j] - gprev_b[j] : dprev[j]; };
    /* Which of the 54 comparisons runs first does not change their conjunction.  The voxel itself in the two neighbour
     * levels is the likeliest to refute an own-level extremum (adjacent DoG levels are strongly correlated there), so it is
     * asked first -- one or two loads per listed voxel, of which there are 0.4 - 0.5 % of the volume -- and the 26 around it
     * only for what is left. */
    if (ok) {
        hval = prev_at(sv.idx);
        ok = mx ? (hval < c) : (hval > c);
        if (!DEFER && dnext) {
            lval = dnext[sv.idx];
            ok = ok && (mx ? (lval < c) : (lval > c));
        }
    }
    if (ok) {
        for (int dz = -1; dz <= 1 && ok; dz++) {
            float q[9];
#pragma unroll
            for (int k = 0; k < 9; k++) q[k] = (dz == 0 && k == 4) ? hval : prev_at(sv.idx + dz * XY + (k / 3 - 1) * X + (k % 3 - 1));
#pragma unroll
            for (int k = 0; k < 9; k++) ok = ok && (mx ? (q[k] < c) : (q[k] > c));
        }
    }
    if constexpr (DEFER) {
        /* one returning atomic per wavefront: the entries of a wavefront go to consecutive slots */
        const unsigned long long m = __ballot(ok);
        if (m == 0) continue;
        const int lane = threadIdx.x & 63;
        unsigned long long base = 0;
        if (lane == (int)__builtin_ctzll(m)) base = atomicAdd(list2_count + seg, (unsigned long long)__popcll(m));
        const int src = (int)__builtin_ctzll(m);
        base = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(base >> 32), src) << 32) |
               (unsigned)__builtin_amdgcn_readlane((int)(base & 0xffffffffull), src);
        if (!ok) continue;
        const long long slot = (long long)base + __popcll(m & ((1ull << lane) - 1ull));
        if (slot < list2_cap) { /* list2_cap: entries per segment, as for the own-level list this is a subset of: never binds */
            sift3d_survivor2 e; /* the third phase walks its list one entry per wavefront: the divisions are done here, per lane */
            e.x = (int)(sv.idx % X);
            e.y = (int)((sv.idx / X) % Y);
            e.z = (int)(sv.idx / XY);
            e.is_max = mx ? 1 : 0;
            e.value = c;
            e.h = hval;
            list2[(long long)seg * list2_cap + slot] = e;
        }
        continue;
    } else {
        if (ok && dnext) {
            for (int dz = -1; dz <= 1 && ok; dz++) {
                float q[9];
#pragma unroll
                for (int k = 0; k < 9; k++) q[k] = (dz == 0 && k == 4) ? lval : dnext[sv.idx + dz * XY + (k / 3 - 1) * X + (k % 3 - 1)];
#pragma unroll
                for (int k = 0; k < 9; k++) ok = ok && (mx ? (q[k] < c) : (q[k] > c));
            }
        }
        if (!ok) continue;
        ex_emit(keys, vals, count, cap, lvl_id, mx, sv.idx, c, hval, dnext ? lval : 0.0f);
    }
    }
}

/* Third phase of a level whose upper neighbour is not stored (the last detection level of an octave): the level above
 * would be D_next = G - blur(G), with blur(G) a Gaussian level nothing else ever reads.  The reference filters the whole
 * volume for it (R/src_common/MultiScale.cpp:405-413) and then looks at 27 voxels around each candidate
 * (validateDifference*3D, :1135-1318); here only those 27 voxels are computed, from the (2R+3)^3 block of G around the
 * candidate, with the operations of the full filter in its order: x pass, y pass, z pass, each output = 0, then
 * + f[j] * input in ascending j with a separate multiply and add, inputs outside the volume read as zero
 * (blur_3d_simpleborders, R/src_common/GaussBlur3D.cpp:329-479) -- the same bits as blur_fused_ring_kernel /
 * blur_x_kernel + blur_col_kernel produce for those voxels.
 *
 * One 64-lane workgroup per candidate, taken from the list in a grid-stride loop (the list length is only known on the
 * device).  The kernel is bound by instruction issue (a 512^3 volume has ~22 000 such candidates on its finest octave,
 * ~150 million filter taps), so: the whole block is requested at once through buffer loads (plane base in the descriptor,
 * 32-bit offsets, out-of-volume lanes and planes answered with zeros by the bounds check -- no address arithmetic, no
 * selects) and consumed as it arrives; the x pass takes TWO planes per step as packed pairs (3 (2R+3) lanes, one 8-byte
 * LDS read + one packed multiply + one packed add per tap); then the y pass over all planes (9 (2R+3) outputs), the z
 * pass (27 outputs) and the comparison on 27 lanes. */
typedef float ex_v2f __attribute__((ext_vector_type(2)));
template <int R>
__global__ __launch_bounds__(64) void extrema_validate_lazy_kernel(const float *__restrict__ g, int X, int Xl, int Y, int Z,
                                                                  const sift3d_survivor2 *__restrict__ list,
                                                                  const unsigned long long *__restrict__ list_count, long long list_cap, int lvl_id,
                                                                  unsigned long long *__restrict__ keys, sift3d_cval *__restrict__ vals,
                                                                  unsigned long long *count, long long cap, sift3d_taps t)
{
    constexpr int U = 2 * R + 1, W = 2 * R + 3, PL = W * W, NLD = (PL + 63) / 64, NP = (W + 1) / 2;
    static_assert(3 * W <= 64, "the x pass of a plane pair fits one wavefront");
    __shared__ ex_v2f raw[2][PL];
    __shared__ float t1[2 * NP * W * 3]; /* [plane][row][dx] (one spare plane: W is odd) */
    __shared__ float t2[W * 9];          /* [plane][dy][dx] */
    const int lane = threadIdx.x;
    /* the list comes in EX_SEGS segments of list_cap entries, one per slab of z (lane = segment): position p of the
     * whole list, segments in order, is entry p - before[s] of the segment s with before[s] <= p < before[s] + len[s] */
    long long len = (long long)list_count[lane];
    len = len < list_cap ? len : list_cap;
    long long before = len; /* inclusive prefix sum over the 64 lanes */
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long up = __shfl_up(before, d, 64);
        if (lane >= d) before += up;
    }
    const long long n = __shfl(before, 63, 64);
    before -= len;
    const long long XY = (long long)X * Y;
    const int plane_bytes = (int)(XY * 4); /* the launcher keeps X * Y below 2^29 */
    /* Which candidates a workgroup takes.  The list is in slabs of z (its segments, in order), and consecutive workgroups
     * land on consecutive XCDs: handing out candidate i to workgroup i mod gridDim spreads every slab over all eight L2s,
     * each of which then fetches the same lines of the level.  Instead XCD x (workgroups x, x + 8, ...) walks the x-th
     * eighth of the list in order: its L2 holds one slab's neighbourhood at a time.  (SIFT3D_LAZY_ORDER 0: the round-2 order.) */
#ifndef SIFT3D_LAZY_ORDER
#define SIFT3D_LAZY_ORDER 1
#endif
    const long long nxcd = (gridDim.x & 7u) == 0 && SIFT3D_LAZY_ORDER ? 8 : 1;
    const long long share = (n + nxcd - 1) / nxcd, first_i = (long long)(blockIdx.x % nxcd) * share;
    const long long last_i = first_i + share < n ? first_i + share : n;
    for (long long i = first_i + blockIdx.x / nxcd; i < last_i; i += gridDim.x / nxcd) {
        const int sg = __popcll(__ballot(before <= i)) - 1; /* before[] ascends: the last segment that starts at or before i */
        const long long first = __shfl(before, sg, 64);
        const sift3d_survivor2 e = list[(long long)sg * list_cap + (i - first)];
        const int x = __builtin_amdgcn_readfirstlane(e.x), y = __builtin_amdgcn_readfirstlane(e.y), z = __builtin_amdgcn_readfirstlane(e.z);
        const bool mx = __builtin_amdgcn_readfirstlane(e.is_max) != 0;
        const float c = e.value;
        /* byte offsets of this lane's elements inside a plane; outside the volume: beyond any record count */
        unsigned eoff[NLD];
#pragma unroll
        for (int k = 0; k < NLD; k++) {
            const int el = lane + 64 * k;
            const int gy = y + el / W - (R + 1), gx = x + el % W - (R + 1);
            eoff[k] = (el < PL && gy >= 0 && gy < Y && gx >= 0 && gx < Xl) ? (unsigned)(gy * X + gx) * 4u : 0xFFFFFFFFu;
        }
        float nx[2 * NP][NLD];
#pragma unroll
        for (int pz = 0; pz < 2 * NP; pz++) {
            const int gz = z + pz - (R + 1);
            const bool zin = pz < W && gz >= 0 && gz < Z; /* wave-uniform */
            const __amdgpu_buffer_rsrc_t rs =
                __builtin_amdgcn_make_buffer_rsrc((void *)(g + (zin ? (long long)gz * XY : 0ll)), 0, zin ? plane_bytes : 0, EX_RSRC_FLAGS);
#pragma unroll
            for (int k = 0; k < NLD; k++) nx[pz][k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, (int)eoff[k], 0, 0));
        }
#pragma unroll
        for (int pp = 0; pp < NP; pp++) {
            ex_v2f *rb = raw[pp & 1]; /* two buffers: the x pass of a pair overlaps the arrival of the next */
#pragma unroll
            for (int k = 0; k < NLD; k++)
                if (lane + 64 * k < PL) {
                    ex_v2f v;
                    v.x = nx[2 * pp][k];
                    v.y = nx[2 * pp + 1][k];
                    rb[lane + 64 * k] = v;
                }
            __syncthreads();
            if (lane < 3 * W) {
                const int row = lane / 3, dx = lane % 3;
                ex_v2f acc = ex_v2f(0.0f);
#pragma unroll
                for (int j = 0; j < U; j++) acc = acc + ex_v2f(t.f[j]) * rb[row * W + dx + j];
                t1[((2 * pp) * W + row) * 3 + dx] = acc.x;
                t1[((2 * pp + 1) * W + row) * 3 + dx] = acc.y;
            }
        }
        __syncthreads();
        for (int o = lane; o < W * 9; o += 64) {
            const int pz = o / 9, dy = (o / 3) % 3, dx = o % 3;
            float acc = 0.0f;
#pragma unroll
            for (int j = 0; j < U; j++) acc = acc + t.f[j] * t1[(pz * W + dy + j) * 3 + dx];
            t2[o] = acc;
        }
        __syncthreads();
        bool ok = true;
        float dcen = 0.0f;
        const long long idx = (long long)z * XY + (long long)y * X + x;
        if (lane < 27) {
            const int dz = lane / 9, dy = (lane / 3) % 3, dx = lane % 3;
            float acc = 0.0f;
#pragma unroll
            for (int j = 0; j < U; j++) acc = acc + t.f[j] * t2[(dz + j) * 9 + dy * 3 + dx];
            const float d = g[idx + (long long)(dz - 1) * XY + (long long)(dy - 1) * X + (dx - 1)] - acc;
            ok = mx ? (d < c) : (d > c);
            dcen = d;
        }
        const bool all = __ballot(!ok) == 0ull;
        const float lval = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, dcen), 13));
        if (all && lane == 0) ex_emit(keys, vals, count, cap, lvl_id, mx, idx, c, e.h, lval);
        __syncthreads(); /* raw / t1 / t2 are free for the next candidate */
    }
}

/* Fallback for row lengths that are not a multiple of 4 (no aligned 16-byte rows) and for tiny volumes:
 * lanes along x, 27 direct loads per voxel, wavefront-wide early-out.  The body serves one detection level; the second
 * kernel below runs the three detection levels of an octave in one launch (blockIdx.z = level * planes + plane). */
__device__ __forceinline__ void extrema_generic_body(const float *__restrict__ dprev, const float *__restrict__ dcur, const float *__restrict__ dnext,
                                                     int X, int Xl, int Y, int z, int lvl_id, unsigned long long *__restrict__ keys,
                                                     sift3d_cval *__restrict__ vals, unsigned long long *count, long long cap)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const bool inside = (x >= 1 && x < Xl - 1 && y >= 1 && y < Y - 1);
    const long long XY = (long long)X * Y;
    const long long idx = (long long)z * XY + (long long)y * X + x;
    bool mx = inside, mn = inside;
    float c = 0.0f;
    if (inside) c = dcur[idx];
#pragma unroll
    for (int dz = -1; dz <= 1; dz++) {
        if (inside) {
#pragma unroll
            for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                for (int dx = -1; dx <= 1; dx++) {
                    if (dz == 0 && dy == 0 && dx == 0) continue;
                    float v = dcur[idx + dz * XY + dy * X + dx];
                    mx = mx && (v < c);
                    mn = mn && (v > c);
                }
        }
        if (!__any(mx || mn)) return;
    }
    if (mx || mn) {
        const float *lv[2] = {dprev, dnext};
        for (int l = 0; l < 2; l++) {
            const float *d = lv[l];
            if (!d) continue;
            for (int dz = -1; dz <= 1 && (mx || mn); dz++)
                for (int dy = -1; dy <= 1; dy++)
                    for (int dx = -1; dx <= 1; dx++) {
                        float v = d[idx + dz * XY + dy * X + dx];
                        mx = mx && (v < c);
                        mn = mn && (v > c);
                    }
        }
    }
    if (mx || mn) ex_emit(keys, vals, count, cap, lvl_id, mx, idx, c, dprev[idx], dnext ? dnext[idx] : 0.0f);
}

__global__ __launch_bounds__(256) void extrema_generic_kernel(const float *__restrict__ dprev, const float *__restrict__ dcur,
                                                              const float *__restrict__ dnext, int X, int Xl, int Y, int Z, int z_first, int lvl_id,
                                                              unsigned long long *__restrict__ keys, sift3d_cval *__restrict__ vals,
                                                              unsigned long long *count, long long cap)
{
    extrema_generic_body(dprev, dcur, dnext, X, Xl, Y, (int)blockIdx.z + z_first, lvl_id, keys, vals, count, cap);
}

struct ex_octave5 {
    const float *d[5]; /* the five DoG levels of an octave: detection level l tests d[l + 1] against d[l] and d[l + 2] */
};
__global__ __launch_bounds__(256) void extrema_generic_octave_kernel(ex_octave5 o, int X, int Xl, int Y, int Z, int lvl_id0, unsigned long long *__restrict__ keys,
                                                                     sift3d_cval *__restrict__ vals, unsigned long long *count, long long cap)
{
    const int planes = Z - 2, l = (int)blockIdx.z / planes, z = 1 + (int)blockIdx.z % planes;
    extrema_generic_body(o.d[l], o.d[l + 1], o.d[l + 2], X, Xl, Y, z, lvl_id0 + l, keys, vals, count, cap);
}

/* First phase for the volumes that sift3d_volume_needs_strict flags: the 26 own-level comparisons one by one, as the
 * reference makes them (a NaN neighbour fails both "v < c" and "v > c"; MultiScale.cpp:2408-2524), appended to the same
 * segmented own-level list as the march -- one thread per voxel, 64 x 4 voxels of one plane per workgroup, blockIdx.y =
 * the plane -- so that the second phase, which already compares element by element, is the same launch.  Never taken for
 * finite volumes of ordinary magnitude: those keep the march and its instruction stream. */
__global__ __launch_bounds__(256) void extrema_strict_kernel(const float *__restrict__ dcur, int X, int Xl, int Y, int z_first, int xblocks,
                                                             sift3d_survivor *__restrict__ surv, unsigned long long *surv_count, long long surv_cap)
{
    const int x = (int)(blockIdx.x % (unsigned)xblocks) * 64 + (threadIdx.x & 63);
    const int y = (int)(blockIdx.x / (unsigned)xblocks) * 4 + (threadIdx.x >> 6);
    const int z = z_first + (int)blockIdx.y;
    if (x < 1 || x >= Xl - 1 || y < 1 || y >= Y - 1) return;
    const long long XY = (long long)X * Y;
    const long long idx = (long long)z * XY + (long long)y * X + x;
    const float c = dcur[idx];
    bool mx = true, mn = true;
#pragma unroll
    for (int dz = -1; dz <= 1; dz++)
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                if (dz == 0 && dy == 0 && dx == 0) continue;
                const float v = dcur[idx + dz * XY + dy * X + dx];
                mx = mx && (v < c);
                mn = mn && (v > c);
            }
    if (mx || mn) ex_append_own(surv, surv_count, surv_cap, ex_my_segment(), idx, c, mx);
}

/* !(|v| <= FLT_MAX / 4) is true for NaN, for +-inf and for magnitudes the pyramid's arithmetic could overflow */
__host__ __device__ __forceinline__ bool strict_value(float v) { return !(fabsf(v) <= 3.4028234663852886e38f / 4.0f); }

__global__ __launch_bounds__(256) void scan_strict_kernel(const float *__restrict__ v, long long n, unsigned *flag)
{
    bool bad = false;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) bad = bad || strict_value(v[i]);
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}

hipError_t sift3d_launch_scan_strict(hipStream_t s, const float *v, int64_t n, unsigned *flag)
{
    if (n <= 0) return hipSuccess;
    const long long blocks = (n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096;
    hipLaunchKernelGGL(scan_strict_kernel, dim3((unsigned)blocks), dim3(256), 0, s, v, (long long)n, flag);
    return hipGetLastError();
}

bool sift3d_volume_needs_strict(const float *v, int64_t n)
{
    for (int64_t i = 0; i < n; i++)
        if (strict_value(v[i])) return true;
    return false;
}

/* ---- launchers ---- */
/* The three detection levels of an octave of at most SIFT3D_TINY_VOX voxels, all five DoG levels stored, in one launch
 * (the per-level path is two to three launches per level: fifteen small launches at the very end of the pyramid's chain
 * for the three smallest octaves of a 512^3 volume). */
hipError_t sift3d_launch_extrema_octave_small(hipStream_t s, const float *const d[5], int64_t X, int64_t Xl, int64_t Y, int64_t Z,
                                              int lvl_id0, const cand_target &out)
{
    if (Xl < 3 || Y < 3 || Z < 3) return hipSuccess;
    ex_octave5 o;
    for (int i = 0; i < 5; i++) o.d[i] = d[i];
    dim3 grid((unsigned)((X + 63) / 64), (unsigned)((Y + 3) / 4), (unsigned)(3 * (Z - 2)));
    hipLaunchKernelGGL(extrema_generic_octave_kernel, grid, dim3(256), 0, s, o, (int)X, (int)Xl, (int)Y, (int)Z, lvl_id0, out.keys, out.vals,
                       out.count, (long long)out.cap);
    return hipGetLastError();
}

/* the second launch covers the list capacity, reads the true length on the device, and flags an overflow for cand_finalize
 * to widen the list and replay */
template <bool PAIR, bool DEFER>
static void launch_validate(hipStream_t s, const sift3d_extrema_pass &a, const extrema_plan &p)
{
    const sift3d_extrema_lazy *lz = a.lazy;
    hipLaunchKernelGGL((extrema_validate_kernel<PAIR, DEFER>), dim3(p.vgrid.x, p.vgrid.y), dim3(256), 0, s, a.dprev, PAIR ? lz->prev_b : nullptr,
                       DEFER ? nullptr : a.dnext, (int)a.X, (int)a.Y, a.surv, a.surv_count, p.seg_cap, a.surv_overflow, a.lvl_id, a.out.keys,
                       a.out.vals, a.out.count, (long long)a.out.cap, DEFER ? lz->list2 : nullptr, DEFER ? lz->list2_count : nullptr,
                       p.list2_seg_cap);
}

hipError_t sift3d_launch_extrema(hipStream_t s, const sift3d_extrema_pass &a)
{
    const sift3d_extrema_lazy *lz = a.lazy;
    const bool pair = lz && lz->prev_b, defer = lz && lz->next_g;
    const extrema_plan p = extrema_plan_for(a.X, a.Xl, a.Y, a.Z, a.z_lo, a.z_hi, a.surv != nullptr, a.surv_cap, a.strict, pair, defer,
                                            defer ? lz->ntaps : 0, defer && lz->list2 && lz->list2_count ? lz->list2_cap : 0);
    if (p.status != EX_PLAN_OK)
        return p.status == EX_PLAN_NOTHING ? hipSuccess : (p.status == EX_PLAN_INVALID ? hipErrorInvalidValue : hipErrorNotSupported);
    const dim3 grid(p.grid.x, p.grid.y, p.grid.z);
    const int X = (int)a.X, Xl = (int)a.Xl, Y = (int)a.Y, Z = (int)a.Z;
    if (p.form == EX_FORM_GENERIC) {
        hipLaunchKernelGGL(extrema_generic_kernel, grid, dim3(256), 0, s, a.dprev, a.dcur, a.dnext, X, Xl, Y, Z, p.z0, a.lvl_id, a.out.keys,
                           a.out.vals, a.out.count, (long long)a.out.cap);
        return hipGetLastError();
    }
    if (a.zero_counters) {
        hipError_t e = hipMemsetAsync(a.surv_count, 0, sizeof(unsigned long long) * SIFT3D_SURV_COUNTERS, s);
        if (e != hipSuccess) return e;
    }
    if (p.form == EX_FORM_STRICT)
        hipLaunchKernelGGL(extrema_strict_kernel, grid, dim3(256), 0, s, a.dcur, X, Xl, Y, p.z0, p.tiles_x, a.surv, a.surv_count, p.seg_cap);
    else if (p.form == EX_FORM_MARCH)
        hipLaunchKernelGGL(extrema_march_kernel, grid, dim3(256), 0, s, a.dcur, X, Xl, Y, Z, p.z0, p.z1, p.zchunk, p.tiles_x, p.tiles_y, a.surv,
                           a.surv_count, p.seg_cap);
    else
        hipLaunchKernelGGL(extrema_kernel, grid, dim3(256), 0, s, a.dcur, X, Xl, Y, Z, p.z0, p.z1, p.zchunk, p.tiles_x, a.surv, a.surv_count,
                           p.seg_cap);
    static constexpr decltype(&launch_validate<false, false>) validate[2][2] = {{launch_validate<false, false>, launch_validate<false, true>},
                                                                                 {launch_validate<true, false>, launch_validate<true, true>}};
    validate[p.pair][p.defer](s, a, p);
    if (p.lazy_wgs) { /* a grid-stride loop over a list whose length only the device knows */
        sift3d_taps t;
        for (int i = 0; i < 2 * SIFT3D_FAST_MAX_R + 1; i++) t.f[i] = i < lz->ntaps ? lz->taps[i] : 0.0f;
        hipLaunchKernelGGL(extrema_validate_lazy_kernel<SIFT3D_FAST_MAX_R>, dim3(p.lazy_wgs), dim3(64), 0, s, lz->next_g, X, Xl, Y, Z, lz->list2,
                           lz->list2_count, p.list2_seg_cap, a.lvl_id, a.out.keys, a.out.vals, a.out.count, (long long)a.out.cap, t);
    }
    return hipGetLastError();
}
