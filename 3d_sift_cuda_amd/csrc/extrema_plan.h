/*
 * extrema_plan.h -- the launch plan of an extrema pass (kernels_extrema.hip): which form of the first phase runs for a shape, how
 * the z range is cut into blocks, how many segments of the own-level list are in use and what each holds, the three grids, which
 * (PAIR, DEFER) form of the second phase runs, and the limits of the lazily evaluated neighbour levels.  Every form gives the
 * same lists, so a wrong choice here costs only time, and silently: the choice is written once, in plain host C++ without a HIP
 * include, and tests/extrema_plan_check.cpp prints it for tests/test_extrema_plan.py to hold against a restatement of the rules
 * (as tests/blur_plan_check.cpp does for blur_plan.h).
 */
#ifndef EXTREMA_PLAN_H
#define EXTREMA_PLAN_H

#include <stdint.h>

/* what the kernels and the host share */
#define EX_SEGS 64       /* segments of the own-level extrema list (one atomic counter each) */
#define EX_SEG_STRIDE 32 /* counters 32 x 8 bytes apart: different cache lines / L2 channels */
#define EX_ROWS 2        /* plane-per-block form: output rows per wavefront */
#define EX_XOUT 248      /* ... and output voxels along x: 64 lanes x float4 minus one halo lane each side */
#define EXM_ROWS 4       /* march: by measurement 2, 3 and 4 rows per wavefront (149 / 196 / 234 registers) take the same time; 4 loads least */
#define EXM_XOUT 256     /* march: x per wavefront, 64 lanes x float4, every lane an output lane */

/* The own-level list is cut into EX_SEGS segments, each with its own counter (one returning atomic on a single word
 * saturates near 88 per microsecond chip-wide; the marching kernel appends in batches of 64 or more, so the rate per
 * counter is low).  A segment holds one contiguous range of z: a z block is a plane or a chunk of planes (blockIdx.y of the
 * first phase), so the segments taken in order are the volume taken in slabs -- which is what lets the third phase of a
 * lazily evaluated level walk its candidates slab by slab and find the blocks it reads still in the caches.  With fewer z
 * blocks than segments the segment is the z block, and the list's capacity is divided by the segments in use. */
constexpr int ex_segments_in_use(unsigned z_blocks) { return z_blocks >= EX_SEGS ? EX_SEGS : (int)z_blocks; }
constexpr int ex_segment_of_z_block(unsigned z_block, unsigned z_blocks)
{
    return z_blocks >= EX_SEGS ? (int)(((unsigned long long)z_block * EX_SEGS) / z_blocks) : (int)z_block;
}

/* The limits of the lazy forms (a level below taken as the difference of two Gaussian levels, a level above evaluated around
 * the candidates only).  Shapes (row pitch, rows, slices held) they take: rows of whole 16-byte vectors, a plane below 2^31
 * bytes (32-bit buffer offsets); the pitch is always a multiple of 4 on one device, a slab's rows are its logical rows. */
#define EX_LAZY_MAX_PLANE (1ll << 29)
constexpr bool lazy_shape_ok(int64_t nx, int64_t ny, int64_t nz_local)
{
    return nx % 4 == 0 && nx >= 8 && ny >= 3 && nz_local >= 3 && nx * ny < EX_LAZY_MAX_PLANE;
}
/* the level above the last detection level is always the 17-tap one (sigma 3.09: the schedule of MultiScale.cpp:288-294 does
 * not depend on the input), so that is the one instantiation of the third phase */
#define EX_LAZY_NTAPS 17

enum extrema_form { EX_FORM_NONE, EX_FORM_GENERIC, EX_FORM_PLANE, EX_FORM_MARCH, EX_FORM_STRICT };
enum extrema_status { EX_PLAN_NOTHING, EX_PLAN_OK, EX_PLAN_NOT_SUPPORTED, EX_PLAN_INVALID };

/* the third phase's filter and second list: an odd length up to 17 taps and a list that holds something, or the request is
 * invalid; of the valid lengths only 17 is built */
constexpr extrema_status extrema_lazy_status(int ntaps, int64_t X, int64_t Y, int64_t list2_cap)
{
    if (ntaps < 3 || ntaps > EX_LAZY_NTAPS || !(ntaps & 1) || list2_cap <= 0 || X * Y >= EX_LAZY_MAX_PLANE) return EX_PLAN_INVALID;
    return ntaps != EX_LAZY_NTAPS ? EX_PLAN_NOT_SUPPORTED : EX_PLAN_OK;
}

struct ex_grid {
    unsigned x, y, z;
};
struct extrema_plan {
    extrema_status status; /* anything but EX_PLAN_OK: nothing is launched */
    extrema_form form;
    int z0, z1;           /* planes searched: [z0, z1) */
    int zchunk;           /* planes per z block */
    unsigned z_blocks;
    int segments;         /* of the own-level list in use (0: the generic form has no lists) */
    long long seg_cap;    /* entries per segment */
    int tiles_x, tiles_y; /* first phase: march 256 x (4 wavefronts x EXM_ROWS), plane EX_XOUT x EX_ROWS, strict and generic 64 x 4 */
    ex_grid grid;         /* first phase */
    ex_grid vgrid;        /* second phase: extrema_validate_kernel<pair, defer> */
    bool pair, defer;
    unsigned lazy_wgs;       /* third phase: single-wavefront workgroups (0: none) */
    long long list2_seg_cap; /* ... and entries per segment of the second list */
};

/* X: row pitch (== Xl for a dense volume), Xl: logical row length; interior planes 1 .. Z-2, further restricted to [z_lo, z_hi)
 * (Z-slab mode keeps only its own slices).  have_own_list / surv_cap: the own-level list offered; without one, and for rows
 * that are no whole 16-byte vectors, the generic form tests every voxel in one launch.  pair / defer: the level below / above
 * is not stored (sift3d_extrema_lazy); lazy_ntaps / list2_cap are looked at under defer only. */
constexpr extrema_plan extrema_plan_for(int64_t X, int64_t Xl, int64_t Y, int64_t Z, int z_lo, int z_hi, bool have_own_list, int64_t surv_cap,
                                        bool strict, bool pair, bool defer, int lazy_ntaps, int64_t list2_cap)
{
    extrema_plan p = {}; /* nothing to do, no form */
    const int z0 = z_lo > 1 ? z_lo : 1, z1 = z_hi < (int)Z - 1 ? z_hi : (int)Z - 1;
    if (Xl < 3 || Y < 3 || Z < 3 || z1 <= z0) return p;
    p.z0 = z0;
    p.z1 = z1;
    p.pair = pair;
    p.defer = defer;
    const int bx = (int)((X + 63) / 64), by = (int)((Y + 3) / 4); /* strict and generic: a workgroup takes 64 x 4 voxels of a plane */
    if (!(X % 4 == 0 && X >= 8 && have_own_list && surv_cap > 0)) {
        p.form = EX_FORM_GENERIC;
        p.status = pair || defer ? EX_PLAN_NOT_SUPPORTED : EX_PLAN_OK; /* the caller keeps such shapes on stored DoG levels */
        p.zchunk = 1;
        p.z_blocks = (unsigned)(z1 - z0);
        p.tiles_x = bx;
        p.tiles_y = by;
        p.grid = {(unsigned)bx, (unsigned)by, p.z_blocks};
        return p;
    }
    /* marching form when chunks of >= 8 planes still give the chip a few thousand wavefronts (a wavefront of the march
     * takes EXM_ROWS rows, the four of a workgroup are neighbours in y); its buffer descriptor covers a chunk and the two
     * planes around it, which must stay below 4 GiB */
    const int xtiles_m = (int)((X + EXM_XOUT - 1) / EXM_XOUT);
    const int ytiles_m = (int)((Y - 2 + EXM_ROWS - 1) / EXM_ROWS), ygroups = (ytiles_m + 3) / 4;
    const long long waves_m = (long long)xtiles_m * ytiles_m;
    const long long plane_bytes = X * Y * 4;
    /* the longest chunk that still gives the chip 2 048 wavefronts (two per SIMD: what the kernel's registers allow) --
     * 512^3: 64 planes, 256^3: 8 --, else the longest that gives 512 (128^3: 8); below that the plane-per-block form */
    int zchunk = 1;
    for (int need = 2048; need >= 512 && zchunk == 1 && !strict; need /= 4) /* the strict form takes one plane per block */
        for (int zc = 64; zc >= 8; zc /= 2)
            if (waves_m * ((z1 - z0 + zc - 1) / zc) >= need && (zc + 2) * plane_bytes < (1ll << 32)) {
                zchunk = zc;
                break;
            }
    p.zchunk = zchunk;
    p.z_blocks = (unsigned)((z1 - z0 + zchunk - 1) / zchunk);
    p.segments = ex_segments_in_use(p.z_blocks);
    p.seg_cap = surv_cap / p.segments;
    p.form = strict ? EX_FORM_STRICT : (zchunk >= 2 ? EX_FORM_MARCH : EX_FORM_PLANE);
    p.tiles_x = strict ? bx : (zchunk >= 2 ? xtiles_m : (int)((X - 2 + EX_XOUT - 1) / EX_XOUT));
    p.tiles_y = strict ? by : (zchunk >= 2 ? ygroups : (int)((Y - 2 + EX_ROWS - 1) / EX_ROWS));
    const long long tiles = (long long)p.tiles_x * p.tiles_y; /* the plane form's are a wavefront's: four to a workgroup */
    p.grid = {(unsigned)(p.form == EX_FORM_PLANE ? (tiles + 3) / 4 : tiles), p.z_blocks, 1};
    /* the second launch covers the list capacity and reads the true length on the device */
    p.vgrid = {(unsigned)((p.seg_cap + 255) / 256), (unsigned)p.segments, 1};
    p.status = EX_PLAN_OK;
    if (defer) {
        p.status = extrema_lazy_status(lazy_ntaps, X, Y, list2_cap);
        if (p.status != EX_PLAN_OK) return p;
        /* a grid-stride loop over a list whose length only the device knows: enough single-wavefront workgroups to fill
         * the chip (256 CUs x 16), never more than the list can hold */
        long long wgs = X * Y * Z / 2048; /* the finest octaves fill the chip; a coarse one does not pay for 4096 idle workgroups */
        wgs = wgs < 64 ? 64 : (wgs > 4096 ? 4096 : wgs);
        if (wgs > list2_cap) wgs = list2_cap;
        if (wgs >= 8) wgs = wgs / 8 * 8; /* whole rounds of the eight XCDs: the kernel gives each an eighth of the list */
        p.lazy_wgs = (unsigned)wgs;
        p.list2_seg_cap = list2_cap / p.segments;
    }
    return p;
}

#endif
