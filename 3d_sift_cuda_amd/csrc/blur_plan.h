/*
 * blur_plan.h -- the launch plan of the fused blur: whether a blur takes the one-launch form at all, which form of
 * blur_fused_ring_kernel (kernels_blur_fused.hip) runs for a filter, a shape, a set of outputs and the knobs, how the z range is
 * cut into chunks, and which tile order is passed.  Every form gives the same bits, so a wrong choice here costs only time, and
 * silently: the choice is written once, in plain host C++ without a HIP include, and tests/blur_plan_check.cpp prints it for
 * tests/test_blur_plan.py to hold against a restatement of the rules (as tests/crew_check.cpp does for zs_crew.h).
 */
#ifndef BLUR_PLAN_H
#define BLUR_PLAN_H

#include <stdint.h>

#define BLUR_PLAN_MAX_R 8 /* the widest filter the kernel is built for: 17 taps (SIFT3D_FAST_MAX_R) */

/* what sift3d_set_tuning forces; 0 = the plan's own choice */
struct sift3d_blur_tuning {
    int z_chunks;        /* SIFT3D_TUNE_FUSED_CHUNKS */
    int rows_per_thread; /* SIFT3D_TUNE_FUSED_ROWS: 2 = 512 threads, two planes of prefetch; 1 = 1024 threads, one plane */
    int tile;            /* SIFT3D_TUNE_FUSED_TILE: 1 = 64 x 32, 2 = 128 x 16 (two-rows-per-thread mapping, up to 13 taps) */
    int order;           /* SIFT3D_TUNE_FUSED_ORDER: which workgroup takes which tile (0 = by measurement, 1 .. 3: see the kernel) */
    int stagger;         /* SIFT3D_TUNE_FUSED_STAGGER: the second half of a workgroup's wavefronts half a step behind the first (0 = by measurement, 1 = off, 2 = on) */
};

/* a form of the kernel: its template parameters and nothing else */
struct blur_form {
    int R, rows;
    bool has_out, has_dog;
    int pf, tx, ty;
    bool has_sub, stg;
};
constexpr bool operator==(const blur_form &a, const blur_form &b)
{
    return a.R == b.R && a.rows == b.rows && a.has_out == b.has_out && a.has_dog == b.has_dog && a.pf == b.pf && a.tx == b.tx &&
           a.ty == b.ty && a.has_sub == b.has_sub && a.stg == b.stg;
}

/* Is the shape inside the kernel?  Rows must be whole 16-byte vectors, a plane below 2^31 bytes (32-bit buffer offsets), the
 * filter 3 to 17 taps. */
constexpr bool blur_shape_inside(int ntaps, int64_t X, int64_t Y)
{
    return ntaps >= 3 && ntaps <= 2 * BLUR_PLAN_MAX_R + 1 && (ntaps & 1) && X % 4 == 0 && X * Y < (1ll << 29);
}

/* Does a blur of N voxels take the fused launch?  One launch per level where the volume fills the chip (it marches along z with
 * few, fat workgroups); coarse octaves keep the three-pass path.  fmode = SIFT3D_TUNE_BLUR_FUSED: 0 never, 2 wherever the shape
 * allows (tests, A/B timing), 1 by measurement (standalone, tools/bench_blur_ab.sh 128 / 64): below 2^22 voxels the one launch
 * still beats the three for 7 and 9 taps (0.020 / 0.026 against 0.042 / 0.043 ms at 128^3), ties at 11-13 and loses at 17. */
constexpr bool blur_takes_fused(int fmode, int ntaps, double N)
{
    return fmode == 2 || (fmode == 1 && (N >= (double)(1 << 22) || (N >= (double)(1 << 18) && ntaps <= 9)));
}

/* The two mappings, by measurement at 512^3 and 256^3: two rows per thread, two planes of window
 * prefetch and one workgroup per CU up to 13 taps; one row per thread (1024 threads, 128 registers) with one plane for 15
 * and 17 taps, and for every filter below 2^22 voxels, where a volume has fewer tiles than the chip has CUs and sixteen
 * wavefronts per workgroup help.  The knob forces one of the two (tests run both on every shape). */
constexpr int blur_rows(int R, int64_t voxels, int knob)
{
    return knob == 1 || knob == 2 ? knob : ((R >= 7 || voxels < (1ll << 22)) ? 1 : 2);
}

/* Which form runs, given the rows per thread (blur_rows), whether a row holds a 128-wide tile (X >= 128) and whether the shape
 * lets the launch carry the half-size volume (blur_carry_shape). */
constexpr blur_form blur_pick_form(int R, bool out, bool dog, int rows, bool x128, bool carry_shape, int tile, int stagger)
{
    if (rows == 1) return {R, 1, out, dog, 1, 64, 32, false, false};
    const bool both = out && dog;
    /* the half-step stagger of the second half of the wavefronts with one copy of the march per (half, role) -- the kernel's STG:
     * built for the two-rows-per-thread mapping (eight wavefronts, two per SIMD) and the filters the pyramid launches (7 - 13
     * taps).  By measurement at 512^3 (profiles/r06_stagger_ab.txt; ms per launch off -> on): 11 taps + DoG + half-size volume
     * 0.357 - 0.363 -> 0.346 - 0.354, 13 taps + DoG 0.365 - 0.373 -> 0.352 - 0.367, 9 taps + DoG equal (0.300 - 0.307 / 0.297 -
     * 0.305), the two level-only launches 2 - 3 % SLOWER (7 taps 0.201 - 0.203 -> 0.205 - 0.212, 9 taps 0.217 - 0.225 -> 0.220 -
     * 0.228): on from 11 taps up. */
    const bool stg = R >= 3 && R <= 6 && (stagger == 2 || (stagger == 0 && R >= 5));
    /* the half-size volume beside the level (the kernel's HAS_SUB): built for the one filter the pyramid asks it of -- level 3 is
     * 11 taps in every octave (oracle: sigma_extra[3]) -- with both arrays stored; anything else leaves it to the caller, who
     * launches the subsample itself.  128 x 16 under the stagger (round 6, profiles/r06_stagger_ab.txt section 8: 0.354 -> 0.340 -
     * 0.344 ms at 512^3; without the stagger the two tiles measured equal in round 4). */
    if (R == 5 && both && carry_shape) {
        const bool wide5 = (tile == 2 || (tile == 0 && stg)) && x128;
        return {5, 2, true, true, 2, wide5 ? 128 : 64, wide5 ? 16 : 32, true, stg};
    }
    /* tile shape, by measurement at 512^3 (profiles/r04_tile_ab.txt, dense random data, ms per launch 64 x 32 -> 128 x 16): 7 taps
     * level only 0.217 -> 0.201 - 0.207, 9 taps level + DoG 0.333 - 0.337 -> 0.318 - 0.323, 7 taps level + DoG 0.329 - 0.331 ->
     * 0.321 - 0.326; no gain at 11 taps (0.356 - 0.358 both) and a loss where the taller y halo meets more arithmetic or three
     * planes of prefetch: 13 taps 0.364 - 0.368 -> 0.370 - 0.375, 9 taps level only 0.216 - 0.220 -> 0.225 - 0.234 */
    const bool wide = (tile == 2 || (tile == 0 && (R == 3 || (R == 4 && both)))) && R <= 6 && x128;
    /* three planes of window prefetch where the registers are there and only one array is stored (7 and 9 taps, level
     * only: 0.213 / 0.224 ms at 512^3 against 0.225 - 0.232 / 0.233 - 0.237 with two; with the DoG store beside it three planes
     * change nothing: 0.324 / 0.338 against 0.328 / 0.334 - 0.342; four planes, level only: 0.225 / 0.220, no better than three;
     * round 6, under the stagger, whose role copies leave the registers for it: 11 / 13 taps with three planes 0.351 - 0.354 /
     * 0.362 - 0.369 against 0.346 - 0.351 / 0.352 - 0.359 with two; ONE plane: 0.43 / 0.44) */
    return {R, 2, out, dog, R <= 4 && !both ? 3 : 2, wide ? 128 : 64, wide ? 16 : 32, false, stg};
}

/* The launch can write the next octave's level 0 where a half-size volume was offered, the whole volume is produced and rows
 * halve into whole 16-byte vectors. */
constexpr bool blur_carry_shape(bool sub_offered, int64_t X, int64_t Y, int64_t Z, int64_t zo0, int64_t zo1)
{
    return sub_offered && zo0 == 0 && zo1 == Z && X % 8 == 0 && Z >= 2 && Y >= 2;
}

/* the form for output planes [zo0, zo1) of an X x Y x Z volume */
constexpr blur_form blur_choose_form(int R, bool out, bool dog, int64_t X, int64_t Y, int64_t Z, int64_t zo0, int64_t zo1, bool sub_offered,
                                     const sift3d_blur_tuning &k)
{
    return blur_pick_form(R, out, dog, blur_rows(R, X * Y * (zo1 - zo0), k.rows_per_thread), X >= 128,
                          blur_carry_shape(sub_offered, X, Y, Z, zo0, zo1), k.tile, k.stagger);
}

/* The forms worth building are those blur_pick_form can return: candidate i of BLUR_FORM_CANDIDATES walks every combination of
 * template parameters, and one exists when some input picks it.  The kernel table is generated from exactly this. */
#define BLUR_FORM_CANDIDATES (BLUR_PLAN_MAX_R * 2 * 3 * 3 * 2 * 2 * 2)
constexpr blur_form blur_form_candidate(int i)
{
    const int pair = i / 2 % 3; /* level, DoG, both */
    return {1 + i / 144, 1 + i % 2, pair != 1, pair != 0, 1 + i / 6 % 3, i / 18 % 2 ? 128 : 64, i / 18 % 2 ? 16 : 32, i / 36 % 2 != 0, i / 72 % 2 != 0};
}
constexpr bool blur_form_exists(const blur_form &f)
{
    for (int x128 = 0; x128 < 2; x128++)
        for (int carry = 0; carry < 2; carry++)
            for (int tile = 0; tile <= 2; tile++)
                for (int stagger = 0; stagger <= 2; stagger++)
                    if (blur_pick_form(f.R, f.has_out, f.has_dog, f.rows, x128, carry, tile, stagger) == f) return true;
    return false;
}

/* How the planes to produce are cut into chunks along z (each recomputes 2R lead-in planes), and the tile order passed. */
struct blur_chunking {
    int tiles_x, tiles_y; /* tiles of the form's shape that cover a plane */
    int zlen, nch;        /* planes per chunk, chunks */
    long long total;      /* workgroups that have a tile: tiles_x * tiles_y * nch (the grid is the next multiple of 8) */
    int order;            /* 1 .. 3, see the kernel */
};

/* chunks along z: enough workgroups to fill every CU's resident slots while the 2R lead-in planes stay cheap */
inline int blur_chunk_count(int R, int64_t Z, long long tiles, int resident, int forced)
{
    if (forced >= 1) return forced;
    /* time ~ rounds of resident workgroups x planes marched per workgroup */
    const double slots = 256.0 * resident;
    int best = 1;
    double best_cost = 0;
    for (int n = 1; n <= 256; n++) {
        const int64_t zlen = (Z + n - 1) / n;
        if (n > 1 && zlen < 4 * R) break;
        const double wgs = (double)tiles * (double)((Z + zlen - 1) / zlen);
        const double cost = (wgs <= slots ? 1.0 : wgs / slots) * (double)(zlen + 2 * R);
        if (n == 1 || cost < best_cost) {
            best = n;
            best_cost = cost;
        }
    }
    return best;
}

/* resident: workgroups of the form one CU holds.  Returns false when the shape is outside the kernel (32-bit buffer offsets: a
 * chunk with its lead-in planes must stay below 4 GiB -- a volume whose planes are that large gets more z chunks, and only a
 * plane pair beyond 4 GiB has none). */
inline bool blur_plan_chunks(const blur_form &f, int64_t X, int64_t Y, int64_t zo0, int64_t zo1, int resident, const sift3d_blur_tuning &k,
                             blur_chunking *c)
{
    const int64_t max_planes = (int64_t)0xFFFFFFF0ll / (X * Y * 4) - 2 * f.R - 2; /* planes per chunk the offsets can address */
    if (max_planes < 1) return false;
    c->tiles_x = (int)((X + f.tx - 1) / f.tx);
    c->tiles_y = (int)((Y + f.ty - 1) / f.ty);
    const long long tiles = (long long)c->tiles_x * c->tiles_y;
    const int64_t Zo = zo1 - zo0; /* planes to produce */
    int n = blur_chunk_count(f.R, Zo, tiles, resident, k.z_chunks);
    if ((Zo + n - 1) / n > max_planes) n = (int)((Zo + max_planes - 1) / max_planes);
    c->zlen = (int)((Zo + n - 1) / n);
    if (f.has_sub && (c->zlen & 1)) c->zlen++; /* a pair of planes never straddles two chunks (the window starts at plane 0) */
    c->nch = (int)((Zo + c->zlen - 1) / c->zlen);
    c->total = tiles * c->nch;
    /* the column-strip order needs counts that divide: 8 | tiles_x, or tiles_x | 8 with the (y, chunk) list of a column cut
     * evenly over the 8 / tiles_x XCDs that share it; everything else keeps the order of rounds 1 - 4 */
    c->order = k.order == 0 ? 1 : k.order; /* by measurement: see DESIGN.md section 4 (round 5) */
    if (c->order == 3) {
        const long long M = (long long)c->tiles_y * c->nch;
        const bool ok = c->tiles_x >= 8 ? c->tiles_x % 8 == 0 : (8 % c->tiles_x == 0 && M % (8 / c->tiles_x) == 0);
        if (!ok) c->order = 1;
    }
    return true;
}

#endif
