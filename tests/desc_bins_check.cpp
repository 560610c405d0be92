/*
 * desc_bins_check.cpp -- the descriptor's box walk (3d_sift_cuda_amd/csrc/desc_bins.h) on the CPU against the oracle's
 * o3_desc_sift, on patches fed directly.  Stand-alone (tests/test_desc_bins_cpu.py builds it with sift3d_oracle.c, once plain and
 * once under AddressSanitizer + UndefinedBehaviorSanitizer).  Per patch:
 *   - the gradient pre-pass of descriptor_kernel<true>, restated, fills the magnitude and octant arrays the kernel keeps in LDS;
 *   - every one of the 64 lanes walks its box (desc_bins_walk), or all voxels where the patch asks for it (desc_bins_needs_all);
 *   - where the box walk ran, it must equal the chain over all voxels with the zero weights (desc_bins_walk_all) bit for bit:
 *     the bins before normalisation;
 *   - after msNormalizeDataPositive the 64 values must be the oracle's bit for bit (a NaN matches a NaN), and after o3_rank the
 *     ranks must be the oracle's.
 * Prints "<family> <patches> <bad> <walked all>" per family and exits 1 if any patch was bad.
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "desc_bins.h"
#include "sift3d_oracle.h"

#define PD O3_PATCH_DIM
#define PV O3_PATCH_VOX
static_assert(PD == DESC_BINS_PD && DESC_BINS_NI == PD - 2 && DESC_BINS_NINT == DESC_BINS_NI * DESC_BINS_NI * DESC_BINS_NI, "one patch");

/* ---- a small generator (the same patches everywhere) ---- */
static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd32()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 32);
}
static float rndu() { return (float)(rnd32() >> 8) * (1.0f / 16777216.0f); } /* [0, 1) */
static float rnds() { return 2.0f * rndu() - 1.0f; }

/* ---- vec3D_norm_3d / vec3D_mag / vec3D_dot_3d as the kernel has them ---- */
static void v3_norm(float *p)
{
    float ss = p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
    if (ss > 0) {
        float div = (float)(1.0 / (double)sqrtf(ss));
        p[0] *= div;
        p[1] *= div;
        p[2] *= div;
    } else {
        p[0] = 1;
        p[1] = 0;
        p[2] = 0;
    }
}
static float v3_mag(const float *p)
{
    float ss = p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
    if (ss > 0) return sqrtf(ss);
    return 0;
}
static float v3_dot(const float *a, const float *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

/* the kernel's gradient pre-pass; returns whether a voxel asks for the walk over all voxels */
static bool prepass(const float *patch, float *mag, unsigned char *bin)
{
    bool all = false;
    for (int i = 0; i < DESC_BINS_LEN; i++) { /* the two entries a plane leaves unused are never read: poison them */
        mag[i] = std::numeric_limits<float>::quiet_NaN();
        bin[i] = 0;
    }
    for (int q = 0; q < DESC_BINS_NINT; q++) {
        const int x = q % 9 + 1, y = (q / 9) % 9 + 1, z = q / 81 + 1;
        const int s = (z * PD + y) * PD + x;
        float e[3] = {patch[s + 1] - patch[s - 1], patch[s + PD] - patch[s - PD], patch[s + PD * PD] - patch[s - PD * PD]};
        float mg = v3_mag(e);
        int best = DESC_BINS_NONE;
        if (mg > 0) {
            v3_norm(e);
            const float oa[8][3] = {{1, 1, 1}, {1, 1, -1}, {1, -1, 1}, {1, -1, -1}, {-1, 1, 1}, {-1, 1, -1}, {-1, -1, 1}, {-1, -1, -1}};
            best = 0;
            float bd = v3_dot(oa[0], e);
            for (int t = 1; t < 8; t++) {
                float d = v3_dot(oa[t], e);
                if (d > bd) {
                    bd = d;
                    best = t;
                }
            }
        }
        const int en = desc_bins_entry(x, y, z);
        mag[en] = mg;
        bin[en] = (unsigned char)best;
        if (desc_bins_needs_all(mg)) all = true;
    }
    return all;
}

/* msNormalizeDataPositive as the kernel has it: minimum from 100000 (a NaN never wins), one chain of squares in lane order */
static void normalize_positive(float *v)
{
    float mn = 100000;
    for (int i = 0; i < 64; i++)
        if (v[i] < mn) mn = v[i];
    float ss = 0;
    for (int i = 0; i < 64; i++) {
        v[i] = v[i] - mn;
        ss += v[i] * v[i];
    }
    float div = 1.0f / sqrtf(ss);
    for (int i = 0; i < 64; i++) v[i] = v[i] * div;
}

static bool same(float a, float b)
{
    if (a != a || b != b) return a != a && b != b;
    uint32_t ua, ub;
    memcpy(&ua, &a, 4);
    memcpy(&ub, &b, 4);
    return ua == ub;
}

static int g_all; /* patches of the family that walked all voxels */

/* bins from given arrays: the box walk against the chain over everything */
static bool bins_of(const float *mag, const unsigned char *bin, bool all, float *acc)
{
    bool ok = true;
    for (int lane = 0; lane < 64; lane++) {
        const float full = desc_bins_walk_all(mag, bin, lane);
        acc[lane] = all ? full : desc_bins_walk(mag, bin, lane);
        if (!same(acc[lane], full)) ok = false;
    }
    return ok;
}

static bool check_patch(const float *patch)
{
    static o3_feature ft;
    memset(&ft, 0, sizeof ft);
    memcpy(ft.data, patch, sizeof(float) * PV);
    o3_desc_sift(&ft);
    float want[64], want_rank[64];
    memcpy(want, ft.pc, sizeof want);
    memcpy(want_rank, ft.pc, sizeof want);
    o3_rank(want_rank);

    float mag[DESC_BINS_LEN];
    unsigned char bin[DESC_BINS_LEN];
    const bool all = prepass(patch, mag, bin);
    g_all += all;
    float got[64], got_rank[64];
    bool ok = bins_of(mag, bin, all, got);
    normalize_positive(got);
    memcpy(got_rank, got, sizeof got);
    o3_rank(got_rank);
    for (int i = 0; i < 64; i++) ok = ok && same(got[i], want[i]) && same(got_rank[i], want_rank[i]);
    return ok;
}

static int g_bad_total;
static void report(const char *family, int n, int bad)
{
    printf("%s %d %d %d\n", family, n, bad, g_all);
    g_bad_total += bad;
    g_all = 0;
}

int main()
{
    static float p[PV];
    int bad;

    /* random patches, normalised as the pipeline leaves them */
    bad = 0;
    for (int it = 0; it < 400; it++) {
        for (int i = 0; i < PV; i++) p[i] = rnds();
        o3_normalize_patch(p);
        bad += !check_patch(p);
    }
    report("random", 400, bad);

    /* all gradients in one octant: a ramp whose slopes have the octant's signs, with noise too small to turn one */
    bad = 0;
    for (int it = 0; it < 64; it++) {
        const int o = it & 7;
        const float sx = (o & 4) ? -1.0f : 1.0f, sy = (o & 2) ? -1.0f : 1.0f, sz = (o & 1) ? -1.0f : 1.0f;
        const float ax = 0.5f + rndu(), ay = 0.5f + rndu(), az = 0.5f + rndu();
        for (int z = 0; z < PD; z++)
            for (int y = 0; y < PD; y++)
                for (int x = 0; x < PD; x++) p[(z * PD + y) * PD + x] = sx * ax * x + sy * ay * y + sz * az * z + (it < 8 ? 0.0f : 0.05f * rnds());
        o3_normalize_patch(p);
        bad += !check_patch(p);
    }
    report("one_octant", 64, bad);

    /* flat except on a centre plane x, y or z = 5 (and on all three) */
    bad = 0;
    for (int it = 0; it < 64; it++) {
        const int axis = it & 3;
        for (int z = 0; z < PD; z++)
            for (int y = 0; y < PD; y++)
                for (int x = 0; x < PD; x++) {
                    const bool on = axis == 0 ? x == 5 : (axis == 1 ? y == 5 : (axis == 2 ? z == 5 : (x == 5 || y == 5 || z == 5)));
                    p[(z * PD + y) * PD + x] = on ? rnds() : 0.25f;
                }
        bad += !check_patch(p);
    }
    report("centre_planes", 64, bad);

    /* most gradients exactly zero: a constant with a few voxels raised, and plateaus */
    bad = 0;
    for (int it = 0; it < 64; it++) {
        for (int i = 0; i < PV; i++) p[i] = (it & 1) ? (float)((i / 3) % 2) : 0.5f;
        for (int k = 0; k < 1 + it / 4; k++) p[rnd32() % PV] = rnds();
        bad += !check_patch(p);
    }
    report("mostly_zero", 64, bad);

    /* faint patches: the squares of the gradient are denormal or vanish, so magnitudes come out of sqrtf at the bottom of
     * their range (about 3.7e-23: no smaller positive magnitude exists) or as 0 */
    bad = 0;
    {
        const float scales[8] = {1e-17f, 1e-19f, 1e-20f, 1e-21f, 3e-22f, 1e-22f, 3e-23f, 1e-30f};
        for (int it = 0; it < 64; it++) {
            for (int i = 0; i < PV; i++) p[i] = rnds() * scales[it & 7];
            bad += !check_patch(p);
        }
    }
    report("faint", 64, bad);

    /* magnitudes that ARE denormal, planted into the arrays (no patch yields them): mg * 0.5 rounds, and the box walk must
     * still equal the chain over everything bit for bit */
    bad = 0;
    for (int it = 0; it < 200; it++) {
        float mag[DESC_BINS_LEN], acc[64];
        unsigned char bin[DESC_BINS_LEN];
        for (int i = 0; i < DESC_BINS_LEN; i++) {
            const uint32_t bits = (rnd32() & 0x7FFFFFu) >> (rnd32() % 20); /* a denormal, down to a few last bits */
            memcpy(&mag[i], &bits, 4);
            bin[i] = (unsigned char)((it & 1) ? rnd32() % 9 : rnd32() % 8);
            if (bin[i] == DESC_BINS_NONE || mag[i] == 0) { mag[i] = 0; bin[i] = DESC_BINS_NONE; }
        }
        bad += !bins_of(mag, bin, false, acc);
    }
    report("denormal_planted", 200, bad);

    /* all NaN */
    for (int i = 0; i < PV; i++) p[i] = std::numeric_limits<float>::quiet_NaN();
    bad = !check_patch(p);
    report("all_nan", 1, bad);

    /* infinite values without a NaN (what one normalisation by 1 / 0 leaves of a patch whose squares vanish): a magnitude of
     * +Inf with an octant, whose zero-weight terms are NaN -- the walk over all voxels */
    bad = 0;
    for (int it = 0; it < 32; it++) {
        for (int i = 0; i < PV; i++) p[i] = rnds();
        if (it < 8) { /* one infinite voxel next to the patch centre or far from it */
            p[((it < 4 ? 5 : 2) * PD + 5) * PD + 4 + (it & 3)] = std::numeric_limits<float>::infinity();
        } else {
            for (int k = 0; k < it; k++) p[rnd32() % PV] = (rnd32() & 1) ? std::numeric_limits<float>::infinity() : -std::numeric_limits<float>::infinity();
        }
        bad += !check_patch(p);
    }
    report("infinite", 32, bad);

    return g_bad_total ? 1 : 0;
}
