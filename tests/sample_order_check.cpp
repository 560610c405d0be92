/*
 * sample_order_check.cpp -- the descriptor kernel's sampling order (3d_sift_cuda_amd/csrc/sample_order.h) on the CPU.
 * Stand-alone (tests/test_sample_order_cpu.py builds it once plain and once under AddressSanitizer +
 * UndefinedBehaviorSanitizer).  Per record (a frame, a scale, a centre, a volume):
 *   - every sample's key lies inside the record's bins, and the bins fit the counters;
 *   - where the sample's position is finite, the key is the one that follows from the cells trilinear (keypoint_device.h)
 *     takes for it: interp_coord per axis, before the slab's z offset is subtracted;
 *   - the counting sort, emulated the way the kernel runs it (packed 16-bit counters, the old value of an add as the rank,
 *     SAMPLE_ORDER_LANES chunks for the prefix), yields a permutation of 0 .. 1330 -- with the samples arriving in index order
 *     and in a shuffled order, as the LDS atomics of two wavefronts may.
 * Then the line model: over finite orthonormal frames in the interior of a 512^3 volume, the 128-byte lines the four lanes of a
 * quad touch in one gather instruction, summed over the quads, the four gathers of a sample and the instructions of a record
 * (64-lane instructions, 128 lanes, three samples per lane per trip) -- for the patch order wave_sample_patch takes from the
 * header, and for the new order.
 * Prints "<family> <records> <bad>" per family and "lines <step> <patch order> <image order>" per step; exits 1 if any record
 * was bad.
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "keypoint_math.h" /* invert3 */
#include "sample_order.h"

#define PD SAMPLE_ORDER_PD
#define PV SAMPLE_ORDER_PV
#define NT SAMPLE_ORDER_LANES

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd32()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 32);
}
static float rndu() { return (float)(rnd32() >> 8) * (1.0f / 16777216.0f); } /* [0, 1) */
static float rnds() { return 2.0f * rndu() - 1.0f; }

static void frame_random(float *f) /* a rotation from a random unit quaternion */
{
    float q[4], n = 0;
    do {
        n = 0;
        for (int i = 0; i < 4; i++) {
            q[i] = rnds();
            n += q[i] * q[i];
        }
    } while (n < 1e-3f || n > 1.0f);
    n = 1.0f / sqrtf(n);
    const float w = q[0] * n, x = q[1] * n, y = q[2] * n, z = q[3] * n;
    f[0] = 1 - 2 * (y * y + z * z); f[1] = 2 * (x * y - z * w);     f[2] = 2 * (x * z + y * w);
    f[3] = 2 * (x * y + z * w);     f[4] = 1 - 2 * (x * x + z * z); f[5] = 2 * (y * z - x * w);
    f[6] = 2 * (x * z - y * w);     f[7] = 2 * (y * z + x * w);     f[8] = 1 - 2 * (x * x + y * y);
}
static void frame_identity(float *f)
{
    for (int i = 0; i < 9; i++) f[i] = (i % 4 == 0) ? 1.0f : 0.0f;
}
static void frame_permutation(float *f) /* an axis permutation with sign flips */
{
    static const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    const int *p = perms[rnd32() % 6];
    for (int i = 0; i < 9; i++) f[i] = 0;
    for (int r = 0; r < 3; r++) f[r * 3 + p[r]] = (rnd32() & 1) ? 1.0f : -1.0f;
}
static void frame_skewed(float *f) /* slightly off an orthonormal one */
{
    frame_random(f);
    for (int i = 0; i < 9; i++) f[i] += 0.05f * rnds();
}
static void frame_nonfinite(float *f)
{
    frame_random(f);
    const float bad[3] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()};
    f[rnd32() % 9] = bad[rnd32() % 3];
}

struct record {
    float inv[9], sc, rad, fx, fy, fz;
    int X, XP, Y, Z;
};

/* the cells trilinear takes (before it subtracts the slab's z offset); false where a coordinate is a NaN */
static bool trilinear_cells(const record &r, const float *o, int &ix, int &iy, int &iz)
{
    if (o[0] != o[0] || o[1] != o[1] || o[2] != o[2]) return false;
    float w;
    interp_coord(o[0], 0, (float)r.X, ix, w);
    interp_coord(o[1], 0, (float)r.Y, iy, w);
    interp_coord(o[2], 0, (float)r.Z, iz, w);
    return true;
}

/* the counting sort as the kernel runs it; arrival[i]: the i-th sample to reach its counter.  false: not a permutation, or a
 * key outside the bins, or a key that is not the one of trilinear's cells */
static bool sort_record(const record &r, const int *arrival, unsigned short *order)
{
    static sample_order_scratch so;
    static unsigned tmp[PV];
    const sample_order_bins b = sample_order_bins_of(r.rad, r.fy, r.fz);
    const int nbins = sample_order_nbins(b);
    if (nbins < 1 || nbins > SAMPLE_ORDER_MAX_BINS || b.ny < 1 || b.nz < 1) return false;
    /* the words the kernel does not clear are poisoned: nothing may read them */
    for (int w = 0; w < SAMPLE_ORDER_WORDS; w++) so.count[w] = w < (nbins + 1) / 2 ? 0u : 0xdeadbeefu;
    for (int i = 0; i <= PV; i++) so.order[i] = 0xffff;
    for (int i = 0; i < PV; i++) {
        const int s = arrival[i];
        float o[3];
        sample_order_position(r.inv, r.sc, r.fx, r.fy, r.fz, s, o);
        const int key = sample_order_key(b, o[1], o[2], r.Y, r.Z);
        if (key < 0 || key >= nbins) return false;
        int ix, iy, iz;
        if (trilinear_cells(r, o, ix, iy, iz)) {
            const int want = (sample_order_rel(iz, b.cz, b.half) >> b.shz) * b.ny + (sample_order_rel(iy, b.cy, b.half) >> b.shy);
            if (want != key || sample_order_cell(o[1], r.Y) != iy || sample_order_cell(o[2], r.Z) != iz) return false;
        }
        unsigned &word = so.count[sample_order_word(key)];
        const unsigned old = word;
        word += sample_order_one(key);
        tmp[s] = ((unsigned)key << 16) | (unsigned)sample_order_field(old, key);
    }
    unsigned total[NT], base = 0;
    int first[NT], last[NT];
    for (int l = 0; l < NT; l++) {
        sample_order_chunk(nbins, l, first[l], last[l]);
        if (first[l] < 0 || last[l] > (nbins + 1) / 2 || first[l] > last[l] || (l > 0 && first[l] != last[l - 1])) return false;
        total[l] = sample_order_chunk_total(so.count, first[l], last[l]);
    }
    if (first[0] != 0 || last[NT - 1] != (nbins + 1) / 2) return false;
    for (int l = 0; l < NT; l++) {
        sample_order_chunk_prefix(so.count, first[l], last[l], base);
        base += total[l];
    }
    if (base != PV) return false;
    for (int s = 0; s < PV; s++) {
        const int slot = sample_order_slot(so.count, (int)(tmp[s] >> 16), (int)(tmp[s] & 0xffffu));
        if (slot < 0 || slot >= PV || so.order[slot] != 0xffff) return false;
        so.order[slot] = (unsigned short)s;
    }
    memcpy(order, so.order, sizeof(unsigned short) * PV);
    return true;
}

/* wave_sample_patch's patch order: the t-th sample taken is patch voxel order[t] */
static void patch_order(const float *inv, unsigned short *order)
{
    const sample_order_strides st = sample_order_patch_strides(inv);
    for (int t = 0; t < PV; t++) order[t] = (unsigned short)sample_order_patch_voxel(t, st);
}

/* 128-byte lines per quad and gather instruction, summed over a record */
static long quad_lines(const record &r, const unsigned short *order)
{
    long lines = 0;
    for (int s0 = 0; s0 < PV; s0 += 3 * NT)      /* a trip */
        for (int u = 0; u < 3; u++)              /* an instruction group: lane l takes sample s0 + l + NT * u */
            for (int q = 0; q < NT / 4; q++)     /* a quad */
                for (int g = 0; g < 4; g++) {    /* one of the sample's four 8-byte gathers */
                    long long seen[8];
                    int n = 0;
                    for (int l = 0; l < 4; l++) {
                        const int t = s0 + q * 4 + l + NT * u;
                        if (t >= PV) continue;
                        float o[3];
                        sample_order_position(r.inv, r.sc, r.fx, r.fy, r.fz, order[t], o);
                        if (o[0] < 0 || o[0] >= r.X) continue;
                        int ix, iy, iz;
                        if (!trilinear_cells(r, o, ix, iy, iz)) continue;
                        const long long a = ((long long)(iz + (g >> 1)) * r.Y + (iy + (g & 1))) * r.XP + ix;
                        for (int e = 0; e < 2; e++) { /* the two floats may lie in two lines */
                            const long long line = (a + e) >> 5;
                            bool have = false;
                            for (int i = 0; i < n; i++) have = have || seen[i] == line;
                            if (!have) seen[n++] = line;
                        }
                    }
                    lines += n;
                }
    return lines;
}

int main()
{
    struct {
        const char *name;
        void (*make)(float *);
        int n;
    } families[] = {{"orthonormal", frame_random, 2000}, {"identity", frame_identity, 200}, {"permutation", frame_permutation, 400},
                    {"skewed", frame_skewed, 1000}, {"nonfinite", frame_nonfinite, 600}};
    static const int dims[4][3] = {{48, 40, 36}, {45, 37, 33}, {512, 512, 512}, {64, 64, 640}};
    static unsigned short order[PV];
    int arrival[PV];
    int any_bad = 0;
    for (auto &fam : families) {
        int bad = 0;
        for (int k = 0; k < fam.n; k++) {
            record r;
            float f[9];
            fam.make(f);
            invert3(f, r.inv);
            const int *d = dims[k % 4];
            r.X = d[0]; r.Y = d[1]; r.Z = d[2];
            r.XP = (r.X + 3) & ~3;
            const float scale = k % 7 == 0 ? 0.5f : (k % 7 == 1 ? 8.0f : 0.5f + 7.5f * rndu());
            r.rad = 2.0f * scale;
            r.sc = r.rad / (float)(PD / 2);
            const float dim[3] = {(float)r.X, (float)r.Y, (float)r.Z};
            float c[3];
            for (int a = 0; a < 3; a++) {
                const int where = (k / 4 + a) % 3; /* interior, within a radius of the low face, of the high face */
                const float reach = r.rad < dim[a] / 2 ? r.rad : dim[a] / 2;
                c[a] = where == 0 ? reach + (dim[a] - 2 * reach) * rndu() : (where == 1 ? reach * rndu() : dim[a] - reach * rndu());
            }
            /* the last volume is a slab context's octave: Z slices of which a slab holds some; the centre deep inside it */
            if (k % 4 == 3) c[2] = 300.0f + 200.0f * rndu();
            r.fx = c[0]; r.fy = c[1]; r.fz = c[2];
            for (int i = 0; i < PV; i++) arrival[i] = i;
            bool ok = sort_record(r, arrival, order);
            for (int i = PV - 1; i > 0; i--) { /* a shuffled arrival */
                const int j = (int)(rnd32() % (uint32_t)(i + 1)), t = arrival[i];
                arrival[i] = arrival[j];
                arrival[j] = t;
            }
            ok = sort_record(r, arrival, order) && ok;
            if (!ok) bad++;
        }
        printf("%s %d %d\n", fam.name, fam.n, bad);
        any_bad |= bad;
    }
    {   /* a centre and a radius that hold anything */
        const float odd[5] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), 3e38f, -1e30f};
        int bad = 0, n = 0;
        for (int i = 0; i < 5; i++)
            for (int j = 0; j < 4; j++) {
                record r;
                float f[9];
                frame_random(f);
                invert3(f, r.inv);
                r.X = 48; r.Y = 40; r.Z = 36; r.XP = 48;
                r.rad = j == 0 ? odd[i] : 6.0f;
                r.sc = r.rad / (float)(PD / 2);
                r.fx = j == 1 ? odd[i] : 20.0f;
                r.fy = j == 2 ? odd[i] : 20.0f;
                r.fz = j == 3 ? odd[i] : 20.0f;
                for (int t = 0; t < PV; t++) arrival[t] = PV - 1 - t;
                if (!sort_record(r, arrival, order)) bad++;
                n++;
            }
        printf("odd_record %d %d\n", n, bad);
        any_bad |= bad;
    }
    /* the line model */
    static unsigned short porder[PV];
    const float steps[2] = {1.3f, 2.6f};
    for (float step : steps) {
        double sum_patch = 0, sum_image = 0;
        const int frames = 40;
        for (int k = 0; k < frames; k++) {
            record r;
            float f[9];
            frame_random(f);
            invert3(f, r.inv);
            r.X = r.XP = r.Y = r.Z = 512;
            r.sc = step;
            r.rad = step * (float)(PD / 2);
            r.fx = 100.0f + 300.0f * rndu(); r.fy = 100.0f + 300.0f * rndu(); r.fz = 100.0f + 300.0f * rndu();
            for (int i = 0; i < PV; i++) arrival[i] = i;
            if (!sort_record(r, arrival, order)) any_bad |= 1;
            patch_order(r.inv, porder);
            sum_patch += (double)quad_lines(r, porder);
            sum_image += (double)quad_lines(r, order);
        }
        printf("lines %.1f %.1f %.1f\n", (double)step, sum_patch / frames, sum_image / frames);
    }
    return any_bad ? 1 : 0;
}
