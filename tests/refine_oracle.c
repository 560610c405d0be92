/*
 * refine_oracle.c -- independent CPU restatement of the guided search of the re-matching step, for
 * tests/test_refine_cpu.py and tests/test_gpu_refine.py (compiled by tests/refine_cases.py with cc -O2 -ffp-contract=off into
 * a temporary directory and loaded with ctypes).  Written from the contract, not from the product's sources: a serial brute
 * force over ALL fixed records, no spatial index.
 *
 * For every moving record m and every fixed record f, the pair passes when, in float and in this order of operations:
 *   - the line flags (0x100 of info) are equal;
 *   - r = f.scale / (m.scale * s) satisfies lo <= r <= hi;
 *   - q = s * (rot (x_m - c0)) + c1, each row summed ((r0 d0 + r1 d1) + r2 d2), and ((dx dx + dy dy) + dz dz) < radius * radius
 *     with dx = f.x - q.x.
 * Of the passing f the best two by (squared distance of the 64 rank components as integers, fixed index); -1 / INT32_MAX
 * where there are fewer.
 */
#include <stdint.h>

typedef struct {
    float x, y, z, scale;
    float ori[9];
    float eigs[3];
    uint32_t info;
    float pc[64];
} Rec;

void orf_predict(const float *p, const float *c0, const float *c1, const float *rot, float s, float *q)
{
    const float d0 = p[0] - c0[0], d1 = p[1] - c0[1], d2 = p[2] - c0[2];
    for (int r = 0; r < 3; r++) {
        const float o = (rot[3 * r] * d0 + rot[3 * r + 1] * d1) + rot[3 * r + 2] * d2;
        q[r] = c1[r] + o * s;
    }
}

int orf_search(const Rec *fixed, int64_t nf, const Rec *moving, int64_t nm, const float *c0, const float *c1, const float *rot, float s, float radius,
               float lo, float hi, int32_t *o_i1, int32_t *o_d1, int32_t *o_i2, int32_t *o_d2)
{
    const float rr = radius * radius;
    for (int64_t m = 0; m < nm; m++) {
        const Rec *a = &moving[m];
        const float p[3] = {a->x, a->y, a->z};
        float q[3];
        orf_predict(p, c0, c1, rot, s, q);
        const float ms = a->scale * s;
        int32_t i1 = -1, d1 = INT32_MAX, i2 = -1, d2 = INT32_MAX;
        for (int64_t j = 0; j < nf; j++) {
            const Rec *b = &fixed[j];
            if ((a->info & 0x100u) != (b->info & 0x100u)) continue;
            const float r = b->scale / ms;
            if (!(r >= lo && r <= hi)) continue;
            const float dx = b->x - q[0], dy = b->y - q[1], dz = b->z - q[2];
            if (!((dx * dx + dy * dy) + dz * dz < rr)) continue;
            int32_t d = 0;
            for (int c = 0; c < 64; c++) {
                const int32_t e = (int32_t)a->pc[c] - (int32_t)b->pc[c];
                d += e * e;
            }
            if (d < d1 || (d == d1 && j < i1)) {
                d2 = d1;
                i2 = i1;
                d1 = d;
                i1 = (int32_t)j;
            } else if (d < d2 || (d == d2 && j < i2)) {
                d2 = d;
                i2 = (int32_t)j;
            }
        }
        o_i1[m] = i1;
        o_d1[m] = d1;
        o_i2[m] = i2;
        o_d2[m] = d2;
    }
    return 0;
}
