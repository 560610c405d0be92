/*
 * compose_oracle.c -- the CPU oracle of the composition of two alignments, written from the contract in
 * include/sift3d.h: the composite matrix, the composite field node by node and its interpolation residual cell by cell, all
 * serial.  Built by tests/_helpers.c_oracle with -O2 -ffp-contract=off.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define MAX_DISP 128.0

/* Mc = M1 M2 in double, each entry ((a0 b0 + a1 b1) + a2 b2), plus a3 in the last column; rounded to float once */
void ocp_matrix(const float *m1, const float *m2, float *out)
{
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) {
            double s = ((double)m1[4 * r] * (double)m2[c] + (double)m1[4 * r + 1] * (double)m2[4 + c]) + (double)m1[4 * r + 2] * (double)m2[8 + c];
            if (c == 3) s = s + (double)m1[4 * r + 3];
            out[4 * r + c] = (float)s;
        }
    out[12] = out[13] = out[14] = 0.0f;
    out[15] = 1.0f;
}

/* adjugate over determinant, then the translation; -1 for a singular matrix or a last row other than 0 0 0 1 */
static int affine_inverse(const float *m, double *o)
{
    double a[16];
    for (int k = 0; k < 16; k++) a[k] = (double)m[k];
    if (a[12] != 0.0 || a[13] != 0.0 || a[14] != 0.0 || a[15] != 1.0) return -1;
    const double c00 = a[5] * a[10] - a[6] * a[9], c01 = a[6] * a[8] - a[4] * a[10], c02 = a[4] * a[9] - a[5] * a[8];
    const double det = (a[0] * c00 + a[1] * c01) + a[2] * c02;
    if (!(det != 0.0) || !isfinite(det)) return -1;
    o[0] = c00 / det;
    o[1] = (a[2] * a[9] - a[1] * a[10]) / det;
    o[2] = (a[1] * a[6] - a[2] * a[5]) / det;
    o[4] = c01 / det;
    o[5] = (a[0] * a[10] - a[2] * a[8]) / det;
    o[6] = (a[2] * a[4] - a[0] * a[6]) / det;
    o[8] = c02 / det;
    o[9] = (a[1] * a[8] - a[0] * a[9]) / det;
    o[10] = (a[0] * a[5] - a[1] * a[4]) / det;
    for (int r = 0; r < 3; r++) o[4 * r + 3] = -((o[4 * r] * a[3] + o[4 * r + 1] * a[7]) + o[4 * r + 2] * a[11]);
    return 0;
}

typedef struct {
    const float *disp; /* component-major, NULL: no field */
    int64_t n[3];
    float o[3], h;
} field;

static void set_field(field *f, const float *disp, const int64_t *n, const float *o, float h)
{
    memset(f, 0, sizeof *f);
    f->disp = disp;
    f->h = h;
    if (disp)
        for (int k = 0; k < 3; k++) {
            f->n[k] = n[k];
            f->o[k] = o[k];
        }
}

/* the field at a key position: 0 outside the grid; inside, trilinear in float, x then y then z, the upper index clamped.
 * Returns whether the position was inside. */
static int field_at(const field *f, const float y[3], float out[3])
{
    out[0] = out[1] = out[2] = 0.0f;
    if (!f->disp) return 0;
    float g[3], w[3];
    int64_t lo[3], hi[3];
    for (int r = 0; r < 3; r++) {
        g[r] = (y[r] - f->o[r]) / f->h;
        if (!(g[r] >= 0.0f && g[r] <= (float)(f->n[r] - 1))) return 0;
    }
    for (int r = 0; r < 3; r++) {
        const float fl = floorf(g[r]);
        w[r] = g[r] - fl;
        lo[r] = (int64_t)fl;
        hi[r] = lo[r] + 1 < f->n[r] - 1 ? lo[r] + 1 : f->n[r] - 1;
    }
    const int64_t n0 = f->n[0], n1 = f->n[1], N = n0 * n1 * f->n[2];
    const float u0 = 1.0f - w[0], u1 = 1.0f - w[1], u2 = 1.0f - w[2];
    for (int c = 0; c < 3; c++) {
        const float *d = f->disp + c * N;
#define AT(x, y, z) d[((z) * n1 + (y)) * n0 + (x)]
        const float e00 = u0 * AT(lo[0], lo[1], lo[2]) + w[0] * AT(hi[0], lo[1], lo[2]);
        const float e10 = u0 * AT(lo[0], hi[1], lo[2]) + w[0] * AT(hi[0], hi[1], lo[2]);
        const float e01 = u0 * AT(lo[0], lo[1], hi[2]) + w[0] * AT(hi[0], lo[1], hi[2]);
        const float e11 = u0 * AT(lo[0], hi[1], hi[2]) + w[0] * AT(hi[0], hi[1], hi[2]);
#undef AT
        const float a = u1 * e00 + w[1] * e10, b = u1 * e01 + w[1] * e11;
        out[c] = u2 * a + w[2] * b;
    }
    return 1;
}

static void rows(const double *P, const double x[3], double out[3])
{
    for (int r = 0; r < 3; r++) out[r] = ((P[4 * r] * x[0] + P[4 * r + 1] * x[1]) + P[4 * r + 2] * x[2]) + P[4 * r + 3];
}

/* t = phi2(phi1(y)), c = inv(Mc') y at the float position y; returns bits 0 and 1 of the status word */
static uint32_t chain(const double *P1, const double *P2, const double *Pc, const field *f1, const field *f2, const float yf[3], double t[3], double c[3])
{
    const double y[3] = {(double)yf[0], (double)yf[1], (double)yf[2]};
    double a[3], s[3], b[3];
    float v[3], sf[3];
    uint32_t st = 0;
    rows(P1, y, a);
    if (!field_at(f1, yf, v) && f1->disp) st |= 1u;
    for (int r = 0; r < 3; r++) {
        s[r] = a[r] + (double)v[r];
        sf[r] = (float)s[r];
    }
    rows(P2, s, b);
    if (!field_at(f2, sf, v) && f2->disp) st |= 2u;
    for (int r = 0; r < 3; r++) t[r] = b[r] + (double)v[r];
    rows(Pc, y, c);
    return st;
}

/* m1, m2, mc: 16 floats (mc: the written composite as read back).  d1, d2 NULL: no field.  The composite grid gn, go, gh.
 * w: 3 N floats component-major, status: N words, res2: (gn0 - 1)(gn1 - 1)(gn2 - 1) doubles or NULL.  0, or -1 for a matrix
 * that cannot be inverted. */
int ocp_compose(const float *m1, const float *m2, const float *mc, const float *d1, const int64_t *n1, const float *o1, float h1, const float *d2,
                const int64_t *n2, const float *o2, float h2, const int64_t *gn, const float *go, float gh, float *w, uint32_t *status, double *res2)
{
    double P1[16], P2[16], Pc[16];
    if (affine_inverse(m1, P1) != 0 || affine_inverse(m2, P2) != 0 || affine_inverse(mc, Pc) != 0) return -1;
    field f1, f2, fw;
    set_field(&f1, d1, n1, o1, h1);
    set_field(&f2, d2, n2, o2, h2);
    const int64_t N = gn[0] * gn[1] * gn[2];
    for (int64_t c = 0; c < gn[2]; c++)
        for (int64_t b = 0; b < gn[1]; b++)
            for (int64_t a = 0; a < gn[0]; a++) {
                const int64_t i = (c * gn[1] + b) * gn[0] + a;
                const float y[3] = {go[0] + (float)a * gh, go[1] + (float)b * gh, go[2] + (float)c * gh};
                double t[3], q[3], ww[3];
                uint32_t st = chain(P1, P2, Pc, &f1, &f2, y, t, q);
                int ok = 1;
                for (int r = 0; r < 3; r++) {
                    ww[r] = t[r] - q[r];
                    ok &= ww[r] <= MAX_DISP && ww[r] >= -MAX_DISP;
                }
                if (!ok) {
                    ww[0] = ww[1] = ww[2] = 0.0;
                    st |= 4u;
                }
                for (int r = 0; r < 3; r++) w[r * N + i] = (float)ww[r];
                status[i] = st;
            }
    if (!res2) return 0;
    set_field(&fw, w, gn, go, gh);
    const int64_t c0 = gn[0] - 1, c1 = gn[1] - 1, c2 = gn[2] - 1;
    for (int64_t c = 0; c < c2; c++)
        for (int64_t b = 0; b < c1; b++)
            for (int64_t a = 0; a < c0; a++) {
                const float z[3] = {go[0] + ((float)a + 0.5f) * gh, go[1] + ((float)b + 0.5f) * gh, go[2] + ((float)c + 0.5f) * gh};
                double t[3], q[3], e[3];
                float wt[3];
                chain(P1, P2, Pc, &f1, &f2, z, t, q);
                field_at(&fw, z, wt);
                for (int r = 0; r < 3; r++) e[r] = t[r] - (q[r] + (double)wt[r]);
                res2[(c * c1 + b) * c0 + a] = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
            }
    return 0;
}
