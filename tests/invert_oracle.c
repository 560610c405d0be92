/*
 * invert_oracle.c -- the CPU oracle of the reverse direction, written from the contract in
 * include/sift3d.h: the inverse of an affine 4 x 4, the fixed-point inversion of a displacement field node by node, and the
 * Jacobian determinant map of a warp voxel by voxel, all serial.  Built by tests/_helpers.c_oracle with -O2 -ffp-contract=off.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define MAX_DISP 128.0

/* adjugate over determinant, then the translation; -1 for a singular matrix or a last row other than 0 0 0 1 */
int oiv_affine_inverse(const float *m, double *o)
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
    o[12] = o[13] = o[14] = 0.0;
    o[15] = 1.0;
    return 0;
}

typedef struct {
    const float *disp; /* component-major, NULL: no field */
    int64_t n[3];
    float o[3], h;
} field;

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

/* m, m_inv: 16 floats.  fdisp NULL: v = 0.  The inverse grid gn, go, gh.  u: 3 N floats component-major, status: N words,
 * res2: N doubles.  0, or -1 for a matrix that cannot be inverted. */
int oiv_invert(const float *m, const float *m_inv, const float *fdisp, const int64_t *fn, const float *fo, float fh, const int64_t *gn,
               const float *go, float gh, int max_iter, float tol, float *u, uint32_t *status, double *res2)
{
    double P[16], Q[16];
    if (oiv_affine_inverse(m_inv, P) != 0 || oiv_affine_inverse(m, Q) != 0) return -1;
    field f;
    memset(&f, 0, sizeof f);
    f.disp = fdisp;
    if (fdisp)
        for (int k = 0; k < 3; k++) {
            f.n[k] = fn[k];
            f.o[k] = fo[k];
        }
    f.h = fh;
    const double tol2 = (double)tol * (double)tol;
    const int64_t N = gn[0] * gn[1] * gn[2];
    for (int64_t c = 0; c < gn[2]; c++)
        for (int64_t b = 0; b < gn[1]; b++)
            for (int64_t a = 0; a < gn[0]; a++) {
                const int64_t i = (c * gn[1] + b) * gn[0] + a;
                const double z[3] = {(double)(go[0] + (float)a * gh), (double)(go[1] + (float)b * gh), (double)(go[2] + (float)c * gh)};
                double base[3], uu[3] = {0.0, 0.0, 0.0}, rr = 0.0;
                for (int r = 0; r < 3; r++) base[r] = ((P[4 * r] * z[0] + P[4 * r + 1] * z[1]) + P[4 * r + 2] * z[2]) + P[4 * r + 3];
                uint32_t state;
                int k = 0;
                for (;;) {
                    double y[3], res[3];
                    float yf[3], v[3];
                    for (int r = 0; r < 3; r++) {
                        y[r] = base[r] + uu[r];
                        yf[r] = (float)y[r];
                    }
                    field_at(&f, yf, v);
                    for (int r = 0; r < 3; r++)
                        res[r] = ((((Q[4 * r] * y[0] + Q[4 * r + 1] * y[1]) + Q[4 * r + 2] * y[2]) + Q[4 * r + 3]) + (double)v[r]) - z[r];
                    rr = (res[0] * res[0] + res[1] * res[1]) + res[2] * res[2];
                    if (rr <= tol2) {
                        state = 0;
                        break;
                    }
                    if (k == max_iter) {
                        state = 1;
                        break;
                    }
                    for (int r = 0; r < 3; r++)
                        uu[r] = uu[r] - (((double)m[4 * r] * res[0] + (double)m[4 * r + 1] * res[1]) + (double)m[4 * r + 2] * res[2]);
                    k++;
                    int ok = 1;
                    for (int r = 0; r < 3; r++) ok &= uu[r] <= MAX_DISP && uu[r] >= -MAX_DISP;
                    if (!ok) {
                        uu[0] = uu[1] = uu[2] = 0.0;
                        state = 2;
                        break;
                    }
                }
                for (int r = 0; r < 3; r++) u[r * N + i] = (float)uu[r];
                status[i] = (uint32_t)k | state << 16;
                res2[i] = rr;
            }
    return 0;
}

/* the output voxel -> source voxel map of the warp at any position p: q = map p, and inside the field's grid at the key
 * position c p the displacement through k is added */
static void warp_q(const float *map, const float *cm, const float *km, const field *f, const float p[3], float q[3])
{
    float key[3], v[3];
    for (int r = 0; r < 3; r++) {
        q[r] = ((map[4 * r] * p[0] + map[4 * r + 1] * p[1]) + map[4 * r + 2] * p[2]) + map[4 * r + 3];
        key[r] = ((cm[4 * r] * p[0] + cm[4 * r + 1] * p[1]) + cm[4 * r + 2] * p[2]) + cm[4 * r + 3];
    }
    if (!f->disp || !field_at(f, key, v)) return;
    for (int r = 0; r < 3; r++) q[r] = q[r] + ((km[3 * r] * v[0] + km[3 * r + 1] * v[1]) + km[3 * r + 2] * v[2]);
}

/* J on the planes z0 .. z1 - 1 of the output grid ox oy oz (out holds those planes alone): central differences of q over one
 * voxel, the determinant in double, times factor */
void oiv_jacobian_planes(int64_t ox, int64_t oy, int64_t oz, const float *map, const float *cm, const float *km, const float *fdisp,
                         const int64_t *fn, const float *fo, float fh, double factor, int64_t z0, int64_t z1, float *out)
{
    field f;
    memset(&f, 0, sizeof f);
    f.disp = fdisp;
    if (fdisp)
        for (int k = 0; k < 3; k++) {
            f.n[k] = fn[k];
            f.o[k] = fo[k];
        }
    f.h = fh;
    if (z0 < 0) z0 = 0;
    if (z1 > oz) z1 = oz;
    for (int64_t k = z0; k < z1; k++)
        for (int64_t j = 0; j < oy; j++)
            for (int64_t i = 0; i < ox; i++) {
                const int64_t at[3] = {i, j, k};
                double J[9];
                for (int a = 0; a < 3; a++) {
                    float pp[3] = {(float)i, (float)j, (float)k}, pm[3] = {(float)i, (float)j, (float)k}, qp[3], qm[3];
                    pp[a] = (float)(at[a] + 1);
                    pm[a] = (float)(at[a] - 1);
                    warp_q(map, cm, km, &f, pp, qp);
                    warp_q(map, cm, km, &f, pm, qm);
                    for (int r = 0; r < 3; r++) J[3 * r + a] = (double)((qp[r] - qm[r]) * 0.5f);
                }
                const double det = J[0] * (J[4] * J[8] - J[5] * J[7]) - J[1] * (J[3] * J[8] - J[5] * J[6]) + J[2] * (J[3] * J[7] - J[4] * J[6]);
                out[((k - z0) * oy + j) * ox + i] = (float)(det * factor);
            }
}

/* J on the whole output grid */
void oiv_jacobian(int64_t ox, int64_t oy, int64_t oz, const float *map, const float *cm, const float *km, const float *fdisp, const int64_t *fn,
                  const float *fo, float fh, double factor, float *out)
{
    oiv_jacobian_planes(ox, oy, oz, map, cm, km, fdisp, fn, fo, fh, factor, 0, oz, out);
}
