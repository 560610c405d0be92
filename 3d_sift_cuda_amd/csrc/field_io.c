/*
 * field_io.c -- <moving>.field.nii: sift3d_write_field and sift3d_read_field over nifti_min's field
 * header.  In libsift3d_host.so and the command lines (featMatchMultiple -u, featResample -u).
 */
#include "nifti_min.h"
#include "sift3d.h"

#define FIELD_DESCRIP "phi(y)=T^-1(y)+v(y); y fixed key, v moving key units"

int sift3d_write_field(const char *path, const sift3d_field *f)
{
    if (!path || !f || !f->disp) return -1;
    int n[3];
    for (int k = 0; k < 3; k++) {
        if (f->n[k] < 2 || f->n[k] > 32767) return -1;
        n[k] = (int)f->n[k];
    }
    if (f->capacity < 3 * f->n[0] * f->n[1] * f->n[2]) return -1;
    return nifti_min_write_field(path, f->disp, n, f->spacing, f->origin, FIELD_DESCRIP);
}

int sift3d_read_field(const char *path, sift3d_field *f)
{
    if (!path || !f) return SIFT3D_ERR_ARG;
    int n[3];
    float h, o[3];
    const int rc = nifti_min_read_field(path, n, &h, o, f->disp, f->disp && f->capacity > 0 ? (size_t)f->capacity : 0);
    if (rc == -1 || rc == -2) return SIFT3D_ERR_ARG;
    for (int k = 0; k < 3; k++) {
        f->n[k] = n[k];
        f->origin[k] = o[k];
    }
    f->spacing = h;
    return rc == -3 ? SIFT3D_ERR_CAPACITY : SIFT3D_OK;
}
