/*
 * cli_common.c -- see cli_common.h.
 */
#include <errno.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include "cli_common.h"

int cli_refuse(void (*usage)(void), const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    printf("Error: ");
    vprintf(fmt, ap);
    printf("\n");
    va_end(ap);
    usage();
    return -1;
}

int cli_bare(const char *opt) { return opt[2] == 0; }

int cli_int(const char *s, int lo, int hi, int *v)
{
    char *end = NULL;
    errno = 0;
    const long x = strtol(s, &end, 10);
    if (end == s || *end != 0 || errno == ERANGE || x < lo || x > hi) return -1;
    *v = (int)x;
    return 0;
}

int cli_float(const char *s, float *v)
{
    char *end = NULL;
    *v = strtof(s, &end);
    return end == s || *end != 0 ? -1 : 0;
}

int cli_world_mode(const char *opt) { return opt[2] == 's' || opt[2] == 'S' ? 2 : 1; }

int cli_device(const char *opt)
{
    if (opt[2] < '0' || opt[2] > '9' || opt[3] != 0 || opt[2] - '0' >= sift3d_device_count()) return -1;
    return opt[2] - '0';
}

void cli_world_matrix(const nifti_min_image *img, int world_mode, float m[16])
{
    const float(*w)[4] = img->qto_xyz;
    if (world_mode == 2) {
        if (img->sform_code > 0) w = img->sto_xyz;
        else printf("Error: sform_code <= 0, using qto_xyz instead of sto_xyz\n");
    }
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) m[4 * r + c] = w[r][c];
    m[12] = m[13] = m[14] = 0.0f;
    m[15] = 1.0f;
}

void cli_image_vox2key(const nifti_min_image *img, int world_mode, float v[16])
{
    const float vox[3] = {img->dx, img->dy, img->dz};
    float w[16];
    if (world_mode) cli_world_matrix(img, world_mode, w);
    sift3d_key_vox2key(vox, world_mode ? w : NULL, v);
}

int cli_alloc_field(sift3d_field *f)
{
    f->capacity = 3 * f->n[0] * f->n[1] * f->n[2];
    f->disp = (float *)malloc(sizeof(float) * (size_t)f->capacity);
    return f->disp ? 0 : -1;
}

int cli_read_field(const char *path, sift3d_field *f)
{
    memset(f, 0, sizeof *f);
    int rc = sift3d_read_field(path, f);
    if (rc == SIFT3D_ERR_CAPACITY) rc = cli_alloc_field(f) == 0 ? sift3d_read_field(path, f) : SIFT3D_ERR_MEMORY;
    if (rc != SIFT3D_OK) {
        printf("Error: could not read displacement field file: %s\n", path);
        return -1;
    }
    return 0;
}

void cli_field_header(FILE *o, const sift3d_field *f)
{
    fprintf(o, "# nodes %lld %lld %lld spacing %f origin %f %f %f", (long long)f->n[0], (long long)f->n[1], (long long)f->n[2], f->spacing, f->origin[0],
            f->origin[1], f->origin[2]);
}

FILE *cli_write_field(const char *stem, const char *name, const sift3d_field *f)
{
    char *path = cli_path(stem, name);
    if (!path) return NULL;
    char *end = path + strlen(path);
    strcpy(end, ".nii");
    FILE *o = NULL;
    if (sift3d_write_field(path, f) == 0) {
        strcpy(end, ".txt");
        o = fopen(path, "w");
    }
    free(path);
    if (o) cli_field_header(o, f);
    return o;
}

char *cli_path(const char *stem, const char *suffix)
{
    /* four more than the two: cli_write_field's extension */
    char *path = (char *)malloc(strlen(stem) + strlen(suffix) + 5);
    if (path) strcat(strcpy(path, stem), suffix);
    return path;
}

int cli_read_image(const char *path, nifti_min_image *img)
{
    if (nifti_min_read(path, img) == 0) return 0;
    printf("Error: could not read input file: %s\n", path);
    return -1;
}

FILE *cli_open_out(const char *path)
{
    FILE *o = path ? fopen(path, "w") : stdout;
    if (!o) printf("Error: could not write output file: %s\n", path);
    return o;
}

int cli_close_out(FILE *o, const char *path)
{
    if ((path ? fclose(o) : fflush(o)) == 0) return 0;
    printf("Error: could not write output file: %s\n", path ? path : "(standard output)");
    return -1;
}
