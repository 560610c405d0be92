/*
 * cli_common.h -- what the command lines beyond the reference share: the refusal, the option values, the key geometry of an image,
 * the field files and the output files.  Command-line code: not part of the C-ABI, linked into the tools only.
 * Every tool keeps its own option loop and its own usage text.
 */
#ifndef SIFT3D_CLI_COMMON_H
#define SIFT3D_CLI_COMMON_H
#include <stdio.h>

#include "nifti_min.h"
#include "sift3d.h"

/* "Error: <formatted>\n" and the usage to the standard output; returns -1, the tool's exit status */
int cli_refuse(void (*usage)(void), const char *fmt, ...) __attribute__((format(printf, 2, 3)));

/* opt, here and below: an argument of two characters at least, "-x...", as every option loop hands on.  It is "-x" and nothing after it */
int cli_bare(const char *opt);
/* the whole of s as a decimal integer in lo .. hi into *v; 0, or -1 with *v untouched */
int cli_int(const char *s, int lo, int hi, int *v);
/* the whole of s as a float into *v; 0 or -1 */
int cli_float(const char *s, float *v);
/* "-w...": 1 (qto_xyz), or 2 (sto_xyz) for -ws, -wS */
int cli_world_mode(const char *opt);
/* "-d[0-9]": the device, or -1 where it is no digit, more follows it or there is no such device */
int cli_device(const char *opt);

/* the qto_xyz / sto_xyz featExtract -w / -ws used (featExtract.c: the same choice and fallback, with its line on the standard output) */
void cli_world_matrix(const nifti_min_image *img, int world_mode, float m[16]);
/* voxel to key coordinates of img as featExtract [-w | -ws] wrote them (sift3d_key_vox2key) */
void cli_image_vox2key(const nifti_min_image *img, int world_mode, float v[16]);

/* f->disp for the f->n nodes, with f->capacity; 0 or -1 */
int cli_alloc_field(sift3d_field *f);
/* the field file at path into f, its disp allocated here; 0, or -1 with the message printed */
int cli_read_field(const char *path, sift3d_field *f);
/* "# nodes <n> spacing <h> origin <o>", no end of line: every .field.txt begins with it */
void cli_field_header(FILE *o, const sift3d_field *f);
/* f to <stem><name>.nii and <stem><name>.txt opened with cli_field_header in it, for the caller's tail; NULL where either fails */
FILE *cli_write_field(const char *stem, const char *name, const sift3d_field *f);

/* stem and suffix joined, to free(); NULL without memory */
char *cli_path(const char *stem, const char *suffix);
/* nifti_min_read; 0, or -1 with the message printed */
int cli_read_image(const char *path, nifti_min_image *img);
/* path opened for writing, or the standard output for NULL; NULL with the message printed */
FILE *cli_open_out(const char *path);
/* closes what cli_open_out gave (flushes the standard output); 0, or -1 with the message printed */
int cli_close_out(FILE *o, const char *path);
#endif
