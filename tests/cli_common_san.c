/*
 * cli_common_san.c -- cli_common.c as a program of its own, for a build with and without -fsanitize=address,undefined
 * (tests/test_cli_refusals_cpu.py): the option values at and around their bounds, paths from empty and long stems, the world matrix
 * with and without an sform, a field file read back, missing and truncated, and the .field.txt prefix.  Linked with field_io.c and
 * nifti_min.c alone, so the two library calls cli_common.c makes beyond them are stated here.
 */
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "cli_common.h"

int sift3d_device_count(void) { return 2; }

/* the identity case of align_host.c's: all that cli_image_vox2key's callers below need */
void sift3d_key_vox2key(const float voxel[3], const float world[16], float m[16])
{
    for (int k = 0; k < 16; k++) m[k] = world ? world[k] : (k % 5 == 0 ? 1.0f : 0.0f);
    if (!world) m[3] = m[7] = m[11] = 0.5f;
    (void)voxel;
}

static void usage(void) { printf("usage\n"); }

static void ints(const char *s, int lo, int hi)
{
    int v = -777;
    const int rc = cli_int(s, lo, hi, &v);
    printf("int [%s] %d..%d: %d %d\n", s, lo, hi, rc, v);
}

static void floats(const char *s)
{
    float v = -777.0f;
    const int rc = cli_float(s, &v);
    if (rc == 0) printf("float [%s]: 0 %g\n", s, (double)v);
    else printf("float [%s]: -1\n", s);
}

static void matrix(const char *title, const float m[16])
{
    printf("%s", title);
    for (int k = 0; k < 16; k++) printf(" %g", (double)m[k]);
    printf("\n");
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    const char *dir = argv[1];

    printf("refuse %d\n", cli_refuse(usage, "-c needs -i"));
    printf("refuse %d\n", cli_refuse(usage, "bad power: %s", "-p3"));
    printf("refuse %d\n", cli_refuse(usage, "unknown device: %s", ""));
    printf("bare %d %d\n", cli_bare("-l"), cli_bare("-lx"));

    static const char *const S[] = {"", " ", "+", "-", "x", "3x", "x3", " 3", "3 ", "+3", "-3", "03", "0x3", "3.0", "99999999999999999999", "-99999999999999999999"};
    for (size_t k = 0; k < sizeof S / sizeof *S; k++) ints(S[k], -5, 5);
    static const int B[][2] = {{0, 8}, {1, 16}, {1, 6}, {0, 2}, {1, 3}, {1, 16777216}, {8, 64}};
    for (size_t k = 0; k < sizeof B / sizeof *B; k++)
        for (int e = 0; e < 2; e++)
            for (int d = -1; d <= 1; d++) {
                char s[32];
                snprintf(s, sizeof s, "%d", B[k][e] + d);
                ints(s, B[k][0], B[k][1]);
            }
    char big[32];
    snprintf(big, sizeof big, "%ld", (long)INT_MAX + 1);
    ints(big, 0, INT_MAX);
    ints("2147483647", 0, INT_MAX);
    ints("-2147483648", INT_MIN, 0);
    snprintf(big, sizeof big, "%ld", (long)INT_MIN - 1);
    ints(big, INT_MIN, 0);

    static const char *const F[] = {"", " ", "+", "-", "x", "1x", " 1", "1 ", "+1.5", "-1.5", "1e3", "1e", "nan", "inf", "-inf", "1e999", "1e-999", "0x10", ".5", "5."};
    for (size_t k = 0; k < sizeof F / sizeof *F; k++) floats(F[k]);

    printf("world %d %d %d %d %d\n", cli_world_mode("-w"), cli_world_mode("-ws"), cli_world_mode("-wS"), cli_world_mode("-W"), cli_world_mode("-wx"));
    static const char *const D[] = {"-d", "-dx", "-d0", "-d1", "-d2", "-d9", "-d0x", "-d10", "-d/", "-d:"};
    for (size_t k = 0; k < sizeof D / sizeof *D; k++) printf("device [%s] %d\n", D[k], cli_device(D[k]));

    char *longstem = (char *)malloc(10001);
    if (!longstem) return 2;
    memset(longstem, 'p', 10000);
    longstem[10000] = 0;
    const char *stems[] = {"", "out.nii", longstem};
    static const char *const suffix[] = {"", ".clean.txt", ".inv.field"};
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
            char *p = cli_path(stems[a], suffix[b]);
            if (!p) return 2;
            printf("path %zu+%zu: %zu %s %d\n", strlen(stems[a]), strlen(suffix[b]), strlen(p), strlen(p) < 40 ? p : "(long)",
                   strncmp(p, stems[a], strlen(stems[a])) == 0 && strcmp(p + strlen(stems[a]), suffix[b]) == 0);
            strcat(p, ".nii"); /* the room cli_write_field uses */
            free(p);
        }
    free(longstem);

    nifti_min_image img;
    memset(&img, 0, sizeof img);
    img.dx = img.dy = img.dz = 1.0f;
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) {
            img.qto_xyz[r][c] = (float)(1 + 4 * r + c);
            img.sto_xyz[r][c] = (float)(101 + 4 * r + c);
        }
    for (int code = 0; code <= 2; code += 2)
        for (int mode = 1; mode <= 2; mode++) {
            float m[16], v[16];
            img.sform_code = code;
            printf("sform_code %d mode %d\n", code, mode);
            cli_world_matrix(&img, mode, m);
            matrix("world_matrix", m);
            cli_image_vox2key(&img, mode, v);
            printf("vox2key is the matrix: %d\n", memcmp(m, v, sizeof m) == 0);
        }
    float v0[16];
    cli_image_vox2key(&img, 0, v0);
    matrix("vox2key mode 0", v0);

    sift3d_field f;
    memset(&f, 0, sizeof f);
    f.n[0] = 4;
    f.n[1] = 3;
    f.n[2] = 2;
    f.spacing = 2.5f;
    f.origin[0] = -1.0f;
    f.origin[1] = 0.5f;
    f.origin[2] = 7.25f;
    if (cli_alloc_field(&f) != 0) return 2;
    printf("alloc capacity %lld\n", (long long)f.capacity);
    for (int64_t k = 0; k < f.capacity; k++) f.disp[k] = (float)k * 0.25f;

    FILE *o = cli_write_field(dir, "/w.field", &f);
    if (!o) return 2;
    fprintf(o, " tail %d\n", 7);
    if (fclose(o) != 0) return 2;
    char *txt = cli_path(dir, "/w.field.txt"), *nii = cli_path(dir, "/w.field.nii"), *cut = cli_path(dir, "/cut.field.nii"), *none = cli_path(dir, "/none.field.nii");
    if (!txt || !nii || !cut || !none) return 2;
    char line[256] = "";
    FILE *t = fopen(txt, "r");
    if (!t || !fgets(line, sizeof line, t)) return 2;
    fclose(t);
    printf("header %d\n", strcmp(line, "# nodes 4 3 2 spacing 2.500000 origin -1.000000 0.500000 7.250000 tail 7\n") == 0);
    printf("no field without a directory: %d\n", cli_write_field(none, "/x/y", &f) == NULL);

    sift3d_field g;
    memset(&g, 0xff, sizeof g); /* the reader starts from nothing */
    printf("read %d\n", cli_read_field(nii, &g));
    printf("read back %lld %lld %lld %g %g %g %g capacity %lld same %d\n", (long long)g.n[0], (long long)g.n[1], (long long)g.n[2], (double)g.spacing,
           (double)g.origin[0], (double)g.origin[1], (double)g.origin[2], (long long)g.capacity,
           g.capacity == f.capacity && memcmp(g.disp, f.disp, sizeof(float) * (size_t)f.capacity) == 0);
    free(g.disp);

    /* the same file without its last voxels, and no file at all: the message names the base name only */
    FILE *in = fopen(nii, "rb"), *out = fopen(cut, "wb");
    if (!in || !out) return 2;
    fseek(in, 0, SEEK_END);
    long size = ftell(in) - 40;
    fseek(in, 0, SEEK_SET);
    for (long k = 0; k < size; k++) fputc(fgetc(in), out);
    fclose(in);
    fclose(out);
    if (chdir(dir) != 0) return 2;
    printf("read cut %d\n", cli_read_field("cut.field.nii", &g));
    free(g.disp);
    printf("read none %d\n", cli_read_field("none.field.nii", &g));
    free(g.disp);

    nifti_min_image none_img;
    printf("image none %d\n", cli_read_image("none.nii", &none_img));
    FILE *so = cli_open_out(NULL);
    printf("stdout is stdout %d, closes %d\n", so == stdout, cli_close_out(so, NULL));
    printf("open none %d\n", cli_open_out("nodir/o.txt") == NULL);
    FILE *fo = cli_open_out("o.txt");
    if (!fo) return 2;
    fprintf(fo, "x\n");
    printf("file closes %d\n", cli_close_out(fo, "o.txt"));

    free(f.disp);
    free(txt);
    free(nii);
    free(cut);
    free(none);
    return 0;
}
