/*
 * featNormalize.c -- an image registered to a reference, written on its own grid on the reference's intensity scale: the two images
 * are compared where they overlap under the image's .trans.txt and its displacement field, and the transfer found there (moment
 * matching or quantile matching) is applied to every voxel of the image (sift3d_normalize_intensity).  Beyond
 * the reference.
 *
 *   featNormalize [-w|-ws] [-m<linear|hist>] [-q<knots>] [-k <mask>] [-d<N>] <reference image> <image> <image.trans.txt|-> <image.field.nii|-> <out>
 *
 * The reference is the fixed image and <image> the moving one, exactly featResample's roles: <image.trans.txt> is what
 * featMatchMultiple -a or featRegister wrote for the image against the reference ("-": the identity), <image.field.nii> the
 * displacement field of -a -e -u or of featResample -i ("-": none).  Writes <out> (float32, the IMAGE's geometry) and
 * <out>.normalize.txt (the report).
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cli_common.h"

static void print_options(void)
{
    printf("Volumetric intensity matching of a registered image v1.0\n");
    printf("Usage: %s [options] <reference image> <image> <image.trans.txt|-> <image.field.nii|-> <out>\n", "featNormalize");
    printf("  <reference image>: nifti (.nii,.hdr,.nii.gz), the image whose intensity scale is wanted.\n");
    printf("  <image>: nifti, the image to put on that scale.\n");
    printf("  <image.trans.txt|->: the 4x4 transform of the image against the reference (featMatchMultiple -a, featRegister), or - for the identity.\n");
    printf("  <image.field.nii|->: the image's displacement field (featMatchMultiple -a -e -u, featResample -i), or - for none.\n");
    printf("  <out>: float32 nifti (.nii,.nii.gz) with the image's geometry; also written: <out>.normalize.txt.\n");
    printf(" [options]\n");
    printf("  -w         : the features were extracted with -w (world coordinates, NIFTI qto_xyz matrix).\n");
    printf("  -ws        : the features were extracted with -ws (world coordinates, NIFTI sto_xyz matrix).\n");
    printf("  -m<linear|hist> : match mean and variance (default), or the quantiles of the two histograms.\n");
    printf("  -q<knots>  : with -mhist: the number of quantile intervals, 2 .. %d (default 64).\n", SIFT3D_NORMALIZE_MAX_KNOTS - 1);
    printf("  -k <mask>  : nifti on the reference's grid; only reference voxels where it is finite and not 0 take part.\n");
    printf("  -d[0-9]    : set device id to be used.\n");
}

int main(int argc, char **argv)
{
    sift3d_normalize_params p;
    sift3d_normalize_defaults(&p);
    int world_mode = 0, arg = 1, knots = 0;
    const char *mask_path = NULL;
    while (arg < argc && argv[arg][0] == '-' && argv[arg][1] != 0) {
        switch (argv[arg][1]) {
        case 'w':
        case 'W':
            world_mode = cli_world_mode(argv[arg]);
            break;
        case 'm':
            if (strcmp(argv[arg] + 2, "linear") == 0) p.mode = SIFT3D_NORMALIZE_LINEAR;
            else if (strcmp(argv[arg] + 2, "hist") == 0) p.mode = SIFT3D_NORMALIZE_HIST;
            else return cli_refuse(print_options, "bad mode: %s", argv[arg]);
            break;
        case 'q':
            if (cli_int(argv[arg] + 2, 2, SIFT3D_NORMALIZE_MAX_KNOTS - 1, &knots) != 0) return cli_refuse(print_options, "bad knots: %s", argv[arg]);
            break;
        case 'k':
            if (!cli_bare(argv[arg]) || arg + 1 >= argc) return cli_refuse(print_options, "-k takes the mask image as the next argument: %s", argv[arg]);
            mask_path = argv[++arg];
            break;
        case 'd':
            if ((p.device = cli_device(argv[arg])) < 0) return cli_refuse(print_options, "unknown device: %s", argv[arg] + 2);
            break;
        default:
            return cli_refuse(print_options, "unknown command line argument: %s", argv[arg]);
        }
        arg++;
    }
    if (knots > 0 && p.mode != SIFT3D_NORMALIZE_HIST) return cli_refuse(print_options, "the knots are the quantile matching's: -q without -mhist");
    if (knots > 0) p.knots = knots;
    if (argc - arg != 5) {
        print_options();
        return -1;
    }
    const char *ref_path = argv[arg], *image_path = argv[arg + 1], *trans_path = argv[arg + 2], *field_path = argv[arg + 3], *out_path = argv[arg + 4];

    nifti_min_image ref, img, msk;
    memset(&msk, 0, sizeof msk);
    if (cli_read_image(ref_path, &ref) != 0 || cli_read_image(image_path, &img) != 0) return -1;
    if (mask_path) {
        if (cli_read_image(mask_path, &msk) != 0) return -1;
        if (msk.nx != ref.nx || msk.ny != ref.ny || msk.nz != ref.nz)
            return cli_refuse(print_options, "the mask's extents %d %d %d differ from the reference's %d %d %d", msk.nx, msk.ny, msk.nz, ref.nx, ref.ny, ref.nz);
    }
    float rv[16], mv[16], t[16];
    cli_image_vox2key(&ref, world_mode, rv);
    cli_image_vox2key(&img, world_mode, mv);
    sift3d_average_image image;
    sift3d_field field;
    memset(&image, 0, sizeof image);
    memset(&field, 0, sizeof field);
    if (strcmp(trans_path, "-") != 0) {
        if (sift3d_read_similarity(trans_path, t) != 0) {
            printf("Error: could not read transform file: %s\n", trans_path);
            return -1;
        }
        image.moving_to_fixed = t;
    }
    if (strcmp(field_path, "-") != 0) {
        if (cli_read_field(field_path, &field) != 0) return -1;
        image.field = &field;
    }
    image.image = img.data;
    image.nx = img.nx;
    image.ny = img.ny;
    image.nz = img.nz;
    image.vox2key = mv;

    const int64_t n = (int64_t)img.nx * img.ny * img.nz;
    float *out = (float *)malloc(sizeof(float) * (size_t)n);
    sift3d_normalize_report *rep = (sift3d_normalize_report *)malloc(sizeof *rep);
    char *report_path = cli_path(out_path, ".normalize.txt");
    if (!out || !rep || !report_path) {
        printf("Error: could not normalize, insufficient memory.\n");
        return -1;
    }
    printf("Normalizing: %s (i=%d j=%d k=%d) to %s (i=%d j=%d k=%d)\n", image_path, img.nx, img.ny, img.nz, ref_path, ref.nx, ref.ny, ref.nz);
    char err[512] = "";
    if (sift3d_normalize_intensity(ref.data, ref.nx, ref.ny, ref.nz, rv, mask_path ? msk.data : NULL, &image, &p, out, rep, err, sizeof err) != SIFT3D_OK) {
        printf("Error: could not normalize: %s\n", err);
        return -1;
    }
    const int64_t need = sift3d_normalize_report_text(rep, NULL, 0);
    char *text = need >= 0 ? (char *)malloc((size_t)need + 1) : NULL;
    if (!text || sift3d_normalize_report_text(rep, text, need + 1) != need) {
        printf("Error: insufficient memory.\n");
        return -1;
    }
    if (nifti_min_write_f32_geom(out_path, out, image_path) != 0) {
        printf("Error: could not write output file: %s\n", out_path);
        return -1;
    }
    FILE *o = cli_open_out(report_path);
    if (!o) return -1;
    fprintf(o, "# featNormalize v1.0\n%s", text);
    if (cli_close_out(o, report_path) != 0) return -1;
    printf("\nDone.\n");
    free(text);
    free(report_path);
    free(rep);
    free(out);
    free(field.disp);
    if (mask_path) nifti_min_free(&msk);
    nifti_min_free(&img);
    nifti_min_free(&ref);
    return 0;
}
