/*
 * featAverage.c -- a template from a group of registered images: every image through its .trans.txt and its displacement field onto
 * the grid of one image, and there the mean, a trimmed mean or the median of the images that reach the voxel, their standard
 * deviation and their number (sift3d_average_warped).  Beyond the reference.
 *
 *   featAverage [-w|-ws] [-m<mean|median|trim>] [-t<n>] [-k<min count>] [-f<v>] [-u] [-d<N>] <grid image> <out> <image> <image.trans.txt|-> <image.field.nii|-> [...]
 *
 * Only the grid image's geometry is used.  Every image is a moving one against the grid, exactly featResample's roles: <image.trans.txt>
 * is what featMatchMultiple -a or featRegister wrote for the image against the grid image ("-": the identity), <image.field.nii> the
 * displacement field of -a -e -u or of featResample -i ("-": none).  Three arguments per image, 1 .. 32 images.
 * Writes <out> (float32, the grid's geometry), <out>.sd.nii (the square root of the variance, taken here), <out>.count.nii (the
 * number of images that reach the voxel) and <out>.average.txt (the report); with -u, and a field in every group, the node-wise mean
 * of the fields as <out>.mean.field.nii and <out>.mean.field.txt.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cli_common.h"

static void print_options(void)
{
    printf("Volumetric template from a group of registered images v1.0\n");
    printf("Usage: %s [options] <grid image> <out> <image> <image.trans.txt|-> <image.field.nii|-> [...]\n", "featAverage");
    printf("  <grid image>: nifti (.nii,.hdr,.nii.gz); only its geometry is used: the grid of the output.\n");
    printf("  <out>: float32 nifti (.nii,.nii.gz); also written: <out>.sd.nii, <out>.count.nii and <out>.average.txt.\n");
    printf("  then three arguments per image, for 1 to %d images:\n", SIFT3D_AVERAGE_MAX_IMAGES);
    printf("  <image>: nifti, the image's intensities.\n");
    printf("  <image.trans.txt|->: the 4x4 transform of the image against the grid image (featMatchMultiple -a, featRegister), or - for the identity.\n");
    printf("  <image.field.nii|->: the image's displacement field (featMatchMultiple -a -e -u, featResample -i), or - for none.\n");
    printf(" [options]\n");
    printf("  -w         : the features were extracted with -w (world coordinates, NIFTI qto_xyz matrix).\n");
    printf("  -ws        : the features were extracted with -ws (world coordinates, NIFTI sto_xyz matrix).\n");
    printf("  -m<mean|median|trim> : the average (default: mean); trim drops the -t lowest and highest values at every voxel.\n");
    printf("  -t<n>      : with -mtrim, or alone: the values dropped at either end, 1 .. %d (default 1).\n", SIFT3D_AVERAGE_MAX_TRIM);
    printf("  -k<count>  : the least number of images a voxel needs, 1 .. the number of images (default 1).\n");
    printf("  -f<value>  : value of output voxels that fewer images reach (default NaN).\n");
    printf("  -u         : also write the mean of the images' displacement fields; every image needs one, all on one node grid.\n");
    printf("  -d[0-9]    : set device id to be used.\n");
}

int main(int argc, char **argv)
{
    sift3d_average_params p;
    sift3d_average_defaults(&p);
    int world_mode = 0, arg = 1, mode = 0 /* 0 mean, 1 median, 2 trim */, trim = 0, mean_field = 0;
    while (arg < argc && argv[arg][0] == '-' && argv[arg][1] != 0) {
        switch (argv[arg][1]) {
        case 'w':
        case 'W':
            world_mode = cli_world_mode(argv[arg]);
            break;
        case 'm':
            if (strcmp(argv[arg] + 2, "mean") == 0) mode = 0;
            else if (strcmp(argv[arg] + 2, "median") == 0) mode = 1;
            else if (strcmp(argv[arg] + 2, "trim") == 0) mode = 2;
            else return cli_refuse(print_options, "bad average: %s", argv[arg]);
            break;
        case 't':
            if (cli_int(argv[arg] + 2, 1, SIFT3D_AVERAGE_MAX_TRIM, &trim) != 0) return cli_refuse(print_options, "bad trim: %s", argv[arg]);
            break;
        case 'k':
            if (cli_int(argv[arg] + 2, 1, SIFT3D_AVERAGE_MAX_IMAGES, &p.min_count) != 0) return cli_refuse(print_options, "bad minimum count: %s", argv[arg]);
            break;
        case 'f':
            if (cli_float(argv[arg] + 2, &p.fill) != 0) return cli_refuse(print_options, "bad fill value: %s", argv[arg]);
            break;
        case 'u':
            if (!cli_bare(argv[arg])) return cli_refuse(print_options, "unknown command line argument: %s", argv[arg]);
            mean_field = 1;
            break;
        case 'd':
            if ((p.device = cli_device(argv[arg])) < 0) return cli_refuse(print_options, "unknown device: %s", argv[arg] + 2);
            break;
        default:
            return cli_refuse(print_options, "unknown command line argument: %s", argv[arg]);
        }
        arg++;
    }
    if (trim > 0 && mode == 1) return cli_refuse(print_options, "the median drops all but the middle: -t with -mmedian");
    if (trim > 0 && mode == 0) mode = 2; /* -t alone */
    p.trim = mode == 0 ? 0 : (mode == 1 ? SIFT3D_AVERAGE_MAX_TRIM : (trim > 0 ? trim : 1));
    const int rest = argc - arg - 2;
    if (rest < 3 || rest % 3 != 0 || rest / 3 > SIFT3D_AVERAGE_MAX_IMAGES) {
        if (rest > 0 && rest % 3 != 0) printf("Error: every image takes three arguments: <image> <image.trans.txt|-> <image.field.nii|->\n");
        else if (rest / 3 > SIFT3D_AVERAGE_MAX_IMAGES) printf("Error: more than %d images\n", SIFT3D_AVERAGE_MAX_IMAGES);
        print_options();
        return -1;
    }
    const int K = rest / 3;
    if (p.min_count > K) return cli_refuse(print_options, "the minimum count exceeds the %d images: -k%d", K, (int)p.min_count);
    const char *grid_path = argv[arg], *out_path = argv[arg + 1];
    char **group = argv + arg + 2;

    nifti_min_image grid;
    if (cli_read_image(grid_path, &grid) != 0) return -1;
    float gv[16];
    cli_image_vox2key(&grid, world_mode, gv);
    const int64_t n = (int64_t)grid.nx * grid.ny * grid.nz;

    sift3d_average_image *image = (sift3d_average_image *)calloc((size_t)K, sizeof *image);
    nifti_min_image *img = (nifti_min_image *)calloc((size_t)K, sizeof *img);
    sift3d_field *field = (sift3d_field *)calloc((size_t)K + 1, sizeof *field); /* the last: the mean field */
    float *mats = (float *)calloc((size_t)K, sizeof(float) * 32);
    sift3d_average_report *rep = (sift3d_average_report *)malloc(sizeof *rep);
    if (!image || !img || !field || !mats || !rep) {
        printf("Error: insufficient memory.\n");
        return -1;
    }
    int fields = 0;
    for (int k = 0; k < K; k++) {
        const char *image_path = group[3 * k], *trans_path = group[3 * k + 1], *field_path = group[3 * k + 2];
        float *mv = mats + 32 * k, *t = mv + 16;
        if (cli_read_image(image_path, &img[k]) != 0) return -1;
        if (strcmp(trans_path, "-") != 0) {
            if (sift3d_read_similarity(trans_path, t) != 0) {
                printf("Error: could not read transform file: %s\n", trans_path);
                return -1;
            }
            image[k].moving_to_fixed = t;
        }
        cli_image_vox2key(&img[k], world_mode, mv);
        if (strcmp(field_path, "-") != 0) {
            if (cli_read_field(field_path, &field[k]) != 0) return -1;
            image[k].field = &field[k];
            fields++;
        }
        image[k].image = img[k].data;
        image[k].nx = img[k].nx;
        image[k].ny = img[k].ny;
        image[k].nz = img[k].nz;
        image[k].vox2key = mv;
    }
    char err[512] = "";
    sift3d_field *mean = &field[K];
    if (mean_field) {
        if (fields != K) {
            printf("Error: -u takes the mean of the displacement fields: %d of %d images have none\n", K - fields, K);
            return -1;
        }
        int rc = sift3d_mean_field(K, field, mean, err, sizeof err);
        if (rc == SIFT3D_ERR_CAPACITY) rc = cli_alloc_field(mean) == 0 ? sift3d_mean_field(K, field, mean, err, sizeof err) : SIFT3D_ERR_MEMORY;
        if (rc != SIFT3D_OK) {
            printf("Error: could not average the displacement fields: %s\n", rc == SIFT3D_ERR_MEMORY ? "insufficient memory" : err);
            return -1;
        }
    }
    printf("Averaging: %d images onto %s (i=%d j=%d k=%d)\n", K, grid_path, grid.nx, grid.ny, grid.nz);
    float *avg = (float *)malloc(sizeof(float) * (size_t)n), *var = (float *)malloc(sizeof(float) * (size_t)n);
    uint32_t *mask = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)n);
    char *sd_path = cli_path(out_path, ".sd.nii"), *count_path = cli_path(out_path, ".count.nii"), *report_path = cli_path(out_path, ".average.txt");
    if (!avg || !var || !mask || !sd_path || !count_path || !report_path) {
        printf("Error: could not average, insufficient memory.\n");
        return -1;
    }
    if (sift3d_average_warped(grid.nx, grid.ny, grid.nz, gv, K, image, &p, avg, var, mask, rep, err, sizeof err) != SIFT3D_OK) {
        printf("Error: could not average: %s\n", err);
        return -1;
    }
    const int64_t need = sift3d_average_report_text(rep, NULL, 0);
    char *text = need >= 0 ? (char *)malloc((size_t)need + 1) : NULL;
    if (!text || sift3d_average_report_text(rep, text, need + 1) != need) {
        printf("Error: insufficient memory.\n");
        return -1;
    }
    if (nifti_min_write_f32_geom(out_path, avg, grid_path) != 0) {
        printf("Error: could not write output file: %s\n", out_path);
        return -1;
    }
    /* the two maps reuse the planes: the deviation where the variance is (a short voxel keeps its fill value), the count in avg's */
    for (int64_t i = 0; i < n; i++) {
        int c = 0;
        for (uint32_t m = mask[i]; m; m >>= 1) c += (int)(m & 1u);
        var[i] = c < p.min_count ? var[i] : sqrtf(var[i]);
        avg[i] = (float)c;
    }
    if (nifti_min_write_f32_geom(sd_path, var, grid_path) != 0 || nifti_min_write_f32_geom(count_path, avg, grid_path) != 0) {
        printf("Error: could not write output file: %s\n", sd_path);
        return -1;
    }
    FILE *o = cli_open_out(report_path);
    if (!o) return -1;
    fprintf(o, "# featAverage v1.0\n%s", text);
    if (cli_close_out(o, report_path) != 0) return -1;
    if (mean_field) {
        o = cli_write_field(out_path, ".mean.field", mean);
        if (!o) {
            printf("Error: could not write the mean displacement field of: %s\n", out_path);
            return -1;
        }
        fprintf(o, " mean of %d fields\n", K);
        if (fclose(o) != 0) return -1;
    }
    printf("\nDone.\n");
    for (int k = 0; k < K; k++) {
        nifti_min_free(&img[k]);
        free(field[k].disp);
    }
    free(mean->disp);
    free(text);
    free(sd_path);
    free(count_path);
    free(report_path);
    free(mask);
    free(var);
    free(avg);
    free(rep);
    free(mats);
    free(field);
    free(img);
    free(image);
    nifti_min_free(&grid);
    return 0;
}
