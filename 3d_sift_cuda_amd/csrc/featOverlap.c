/*
 * featOverlap.c -- two label images on one grid scored against each other: the Dice overlap per label, as featFuse -t writes it,
 * and with -m the surface distances per label in mm (sift3d_surface_distances).  The tool for scoring one
 * featResample -n warp of an atlas' labels against a truth.  Beyond the reference.
 *
 *   featOverlap [-m] [-z] [-d<N>] <labels a> <labels b> [<out.txt>]
 *
 * Label voxels are integers 0 .. 65535; a non-finite voxel is unlabelled.  <labels a> takes the columns featFuse gives the fused
 * labels, <labels b> those of the truth.  Without <out.txt> the tables go to the standard output.  Every exit goes through one
 * place that releases what was read.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cli_common.h"
#include "label_report.h"

static void print_options(void)
{
    printf("Overlap and surface distances of two label images v1.0\n");
    printf("Usage: %s [options] <labels a> <labels b> [<out.txt>]\n", "featOverlap");
    printf("  <labels a>, <labels b>: nifti (.nii,.hdr,.nii.gz) on one grid: integers 0 .. 65535, NaN where unlabelled.\n");
    printf("  <out.txt>: the tables (default: the standard output).  Their columns are named as featFuse -t names them: \"fused\" and\n");
    printf("             \"surf_fused\" are <labels a>, \"truth\" and \"surf_truth\" are <labels b>.\n");
    printf(" [options]\n");
    printf("  -m         : also the surface distances per label (Hausdorff, 95th percentile, average symmetric), in mm by the voxel size.\n");
    printf("  -z         : with -m: also the distances of label 0 (default: from label 1 on).\n");
    printf("  -d[0-9]    : set device id to be used.\n");
}

int main(int argc, char **argv)
{
    int device = 0, measure = 0, zero = 0;
    int arg = 1;
    while (arg < argc && argv[arg][0] == '-' && argv[arg][1] != 0) {
        switch (argv[arg][1]) {
        case 'm':
            if (!cli_bare(argv[arg])) return cli_refuse(print_options, "unknown command line argument: %s", argv[arg]);
            measure = 1;
            break;
        case 'z':
            if (!cli_bare(argv[arg])) return cli_refuse(print_options, "unknown command line argument: %s", argv[arg]);
            zero = 1;
            break;
        case 'd':
            if ((device = cli_device(argv[arg])) < 0) return cli_refuse(print_options, "unknown device: %s", argv[arg] + 2);
            break;
        default:
            return cli_refuse(print_options, "unknown command line argument: %s", argv[arg]);
        }
        arg++;
    }
    if (argc - arg < 2 || argc - arg > 3) {
        print_options();
        return -1;
    }
    const char *a_path = argv[arg], *b_path = argv[arg + 1], *out_path = argc - arg == 3 ? argv[arg + 2] : NULL;
    nifti_min_image a, b;
    int64_t *ca = NULL;
    FILE *o = NULL;
    int rc = -1;
    memset(&a, 0, sizeof a);
    memset(&b, 0, sizeof b);
    if (cli_read_image(a_path, &a) != 0) goto done;
    if (cli_read_image(b_path, &b) != 0) goto done;
    if (a.nx != b.nx || a.ny != b.ny || a.nz != b.nz) {
        printf("Error: the images are not on one grid: %d x %d x %d voxels against %d x %d x %d\n", a.nx, a.ny, a.nz, b.nx, b.ny, b.nz);
        goto done;
    }
    char err[512] = "";
    uint32_t spacing_um[3] = {0, 0, 0};
    if (measure && label_report_common_spacing(&a, &b, a_path, b_path, spacing_um) != 0) goto done;
    const int64_t n = (int64_t)a.nx * a.ny * a.nz;
    ca = (int64_t *)malloc(sizeof(int64_t) * 3 * SIFT3D_LABEL_COUNT);
    if (!ca) {
        printf("Error: insufficient memory.\n");
        goto done;
    }
    if (sift3d_label_overlap(a.data, b.data, n, ca, ca + SIFT3D_LABEL_COUNT, ca + 2 * SIFT3D_LABEL_COUNT) < 0) {
        printf("Error: a voxel of an image is neither non-finite nor an integer 0 .. 65535: %s\n",
               sift3d_fuse_check_labels(a.data, n) >= 0 ? a_path : b_path);
        goto done;
    }
    if (!(o = cli_open_out(out_path))) goto done;
    label_report_dice(o, ca, ca + SIFT3D_LABEL_COUNT, ca + 2 * SIFT3D_LABEL_COUNT);
    if (measure && label_report_distances(o, device, a.data, b.data, a.nx, a.ny, a.nz, spacing_um, zero ? 0 : 1, err, sizeof err) != 0) {
        printf("Error: could not take the surface distances: %s\n", err);
        goto done;
    }
    rc = cli_close_out(o, out_path);
    o = NULL;
done:
    if (o && out_path) fclose(o);
    free(ca);
    nifti_min_free(&a);
    nifti_min_free(&b);
    return rc;
}
