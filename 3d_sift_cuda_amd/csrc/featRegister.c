/*
 * featRegister.c -- an affine alignment of two intensity images by mutual information (sift3d_register_affine, DESIGN.md section
 * 7q): up to twelve parameters, driven by the intensities alone, from the .trans.txt of featMatchMultiple -a [-e] or from nothing.
 * The step between the keypoint similarity and the displacement field, and the start for pairs from two modalities or sequences
 * whose keypoints do not match.  Beyond the reference.
 *
 *   featRegister [-w | -ws] [-f<dof>] [-m<mi|nmi>] [-b<bins>] [-o<fraction>] [-d<N>] <fixed image> <moving image> <moving.trans.txt | -> <out>
 *
 * Writes <out>.trans.txt, which featResample, featFuse and featCompose read, and <out>.register.txt, the report.  Every exit goes
 * through one place that releases what was read.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cli_common.h"

static void print_options(void)
{
    printf("Affine registration of two images by mutual information v1.0\n");
    printf("Usage: %s [options] <fixed image> <moving image> <moving.trans.txt | -> <out>\n", "featRegister");
    printf("  <fixed image>, <moving image>: nifti (.nii,.hdr,.nii.gz); voxels that are not finite are left out.\n");
    printf("  <moving.trans.txt>: the alignment to start from (featMatchMultiple -a [-e], featCompose, featRegister); -: none.\n");
    printf("  <out>: <out>.trans.txt, the alignment found (moving keys -> fixed keys), and <out>.register.txt, the report.\n");
    printf(" [options]\n");
    printf("  -w         : keys in world coordinates (qto_xyz), as featExtract -w wrote them.\n");
    printf("  -ws        : keys in world coordinates (sto_xyz), as featExtract -ws wrote them.\n");
    printf("  -f[3|6|7|9|12] : degrees of freedom: translation; and rotation; and one scale; three scales; and shear (default: 12).\n");
    printf("  -m[mi|nmi] : the score: mutual information or its normalised form (default: nmi).\n");
    printf("  -b[8|16|32|64] : bins per image of the joint histogram (default: 32).\n");
    printf("  -o[0-1]    : the least fraction of the lattice voxels a candidate must count (default: 0.25).\n");
    printf("  -d[0-9]    : set device id to be used.\n");
}

int main(int argc, char **argv)
{
    sift3d_register_params p;
    sift3d_register_defaults(&p);
    int world_mode = 0, arg = 1;
    float overlap = 0.0f;
    while (arg < argc && argv[arg][0] == '-' && argv[arg][1] != 0) {
        switch (argv[arg][1]) {
        case 'w':
        case 'W':
            world_mode = cli_world_mode(argv[arg]);
            break;
        case 'f':
            if (cli_int(argv[arg] + 2, 3, 12, &p.dof) != 0 || (p.dof != 3 && p.dof != 6 && p.dof != 7 && p.dof != 9 && p.dof != 12))
                return cli_refuse(print_options, "bad degrees of freedom: %s", argv[arg]);
            break;
        case 'm':
            if (strcmp(argv[arg] + 2, "mi") == 0) p.metric = SIFT3D_REGISTER_METRIC_MI;
            else if (strcmp(argv[arg] + 2, "nmi") == 0) p.metric = SIFT3D_REGISTER_METRIC_NMI;
            else return cli_refuse(print_options, "bad metric: %s", argv[arg]);
            break;
        case 'b':
            if (cli_int(argv[arg] + 2, 8, 64, &p.bins) != 0 || (p.bins != 8 && p.bins != 16 && p.bins != 32 && p.bins != 64))
                return cli_refuse(print_options, "bad number of bins: %s", argv[arg]);
            break;
        case 'o':
            if (cli_float(argv[arg] + 2, &overlap) != 0 || !(overlap >= 0.0f && overlap <= 1.0f)) return cli_refuse(print_options, "bad overlap fraction: %s", argv[arg]);
            p.min_overlap = (double)overlap;
            break;
        case 'd':
            if ((p.device = cli_device(argv[arg])) < 0) return cli_refuse(print_options, "unknown device: %s", argv[arg] + 2);
            break;
        default:
            return cli_refuse(print_options, "unknown command line argument: %s", argv[arg]);
        }
        arg++;
    }
    if (argc - arg != 4) {
        print_options();
        return -1;
    }
    const char *fixed_path = argv[arg], *moving_path = argv[arg + 1], *trans_path = argv[arg + 2], *out_stem = argv[arg + 3];
    nifti_min_image fixed, moving;
    sift3d_register_report *rep = NULL;
    char *text = NULL, *t_path = NULL, *r_path = NULL;
    FILE *o = NULL;
    int rc = -1;
    memset(&fixed, 0, sizeof fixed);
    memset(&moving, 0, sizeof moving);
    if (cli_read_image(fixed_path, &fixed) != 0) goto done;
    if (cli_read_image(moving_path, &moving) != 0) goto done;
    float t[16], fv[16], mv[16];
    const int has_start = strcmp(trans_path, "-") != 0;
    if (has_start && sift3d_read_similarity(trans_path, t) != 0) {
        printf("Error: could not read transform file: %s\n", trans_path);
        goto done;
    }
    cli_image_vox2key(&fixed, world_mode, fv);
    cli_image_vox2key(&moving, world_mode, mv);
    rep = (sift3d_register_report *)malloc(sizeof *rep);
    t_path = cli_path(out_stem, ".trans.txt");
    r_path = cli_path(out_stem, ".register.txt");
    if (!rep || !t_path || !r_path) {
        printf("Error: insufficient memory.\n");
        goto done;
    }
    char err[512] = "";
    if (sift3d_register_affine(fixed.data, fixed.nx, fixed.ny, fixed.nz, moving.data, moving.nx, moving.ny, moving.nz, fv, mv, has_start ? t : NULL, &p, rep, err,
                               sizeof err) != SIFT3D_OK) {
        printf("Error: could not register the images: %s\n", err);
        goto done;
    }
    const int64_t need = sift3d_register_report_text(rep, NULL, 0);
    text = need >= 0 ? (char *)malloc((size_t)need + 1) : NULL;
    if (!text || sift3d_register_report_text(rep, text, need + 1) != need) {
        printf("Error: insufficient memory.\n");
        goto done;
    }
    if (sift3d_write_matrix(t_path, rep->result) != 0) {
        printf("Error: could not write output file: %s\n", t_path);
        goto done;
    }
    if (!(o = cli_open_out(r_path))) goto done;
    fprintf(o, "# featRegister v1.0\n%s", text);
    rc = cli_close_out(o, r_path);
    o = NULL;
done:
    if (o) fclose(o);
    free(text);
    free(t_path);
    free(r_path);
    free(rep);
    nifti_min_free(&fixed);
    nifti_min_free(&moving);
    return rc;
}
