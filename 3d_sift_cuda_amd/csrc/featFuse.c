/*
 * featFuse.c -- the step after registration: the label maps of several atlases, each registered to a target image
 * (featExtract, featMatchMultiple -a [-e -u], featResample -i), fused into a segmentation of the target by locally weighted
 * voting (sift3d_fuse_labels); with -s every atlas votes from its best-matching patch within a radius
 * (sift3d_fuse_labels_search, section 7k).  Beyond the reference.
 *
 *   featFuse [options] <target image> <output labels> <atlas image> <atlas labels> <atlas.trans.txt> <atlas.field.nii|-> [...]
 *
 * The target is the fixed image and every atlas a moving one, exactly featResample's roles: <atlas.trans.txt> is what
 * featMatchMultiple -a wrote for the atlas image against the target, <atlas.field.nii> the displacement field of -a -e -u or of
 * featResample -i ("-": none).  Four arguments per atlas, 1 .. 32 atlases.  Atlas labels are integers 0 .. 65535; a non-finite
 * voxel is unlabelled and does not vote.  -l: the atlases' labels are warped by label-aware linear interpolation (section 7n), not
 * by nearest neighbour; <output labels>.fuse.txt then says so in its second line.
 * Writes <output labels> (float32, the target's geometry, -f's value where no atlas votes), <output labels>.conf.nii (the winning
 * label's share of the vote, 0 .. 1) and <output labels>.fuse.txt (the parameters, the report, the voxels per label and, with -t,
 * the Dice overlap per label with the truth and their mean over the labels either volume has; with -s the radius and per atlas the
 * voxels where it voted from another place and the mean squared distance of its votes; with -t -m the surface distances per label
 * to the truth in mm: Hausdorff, its 95th percentile and the average symmetric surface distance).
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cli_common.h"
#include "label_report.h"

static void print_options(void)
{
    printf("Volumetric multi-atlas label fusion by locally weighted voting v1.0\n");
    printf("Usage: %s [options] <target image> <output labels> <atlas image> <atlas labels> <atlas.trans.txt> <atlas.field.nii|-> [...]\n",
           "featFuse");
    printf("  <target image>: nifti (.nii,.hdr,.nii.gz), the image to segment and the grid of the output.\n");
    printf("  <output labels>: float32 nifti (.nii,.nii.gz); also written: <output labels>.conf.nii and <output labels>.fuse.txt.\n");
    printf("  then four arguments per atlas, for 1 to %d atlases:\n", SIFT3D_FUSE_MAX_ATLASES);
    printf("  <atlas image>: nifti, the atlas' intensities.\n");
    printf("  <atlas labels>: nifti on the atlas image's grid: integers 0 .. 65535, NaN where unlabelled.\n");
    printf("  <atlas.trans.txt>: the 4x4 transform featMatchMultiple -a wrote for the atlas image against the target.\n");
    printf("  <atlas.field.nii|->: the atlas' displacement field (featMatchMultiple -a -e -u, featResample -i), or - for none.\n");
    printf(" [options]\n");
    printf("  -w         : the features were extracted with -w (world coordinates, NIFTI qto_xyz matrix).\n");
    printf("  -ws        : the features were extracted with -ws (world coordinates, NIFTI sto_xyz matrix).\n");
    printf("  -c         : weigh by the patches' normalised correlation: for atlases on other intensity scales (default: squared differences).\n");
    printf("  -b<half>   : half-width of the patch, 1 .. %d (default 2: 5x5x5 voxels).\n", SIFT3D_BLOCKMATCH_MAX_B);
    printf("  -p<0|1|2>  : power of the similarity in the vote; 0 is majority voting (default 2).\n");
    printf("  -s<radius> : every atlas votes with the label and the weight of its best-matching patch within <radius> voxels, 1 .. %d;\n", SIFT3D_FUSE_MAX_SEARCH);
    printf("               half-width + radius at most %d, and not with -p0 (default: no search).\n", SIFT3D_BLOCKMATCH_MAX_B);
    printf("  -l         : warp the atlases' labels by label-aware linear interpolation (default: nearest neighbour).\n");
    printf("  -f<value>  : value of output voxels where no atlas votes (default 0).\n");
    printf("  -t <truth> : label image on the target's grid: also write the Dice overlap per label to <output labels>.fuse.txt.\n");
    printf("  -m         : with -t: also write the surface distances per label to the truth (Hausdorff, 95th percentile, average\n");
    printf("               symmetric), in mm by the target's voxel size.\n");
    printf("  -d[0-9]    : set device id to be used.\n");
}

/* <out>.fuse.txt */
/* spacing_um: NULL, or the target's voxel size for the distance block of -m; -3 with the reason in err where that block fails */
static int write_report(const char *out_path, int K, const sift3d_fuse_params *p, const sift3d_fuse_report *rep, const sift3d_fuse_search_report *srep,
                        const nifti_min_image *target, const float *fused, const float *truth, const uint32_t *spacing_um, int device, char *err,
                        size_t err_len)
{
    const int64_t n = (int64_t)target->nx * target->ny * target->nz;
    int64_t *ca = (int64_t *)malloc(sizeof(int64_t) * 3 * SIFT3D_LABEL_COUNT);
    char *path = cli_path(out_path, ".fuse.txt");
    if (!ca || !path) return -1;
    int64_t *cb = ca + SIFT3D_LABEL_COUNT, *cboth = cb + SIFT3D_LABEL_COUNT;
    FILE *o = fopen(path, "w");
    free(path);
    if (!o) return -1;
    fprintf(o, "# atlases %d block %d metric %s power %d fill %g\n", K, p->block, p->metric == SIFT3D_BLOCKMATCH_NCC ? "ncc" : "ssd", p->power,
            (double)p->fill);
    if (p->label_interp == SIFT3D_INTERP_LABEL) fprintf(o, "# label_interp label\n");
    fprintf(o, "# target quantised over %g .. %g\n", (double)rep->lo, (double)rep->hi);
    fprintf(o, "# voxels %lld none %lld fallback %lld\n", (long long)n, (long long)rep->none, (long long)rep->fallback);
    fprintf(o, "# atlas voters support mean_u empty_range\n");
    for (int k = 0; k < K; k++)
        fprintf(o, "%d\t%lld\t%lld\t%.6f\t%d\n", k + 1, (long long)rep->atlas[k].voters, (long long)rep->atlas[k].support, rep->atlas[k].mean_u,
                rep->atlas[k].empty_range);
    if (srep) {
        fprintf(o, "# search radius %d\n# atlas moved mean_dist2\n", srep->radius);
        for (int k = 0; k < K; k++)
            fprintf(o, "%d\t%lld\t%.6f\n", k + 1, (long long)srep->atlas[k].moved,
                    rep->atlas[k].voters > 0 ? (double)srep->atlas[k].dist2_sum / (double)rep->atlas[k].voters : 0.0);
    }
    /* fused: NaN where no atlas votes, so those voxels have no label here */
    if (sift3d_label_overlap(fused, truth ? truth : fused, n, ca, cb, cboth) < 0) {
        fclose(o);
        free(ca);
        return -2;
    }
    fprintf(o, "# label voxels\n");
    for (int l = 0; l < SIFT3D_LABEL_COUNT; l++)
        if (ca[l] > 0) fprintf(o, "%d\t%lld\n", l, (long long)ca[l]);
    if (truth) label_report_dice(o, ca, cb, cboth);
    free(ca);
    if (truth && spacing_um && label_report_distances(o, device, fused, truth, target->nx, target->ny, target->nz, spacing_um, 1, err, err_len) != 0) {
        fclose(o);
        return -3;
    }
    return fclose(o);
}

int main(int argc, char **argv)
{
    int device = 0, world_mode = 0, measure = 0;
    int32_t search = 0;
    const char *truth_path = NULL;
    sift3d_fuse_params p;
    sift3d_fuse_defaults(&p);
    int arg = 1;
    while (arg < argc && argv[arg][0] == '-' && argv[arg][1] != 0) {
        switch (argv[arg][1]) {
        case 'w':
        case 'W':
            world_mode = cli_world_mode(argv[arg]);
            break;
        case 'c':
            if (!cli_bare(argv[arg])) return cli_refuse(print_options, "unknown command line argument: %s", argv[arg]);
            p.metric = SIFT3D_BLOCKMATCH_NCC;
            break;
        case 'b':
            if (cli_int(argv[arg] + 2, 1, SIFT3D_BLOCKMATCH_MAX_B, &p.block) != 0) return cli_refuse(print_options, "bad patch half-width: %s", argv[arg]);
            break;
        case 'p':
            if (cli_int(argv[arg] + 2, 0, 2, &p.power) != 0) return cli_refuse(print_options, "bad power: %s", argv[arg]);
            break;
        case 's':
            if (cli_int(argv[arg] + 2, 1, SIFT3D_FUSE_MAX_SEARCH, &search) != 0) return cli_refuse(print_options, "bad search radius: %s", argv[arg]);
            break;
        case 'l':
            if (!cli_bare(argv[arg])) return cli_refuse(print_options, "unknown command line argument: %s", argv[arg]);
            p.label_interp = SIFT3D_INTERP_LABEL;
            break;
        case 'f':
            if (cli_float(argv[arg] + 2, &p.fill) != 0) return cli_refuse(print_options, "bad fill value: %s", argv[arg]);
            break;
        case 't':
            if (!cli_bare(argv[arg]) || arg + 1 >= argc) return cli_refuse(print_options, "-t needs a label image: %s", argv[arg]);
            truth_path = argv[++arg];
            break;
        case 'm':
            if (!cli_bare(argv[arg])) return cli_refuse(print_options, "unknown command line argument: %s", argv[arg]);
            measure = 1;
            break;
        case 'd':
            if ((device = cli_device(argv[arg])) < 0) return cli_refuse(print_options, "unknown device: %s", argv[arg] + 2);
            break;
        default:
            return cli_refuse(print_options, "unknown command line argument: %s", argv[arg]);
        }
        arg++;
    }
    if (search > 0 && p.power == 0) return cli_refuse(print_options, "a search needs weights to search by: -s with -p0");
    if (search > 0 && p.block + search > SIFT3D_BLOCKMATCH_MAX_B) return cli_refuse(print_options, "the patch half-width plus the search radius must not exceed 6: -b with -s");
    if (measure && !truth_path) return cli_refuse(print_options, "the surface distances are taken to a truth: -m without -t");
    const int rest = argc - arg - 2;
    if (rest < 4 || rest % 4 != 0 || rest / 4 > SIFT3D_FUSE_MAX_ATLASES) {
        if (rest > 0 && rest % 4 != 0) printf("Error: every atlas takes four arguments: <atlas image> <atlas labels> <atlas.trans.txt> <atlas.field.nii|->\n");
        else if (rest / 4 > SIFT3D_FUSE_MAX_ATLASES) printf("Error: more than %d atlases\n", SIFT3D_FUSE_MAX_ATLASES);
        print_options();
        return -1;
    }
    const int K = rest / 4;
    const char *target_path = argv[arg], *out_path = argv[arg + 1];
    char **group = argv + arg + 2;

    nifti_min_image target, truth;
    memset(&truth, 0, sizeof truth);
    if (cli_read_image(target_path, &target) != 0) return -1;
    if (truth_path && (nifti_min_read(truth_path, &truth) != 0 || truth.nx != target.nx || truth.ny != target.ny || truth.nz != target.nz)) {
        printf("Error: could not read input file, or it is not on the target's grid: %s\n", truth_path);
        return -1;
    }
    char err[512] = "";
    uint32_t spacing_um[3];
    if (measure && label_report_spacing(target.dx, target.dy, target.dz, spacing_um, err, sizeof err) != 0) {
        printf("Error: %s: %s\n", err, target_path);
        return -1;
    }
    float tv[16];
    cli_image_vox2key(&target, world_mode, tv);
    const int64_t n = (int64_t)target.nx * target.ny * target.nz;

    sift3d_fuse_atlas *atlas = (sift3d_fuse_atlas *)calloc((size_t)K, sizeof *atlas);
    nifti_min_image *img = (nifti_min_image *)calloc((size_t)(2 * K), sizeof *img);
    sift3d_field *field = (sift3d_field *)calloc((size_t)K, sizeof *field);
    float *mats = (float *)calloc((size_t)K, sizeof(float) * 32);
    if (!atlas || !img || !field || !mats) {
        printf("Error: insufficient memory.\n");
        return -1;
    }
    for (int k = 0; k < K; k++) {
        const char *image_path = group[4 * k], *labels_path = group[4 * k + 1], *trans_path = group[4 * k + 2], *field_path = group[4 * k + 3];
        nifti_min_image *im = &img[2 * k], *lb = &img[2 * k + 1];
        float *mv = mats + 32 * k, *t = mv + 16;
        if (cli_read_image(image_path, im) != 0) return -1;
        if (nifti_min_read(labels_path, lb) != 0 || lb->nx != im->nx || lb->ny != im->ny || lb->nz != im->nz) {
            printf("Error: could not read input file, or it is not on the atlas image's grid: %s\n", labels_path);
            return -1;
        }
        if (sift3d_read_similarity(trans_path, t) != 0) {
            printf("Error: could not read transform file: %s\n", trans_path);
            return -1;
        }
        cli_image_vox2key(im, world_mode, mv);
        if (strcmp(field_path, "-") != 0) {
            if (cli_read_field(field_path, &field[k]) != 0) return -1;
            atlas[k].field = &field[k];
        }
        atlas[k].image = im->data;
        atlas[k].labels = lb->data;
        atlas[k].nx = im->nx;
        atlas[k].ny = im->ny;
        atlas[k].nz = im->nz;
        atlas[k].vox2key = mv;
        atlas[k].moving_to_fixed = t;
    }
    printf("Fusing: %d atlases onto %s (i=%d j=%d k=%d)\n", K, target_path, target.nx, target.ny, target.nz);
    uint32_t *words = (uint32_t *)malloc(sizeof(uint32_t) * 2 * (size_t)n);
    float *labels = (float *)malloc(sizeof(float) * (size_t)n), *conf = (float *)malloc(sizeof(float) * (size_t)n);
    char *path = cli_path(out_path, ".conf.nii");
    if (!words || !labels || !conf || !path) {
        printf("Error: could not fuse, insufficient memory.\n");
        return -1;
    }
    sift3d_fuse_report rep;
    sift3d_fuse_search_report srep;
    const int frc = search > 0 ? sift3d_fuse_labels_search(device, target.data, target.nx, target.ny, target.nz, tv, K, atlas, &p, search, words, &rep, &srep, err,
                                                           sizeof err)
                               : sift3d_fuse_labels(device, target.data, target.nx, target.ny, target.nz, tv, K, atlas, &p, words, &rep, err, sizeof err);
    if (frc != SIFT3D_OK) {
        printf("Error: could not fuse: %s\n", err);
        return -1;
    }
    for (int64_t i = 0; i < n; i++) {
        labels[i] = (words[2 * i] & SIFT3D_FUSE_NONE) ? p.fill : (float)(words[2 * i] & 0xffffu);
        conf[i] = (float)words[2 * i + 1] / 65535.0f;
    }
    if (nifti_min_write_f32_geom(out_path, labels, target_path) != 0 || nifti_min_write_f32_geom(path, conf, target_path) != 0) {
        printf("Error: could not write output file: %s\n", out_path);
        return -1;
    }
    for (int64_t i = 0; i < n; i++)
        if (words[2 * i] & SIFT3D_FUSE_NONE) labels[i] = NAN;
    const int wrc = write_report(out_path, K, &p, &rep, search > 0 ? &srep : NULL, &target, labels, truth_path ? truth.data : NULL,
                                 measure ? spacing_um : NULL, device, err, sizeof err);
    if (wrc != 0) {
        if (wrc == -3) printf("Error: could not take the surface distances: %s\n", err);
        else if (wrc == -2) printf("Error: a voxel of the truth is neither non-finite nor an integer 0 .. 65535: %s\n", truth_path);
        else printf("Error: could not write the report of: %s\n", out_path);
        return -1;
    }
    printf("\nDone.\n");
    for (int k = 0; k < K; k++) {
        nifti_min_free(&img[2 * k]);
        nifti_min_free(&img[2 * k + 1]);
        free(field[k].disp);
    }
    free(path);
    free(conf);
    free(labels);
    free(words);
    free(mats);
    free(field);
    free(img);
    free(atlas);
    nifti_min_free(&target);
    if (truth_path) nifti_min_free(&truth);
    return 0;
}
