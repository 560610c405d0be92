/*
 * featClean.c -- a label image with its small connected components merged into what surrounds them (sift3d_clean_labels, DESIGN.md
 * section 7m): the step that follows a voxel-wise vote such as featFuse's, which leaves specks of one label inside another and
 * pinholes of background inside a structure.  Beyond the reference.
 *
 *   featClean [-v<min voxels>] [-c6|-c26] [-r<rounds>] [-t <truth> [-m]] [-d<N>] <labels in> <labels out>
 *
 * Label voxels are integers 0 .. 65535; a non-finite voxel is unlabelled and stays so.  <labels out> is float32 with the input's
 * geometry; <labels out>.clean.txt holds the parameters, the report per round, the components per label before and after and, with
 * -t, the Dice table of the input and of the output against the truth as featOverlap writes it (with -m their distance blocks too).
 * Every exit goes through one place that releases what was read.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cli_common.h"
#include "label_report.h"

static void print_options(void)
{
    printf("Island removal on a label image v1.0\n");
    printf("Usage: %s [options] <labels in> <labels out>\n", "featClean");
    printf("  <labels in>: nifti (.nii,.hdr,.nii.gz): integers 0 .. 65535, NaN where unlabelled (what featFuse writes).\n");
    printf("  <labels out>: the cleaned labels, float32 on the input's grid; the report goes to <labels out>.clean.txt.\n");
    printf(" [options]\n");
    printf("  -v[1-16777216] : connected components of fewer voxels take the label of most of their face neighbours (default 8).\n");
    printf("  -c6 | -c26     : voxels of one label are joined across faces (default), or across faces, edges and corners.\n");
    printf("  -r[1-16]       : rounds at the most; a round that changes nothing is the last (default 4).\n");
    printf("  -t <truth>     : label image on the input's grid: also the Dice overlap per label of the input and of the output with it.\n");
    printf("  -m             : with -t: also the surface distances per label of both to the truth, in mm by the voxel size.\n");
    printf("  -d[0-9]        : set device id to be used.\n");
}

/* per_label[l]: the components of the label l; returns their total, or -1 with the reason in err */
static int64_t count_components(int device, const float *labels, int64_t nx, int64_t ny, int64_t nz, int32_t connectivity, int64_t *per_label, char *err,
                                size_t err_len)
{
    int64_t room = 1 << 16, n = 0;
    for (int attempt = 0; attempt < 2; attempt++) {
        sift3d_component_record *rec = (sift3d_component_record *)malloc(sizeof *rec * (size_t)(room > 0 ? room : 1));
        if (!rec) {
            snprintf(err, err_len, "insufficient memory");
            return -1;
        }
        const int rc = sift3d_label_components(device, labels, nx, ny, nz, connectivity, NULL, rec, room, &n, NULL, err, (int64_t)err_len);
        if (rc == SIFT3D_OK) {
            memset(per_label, 0, sizeof(int64_t) * SIFT3D_LABEL_COUNT);
            for (int64_t k = 0; k < n; k++) per_label[rec[k].label]++;
            free(rec);
            return n;
        }
        free(rec);
        if (n <= room) return -1; /* refused for another reason than the room */
        room = n;
    }
    return -1;
}

/* the Dice table of labels against the truth and, with spacing_um, the distance block; 0, -1 with err, -2 for a voxel that is no label */
static int score(FILE *o, const char *title, int device, const float *labels, const nifti_min_image *truth, const uint32_t *spacing_um, int64_t *counts, char *err,
                 size_t err_len)
{
    const int64_t n = (int64_t)truth->nx * truth->ny * truth->nz;
    if (sift3d_label_overlap(labels, truth->data, n, counts, counts + SIFT3D_LABEL_COUNT, counts + 2 * SIFT3D_LABEL_COUNT) < 0) return -2;
    fprintf(o, "# %s against the truth\n", title);
    label_report_dice(o, counts, counts + SIFT3D_LABEL_COUNT, counts + 2 * SIFT3D_LABEL_COUNT);
    if (spacing_um && label_report_distances(o, device, labels, truth->data, truth->nx, truth->ny, truth->nz, spacing_um, 1, err, err_len) != 0) return -1;
    return 0;
}

int main(int argc, char **argv)
{
    int measure = 0;
    const char *truth_path = NULL;
    sift3d_clean_params p;
    sift3d_clean_defaults(&p);
    int arg = 1;
    while (arg < argc && argv[arg][0] == '-' && argv[arg][1] != 0) {
        switch (argv[arg][1]) {
        case 'v':
            if (cli_int(argv[arg] + 2, 1, SIFT3D_CLEAN_MAX_MIN_VOXELS, &p.min_voxels) != 0) return cli_refuse(print_options, "bad minimum of voxels: %s", argv[arg]);
            break;
        case 'c':
            if (strcmp(argv[arg], "-c6") != 0 && strcmp(argv[arg], "-c26") != 0) return cli_refuse(print_options, "bad connectivity: %s", argv[arg]);
            p.connectivity = argv[arg][2] == '6' ? 6 : 26;
            break;
        case 'r':
            if (cli_int(argv[arg] + 2, 1, SIFT3D_CLEAN_MAX_ROUNDS, &p.rounds) != 0) return cli_refuse(print_options, "bad number of rounds: %s", argv[arg]);
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
            if ((p.device = cli_device(argv[arg])) < 0) return cli_refuse(print_options, "unknown device: %s", argv[arg] + 2);
            break;
        default:
            return cli_refuse(print_options, "unknown command line argument: %s", argv[arg]);
        }
        arg++;
    }
    if (measure && !truth_path) return cli_refuse(print_options, "the surface distances are taken to a truth: -m without -t");
    if (argc - arg != 2) {
        print_options();
        return -1;
    }
    const char *in_path = argv[arg], *out_path = argv[arg + 1];
    nifti_min_image in, truth;
    float *out = NULL;
    int64_t *counts = NULL;
    char *path = NULL;
    FILE *o = NULL;
    int rc = -1;
    memset(&in, 0, sizeof in);
    memset(&truth, 0, sizeof truth);
    if (cli_read_image(in_path, &in) != 0) goto done;
    if (truth_path && cli_read_image(truth_path, &truth) != 0) goto done;
    if (truth_path && (in.nx != truth.nx || in.ny != truth.ny || in.nz != truth.nz)) {
        printf("Error: the images are not on one grid: %d x %d x %d voxels against %d x %d x %d\n", in.nx, in.ny, in.nz, truth.nx, truth.ny, truth.nz);
        goto done;
    }
    char err[512] = "";
    uint32_t spacing_um[3] = {0, 0, 0};
    if (measure && label_report_common_spacing(&in, &truth, in_path, truth_path, spacing_um) != 0) goto done;
    const int64_t n = (int64_t)in.nx * in.ny * in.nz;
    out = (float *)malloc(sizeof(float) * (size_t)n);
    counts = (int64_t *)malloc(sizeof(int64_t) * 5 * SIFT3D_LABEL_COUNT); /* three of the overlap, the components per label before and after */
    if (!out || !counts) {
        printf("Error: insufficient memory.\n");
        goto done;
    }
    sift3d_clean_report rep;
    if (sift3d_clean_labels(in.data, in.nx, in.ny, in.nz, &p, out, &rep, NULL, err, sizeof err) != SIFT3D_OK) {
        printf("Error: could not clean the labels: %s: %s\n", err, in_path);
        goto done;
    }
    int64_t *before = counts + 3 * SIFT3D_LABEL_COUNT, *after = counts + 4 * SIFT3D_LABEL_COUNT;
    const int64_t n_before = count_components(p.device, in.data, in.nx, in.ny, in.nz, p.connectivity, before, err, sizeof err);
    const int64_t n_after = n_before < 0 ? -1 : count_components(p.device, out, in.nx, in.ny, in.nz, p.connectivity, after, err, sizeof err);
    if (n_before < 0 || n_after < 0) {
        printf("Error: could not count the components: %s\n", err);
        goto done;
    }
    if (nifti_min_write_f32_geom(out_path, out, in_path) != 0) {
        printf("Error: could not write output file: %s\n", out_path);
        goto done;
    }
    char text[4096];
    path = cli_path(out_path, ".clean.txt");
    if (!path || !(o = fopen(path, "w"))) {
        printf("Error: could not write output file: %s.clean.txt\n", out_path);
        goto done;
    }
    fprintf(o, "# featClean min_voxels %d connectivity %d rounds %d\n", (int)p.min_voxels, (int)p.connectivity, (int)p.rounds);
    sift3d_clean_report_text(&rep, text, sizeof text);
    fputs(text, o);
    fprintf(o, "# label components_before components_after\n");
    for (int l = 0; l < SIFT3D_LABEL_COUNT; l++)
        if (before[l] > 0 || after[l] > 0) fprintf(o, "%d\t%lld\t%lld\n", l, (long long)before[l], (long long)after[l]);
    fprintf(o, "# components %lld before %lld after\n", (long long)n_before, (long long)n_after);
    if (truth_path) {
        const float *vols[2] = {in.data, out};
        const char *title[2] = {"input", "output"};
        for (int v = 0; v < 2; v++) {
            const int src = score(o, title[v], p.device, vols[v], &truth, measure ? spacing_um : NULL, counts, err, sizeof err);
            if (src == -2) printf("Error: a voxel of the truth is neither non-finite nor an integer 0 .. 65535: %s\n", truth_path);
            else if (src != 0) printf("Error: could not take the surface distances: %s\n", err);
            if (src != 0) goto done;
        }
    }
    const int closed = fclose(o);
    o = NULL;
    if (closed != 0) {
        printf("Error: could not write output file: %s\n", path);
        goto done;
    }
    rc = 0;
done:
    if (o) fclose(o);
    free(path);
    free(out);
    free(counts);
    nifti_min_free(&in);
    nifti_min_free(&truth);
    return rc;
}
