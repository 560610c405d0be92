/*
 * featCompose.c -- two alignments chained into one.  Beyond the reference.
 *
 *   featCompose [options] <image A> <1.trans.txt> <2.trans.txt> <out>
 *
 * Pair 1 registers moving B to fixed A (<1.trans.txt>, -u1 <field1.nii>), pair 2 moving C to fixed B (<2.trans.txt>,
 * -u2 <field2.nii>), each as featMatchMultiple -a [-e -u] and featResample -i / -r write them.  The output is the pair of "C
 * moving, A fixed": <out>.trans.txt (M1 M2), <out>.field.nii on a node grid over image A (sift3d_compose_field) and
 * <out>.field.txt (the grid, the parameters and the report line), so that
 *   featResample -u <out>.field.nii <image A> <image C> <out>.trans.txt <x>
 * puts C on A's grid with one interpolation, and -r and -j work on the pair unchanged.  Only image A's header is read; image B
 * is not needed.  A longer chain is a left fold: feed the output pair back in as pair 1.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cli_common.h"

static void print_options(void)
{
    printf("Composition of two feature alignment transforms and displacement fields v1.0\n");
    printf("Usage: %s [options] <image A> <1.trans.txt> <2.trans.txt> <out>\n", "featCompose");
    printf("  <image A>: nifti (.nii,.hdr,.nii.gz), the fixed image of pair 1: its grid carries the composite field.\n");
    printf("  <1.trans.txt>: the 4x4 transform of pair 1 (moving B, fixed A).\n");
    printf("  <2.trans.txt>: the 4x4 transform of pair 2 (moving C, fixed B).\n");
    printf("  <out>: writes <out>.trans.txt, <out>.field.nii and <out>.field.txt, the pair of moving C, fixed A.\n");
    printf(" [options]\n");
    printf("  -w          : the features were extracted with -w (world coordinates, NIFTI qto_xyz matrix).\n");
    printf("  -ws         : the features were extracted with -ws (world coordinates, NIFTI sto_xyz matrix).\n");
    printf("  -u1 <field> : the displacement field of pair 1.\n");
    printf("  -u2 <field> : the displacement field of pair 2.\n");
    printf("  -h<spacing> : node spacing of the composite field (default: field 1's, else field 2's, else 4).\n");
    printf("  -d[0-9]     : set device id to be used.\n");
}

/* the composite field to <out>.field.nii, its grid, the parameters and the report to <out>.field.txt */
static int write_composite(const char *out_path, const sift3d_field *f, const sift3d_compose_params *p, const sift3d_compose_report *rep)
{
    FILE *o = cli_write_field(out_path, ".field", f);
    if (!o) return -1;
    fprintf(o, " radius %f margin %d\n", p->radius, p->margin);
    fprintf(o, "# nodes outside1 outside2 zeroed max_disp folds residual_cells rms_residual max_residual\n");
    fprintf(o, "%lld\t%lld\t%lld\t%lld\t%f\t%lld\t%lld\t%g\t%g\n", (long long)rep->nodes, (long long)rep->outside1, (long long)rep->outside2,
            (long long)rep->zeroed, rep->max_disp, (long long)rep->folds, (long long)rep->residual_cells, rep->rms_residual, rep->max_residual);
    return fclose(o);
}

int main(int argc, char **argv)
{
    int device = 0, world_mode = 0;
    const char *field_path[2] = {NULL, NULL};
    float spacing = 0.0f;
    int arg = 1;
    while (arg < argc && argv[arg][0] == '-') {
        switch (argv[arg][1]) {
        case 'w':
        case 'W':
            world_mode = cli_world_mode(argv[arg]);
            break;
        case 'd':
            if ((device = cli_device(argv[arg])) < 0) return cli_refuse(print_options, "unknown device: %s", argv[arg] + 2);
            break;
        case 'h':
            if (cli_float(argv[arg] + 2, &spacing) != 0 || !(spacing > 0.0f)) return cli_refuse(print_options, "bad spacing: %s", argv[arg]);
            break;
        case 'u':
            if ((argv[arg][2] != '1' && argv[arg][2] != '2') || argv[arg][3] != 0 || arg + 1 >= argc)
                return cli_refuse(print_options, "-u1 and -u2 need a field file");
            field_path[argv[arg][2] - '1'] = argv[arg + 1];
            arg++;
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
    const char *a_path = argv[arg], *trans_path[2] = {argv[arg + 1], argv[arg + 2]}, *out_path = argv[arg + 3];

    nifti_min_image a;
    nifti_min_stream *as = NULL;
    if (nifti_min_open(a_path, &a, &as) != 0) { /* the header is all image A gives */
        printf("Error: could not read input file: %s\n", a_path);
        return -1;
    }
    nifti_min_close(as);
    float m[2][16], mc[16], mr[16], av[16];
    for (int k = 0; k < 2; k++)
        if (sift3d_read_similarity(trans_path[k], m[k]) != 0) {
            printf("Error: could not read transform file: %s\n", trans_path[k]);
            return -1;
        }
    cli_image_vox2key(&a, world_mode, av);
    sift3d_field field[2];
    for (int k = 0; k < 2; k++)
        if (field_path[k] && cli_read_field(field_path[k], &field[k]) != 0) return -1;
    const sift3d_field *f1 = field_path[0] ? &field[0] : NULL, *f2 = field_path[1] ? &field[1] : NULL;

    char *path = cli_path(out_path, ".trans.txt");
    if (!path) return -1;
    /* the composite matrix as a reader of the file gets it: the field below is solved against these digits */
    if (sift3d_compose_matrix(m[0], m[1], mc) != 0 || sift3d_write_matrix(path, mc) != 0 || sift3d_read_similarity(path, mr) != 0) {
        printf("Error: could not compose the transforms or write: %s\n", path);
        return -1;
    }
    free(path);
    sift3d_compose_params p;
    sift3d_compose_defaults(&p);
    p.spacing = spacing;
    sift3d_field out;
    memset(&out, 0, sizeof out);
    if (sift3d_compose_grid(a.nx, a.ny, a.nz, av, &p, f1, f2, &out) != SIFT3D_OK) {
        /* sift3d_field_size refuses a spacing that is not positive and finite, and a grid too long or too large */
        const float h = sift3d_compose_spacing(&p, f1, f2);
        if (!(h > 0.0f) || h > 3.0e38f) printf("Error: bad node spacing for the composite field: %g (set one with -h)\n", h);
        else printf("Error: the composite field's grid at spacing %g has more than %lld nodes (or 2^24 along an axis)\n", h, (long long)p.max_nodes);
        return -1;
    }
    printf("Composing: %s . %s on %s (i=%d j=%d k=%d): %lld x %lld x %lld nodes, spacing %g\n", trans_path[0], trans_path[1], a_path, a.nx, a.ny, a.nz,
           (long long)out.n[0], (long long)out.n[1], (long long)out.n[2], out.spacing);
    char err[512] = "";
    sift3d_compose_report rep;
    if (cli_alloc_field(&out) != 0 || sift3d_compose_field(device, m[0], m[1], mr, f1, f2, &p, &out, &rep, err, sizeof err) != SIFT3D_OK) {
        printf("Error: could not compose the fields: %s\n", out.disp ? err : "insufficient memory");
        return -1;
    }
    if (write_composite(out_path, &out, &p, &rep) != 0) {
        printf("Error: could not write the field files of: %s\n", out_path);
        return -1;
    }
    if (rep.zeroed)
        printf("Warning: the composite field is out of range at %lld of %lld nodes (set to 0)\n", (long long)rep.zeroed, (long long)rep.nodes);
    if (rep.max_residual > 0.5)
        printf("Warning: the composite field's grid is too coarse: interpolation residual up to %g key units (rms %g over %lld cells); "
               "use a smaller -h\n",
               rep.max_residual, rep.rms_residual, (long long)rep.residual_cells);
    free(out.disp);
    for (int k = 0; k < 2; k++)
        if (field_path[k]) free(field[k].disp);
    printf("\nDone.\n");
    return 0;
}
