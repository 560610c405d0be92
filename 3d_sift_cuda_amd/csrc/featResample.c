/*
 * featResample.c -- the third step after featExtract and featMatchMultiple -a: the moving image resampled onto the fixed
 * image's grid through the <moving>.trans.txt that -a wrote.  Beyond the reference, which stops at
 * the matrix.
 *
 *   featResample [options] <fixed image> <moving image> <moving.trans.txt> <output image>
 *
 * .trans.txt maps the moving image's key coordinates to the fixed image's.  A blob centred on voxel x gets a key at
 * x + 0.5 by default, and at qto_xyz / sto_xyz . (x + 0.5 f) under featExtract -w / -ws, f = min(voxel) / voxel
 * (sift3d_key_vox2key; tests/test_resample_cpu.py pins both forms on the oracle's extraction).  Keys of -2+ / -2-
 * extractions are not supported.  The output is float32 with the fixed image's dims, voxel sizes, qform and sform.
 * -u <moving.field.nii>: through the transform and the displacement field featMatchMultiple -a -e -u wrote
 * (sift3d_resample_field).
 * -i[<rounds>]: refine the field (-u's, or zero) from the two images by block matching first
 * (sift3d_refine_field_intensity; default 2 rounds), write it to <output image>.field.nii and its
 * report to <output image>.field.txt, and resample through it.
 * -c (with -i): match the blocks by their normalised correlation instead of their squared differences
 * (sift3d_refine_field_intensity_metric): for images that do not share an intensity scale.
 * -r: the other direction: <output image> is the FIXED image on the MOVING image's grid.  The inverse of
 * the transform goes to <output image>.inv.trans.txt; with -u and / or -i the inverse of the field (of the refined one under
 * -i) goes to <output image>.inv.field.nii and its report to <output image>.inv.field.txt (sift3d_invert_field).  The pair is an
 * ordinary transform and field with the two images' roles swapped:
 *   featResample -u <out>.inv.field.nii <moving image> <fixed image> <out>.inv.trans.txt <x>   writes the same voxels.
 * -j: also <output image>.jac.nii, the Jacobian determinant of the map that was applied, on the output grid
 * (sift3d_jacobian_map): below or at 0 where the map folds.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cli_common.h"

static void print_options(void)
{
    printf("Volumetric image resampling by a feature alignment transform v1.0\n");
    printf("Usage: %s [options] <fixed image> <moving image> <moving.trans.txt> <output image>\n", "featResample");
    printf("  <fixed image>: nifti (.nii,.hdr,.nii.gz), the grid of the output.\n");
    printf("  <moving image>: nifti (.nii,.hdr,.nii.gz), the image to resample.\n");
    printf("  <moving.trans.txt>: the 4x4 transform featMatchMultiple -a wrote for the moving image.\n");
    printf("  <output image>: float32 nifti (.nii,.nii.gz) on the fixed image's grid.\n");
    printf(" [options]\n");
    printf("  -w         : the features were extracted with -w (world coordinates, NIFTI qto_xyz matrix).\n");
    printf("  -ws        : the features were extracted with -ws (world coordinates, NIFTI sto_xyz matrix).\n");
    printf("  -n         : nearest-neighbour interpolation (label maps; default is trilinear).\n");
    printf("  -l         : label-aware linear interpolation (label maps: the label with the largest trilinear weight; not with -n).\n");
    printf("  -f<value>  : value of output voxels that map outside the moving image (default 0).\n");
    printf("  -d[0-9]    : set device id to be used.\n");
    printf("  -u <field> : also through the displacement field featMatchMultiple -a -e -u wrote (<moving>.field.nii).\n");
    printf("  -i[rounds] : refine the field (-u's, or zero) from the image intensities by block matching (default 2 rounds),\n");
    printf("               write <output image>.field.nii and .field.txt, and resample through the refined field.\n");
    printf("  -c         : with -i, match blocks by normalised correlation: for images on different intensity scales.\n");
    printf("  -r         : reverse: resample the fixed image onto the moving image's grid through the inverse map; writes\n");
    printf("               <output image>.inv.trans.txt and, with -u or -i, <output image>.inv.field.nii and .inv.field.txt.\n");
    printf("  -j         : also write <output image>.jac.nii, the Jacobian determinant of the applied map (<= 0: a fold).\n");
}

/* -i: the refined field to <out>.field.nii, its grid and the report of every round to <out>.field.txt */
static int write_refined(const char *out_path, const sift3d_field *f, const sift3d_blockmatch_params *p, const sift3d_blockmatch_report *rep,
                         int metric, const float moving_range[2])
{
    FILE *o = cli_write_field(out_path, ".field", f);
    if (!o) return -1;
    fprintf(o, " radius %f lambda %f\n", p->radius, p->lambda);
    fprintf(o, "# stride %d block %d search %d rounds %d variance_quantile %f cost_fraction %f quantised over %g .. %g%s\n", p->stride, p->block,
            p->search, p->rounds, p->variance_quantile, p->cost_fraction, rep->lo, rep->hi,
            rep->empty_range ? " (empty: nothing matched)" : "");
    if (metric == SIFT3D_BLOCKMATCH_NCC)
        fprintf(o, "# metric ncc fixed quantised over %g .. %g moving quantised over %g .. %g\n", rep->lo, rep->hi, moving_range[0],
                moving_range[1]);
    fprintf(o, "# round nodes samples kept flagged gated_variance gated_border gated_cost rms_before rms_after max_disp folds\n");
    for (int k = 0; k < rep->rounds; k++) {
        const sift3d_blockmatch_round *r = &rep->round[k];
        fprintf(o, "%d\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%f\t%f\t%f\t%lld\n", k + 1, (long long)r->nodes, (long long)r->samples,
                (long long)r->kept, (long long)r->flagged, (long long)r->gated_variance, (long long)r->gated_border, (long long)r->gated_cost,
                r->rms_before, r->rms_after, r->max_disp, (long long)r->folds);
    }
    return fclose(o);
}

/* -r: the inverse field to <out>.inv.field.nii, its grid, the parameters and the report to <out>.inv.field.txt */
static int write_inverse(const char *out_path, const sift3d_field *f, const sift3d_invert_params *p, const sift3d_invert_report *rep)
{
    FILE *o = cli_write_field(out_path, ".inv.field", f);
    if (!o) return -1;
    fprintf(o, " radius %f\n", p->radius);
    fprintf(o, "# max_iter %d tol %g\n", p->max_iter, p->tol);
    fprintf(o, "# nodes converged not_converged diverged max_steps rms_residual max_residual max_disp folds\n");
    fprintf(o, "%lld\t%lld\t%lld\t%lld\t%d\t%g\t%g\t%f\t%lld\n", (long long)rep->nodes, (long long)rep->converged, (long long)rep->not_converged,
            (long long)rep->diverged, rep->max_steps, rep->rms_residual, rep->max_residual, rep->max_disp, (long long)rep->folds);
    return fclose(o);
}

/* -j: the Jacobian determinant map of (map, out_vox2key, src_vox2key, field) to <out>.jac.nii with the geometry of geom_path */
static int write_jacobian(int device, const char *out_path, const char *geom_path, int nx, int ny, int nz, const float map[12],
                          const float out_vox2key[16], const float src_vox2key[16], const sift3d_field *field)
{
    char err[512] = "";
    char *path = cli_path(out_path, ".jac.nii");
    float *jac = (float *)malloc(sizeof(float) * (size_t)nx * ny * nz);
    int rc = -1;
    if (path && jac) {
        if (sift3d_jacobian_map(device, nx, ny, nz, map, out_vox2key, src_vox2key, field, jac, -1, NULL, err, sizeof err) != SIFT3D_OK)
            printf("Error: could not compute the Jacobian map: %s\n", err);
        else if (nifti_min_write_f32_geom(path, jac, geom_path) != 0) printf("Error: could not write output file: %s\n", path);
        else rc = 0;
    }
    free(path);
    free(jac);
    return rc;
}

/* -r: everything after the forward field is known.  t: the forward transform; field: the forward field, or NULL. */
static int reverse(int device, const char *fixed_path, const char *moving_path, const char *out_path, const nifti_min_image *fixed,
                   const nifti_min_image *moving, const float t[16], const float fv[16], const float mv[16], const sift3d_field *field, int interp,
                   float fill, int jacobian)
{
    char err[512] = "";
    float ti[16], tr[16], rmap[12];
    char *path = cli_path(out_path, ".inv.trans.txt");
    if (!path) return -1;
    /* the inverse as a reader of the file gets it: the field below is solved against these digits */
    if (sift3d_affine_invert(t, ti) != 0 || sift3d_write_matrix(path, ti) != 0 || sift3d_read_similarity(path, tr) != 0 ||
        sift3d_resample_map(tr, mv, fv, rmap) != 0) {
        printf("Error: could not invert the transform or write: %s\n", path);
        free(path);
        return -1;
    }
    free(path);
    const size_t n_out = (size_t)moving->nx * moving->ny * moving->nz;
    float *out = (float *)malloc(sizeof(float) * n_out);
    if (!out) {
        printf("Error: could not resample, insufficient memory.\n");
        return -1;
    }
    sift3d_field inv;
    memset(&inv, 0, sizeof inv);
    double ms = 0;
    int rc;
    if (field) {
        sift3d_invert_params ip;
        sift3d_invert_defaults(&ip);
        ip.spacing = field->spacing;
        sift3d_invert_report rep;
        if (sift3d_invert_grid(moving->nx, moving->ny, moving->nz, mv, &ip, &inv) != SIFT3D_OK) {
            printf("Error: the inverse field's grid has more than %lld nodes\n", (long long)ip.max_nodes);
            return -1;
        }
        if (cli_alloc_field(&inv) != 0 || sift3d_invert_field(device, t, tr, field, &ip, &inv, &rep, err, sizeof err) != SIFT3D_OK) {
            printf("Error: could not invert the field: %s\n", inv.disp ? err : "insufficient memory");
            return -1;
        }
        if (write_inverse(out_path, &inv, &ip, &rep) != 0) {
            printf("Error: could not write the inverse field files of: %s\n", out_path);
            return -1;
        }
        if (rep.not_converged || rep.diverged)
            printf("Warning: the inverse field did not converge everywhere: %lld of %lld nodes not converged, %lld diverged (set to 0)\n",
                   (long long)rep.not_converged, (long long)rep.nodes, (long long)rep.diverged);
        rc = sift3d_resample_field(device, fixed->data, fixed->nx, fixed->ny, fixed->nz, out, moving->nx, moving->ny, moving->nz, rmap, mv, fv, &inv,
                                   interp, fill, &ms, err, sizeof err);
    } else {
        rc = sift3d_resample_affine(device, fixed->data, fixed->nx, fixed->ny, fixed->nz, out, moving->nx, moving->ny, moving->nz, rmap, interp, fill,
                                    &ms, err, sizeof err);
    }
    if (rc != SIFT3D_OK) {
        printf("Error: could not resample: %s\n", err);
        return -1;
    }
    if (nifti_min_write_f32_geom(out_path, out, moving_path) != 0) {
        printf("Error: could not write output file: %s\n", out_path);
        return -1;
    }
    free(out);
    if (jacobian && write_jacobian(device, out_path, moving_path, moving->nx, moving->ny, moving->nz, rmap, mv, fv, field ? &inv : NULL) != 0) return -1;
    free(inv.disp);
    (void)fixed_path;
    return 0;
}

int main(int argc, char **argv)
{
    int device = 0, world_mode = 0, nearest = 0, label = 0;
    float fill = 0.0f;
    const char *field_path = NULL;
    int intensity = 0, rounds = -1, metric = SIFT3D_BLOCKMATCH_SSD, backward = 0, jacobian = 0;
    int arg = 1;
    while (arg < argc && argv[arg][0] == '-') {
        switch (argv[arg][1]) {
        case 'w':
        case 'W':
            world_mode = cli_world_mode(argv[arg]);
            break;
        case 'n':
            nearest = 1;
            break;
        case 'l':
            if (!cli_bare(argv[arg])) return cli_refuse(print_options, "unknown command line argument: %s", argv[arg]);
            label = 1;
            break;
        case 'f':
            if (cli_float(argv[arg] + 2, &fill) != 0) return cli_refuse(print_options, "bad fill value: %s", argv[arg]);
            break;
        case 'd':
            if ((device = cli_device(argv[arg])) < 0) return cli_refuse(print_options, "unknown device: %s", argv[arg] + 2);
            break;
        case 'i':
            intensity = 1;
            if (!cli_bare(argv[arg]) && cli_int(argv[arg] + 2, 0, SIFT3D_BLOCKMATCH_MAX_ROUNDS, &rounds) != 0)
                return cli_refuse(print_options, "bad number of rounds: %s", argv[arg]);
            break;
        case 'c':
            if (!cli_bare(argv[arg])) return cli_refuse(print_options, "unknown command line argument: %s", argv[arg]);
            metric = SIFT3D_BLOCKMATCH_NCC;
            break;
        case 'r':
        case 'j':
            if (!cli_bare(argv[arg])) return cli_refuse(print_options, "unknown command line argument: %s", argv[arg]);
            if (argv[arg][1] == 'r') backward = 1;
            else jacobian = 1;
            break;
        case 'u':
            if (!cli_bare(argv[arg]) || arg + 1 >= argc) return cli_refuse(print_options, "-u needs a field file");
            field_path = argv[++arg];
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
    if (nearest && label) return cli_refuse(print_options, "-n and -l are two interpolations: give one");
    const int interp = label ? SIFT3D_INTERP_LABEL : (nearest ? SIFT3D_INTERP_NEAREST : SIFT3D_INTERP_LINEAR);
    if (metric != SIFT3D_BLOCKMATCH_SSD && !intensity) return cli_refuse(print_options, "-c needs -i");
    const char *fixed_path = argv[arg], *moving_path = argv[arg + 1], *trans_path = argv[arg + 2], *out_path = argv[arg + 3];

    nifti_min_image fixed, moving;
    nifti_min_stream *fs = NULL;
    if (nifti_min_open(fixed_path, &fixed, &fs) != 0) { /* the header is all the fixed image gives */
        printf("Error: could not read input file: %s\n", fixed_path);
        return -1;
    }
    nifti_min_close(fs);
    /* -i matches against the fixed image's voxels, -r resamples them */
    if ((intensity || backward) && cli_read_image(fixed_path, &fixed) != 0) return -1;
    if (cli_read_image(moving_path, &moving) != 0) return -1;
    float t[16], fv[16], mv[16], map[12];
    if (sift3d_read_similarity(trans_path, t) != 0) {
        printf("Error: could not read transform file: %s\n", trans_path);
        return -1;
    }
    cli_image_vox2key(&fixed, world_mode, fv);
    cli_image_vox2key(&moving, world_mode, mv);
    if (sift3d_resample_map(t, fv, mv, map) != 0) {
        printf("Error: singular transform: %s\n", trans_path);
        return -1;
    }
    if (!backward)
        printf("Resampling: %s (i=%d j=%d k=%d) onto %s (i=%d j=%d k=%d)\n", moving_path, moving.nx, moving.ny, moving.nz, fixed_path, fixed.nx,
               fixed.ny, fixed.nz);
    const size_t n_out = (size_t)fixed.nx * fixed.ny * fixed.nz;
    float *out = (float *)malloc(sizeof(float) * n_out);
    if (!out) {
        printf("Error: could not resample, insufficient memory.\n");
        return -1;
    }
    char err[512] = "";
    double ms = 0;
    sift3d_field field;
    memset(&field, 0, sizeof field);
    if (field_path && cli_read_field(field_path, &field) != 0) return -1;
    if (intensity) {
        sift3d_blockmatch_params bp;
        sift3d_blockmatch_defaults(&bp);
        if (rounds >= 0) bp.rounds = rounds;
        sift3d_blockmatch_report rep;
        sift3d_field refined;
        memset(&refined, 0, sizeof refined);
        float mrange[2] = {0, 0};
        int irc = sift3d_refine_field_intensity_metric(device, fixed.data, fixed.nx, fixed.ny, fixed.nz, moving.data, moving.nx, moving.ny, moving.nz,
                                                       fv, mv, t, field_path ? &field : NULL, &bp, metric, &refined, &rep, mrange, err, sizeof err);
        if (irc == SIFT3D_ERR_CAPACITY) {
            refined.capacity = 3 * refined.n[0] * refined.n[1] * refined.n[2];
            if (field_path && field.capacity > refined.capacity) refined.capacity = field.capacity;
            refined.disp = (float *)malloc(sizeof(float) * (size_t)refined.capacity);
            irc = refined.disp ? sift3d_refine_field_intensity_metric(device, fixed.data, fixed.nx, fixed.ny, fixed.nz, moving.data, moving.nx,
                                                                      moving.ny, moving.nz, fv, mv, t, field_path ? &field : NULL, &bp, metric,
                                                                      &refined, &rep, mrange, err, sizeof err)
                               : SIFT3D_ERR_MEMORY;
        }
        if (irc != SIFT3D_OK) {
            printf("Error: could not refine the field: %s\n", err);
            return -1;
        }
        if (write_refined(out_path, &refined, &bp, &rep, metric, mrange) != 0) {
            printf("Error: could not write the field files of: %s\n", out_path);
            return -1;
        }
        free(field.disp);
        field = refined;
    }
    if (backward) {
        printf("Resampling: %s (i=%d j=%d k=%d) onto %s (i=%d j=%d k=%d)\n", fixed_path, fixed.nx, fixed.ny, fixed.nz, moving_path, moving.nx, moving.ny,
               moving.nz);
        if (reverse(device, fixed_path, moving_path, out_path, &fixed, &moving, t, fv, mv, field_path || intensity ? &field : NULL, interp, fill,
                    jacobian) != 0)
            return -1;
        printf("\nDone.\n");
        free(field.disp);
        free(out);
        nifti_min_free(&moving);
        return 0;
    }
    /* the first volume of a 4-D moving image */
    const int rc = field_path || intensity
                       ? sift3d_resample_field(device, moving.data, moving.nx, moving.ny, moving.nz, out, fixed.nx, fixed.ny, fixed.nz, map, fv, mv,
                                               &field, interp, fill, &ms, err, sizeof err)
                       : sift3d_resample_affine(device, moving.data, moving.nx, moving.ny, moving.nz, out, fixed.nx, fixed.ny, fixed.nz, map,
                                                interp, fill, &ms, err, sizeof err);
    if (rc != SIFT3D_OK) {
        printf("Error: could not resample: %s\n", err);
        return -1;
    }
    if (nifti_min_write_f32_geom(out_path, out, fixed_path) != 0) {
        printf("Error: could not write output file: %s\n", out_path);
        return -1;
    }
    if (jacobian && write_jacobian(device, out_path, fixed_path, fixed.nx, fixed.ny, fixed.nz, map, fv, mv, field_path || intensity ? &field : NULL) != 0)
        return -1;
    free(field.disp);
    printf("\nDone.\n");
    free(out);
    nifti_min_free(&moving);
    return 0;
}
