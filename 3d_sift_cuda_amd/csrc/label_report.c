/*
 * label_report.c -- see label_report.h.
 */
#include <stdlib.h>
#include <string.h>

#include "label_report.h"
#include "sift3d.h"

void label_report_dice(FILE *o, const int64_t *ca, const int64_t *cb, const int64_t *cboth)
{
    double sum = 0;
    int64_t present = 0;
    fprintf(o, "# label fused truth both dice\n");
    for (int l = 0; l < SIFT3D_LABEL_COUNT; l++)
        if (ca[l] > 0 || cb[l] > 0) {
            const double dice = (double)(2 * cboth[l]) / (double)(ca[l] + cb[l]);
            fprintf(o, "%d\t%lld\t%lld\t%lld\t%.6f\n", l, (long long)ca[l], (long long)cb[l], (long long)cboth[l], dice);
            sum += dice;
            present++;
        }
    fprintf(o, "# mean dice %.6f over %lld labels\n", present > 0 ? sum / (double)present : 0.0, (long long)present);
}

int label_report_spacing(float dx, float dy, float dz, uint32_t spacing_um[3], char *err, size_t err_len)
{
    const float mm[3] = {dx, dy, dz};
    for (int c = 0; c < 3; c++)
        if (sift3d_spacing_um(mm[c], &spacing_um[c]) != 0) {
            snprintf(err, err_len, "the voxel size %g mm along %c is not 0.001 .. 65.535 mm: no distances in micrometres", (double)mm[c], "xyz"[c]);
            return -1;
        }
    return 0;
}

int label_report_common_spacing(const nifti_min_image *a, const nifti_min_image *b, const char *a_path, const char *b_path, uint32_t spacing_um[3])
{
    char err[512] = "";
    uint32_t other_um[3];
    if (label_report_spacing(a->dx, a->dy, a->dz, spacing_um, err, sizeof err) != 0) {
        printf("Error: %s: %s\n", err, a_path);
        return -1;
    }
    if (label_report_spacing(b->dx, b->dy, b->dz, other_um, err, sizeof err) != 0) {
        printf("Error: %s: %s\n", err, b_path);
        return -1;
    }
    if (memcmp(spacing_um, other_um, sizeof other_um) != 0) {
        printf("Error: the images are not on one grid: voxels of %u x %u x %u um against %u x %u x %u um\n", (unsigned)spacing_um[0], (unsigned)spacing_um[1],
               (unsigned)spacing_um[2], (unsigned)other_um[0], (unsigned)other_um[1], (unsigned)other_um[2]);
        return -1;
    }
    return 0;
}

int label_report_distances(FILE *o, int device, const float *a, const float *b, int64_t nx, int64_t ny, int64_t nz, const uint32_t spacing_um[3],
                           int32_t first_label, char *err, size_t err_len)
{
    sift3d_surface_params p;
    sift3d_surface_defaults(&p);
    p.first_label = first_label;
    p.device = device;
    sift3d_surface_record *rec = (sift3d_surface_record *)malloc(sizeof *rec * (size_t)p.max_labels);
    int32_t n = 0;
    if (!rec) {
        snprintf(err, err_len, "insufficient memory");
        return -1;
    }
    if (sift3d_surface_distances(a, b, nx, ny, nz, spacing_um, &p, rec, &n, NULL, err, (int64_t)err_len) != SIFT3D_OK) {
        free(rec);
        return -1;
    }
    double hd = 0, hd95 = 0, assd = 0;
    int both = 0;
    fprintf(o, "# spacing_um %u %u %u\n", (unsigned)spacing_um[0], (unsigned)spacing_um[1], (unsigned)spacing_um[2]);
    fprintf(o, "# label surf_fused surf_truth hausdorff_mm hd95_mm assd_mm\n");
    for (int32_t k = 0; k < n; k++) {
        fprintf(o, "%d\t%lld\t%lld\t%.6f\t%.6f\t%.6f\n", rec[k].label, (long long)rec[k].n_a, (long long)rec[k].n_b, rec[k].hausdorff_mm, rec[k].hd95_mm,
                rec[k].assd_mm);
        if (rec[k].n_a > 0 && rec[k].n_b > 0) {
            hd += rec[k].hausdorff_mm;
            hd95 += rec[k].hd95_mm;
            assd += rec[k].assd_mm;
            both++;
        }
    }
    fprintf(o, "# mean hausdorff_mm %.6f hd95_mm %.6f assd_mm %.6f over %d labels\n", both ? hd / both : 0.0, both ? hd95 / both : 0.0, both ? assd / both : 0.0,
            both);
    free(rec);
    return 0;
}
