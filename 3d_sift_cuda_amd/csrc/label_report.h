/*
 * label_report.h -- the two tables with which featFuse -t [-m] and featOverlap score one label volume against another: the Dice
 * overlap per label and the surface distances per label (DESIGN.md sections 7j and 7l).  Command-line code: not part of the C-ABI.
 */
#ifndef SIFT3D_LABEL_REPORT_H
#define SIFT3D_LABEL_REPORT_H
#include <stdint.h>
#include <stdio.h>

#include "nifti_min.h"

/* "# label fused truth both dice", a line per label that either volume has and the mean line, from sift3d_label_overlap's counts */
void label_report_dice(FILE *o, const int64_t *count_a, const int64_t *count_b, const int64_t *count_both);
/* The voxel sizes of an image header in micrometres (sift3d_spacing_um); 0, or -1 with the reason in err */
int label_report_spacing(float dx, float dy, float dz, uint32_t spacing_um[3], char *err, size_t err_len);
/* label_report_spacing of two images that must agree in it, into spacing_um; 0, or -1 with the message printed: either image's voxel
 * size refused (with its path), or "not on one grid" */
int label_report_common_spacing(const nifti_min_image *a, const nifti_min_image *b, const char *a_path, const char *b_path, uint32_t spacing_um[3]);
/* The "# spacing_um" line, "# label surf_fused surf_truth hausdorff_mm hd95_mm assd_mm", a line per label from first_label on
 * (sift3d_surface_distances of a against b on the device) and the mean line over the labels both volumes have; 0, or -1 with the
 * library's reason in err */
int label_report_distances(FILE *o, int device, const float *a, const float *b, int64_t nx, int64_t ny, int64_t nz, const uint32_t spacing_um[3],
                           int32_t first_label, char *err, size_t err_len);
#endif
