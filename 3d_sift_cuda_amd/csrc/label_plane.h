/*
 * label_plane.h -- how the label tools read a label on the device (DESIGN.md sections 7j, 7l, 7m, 7o): a finite float label is an
 * integer 0 .. 65535 (the host has checked it: sift3d_fuse_check_labels), kept as its 16 bits; a label plane is those uint16 and
 * one validity bit per voxel, bit i & 63 of word i >> 6 (label_plane_kernel of kernels_label.hip writes both).  Device inlines
 * only.
 */
#ifndef SIFT3D_LABEL_PLANE_H
#define SIFT3D_LABEL_PLANE_H

/* the 16 bits of a finite label */
__device__ __forceinline__ unsigned label_bits(float v) { return (unsigned)(int)v & 0xffffu; }

/* the voxel holds a label: its float was finite */
__device__ __forceinline__ bool label_valid(const unsigned long long *valid, long long i) { return ((valid[i >> 6] >> (i & 63)) & 1ull) != 0; }

#endif
