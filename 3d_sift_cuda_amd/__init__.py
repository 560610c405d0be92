"""3d_sift_cuda_amd -- MI355X-native 3D SIFT extraction path (Python mirror of the C-ABI).

Thin ctypes layer over ``csrc/_build/libsift3d_hip.so`` (``include/sift3d.h``).  The
names follow the reference's operator interface for this path
(R/cuda_common/SIFT_cuda_Tools.cuh, R/src_common/MultiScale.h; R/ =
/root/reference/3dsift_cleanup-softVote_App_Weight_SoftMax/):

=====================  =====================================================================
here                   reference entry point it replaces
=====================  =====================================================================
``gauss_blur``         gb3d_blur3d -> blur_3d_simpleborders_CUDA_Row_Col_Shared_mem (.cuh:69-76)
``dog``                fioMultSum_interleave(.., -1.0f) -> fioCudaMultSum (.cuh:213-217)
``subsample2``         Subsample_interleave -> SubSampleInterpolateCuda (.cuh:202-205)
``extrema``            detectExtrema4D_test_interleave -> detectExtrema4D_test_cuda (.cuh:32-38)
``detect``/``extract`` msGeneratePyramidDOG3D_efficient (MultiScale.h:534-543) + main()'s descriptor loop
=====================  =====================================================================

There is no CPU fallback: importing works everywhere (the library is only
dlopen'ed on first use), but every compute call raises if the HIP library is
missing or no HIP device is usable.  The package name starts with a digit, so
load it with ``importlib.import_module("3d_sift_cuda_amd")``.
"""
import contextlib
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_HIP = os.path.join(CSRC, "_build", "libsift3d_hip.so")
LIB_HOST = os.path.join(CSRC, "_build", "libsift3d_host.so")
FEATEXTRACT = os.path.join(CSRC, "_build", "featExtract")
FEATRESAMPLE = os.path.join(CSRC, "_build", "featResample")
FEATCOMPOSE = os.path.join(CSRC, "_build", "featCompose")
FEATFUSE = os.path.join(CSRC, "_build", "featFuse")
FEATOVERLAP = os.path.join(CSRC, "_build", "featOverlap")
FEATCLEAN = os.path.join(CSRC, "_build", "featClean")
FEATCOMPARE = os.path.join(CSRC, "_build", "featCompare")
FEATREGISTER = os.path.join(CSRC, "_build", "featRegister")
FEATAVERAGE = os.path.join(CSRC, "_build", "featAverage")
FEATNORMALIZE = os.path.join(CSRC, "_build", "featNormalize")

DESC_SIFT, DESC_BRIEF, DESC_RRIEF, DESC_NRRIEF = 0, 1, 2, 3
ABI_VERSION = 7   # SIFT3D_ABI_VERSION of include/sift3d.h: the structure layouts this file mirrors
INFO_MIN0MAX1, INFO_REORIENT = 0x10, 0x20
STAGES = ("blur_x", "blur_y", "blur_z_dog", "subsample", "extrema", "keypoint", "descriptor", "blur_fused", "octave_tiny")

# sift3d_tuning (include/sift3d.h)
TUNE_BLUR_FUSED, TUNE_FUSED_CHUNKS, TUNE_FUSED_ROWS, TUNE_LAZY_LEVELS, TUNE_TINY_OCTAVE, TUNE_SAMPLER_CAP, TUNE_KP_CHUNKS, TUNE_BANDS_FIRST, TUNE_HOST_RECORDS, TUNE_FUSED_TILE, TUNE_FUSED_SUB, TUNE_SPLIT_TAIL, TUNE_DESC_SEGMENT, TUNE_FUSED_ORDER, TUNE_FUSED_STAGGER, TUNE_DESC_ORDER = range(16)

EXTREMUM_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("z", "<i4"), ("value", "<f4")])
FEATURE_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("scale", "<f4"), ("ori", "<f4", (9,)),
                          ("eigs", "<f4", (3,)), ("info", "<u4"), ("desc", "<f4", (64,))])
CANDIDATE_DTYPE = np.dtype([("octave", "<i4"), ("level", "<i4"), ("is_max", "<i4"), ("x", "<i4"), ("y", "<i4"),
                            ("z", "<i4"), ("value", "<f4"), ("h_value", "<f4"), ("l_value", "<f4")])


class Sift3DError(RuntimeError):
    pass


class _Timings(C.Structure):
    _fields_ = [("ms", C.c_double * len(STAGES)), ("launches", C.c_int64 * len(STAGES)), ("alg_bytes", C.c_double * len(STAGES)),
                ("n_octaves", C.c_int64), ("n_extrema", C.c_int64), ("n_keypoints", C.c_int64),
                ("n_records", C.c_int64), ("total_ms", C.c_double)]


class LevelDesc(C.Structure):
    """sift3d_level_desc (include/sift3d.h)"""
    _fields_ = [("img", C.c_void_p), ("dogc", C.c_void_p), ("nx", C.c_int64), ("ny", C.c_int64), ("nz_local", C.c_int64),
                ("nz_global", C.c_int64), ("z_offset", C.c_int64), ("sigma_h", C.c_float), ("sigma_c", C.c_float),
                ("sigma_l", C.c_float), ("octave_factor", C.c_float)]


LAUNCH_DTYPE = np.dtype([("stage", "<i4"), ("ntaps", "<i4"), ("nvox", "<i8"), ("alg_bytes", "<f8"), ("ms", "<f8"),
                         ("start_ms", "<f8")])


def build(verbose=False):
    """Compile the HIP library, the host helpers and the CLI for gfx950 (in-tree)."""
    r = subprocess.run(["make", "-C", CSRC, "-j4"], capture_output=True, text=True)
    if verbose or r.returncode != 0:
        print(r.stdout[-4000:])
        print(r.stderr[-4000:])
    if r.returncode != 0:
        raise Sift3DError("building 3d_sift_cuda_amd/csrc failed")


_hip = None
_host = None


def _sig(fn, res, *args):
    fn.restype = res
    fn.argtypes = list(args)


def hip_lib():
    """dlopen libsift3d_hip.so and declare the C-ABI; raises if it is not built."""
    global _hip
    if _hip is not None:
        return _hip
    if not os.path.exists(LIB_HIP):
        raise Sift3DError("%s is missing: run __graft_entry__.build() (there is no CPU fallback)" % LIB_HIP)
    L = C.CDLL(LIB_HIP)
    P, I64, F, I = C.c_void_p, C.c_int64, C.c_float, C.c_int
    _sig(L.sift3d_abi_version, I)
    if L.sift3d_abi_version() != ABI_VERSION:   # the library writes whole structures through our pointers
        raise Sift3DError("%s has ABI version %d, this mirror of include/sift3d.h is version %d: rebuild (__graft_entry__.build())"
                          % (LIB_HIP, L.sift3d_abi_version(), ABI_VERSION))
    _sig(L.sift3d_device_count, I)
    _sig(L.sift3d_create, P, I, I64, I64, I64)
    _sig(L.sift3d_create_slab, P, I, I64, I64, I64)
    _sig(L.sift3d_set_tuning, I, P, I, I)
    _sig(L.sift3d_host_buffer_grows, I64, P)
    _sig(L.sift3d_zslab_set_tuning, I, P, I, I)
    _sig(L.sift3d_destroy, None, P)
    _sig(L.sift3d_last_error, C.c_char_p, P)
    _sig(L.sift3d_set_stream, I, P, P)
    _sig(L.sift3d_sync, I, P)
    _sig(L.sift3d_free, None, P)
    _sig(L.sift3d_gauss_taps, I, F, F, P)
    _sig(L.sift3d_set_libm_variant, I, I)
    _sig(L.sift3d_get_libm_variant, I)
    _sig(L.sift3d_gauss_blur, I, P, P, P, I64, I64, I64, F, F)
    _sig(L.sift3d_gauss_blur_dev, I, P, P, P, I64, I64, I64, F, F)
    _sig(L.sift3d_gauss_blur_dog_dev, I, P, P, P, P, I64, I64, I64, F, F)
    _sig(L.sift3d_gauss_blur_dog_half_dev, I, P, P, P, P, P, I64, I64, I64, F, F, C.POINTER(C.c_int))
    _sig(L.sift3d_blur_window_supported, I, I64, I64, F, F)
    _sig(L.sift3d_gauss_blur_dog_window_dev, I, P, P, P, P, I64, I64, I64, I64, I64, F, F)
    _sig(L.sift3d_dog, I, P, P, P, P, I64)
    _sig(L.sift3d_dog_dev, I, P, P, P, P, I64)
    _sig(L.sift3d_subsample2, I, P, P, I64, I64, I64, P)
    _sig(L.sift3d_subsample2_dev, I, P, P, I64, I64, I64, P)
    _sig(L.sift3d_extrema, I, P, P, P, P, I64, I64, I64, P, I64, P, P, I64, P)
    _sig(L.sift3d_double_size, I, P, P, I64, I64, I64, P)
    _sig(L.sift3d_halve_size, I, P, P, I64, I64, I64, P)
    _sig(L.sift3d_selftest_lds_add, I, P, P, P, I64, P, P)
    _sig(L.sift3d_selftest_alloc_fill, I, I, C.POINTER(C.c_uint64))
    _sig(L.sift3d_set_volume, I, P, P, I64, I64, I64)
    _sig(L.sift3d_set_volume_dev, I, P, P, I64, I64, I64)
    _sig(L.sift3d_set_volume_resized, I, P, P, I64, I64, I64, I)
    _sig(L.sift3d_reserve, I, P, I64)
    _sig(L.sift3d_set_volume_begin, I, P, I64, I64, I64, I)
    _sig(L.sift3d_set_volume_planes, I, P, P, I64, I64)
    _sig(L.sift3d_set_volume_end, I, P)
    _sig(L.sift3d_detect, I, P, F, P, P)
    _sig(L.sift3d_extract, I, P, F, I, F, F, P, P)
    _sig(L.sift3d_extract_view, I, P, F, I, F, F, P, P)
    _sig(L.sift3d_enable_timing, I, P, I)
    _sig(L.sift3d_get_timings, I, P, P)
    _sig(L.sift3d_get_launch_log, I, P, P, I64, P)
    _sig(L.sift3d_candidates_reset, I, P)
    _sig(L.sift3d_extrema_append_dev, I, P, P, P, P, I64, I64, I64, I, I64, I64)
    _sig(L.sift3d_lazy_levels_supported, I, I64, I64, I64, F)
    _sig(L.sift3d_extrema_append_lazy_dev, I, P, P, P, P, P, P, P, F, I64, I64, I64, I, I64, I64)
    _sig(L.sift3d_candidates_dev, I, P, P, I, P, P)
    _sig(L.sift3d_describe_dev, I, P, P, I, I, F, F, P, P, P)
    _sig(L.sift3d_describe_dev_counts, I, P, P, I, I, F, F, P, P)
    _sig(L.sift3d_describe_dev_place, I, P, P, P, P, P, P)
    _sig(L.sift3d_host_register, I, P, I64)
    _sig(L.sift3d_host_unregister, I, P)
    _sig(L.sift3d_set_max_octaves, I, P, I)
    _sig(L.sift3d_extract_zslab, I, P, I, P, I64, I64, I64, F, I, F, F, P, P, P, C.c_char_p, I64)
    _sig(L.sift3d_extract_zslab_over, I, I, P, I, P, I64, I64, I64, F, I, F, F, P, P, P, C.c_char_p, I64)
    _sig(L.sift3d_zslab_set_transport_library, None, C.c_char_p)
    _sig(L.sift3d_zslab_create, P, P, I, I64, I64, I64, C.c_char_p, I64)
    _sig(L.sift3d_zslab_extract, I, P, P, F, I, F, F, P, P, P, C.c_char_p, I64)
    _sig(L.sift3d_zslab_destroy, None, P)
    _sig(L.sift3d_zslab_set_volume, I, P, P, C.c_char_p, I64)
    _sig(L.sift3d_zslab_extract_resident, I, P, F, I, F, F, P, P, P, C.c_char_p, I64)
    _sig(L.sift3d_knn64, I, I, P, I64, P, I64, I, P, P, I, P, C.c_char_p, I64)
    _sig(L.sift3d_match_ratio, I, I, P, I64, P, I64, P, P, P, P, P, C.c_char_p, I64)
    _sig(L.sift3d_hough_similarity, I, I, P, P, P, P, P, P, C.c_int32, P, P, P, P, P, C.c_char_p, I64)
    _sig(L.sift3d_match_keys, I, I, P, I64, P, I64, C.c_int32, P, C.c_char_p, I64)
    _sig(L.sift3d_get_level_slice, I, P, I, I, I64, P, P, P)
    _sig(L.sift3d_get_dog_slice, I, P, I, I, I64, P, P, P)
    _sig(L.sift3d_resample_affine, I, I, P, I64, I64, I64, P, I64, I64, I64, P, I, F, P, C.c_char_p, I64)
    _sig(L.sift3d_resample_affine_dev, I, P, P, I64, I64, I64, P, I64, I64, I64, P, I, F)
    _sig(L.sift3d_guided_search_params, I, I, P, I64, P, I64, P, F, P, P, P, P, P, P, P, C.c_char_p, I64)
    _sig(L.sift3d_refine_similarity, I, I, P, I64, P, I64, P, P, P, P, C.c_char_p, I64)
    _sig(L.sift3d_fit_field, I, I, P, P, I64, P, P, P, C.c_char_p, I64)
    _sig(L.sift3d_refine_field, I, I, P, I64, P, I64, P, P, P, P, C.c_char_p, I64)
    _sig(L.sift3d_resample_field, I, I, P, I64, I64, I64, P, I64, I64, I64, P, P, P, P, I, F, P, C.c_char_p, I64)
    _sig(L.sift3d_block_match, I, I, P, P, I64, I64, I64, P, I64, P, I, I, I, P, P, C.c_char_p, I64)
    _sig(L.sift3d_refine_field_intensity, I, I, P, I64, I64, I64, P, I64, I64, I64, P, P, P, P, P, P, P, C.c_char_p, I64)
    _sig(L.sift3d_block_match_ncc, I, I, P, P, I64, I64, I64, P, I64, P, I, I, I, P, P, C.c_char_p, I64)
    _sig(L.sift3d_refine_field_intensity_metric, I, I, P, I64, I64, I64, P, I64, I64, I64, P, P, P, P, P, I, P, P, P, C.c_char_p, I64)
    _sig(L.sift3d_invert_nodes, I, I, P, P, P, P, P, P, P, P, P, C.c_char_p, I64)
    _sig(L.sift3d_invert_field, I, I, P, P, P, P, P, P, C.c_char_p, I64)
    _sig(L.sift3d_jacobian_map, I, I, I64, I64, I64, P, P, P, P, P, I, P, C.c_char_p, I64)
    _sig(L.sift3d_compose_nodes, I, I, P, P, P, P, P, P, P, P, P, P, P, C.c_char_p, I64)
    _sig(L.sift3d_compose_field, I, I, P, P, P, P, P, P, P, P, C.c_char_p, I64)
    _sig(L.sift3d_fuse_weights, I, I, P, P, I64, I64, I64, C.c_int32, C.c_int32, P, C.c_int32, P, P, C.c_char_p, I64)
    _sig(L.sift3d_fuse_vote, I, I, C.c_int32, P, P, I64, C.c_int32, P, P, C.c_char_p, I64)
    _sig(L.sift3d_fuse_labels, I, I, P, I64, I64, I64, P, C.c_int32, P, P, P, P, C.c_char_p, I64)
    _sig(L.sift3d_fuse_search, I, I, P, P, P, I64, I64, I64, C.c_int32, C.c_int32, C.c_int32, P, C.c_int32, P, P, P, P, C.c_char_p, I64)
    _sig(L.sift3d_fuse_labels_search, I, I, P, I64, I64, I64, P, C.c_int32, P, P, C.c_int32, P, P, P, C.c_char_p, I64)
    _sig(L.sift3d_distance_map, I, I, P, I64, I64, I64, P, P, P, C.c_char_p, I64)
    _sig(L.sift3d_surface_distances, I, P, P, I64, I64, I64, P, P, P, P, P, C.c_char_p, I64)
    _sig(L.sift3d_label_components, I, I, P, I64, I64, I64, C.c_int32, P, P, I64, P, P, C.c_char_p, I64)
    _sig(L.sift3d_clean_labels, I, P, I64, I64, I64, P, P, P, P, C.c_char_p, I64)
    _sig(L.sift3d_joint_histogram, I, I, P, P, I64, I64, I64, P, P, C.c_int32, P, P, P, P, C.c_char_p, I64)
    _sig(L.sift3d_image_similarity, I, P, P, P, I64, I64, I64, P, P, P, P, C.c_char_p, I64)
    _sig(L.sift3d_warp_histogram, I, I, P, I64, I64, I64, P, I64, I64, I64, P, C.c_int32, C.c_int32, P, P, C.c_int32, C.c_int32, P, P, P, P, P, C.c_char_p, I64)
    _sig(L.sift3d_register_affine, I, P, I64, I64, I64, P, I64, I64, I64, P, P, P, P, P, C.c_char_p, I64)
    _sig(L.sift3d_average_warped, I, I64, I64, I64, P, C.c_int32, P, P, P, P, P, P, C.c_char_p, I64)
    _sig(L.sift3d_overlap_histograms, I, I, P, I64, I64, I64, P, P, P, P, P, P, P, P, P, P, C.c_char_p, I64)
    _sig(L.sift3d_apply_transfer, I, I, P, I64, P, P, P, C.c_char_p, I64)
    _sig(L.sift3d_normalize_intensity, I, P, I64, I64, I64, P, P, P, P, P, P, C.c_char_p, I64)
    _hip = L
    return L


def host_lib():
    """dlopen libsift3d_host.so (NIfTI I/O, .key writer, synthetic volumes; no GPU needed)."""
    global _host
    if _host is not None:
        return _host
    if not os.path.exists(LIB_HOST):
        raise Sift3DError("%s is missing: run __graft_entry__.build()" % LIB_HOST)
    L = C.CDLL(LIB_HOST)
    P, I64, F, I = C.c_void_p, C.c_int64, C.c_float, C.c_int
    _sig(L.sift3d_synth_blobs, None, P, I64, I64, I64, C.c_uint32)
    _sig(L.sift3d_synth_blobs_slices, None, P, I64, I64, I64, C.c_uint32, I64, I64)
    _sig(L.nifti_min_read, I, C.c_char_p, P)
    _sig(L.nifti_min_free, None, P)
    _sig(L.nifti_min_write_f32, I, C.c_char_p, P, I, I, I, F, F, F)
    _sig(L.nifti_min_write_f32_ex, I, C.c_char_p, P, I, I, I, F, F, F, P, P)
    _sig(L.sift3d_write_key, I, C.c_char_p, P, I64, F, I, P)
    _sig(L.sift3d_write_key_mode, None, I)
    _sig(L.sift3d_write_key_bin, I, C.c_char_p, P, I64, F)
    _sig(L.sift3d_read_key, I, C.c_char_p, P, P)
    _sig(L.sift3d_read_key_mode, None, I)
    _sig(L.sift3d_write_pgm, I, C.c_char_p, P, I, I)
    _sig(L.sift3d_world_transform, None, P, I64, P)
    _sig(L.sift3d_match_filter, I64, P, I64, I, I)
    _sig(L.sift3d_match_descriptors, I, P, I64, P)
    _sig(L.sift3d_match_votes, I, P, P, I, P, I, P, P, I, P, P)
    _sig(L.sift3d_match_write_votes, I, C.c_char_p, C.c_char_p, C.c_char_p, P, P, I, I, I)
    _sig(L.sift3d_log_ratio_interval, I, C.c_double, P, P)
    _sig(L.sift3d_similarity_invert, None, P, P)
    _sig(L.sift3d_write_similarity, I, C.c_char_p, P)
    _sig(L.sift3d_write_alignment_matches, I, C.c_char_p, C.c_char_p, C.c_char_p, P, I64, P, I64, P)
    _sig(L.sift3d_similarity_matrix, None, P, P)
    _sig(L.sift3d_read_similarity, I, C.c_char_p, P)
    _sig(L.sift3d_resample_map, I, P, P, P, P)
    _sig(L.sift3d_key_vox2key, None, P, P, P)
    _sig(L.sift3d_fit_similarity, I, P, P, I64, P)
    _sig(L.sift3d_refine_defaults, None, P)
    _sig(L.sift3d_field_defaults, None, P)
    _sig(L.sift3d_field_size, I, P, I64, P, P)
    _sig(L.sift3d_field_samples, None, P, P, P, I64, P, P)
    _sig(L.sift3d_field_warp_terms, I, P, P, P, P)
    _sig(L.sift3d_field_eval, None, P, P, I64, P)
    _sig(L.sift3d_field_folds, I64, P, P, P)
    _sig(L.sift3d_write_field, I, C.c_char_p, P)
    _sig(L.sift3d_read_field, I, C.c_char_p, P)
    _sig(L.sift3d_blockmatch_defaults, None, P)
    _sig(L.sift3d_blockmatch_range, I, P, I64, P, P)
    _sig(L.sift3d_blockmatch_lattice, I, I64, I64, I64, P, P, P)
    _sig(L.sift3d_blockmatch_grid, I, I64, I64, I64, P, P, P)
    _sig(L.sift3d_blockmatch_samples, I64, P, I64, I64, I64, P, P, P, P, P, P, P)
    _sig(L.sift3d_blockmatch_folds, I64, P, P, P)
    _sig(L.sift3d_invert_defaults, None, P)
    _sig(L.sift3d_invert_grid, I, I64, I64, I64, P, P, P)
    _sig(L.sift3d_affine_invert, I, P, P)
    _sig(L.sift3d_affine_invert_d, I, P, P)
    _sig(L.sift3d_write_matrix, I, C.c_char_p, P)
    _sig(L.sift3d_jacobian_factor, I, P, P, P)
    _sig(L.sift3d_compose_defaults, None, P)
    _sig(L.sift3d_compose_matrix, I, P, P, P)
    _sig(L.sift3d_compose_spacing, F, P, P, P)
    _sig(L.sift3d_compose_grid, I, I64, I64, I64, P, P, P, P, P)
    _sig(L.sift3d_compose_residual, I64, P, P, P, I64, P, P)
    _sig(L.sift3d_fuse_defaults, None, P)
    _sig(L.sift3d_fuse_similarity, C.c_uint32, C.c_int32, I64, I64, I64, I64, I64, I64)
    _sig(L.sift3d_fuse_check_labels, I64, P, I64)
    _sig(L.sift3d_fuse_shift_code, C.c_uint16, C.c_int32, C.c_int32, C.c_int32, C.c_int32)
    _sig(L.sift3d_fuse_shift_of, I, C.c_int32, C.c_uint32, P)
    _sig(L.sift3d_fuse_shift_stats, I64, C.c_int32, P, I64, P, P)
    _sig(L.sift3d_label_overlap, I64, P, P, I64, P, P, P)
    _sig(L.sift3d_surface_defaults, None, P)
    _sig(L.sift3d_spacing_um, I, F, P)
    _sig(L.sift3d_surface_stats, None, P, I64, P, I64, P)
    _sig(L.sift3d_clean_defaults, None, P)
    _sig(L.sift3d_ccl_check_extents, I, I64, I64, I64, C.c_char_p, I64)
    _sig(L.sift3d_clean_check, I, P, C.c_char_p, I64)
    _sig(L.sift3d_clean_report_text, I64, P, C.c_char_p, I64)
    _sig(L.sift3d_similarity_defaults, None, P)
    _sig(L.sift3d_similarity_check, I, P, C.c_char_p, I64)
    _sig(L.sift3d_similarity_measures, I, P, C.c_int32, P, F, F, C.c_int32, P)
    _sig(L.sift3d_similarity_label_measures, None, C.c_int32, P, F, F, C.c_int32, P)
    _sig(L.sift3d_similarity_report_text, I64, P, P, C.c_int32, C.c_char_p, I64)
    _sig(L.sift3d_register_defaults, None, P)
    _sig(L.sift3d_register_check, I, P, C.c_char_p, I64)
    _sig(L.sift3d_register_map, I, P, I64, I64, I64, P, P, P, P)
    _sig(L.sift3d_register_result, I, P, I64, I64, I64, P, P, P)
    _sig(L.sift3d_register_candidates, I, P, C.c_int32, C.c_double, C.c_double, P)
    _sig(L.sift3d_register_lattice, I64, I64, I64, I64, C.c_int32, P, P, P, P)
    _sig(L.sift3d_register_report_text, I64, P, C.c_char_p, I64)
    _sig(L.sift3d_average_defaults, None, P)
    _sig(L.sift3d_average_check, I, P, C.c_int32, C.c_char_p, I64)
    _sig(L.sift3d_average_counts, I, P, I64, C.c_int32, C.c_int32, C.c_int32, P)
    _sig(L.sift3d_average_report_text, I64, P, C.c_char_p, I64)
    _sig(L.sift3d_mean_field, I, C.c_int32, P, P, C.c_char_p, I64)
    _sig(L.sift3d_normalize_defaults, None, P)
    _sig(L.sift3d_normalize_check, I, P, C.c_char_p, I64)
    _sig(L.sift3d_normalize_transfer, I, C.c_int32, C.c_int32, P, P, P, P, P, P, C.c_char_p, I64)
    _sig(L.sift3d_transfer_check, I, P, C.c_char_p, I64)
    _sig(L.sift3d_normalize_report_text, I64, P, C.c_char_p, I64)
    L.free_ptr = C.CDLL(None).free
    L.free_ptr.argtypes = [C.c_void_p]
    _host = L
    return L


class ZSlabStats(C.Structure):
    """sift3d_zslab_stats"""
    _fields_ = [("n_ranks", C.c_int32), ("sharded_octaves", C.c_int32), ("exchanges", C.c_int64), ("halo_bytes_critical", C.c_int64),
                ("halo_bytes_deferred", C.c_int64), ("gather_bytes", C.c_int64), ("n_extrema", C.c_int64), ("n_keypoints", C.c_int64),
                ("n_records", C.c_int64), ("wall_ms", C.c_double), ("halo_bytes_hidden", C.c_int64), ("transport", C.c_int32),
                ("transport_fell_back", C.c_int32), ("rccl_version", C.c_int32), ("comm_sets", C.c_int32), ("resident_volume", C.c_int32),
                ("list_grown", C.c_int32), ("merge_ms", C.c_double), ("halo_bytes_subsample", C.c_int64), ("enqueue_ms", C.c_double)]


ZSLAB_TRANSPORT, TRANSPORT_PEER_COPY, TRANSPORT_RCCL = 1000, 0, 1   # sift3d_zslab_set_tuning(h, SIFT3D_ZSLAB_TRANSPORT, ...)
ZSLAB_SERIAL_CHANNELS, ZSLAB_DUPLICATE_RANKS, ZSLAB_POISON_HALO, ZSLAB_PATCH_WAIT, ZSLAB_LIST_ROOM = 1001, 1002, 1003, 1004, 1005   # include/sift3d.h


def zslab_set_transport_library(path):
    """sift3d_zslab_set_transport_library: the RCCL build the slab driver loads (None: librccl.so.1)."""
    hip_lib().sift3d_zslab_set_transport_library(None if path is None else os.fsencode(path))


def extract_zslab(vol, devices, initial_image_scale=1.0, desc_mode=DESC_SIFT, eig_thres=140.0, size_factor=1.0, transport=TRANSPORT_PEER_COPY):
    """sift3d_extract_zslab_over: the volume cut into one Z-slab per entry of `devices`, one process, halos by peer copies
    or RCCL.  Returns (records, stats dict)."""
    vol = _f32(vol)
    nz, ny, nx = vol.shape
    dev = (C.c_int * len(devices))(*[int(d) for d in devices])
    out, n, st, err = C.c_void_p(), C.c_int64(0), ZSlabStats(), C.create_string_buffer(512)
    rc = hip_lib().sift3d_extract_zslab_over(int(transport), dev, len(devices), vol.ctypes.data, nx, ny, nz, float(initial_image_scale),
                                             int(desc_mode), float(eig_thres), float(size_factor), C.byref(out), C.byref(n), C.byref(st), err, 512)
    if rc != 0:
        e = Sift3DError("sift3d_extract_zslab -> %d: %s" % (rc, err.value.decode(errors="replace")))
        e.code = rc
        raise e
    try:
        recs = np.frombuffer((C.c_char * (n.value * FEATURE_DTYPE.itemsize)).from_address(out.value), FEATURE_DTYPE, n.value).copy() if n.value else np.zeros(0, FEATURE_DTYPE)
    finally:
        hip_lib().sift3d_free(out)
    return recs, {k: getattr(st, k) for k, _ in ZSlabStats._fields_}


class ZSlab:
    """sift3d_zslab_create / _extract / _destroy: the slabs' contexts kept between volumes of one shape."""

    def __init__(self, nx, ny, nz, devices):
        self._L = hip_lib()
        dev = (C.c_int * len(devices))(*[int(d) for d in devices])
        err = C.create_string_buffer(512)
        self._h = self._L.sift3d_zslab_create(dev, len(devices), nx, ny, nz, err, 512)
        if not self._h:
            raise Sift3DError("sift3d_zslab_create: %s" % err.value.decode(errors="replace"))
        self.shape = (nz, ny, nx)

    def extract(self, vol, initial_image_scale=1.0, desc_mode=DESC_SIFT, eig_thres=140.0, size_factor=1.0):
        vol = _f32(vol)
        assert vol.shape == self.shape, (vol.shape, self.shape)
        out, n, st, err = C.c_void_p(), C.c_int64(0), ZSlabStats(), C.create_string_buffer(512)
        rc = self._L.sift3d_zslab_extract(self._h, vol.ctypes.data, float(initial_image_scale), int(desc_mode), float(eig_thres),
                                          float(size_factor), C.byref(out), C.byref(n), C.byref(st), err, 512)
        if rc != 0:
            e = Sift3DError("sift3d_zslab_extract -> %d: %s" % (rc, err.value.decode(errors="replace")))
            e.code = rc
            raise e
        try:
            recs = np.frombuffer((C.c_char * (n.value * FEATURE_DTYPE.itemsize)).from_address(out.value), FEATURE_DTYPE, n.value).copy() if n.value else np.zeros(0, FEATURE_DTYPE)
        finally:
            self._L.sift3d_free(out)
        return recs, {k: getattr(st, k) for k, _ in ZSlabStats._fields_}

    def set_volume(self, vol):
        """sift3d_zslab_set_volume: every rank's input slices uploaded once; extract_resident() then starts from HBM."""
        vol = _f32(vol)
        assert vol.shape == self.shape, (vol.shape, self.shape)
        err = C.create_string_buffer(512)
        rc = self._L.sift3d_zslab_set_volume(self._h, vol.ctypes.data, err, 512)
        if rc != 0:
            e = Sift3DError("sift3d_zslab_set_volume -> %d: %s" % (rc, err.value.decode(errors="replace")))
            e.code = rc
            raise e

    def extract_resident(self, initial_image_scale=1.0, desc_mode=DESC_SIFT, eig_thres=140.0, size_factor=1.0, copy=True):
        """sift3d_zslab_extract_resident: (records, stats).  copy=False: a view of the handle's merge buffer, valid until
        the handle's next call."""
        view, n, st, err = C.c_void_p(), C.c_int64(0), ZSlabStats(), C.create_string_buffer(512)
        rc = self._L.sift3d_zslab_extract_resident(self._h, float(initial_image_scale), int(desc_mode), float(eig_thres), float(size_factor),
                                                   C.byref(view), C.byref(n), C.byref(st), err, 512)
        if rc != 0:
            e = Sift3DError("sift3d_zslab_extract_resident -> %d: %s" % (rc, err.value.decode(errors="replace")))
            e.code = rc
            raise e
        if n.value:
            recs = np.frombuffer((C.c_char * (n.value * FEATURE_DTYPE.itemsize)).from_address(view.value), FEATURE_DTYPE, n.value)
            recs = recs.copy() if copy else recs
        else:
            recs = np.zeros(0, FEATURE_DTYPE)
        return recs, {k: getattr(st, k) for k, _ in ZSlabStats._fields_}

    def set_tuning(self, knob, value):
        rc = self._L.sift3d_zslab_set_tuning(self._h, int(knob), int(value))
        if rc != 0:
            raise Sift3DError("sift3d_zslab_set_tuning(%d, %d) -> %d" % (knob, value, rc))

    def close(self):
        if self._h:
            self._L.sift3d_zslab_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


GROUPS = 193   # include/sift3d.h: SIFT3D_GROUPS


def host_register(address, nbytes):
    """hipHostRegister (portable, mapped) on the caller's pages: every device of this process may store into them."""
    rc = hip_lib().sift3d_host_register(C.c_void_p(int(address)), int(nbytes))
    if rc != 0:
        raise Sift3DError("sift3d_host_register failed (%d)" % rc)


def host_unregister(address):
    hip_lib().sift3d_host_unregister(C.c_void_p(int(address)))


def device_count():
    return int(hip_lib().sift3d_device_count())


def _alloc_fill(byte):
    stats = (C.c_uint64 * 2)()
    rc = hip_lib().sift3d_selftest_alloc_fill(int(byte), stats)
    if rc != 0:
        raise Sift3DError("sift3d_selftest_alloc_fill(%d) failed (%d): a block of the allocator did not hold the fill byte" % (byte, rc))
    return int(stats[0]), int(stats[1])


@contextlib.contextmanager
def alloc_fill(byte):
    """sift3d_selftest_alloc_fill (include/sift3d_dev.h): inside the block every device and pinned host allocation of the
    library, in any thread, is filled with `byte` (0..255) before the library uses it; the fill is off again afterwards.
    Yields a function that returns (blocks, bytes) filled since it was last called.  For tests: a result must not depend
    on what an allocation held.  Each fill waits for the device, so nothing timed belongs inside."""
    if not 0 <= int(byte) <= 255:
        raise ValueError("fill byte %r is not in 0..255" % (byte,))
    _alloc_fill(byte)
    try:
        yield lambda: _alloc_fill(byte)
    finally:
        _alloc_fill(-1)


# ---- matcher: exact nearest neighbours on the GPU, votes on the host ---------------------------
FEATMATCH = os.path.join(CSRC, "_build", "featMatchMultiple")


def knn64(db, queries, k, device=0, repeats=1):
    """sift3d_knn64: for every row of `queries` (n_q x 64 int8, components 0..127) the k nearest rows of `db`, ascending
    by (squared distance, index).  Returns (idx, dist2, kernel_ms), idx / dist2 of shape (n_q, k)."""
    db = np.ascontiguousarray(db, np.int8)
    queries = np.ascontiguousarray(queries, np.int8)
    assert db.ndim == 2 and db.shape[1] == 64 and queries.ndim == 2 and queries.shape[1] == 64
    idx = np.empty((len(queries), k), np.int32)
    d2 = np.empty((len(queries), k), np.int32)
    ms = C.c_double(0.0)
    _call("sift3d_knn64", int(device), db.ctypes.data, len(db), queries.ctypes.data, len(queries), int(k), idx.ctypes.data, d2.ctypes.data,
          int(repeats), C.byref(ms))
    return idx, d2, ms.value


def match_filter(feats, reoriented=1, peaks=4):
    """sift3d_match_filter: the reference matcher's feature filters; returns the kept records."""
    f = np.ascontiguousarray(feats, FEATURE_DTYPE).copy()
    n = host_lib().sift3d_match_filter(f.ctypes.data, len(f), int(reoriented), int(peaks))
    return f[:n].copy()


def match_descriptors(feats):
    f = np.ascontiguousarray(feats, FEATURE_DTYPE)
    out = np.empty((len(f), 64), np.int8)
    if host_lib().sift3d_match_descriptors(f.ctypes.data, len(f), out.ctypes.data) != 0:
        raise Sift3DError("a descriptor value is outside 0..127")
    return out


# ---- matcher, alignment path (featMatchMultiple -a): ratio matching and Hough similarity, DESIGN.md section 7b -------------
class Similarity(C.Structure):
    """sift3d_similarity"""
    _fields_ = [("scale", C.c_float), ("rot", C.c_float * 9), ("trans", C.c_float * 3), ("center0", C.c_float * 3),
                ("center1", C.c_float * 3), ("n_matches", C.c_int32), ("inliers", C.c_int32), ("winner", C.c_int32),
                ("capacity", C.c_int32), ("moving_idx", C.c_void_p), ("fixed_idx", C.c_void_p), ("inlier", C.c_void_p),
                ("dist2", C.c_void_p)]


_PAIRS = ("moving_idx", "fixed_idx", "inlier", "dist2")   # the per-match arrays of sift3d_similarity


def _call(entry, *args, name=None):
    """libsift3d_hip.so's host-array entry point `entry` on args and an error buffer; where it returns nonzero, raises
    Sift3DError "<name> -> <code>: <the library's message>" (name: entry by default) with the code in .code."""
    err = C.create_string_buffer(512)
    rc = getattr(hip_lib(), entry)(*args, err, len(err))
    if rc != 0:
        e = Sift3DError("%s -> %d: %s" % (name or entry, rc, err.value.decode(errors="replace")))
        e.code = rc
        raise e


def _similarity_out(cap):
    """a Similarity with room for cap matches: (struct, {name: the int32 array it points to})"""
    arrays = {k: np.zeros(cap, np.int32) for k in _PAIRS}
    t = Similarity()
    t.capacity = cap
    for k, a in arrays.items():
        setattr(t, k, a.ctypes.data)
    return t, arrays


def match_ratio(db_feats, q_feats, device=0):
    """sift3d_match_ratio: the reference's ratio search of every query record over all database records (>= 2), in index
    order.  Returns (i1, d1, i2, d2, kernel_ms); the reference's ratio is float32(d1) / float32(d2)."""
    db = np.ascontiguousarray(db_feats, FEATURE_DTYPE)
    q = np.ascontiguousarray(q_feats, FEATURE_DTYPE)
    out = [np.empty(len(q), np.int32) for _ in range(4)]
    ms = C.c_double(0.0)
    _call("sift3d_match_ratio", int(device), db.ctypes.data, len(db), q.ctypes.data, len(q), *[o.ctypes.data for o in out], C.byref(ms))
    return tuple(out) + (ms.value,)


def hough_similarity(p0, p1, s0, s1, o0, o1, device=0):
    """sift3d_hough_similarity on M correspondences (moving side p0 / s0 / o0, fixed side p1 / s1 / o1; points M x 3,
    scales M, frames M x 3 x 3 row-major).  Returns a dict: counts (-1: degenerate hypothesis), winner (-1: none), rot
    (3 x 3), scale, flags."""
    arr = [np.ascontiguousarray(a, np.float32) for a in (p0, p1, s0, s1, o0, o1)]
    m = len(arr[2])
    assert arr[0].size == 3 * m and arr[1].size == 3 * m and arr[3].size == m and arr[4].size == 9 * m and arr[5].size == 9 * m
    counts, flags = np.empty(m, np.int32), np.empty(m, np.int32)
    rot, scale, winner = np.zeros(9, np.float32), C.c_float(0.0), C.c_int32(-1)
    _call("sift3d_hough_similarity", int(device), *[a.ctypes.data for a in arr], m, counts.ctypes.data, C.byref(winner), rot.ctypes.data,
          C.byref(scale), flags.ctypes.data)
    return {"counts": counts, "winner": winner.value, "rot": rot.reshape(3, 3), "scale": np.float32(scale.value), "flags": flags}


def _similarity_dict(t, arrays):
    n = t.n_matches
    d = {"scale": np.float32(t.scale), "rot": np.array(t.rot, np.float32).reshape(3, 3), "trans": np.array(t.trans, np.float32),
         "center0": np.array(t.center0, np.float32), "center1": np.array(t.center1, np.float32), "n_matches": n,
         "inliers": t.inliers, "winner": t.winner}
    for k, a in arrays.items():
        d[k] = a[:n].copy()
    return d


def _similarity_struct(d):
    """a sift3d_similarity from a match_keys dict (the arrays kept alive in the returned tuple)"""
    t = Similarity()
    t.scale = float(d["scale"])
    t.rot[:] = [float(v) for v in np.asarray(d["rot"], np.float32).ravel()]
    t.trans[:] = [float(v) for v in np.asarray(d["trans"], np.float32)]
    t.center0[:] = [float(v) for v in np.asarray(d.get("center0", np.zeros(3)), np.float32)]
    t.center1[:] = [float(v) for v in np.asarray(d.get("center1", np.zeros(3)), np.float32)]
    t.n_matches, t.inliers, t.winner = int(d.get("n_matches", 0)), int(d.get("inliers", 0)), int(d.get("winner", -1))
    keep = {}
    for k in _PAIRS:
        a = np.ascontiguousarray(d.get(k, np.zeros(0)), np.int32)
        keep[k] = a
        setattr(t, k, a.ctypes.data if len(a) else None)
    t.capacity = min(len(a) for a in keep.values()) if keep else 0
    return t, keep


def match_keys(fixed, moving, device=0, max_matches=3000):
    """sift3d_match_keys: MatchKeys of `moving` onto `fixed` (records as FEATURE_DTYPE).  Returns a dict: scale, rot (3 x 3),
    trans, center0, center1, n_matches, inliers, winner and per match (sorted by ratio) moving_idx, fixed_idx, inlier,
    dist2.  x_fixed = scale * rot @ x_moving + trans."""
    f = np.ascontiguousarray(fixed, FEATURE_DTYPE)
    m = np.ascontiguousarray(moving, FEATURE_DTYPE)
    t, arrays = _similarity_out(max(1, min(len(m), int(max_matches))))
    _call("sift3d_match_keys", int(device), f.ctypes.data, len(f), m.ctypes.data, len(m), int(max_matches), C.byref(t))
    return _similarity_dict(t, arrays)


def log_ratio_interval(t):
    """sift3d_log_ratio_interval: the float interval [lo, hi] of ratios r with fabsf(logf(r)) < float32(t)."""
    lo, hi = C.c_float(0.0), C.c_float(0.0)
    if host_lib().sift3d_log_ratio_interval(float(t), C.byref(lo), C.byref(hi)) != 0:
        raise Sift3DError("logf is not monotonic near the interval's ends")
    return np.float32(lo.value), np.float32(hi.value)


def similarity_invert(d):
    """sift3d_similarity_invert (TransformSimilarity::Invert) of a match_keys-style dict: (scale, rot, trans)."""
    t, _keep = _similarity_struct(d)
    out = Similarity()
    host_lib().sift3d_similarity_invert(C.byref(t), C.byref(out))
    return np.float32(out.scale), np.array(out.rot, np.float32).reshape(3, 3), np.array(out.trans, np.float32)


def write_similarity(path, d):
    """sift3d_write_similarity: TransformSimilarity::WriteMatrix of a match_keys-style dict."""
    t, _keep = _similarity_struct(d)
    if host_lib().sift3d_write_similarity(os.fsencode(path), C.byref(t)) != 0:
        raise Sift3DError("could not write %s" % path)


def write_alignment_matches(base, fixed_name, moving_name, fixed, moving, d):
    """sift3d_write_alignment_matches: <base>.matches.info.txt, .matches.img1.txt, .matches.img2.txt."""
    f = np.ascontiguousarray(fixed, FEATURE_DTYPE)
    m = np.ascontiguousarray(moving, FEATURE_DTYPE)
    t, _keep = _similarity_struct(d)
    if host_lib().sift3d_write_alignment_matches(os.fsencode(base), os.fsencode(fixed_name), os.fsencode(moving_name), f.ctypes.data, len(f),
                                                 m.ctypes.data, len(m), C.byref(t)) != 0:
        raise Sift3DError("could not write the match files of %s" % base)


# ---- guided re-matching (featMatchMultiple -a -e), DESIGN.md section 7d ---------------------------------------------------
class RefineParams(C.Structure):
    """sift3d_refine_params"""
    _fields_ = [("max_rounds", C.c_int32), ("min_radius", C.c_float), ("max_radius", C.c_float), ("ratio_num", C.c_int32),
                ("ratio_den", C.c_int32), ("stop_shift", C.c_float), ("index_cells_max", C.c_int64)]


REFINE_MAX_ROUNDS = 16
REFINE_STOPS = ("rounds", "converged", "fit", "none")   # sift3d_refine_stop


class RefineRound(C.Structure):
    _fields_ = [("radius", C.c_float), ("visited", C.c_int64), ("accepted", C.c_int32), ("kept", C.c_int32), ("rms", C.c_double),
                ("shift", C.c_double), ("kernel_ms", C.c_double)]


class RefineReport(C.Structure):
    _fields_ = [("rounds", C.c_int32), ("stop", C.c_int32), ("round", RefineRound * REFINE_MAX_ROUNDS)]


def refine_params(**kw):
    """sift3d_refine_defaults, then the given fields (max_rounds, min_radius, max_radius, ratio_num, ratio_den, stop_shift,
    index_cells_max)."""
    p = RefineParams()
    host_lib().sift3d_refine_defaults(C.byref(p))
    for k, v in kw.items():
        if k not in dict(RefineParams._fields_):
            raise ValueError("no refine parameter %s" % k)
        setattr(p, k, v)
    return p


def guided_search(fixed, moving, t, radius, device=0, index_cells_max=None):
    """sift3d_guided_search: for every moving record the best and second-best fixed records near its prediction under t (a
    match_keys-style dict), ordered by (squared descriptor distance, fixed index).  Returns (i1, d1, i2, d2, visited,
    kernel_ms); -1 / INT32_MAX where there is no candidate.  index_cells_max: the index form (1 forces sorted cell keys)."""
    f = np.ascontiguousarray(fixed, FEATURE_DTYPE)
    m = np.ascontiguousarray(moving, FEATURE_DTYPE)
    st, _keep = _similarity_struct(t)
    p = refine_params() if index_cells_max is None else refine_params(index_cells_max=int(index_cells_max))
    out = [np.empty(len(m), np.int32) for _ in range(5)]
    ms = C.c_double(0.0)
    _call("sift3d_guided_search_params", int(device), f.ctypes.data, len(f), m.ctypes.data, len(m), C.byref(st), float(radius), C.byref(p),
          *[o.ctypes.data for o in out], C.byref(ms), name="sift3d_guided_search")
    return tuple(out) + (ms.value,)


def fit_similarity(p_moving, p_fixed, center0=(0.0, 0.0, 0.0)):
    """sift3d_fit_similarity: the least-squares similarity p_moving -> p_fixed (n x 3 each, n >= 3, not collinear).  Returns a
    dict scale, rot (3 x 3), trans, center0, center1 (the fit applied to center0), or None where the fit is refused."""
    a = np.ascontiguousarray(p_moving, np.float32).reshape(-1, 3)
    b = np.ascontiguousarray(p_fixed, np.float32).reshape(-1, 3)
    if len(a) != len(b):
        raise ValueError("p_moving and p_fixed differ in length")
    t = Similarity()
    t.center0[:] = [float(v) for v in np.asarray(center0, np.float32).reshape(3)]
    if host_lib().sift3d_fit_similarity(a.ctypes.data, b.ctypes.data, len(a), C.byref(t)) != 0:
        return None
    return {"scale": np.float32(t.scale), "rot": np.array(t.rot, np.float32).reshape(3, 3), "trans": np.array(t.trans, np.float32),
            "center0": np.array(t.center0, np.float32), "center1": np.array(t.center1, np.float32)}


def _report_dict(r):
    rounds = [{"radius": np.float32(x.radius), "visited": int(x.visited), "accepted": int(x.accepted), "kept": int(x.kept), "rms": float(x.rms),
               "shift": float(x.shift), "kernel_ms": float(x.kernel_ms)} for x in r.round[:r.rounds]]
    return {"rounds": int(r.rounds), "stop": REFINE_STOPS[r.stop], "round": rounds}


def refine_similarity(fixed, moving, init, device=0, **params):
    """sift3d_refine_similarity: the guided re-matching loop from init (match_keys' dict, arrays included).  params: fields of
    sift3d_refine_params.  Returns (dict like match_keys' with the kept pairs as matches, report dict)."""
    f = np.ascontiguousarray(fixed, FEATURE_DTYPE)
    m = np.ascontiguousarray(moving, FEATURE_DTYPE)
    st, _keep = _similarity_struct(init)
    p = refine_params(**params)
    t, arrays = _similarity_out(max(1, len(m), int(init.get("n_matches", 0))))
    rep = RefineReport()
    _call("sift3d_refine_similarity", int(device), f.ctypes.data, len(f), m.ctypes.data, len(m), C.byref(st), C.byref(p), C.byref(t), C.byref(rep))
    return _similarity_dict(t, arrays), _report_dict(rep)


# ---- resampling (featResample), DESIGN.md section 7c ----------------------------------------------------------------------
INTERP = {"linear": 0, "nearest": 1, "label": 2}   # include/sift3d.h: sift3d_interp ("label": label-aware linear)


# ---- nonrigid alignment (featMatchMultiple -a -e -u, featResample -u), DESIGN.md section 7e ----------------------------------
FIELD_MAX_DISP = 128.0   # SIFT3D_FIELD_MAX_DISP


class Field(C.Structure):
    """sift3d_field"""
    _fields_ = [("n", C.c_int64 * 3), ("origin", C.c_float * 3), ("spacing", C.c_float), ("capacity", C.c_int64), ("disp", C.c_void_p)]


class FieldParams(C.Structure):
    """sift3d_field_params"""
    _fields_ = [("spacing", C.c_float), ("radius", C.c_float), ("lambda_", C.c_float), ("search_radius", C.c_float), ("min_tol", C.c_float),
                ("ratio_num", C.c_int32), ("ratio_den", C.c_int32), ("max_nodes", C.c_int64), ("index_cells_max", C.c_int64)]


class FieldReport(C.Structure):
    """sift3d_field_report"""
    _fields_ = [("accepted", C.c_int32), ("kept", C.c_int32), ("rms_before", C.c_double), ("rms_after", C.c_double), ("max_disp", C.c_double),
                ("folds", C.c_int64), ("search_ms", C.c_double), ("fit_ms", C.c_double * 2)]


def field_params(**kw):
    """sift3d_field_defaults, then the given fields (spacing, radius, lam (lambda), search_radius, min_tol, ratio_num, ratio_den,
    max_nodes, index_cells_max)."""
    p = FieldParams()
    host_lib().sift3d_field_defaults(C.byref(p))
    for k, v in kw.items():
        k = "lambda_" if k in ("lam", "lambda") else k
        if k not in dict(FieldParams._fields_):
            raise ValueError("no field parameter %s" % k)
        setattr(p, k, v)
    return p


def _pts(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1, 3)


def _field_dict(f, disp):
    n = tuple(int(x) for x in f.n)
    return {"n": n, "origin": np.array(f.origin, np.float32), "spacing": np.float32(f.spacing),
            "disp": disp[:3 * n[0] * n[1] * n[2]].reshape(3, n[2], n[1], n[0])}


def _field_struct(d):
    """a sift3d_field from a field dict (the array kept alive in the returned tuple)"""
    f = Field()
    disp = np.ascontiguousarray(d["disp"], np.float32).reshape(-1)
    f.n[:] = [int(x) for x in d["n"]]
    f.origin[:] = [float(x) for x in np.asarray(d["origin"], np.float32)]
    f.spacing = float(d["spacing"])
    f.capacity = disp.size
    f.disp = disp.ctypes.data
    return f, disp


def field_size(y, **params):
    """sift3d_field_size: the grid of samples at y (n x 3): dict n, origin, spacing.  Raises where it is refused."""
    y = _pts(y)
    f = Field()
    if host_lib().sift3d_field_size(y.ctypes.data, len(y), C.byref(field_params(**params)), C.byref(f)) != 0:
        raise Sift3DError("sift3d_field_size: bad parameters or too many nodes")
    return {"n": tuple(int(x) for x in f.n), "origin": np.array(f.origin, np.float32), "spacing": np.float32(f.spacing)}


def field_samples(t, p_fixed, p_moving):
    """sift3d_field_samples: (y, v), n x 3 each, of the pairs (p_fixed[i], p_moving[i]) under t (a match_keys-style dict)"""
    pf, pm = _pts(p_fixed), _pts(p_moving)
    st, _keep = _similarity_struct(t)
    y, v = np.empty_like(pf), np.empty_like(pf)
    host_lib().sift3d_field_samples(C.byref(st), pf.ctypes.data, pm.ctypes.data, len(pf), y.ctypes.data, v.ctypes.data)
    return y, v


def fit_field(y, v, device=0, return_ms=False, **params):
    """sift3d_fit_field: one fit on the GPU of samples y, v (n x 3 each).  Returns a field dict: n (n0, n1, n2), origin,
    spacing, disp (3, n2, n1, n0) float32; return_ms=True returns (field, kernel_ms)."""
    y, v = _pts(y), _pts(v)
    if len(y) != len(v):
        raise ValueError("y and v differ in length")
    p = field_params(**params)
    g = field_size(y, **params)
    disp = np.zeros(3 * g["n"][0] * g["n"][1] * g["n"][2], np.float32)
    f = Field()
    f.capacity, f.disp = disp.size, disp.ctypes.data
    ms = C.c_double(0.0)
    _call("sift3d_fit_field", int(device), y.ctypes.data, v.ctypes.data, len(y), C.byref(p), C.byref(f), C.byref(ms))
    d = _field_dict(f, disp)
    return (d, ms.value) if return_ms else d


def _field_report_dict(r):
    return {"accepted": int(r.accepted), "kept": int(r.kept), "rms_before": float(r.rms_before), "rms_after": float(r.rms_after),
            "max_disp": float(r.max_disp), "folds": int(r.folds), "search_ms": float(r.search_ms), "fit_ms": (float(r.fit_ms[0]), float(r.fit_ms[1]))}


def refine_field(fixed, moving, t, device=0, **params):
    """sift3d_refine_field: search at t (a match_keys-style dict), accept, fit, trim, refit.  Returns (field dict, report dict)."""
    f = np.ascontiguousarray(fixed, FEATURE_DTYPE)
    m = np.ascontiguousarray(moving, FEATURE_DTYPE)
    st, _keep = _similarity_struct(t)
    p = field_params(**params)
    g = field_size(np.stack([f["x"], f["y"], f["z"]], 1), **params)   # the fixed records' grid bounds any samples' grid
    disp = np.zeros(3 * g["n"][0] * g["n"][1] * g["n"][2], np.float32)
    out = Field()
    out.capacity, out.disp = disp.size, disp.ctypes.data
    rep = FieldReport()
    _call("sift3d_refine_field", int(device), f.ctypes.data, len(f), m.ctypes.data, len(m), C.byref(st), C.byref(p), C.byref(out), C.byref(rep))
    return _field_dict(out, disp), _field_report_dict(rep)


def field_warp_terms(fixed_vox2key=None, moving_vox2key=None):
    """sift3d_field_warp_terms: (C 3 x 4, K 3 x 3) float32 of the warp"""
    ms = [None if a is None else np.ascontiguousarray(a, np.float32).reshape(16) for a in (fixed_vox2key, moving_vox2key)]
    c, k = np.zeros(12, np.float32), np.zeros(9, np.float32)
    if host_lib().sift3d_field_warp_terms(*[None if a is None else a.ctypes.data for a in ms], c.ctypes.data, k.ctypes.data) != 0:
        raise Sift3DError("sift3d_field_warp_terms: a last row is not 0 0 0 1 or moving_vox2key is singular")
    return c.reshape(3, 4), k.reshape(3, 3)


def resample_field(vol, out_shape, map, field, fixed_vox2key=None, moving_vox2key=None, interp="linear", fill=0.0, device=0, return_ms=False):
    """sift3d_resample_field: resample_affine through the map and the displacement field (a field dict); vox2key 4 x 4 (None:
    identity).  return_ms=True returns (out, kernel_ms)."""
    v = _f32(vol)
    nz, ny, nx = v.shape
    oz, oy, ox = (int(d) for d in out_shape)
    out = np.empty((oz, oy, ox), np.float32)
    m = _map12(map)
    fs, _keep = _field_struct(field)
    ms_ = [None if a is None else np.ascontiguousarray(a, np.float32).reshape(16) for a in (fixed_vox2key, moving_vox2key)]
    ms = C.c_double(0.0)
    _call("sift3d_resample_field", int(device), v.ctypes.data, nx, ny, nz, out.ctypes.data, ox, oy, oz, m.ctypes.data,
          *[None if a is None else a.ctypes.data for a in ms_], C.byref(fs), INTERP[interp], float(fill), C.byref(ms))
    return (out, ms.value) if return_ms else out


def field_eval(field, y):
    """sift3d_field_eval: v at key positions y (n x 3), 0 outside the grid"""
    y = _pts(y)
    fs, _keep = _field_struct(field)
    out = np.empty_like(y)
    host_lib().sift3d_field_eval(C.byref(fs), y.ctypes.data, len(y), out.ctypes.data)
    return out


def field_folds(t, field):
    """sift3d_field_folds: (nodes with det grad phi <= 0, largest |v| over the nodes)"""
    st, _keep = _similarity_struct(t)
    fs, _keep2 = _field_struct(field)
    big = C.c_double(0.0)
    n = host_lib().sift3d_field_folds(C.byref(st), C.byref(fs), C.byref(big))
    return int(n), big.value


def write_field(path, field):
    """sift3d_write_field: <moving>.field.nii"""
    fs, _keep = _field_struct(field)
    if host_lib().sift3d_write_field(os.fsencode(path), C.byref(fs)) != 0:
        raise Sift3DError("could not write %s" % path)


def read_field(path):
    """sift3d_read_field: a field dict; raises Sift3DError (code SIFT3D_ERR_ARG) for anything the writer does not write"""
    f = Field()
    rc = host_lib().sift3d_read_field(os.fsencode(path), C.byref(f))
    if rc == -4:   # SIFT3D_ERR_CAPACITY: the grid is known now
        disp = np.zeros(3 * f.n[0] * f.n[1] * f.n[2], np.float32)
        f.capacity, f.disp = disp.size, disp.ctypes.data
        rc = host_lib().sift3d_read_field(os.fsencode(path), C.byref(f))
        if rc == 0:
            return _field_dict(f, disp)
    e = Sift3DError("sift3d_read_field(%s) -> %d" % (path, rc))
    e.code = rc
    raise e


# ---- intensity refinement of the field by block matching (featResample -i), DESIGN.md section 7f ----------------------------
BLOCKMATCH_WORDS, BLOCKMATCH_NONE, BLOCKMATCH_MAX_ROUNDS = 16, 0xffffffff, 8


class BlockmatchParams(C.Structure):
    """sift3d_blockmatch_params"""
    _fields_ = [("stride", C.c_int32), ("block", C.c_int32), ("search", C.c_int32), ("rounds", C.c_int32), ("variance_quantile", C.c_float),
                ("cost_fraction", C.c_float), ("spacing", C.c_float), ("radius", C.c_float), ("lambda_", C.c_float), ("min_tol", C.c_float),
                ("max_nodes", C.c_int64)]


class BlockmatchRound(C.Structure):
    """sift3d_blockmatch_round"""
    _fields_ = [("nodes", C.c_int64), ("flagged", C.c_int64), ("gated_variance", C.c_int64), ("gated_border", C.c_int64),
                ("gated_cost", C.c_int64), ("samples", C.c_int64), ("kept", C.c_int64), ("rms_before", C.c_double), ("rms_after", C.c_double),
                ("max_disp", C.c_double), ("folds", C.c_int64), ("warp_ms", C.c_double), ("match_ms", C.c_double), ("fit_ms", C.c_double * 2)]


class BlockmatchReport(C.Structure):
    """sift3d_blockmatch_report"""
    _fields_ = [("rounds", C.c_int32), ("empty_range", C.c_int32), ("lo", C.c_float), ("hi", C.c_float),
                ("round", BlockmatchRound * BLOCKMATCH_MAX_ROUNDS)]


def blockmatch_params(**kw):
    """sift3d_blockmatch_defaults, then the given fields (stride, block, search, rounds, variance_quantile, cost_fraction, spacing,
    radius, lam (lambda), min_tol, max_nodes)."""
    p = BlockmatchParams()
    host_lib().sift3d_blockmatch_defaults(C.byref(p))
    for k, v in kw.items():
        k = "lambda_" if k in ("lam", "lambda") else k
        if k not in dict(BlockmatchParams._fields_):
            raise ValueError("no block matching parameter %s" % k)
        setattr(p, k, v)
    return p


def _m16(m):
    """a 4 x 4 as 16 contiguous floats; a match_keys-style dict goes through similarity_matrix; None stays None"""
    if m is None:
        return None
    if isinstance(m, dict):
        m = similarity_matrix(m)
    return np.ascontiguousarray(m, np.float32).reshape(16)


def _ptr(a):
    return None if a is None else a.ctypes.data


def blockmatch_range(vol):
    """sift3d_blockmatch_range: (lo, hi) float32 of the quantisation, or None where vol has no two distinct finite values"""
    v = np.ascontiguousarray(vol, np.float32)
    lo, hi = C.c_float(0), C.c_float(0)
    ok = host_lib().sift3d_blockmatch_range(v.ctypes.data, v.size, C.byref(lo), C.byref(hi))
    return (np.float32(lo.value), np.float32(hi.value)) if ok else None


def blockmatch_lattice(shape, **params):
    """sift3d_blockmatch_lattice of a volume of shape (nz, ny, nx): (first (x, y, z), count (x, y, z)); raises where it is refused"""
    nz, ny, nx = (int(d) for d in shape)
    first, count = (C.c_int64 * 3)(), (C.c_int64 * 3)()
    if host_lib().sift3d_blockmatch_lattice(nx, ny, nz, C.byref(blockmatch_params(**params)), first, count) != 0:
        raise Sift3DError("sift3d_blockmatch_lattice: parameters out of range, or the window is wider than the volume")
    return tuple(first), tuple(count)


def blockmatch_grid(shape, fixed_vox2key=None, **params):
    """sift3d_blockmatch_grid: the output grid (dict n, origin, spacing) of a fixed volume of shape (nz, ny, nx)"""
    nz, ny, nx = (int(d) for d in shape)
    f = Field()
    if host_lib().sift3d_blockmatch_grid(nx, ny, nz, _ptr(_m16(fixed_vox2key)), C.byref(blockmatch_params(**params)), C.byref(f)) != 0:
        raise Sift3DError("sift3d_blockmatch_grid: bad parameters or too many nodes")
    return {"n": tuple(int(x) for x in f.n), "origin": np.array(f.origin, np.float32), "spacing": np.float32(f.spacing)}


def blockmatch_samples(words, shape, t, field=None, fixed_vox2key=None, **params):
    """sift3d_blockmatch_samples: (y, v, counts) from the block search's words over the lattice of a volume of shape
    (nz, ny, nx); counts = (flagged, gated by variance, by border, by cost); t: 4 x 4 or a match_keys-style dict"""
    nz, ny, nx = (int(d) for d in shape)
    w = np.ascontiguousarray(words, np.uint32).reshape(-1, BLOCKMATCH_WORDS)
    _first, count = blockmatch_lattice(shape, **params)
    if len(w) != count[0] * count[1] * count[2]:
        raise ValueError("words do not cover the lattice")
    y, v = np.empty((len(w), 3), np.float32), np.empty((len(w), 3), np.float32)
    counts = (C.c_int64 * 4)()
    fs, _keep = _field_struct(field) if field is not None else (None, None)
    fv, m = _m16(fixed_vox2key), _m16(t)
    n = host_lib().sift3d_blockmatch_samples(w.ctypes.data, nx, ny, nz, C.byref(blockmatch_params(**params)), _ptr(fv), m.ctypes.data,
                                             C.byref(fs) if fs is not None else None, y.ctypes.data, v.ctypes.data, counts)
    if n < 0:
        raise Sift3DError("sift3d_blockmatch_samples: bad arguments")
    return y[:n].copy(), v[:n].copy(), tuple(int(c) for c in counts)


def blockmatch_folds(t, field):
    """sift3d_blockmatch_folds: (nodes with det (L + grad v) <= 0, largest |v|); t: 4 x 4 or a match_keys-style dict"""
    fs, _keep = _field_struct(field)
    big = C.c_double(0.0)
    n = host_lib().sift3d_blockmatch_folds(_m16(t).ctypes.data, C.byref(fs), C.byref(big))
    return int(n), big.value


def block_match(fixed, warped, first, stride, count, block, search, device=0, generic=False, return_ms=False):
    """sift3d_block_match: the block search alone on the GPU.  fixed, warped: (nz, ny, nx) float32 on one grid; first, count:
    (x, y, z).  generic: 0 the specialised kernel where there is one, 1 the form for any b, r, 2 the specialised form without packed
    arithmetic (same words).  Returns uint32 words (count z, count y, count x, 16); return_ms=True returns (words, kernel_ms)."""
    return _block_match("sift3d_block_match", fixed, warped, first, stride, count, block, search, device, generic, return_ms)


def block_match_ncc(fixed, warped, first, stride, count, block, search, device=0, generic=False, return_ms=False):
    """sift3d_block_match_ncc: block_match under the correlation cost of DESIGN.md section 7g (warped quantised with its own
    range).  generic: 0 the register form of the kernel where there is one, 1 the form for any b, r (same words)."""
    return _block_match("sift3d_block_match_ncc", fixed, warped, first, stride, count, block, search, device, generic, return_ms)


def _block_match(entry, fixed, warped, first, stride, count, block, search, device, generic, return_ms):
    f, w = _f32(fixed), _f32(warped)
    if f.shape != w.shape:
        raise ValueError("fixed and warped differ in shape")
    nz, ny, nx = f.shape
    fi, cn = (C.c_int64 * 3)(*[int(x) for x in first]), (C.c_int64 * 3)(*[int(x) for x in count])
    n = max(int(cn[0]), 0) * max(int(cn[1]), 0) * max(int(cn[2]), 0)
    out = np.zeros((max(n, 1), BLOCKMATCH_WORDS), np.uint32)
    ms = C.c_double(0.0)
    _call(entry, int(device), f.ctypes.data, w.ctypes.data, nx, ny, nz, fi, int(stride), cn, int(block), int(search),
          int(generic), out.ctypes.data, C.byref(ms))
    out = out[:n].reshape(int(cn[2]), int(cn[1]), int(cn[0]), BLOCKMATCH_WORDS)
    return (out, ms.value) if return_ms else out


def _blockmatch_report_dict(r):
    rounds = []
    for k in range(BLOCKMATCH_MAX_ROUNDS):
        q = r.round[k]
        d = {name: getattr(q, name) for name, _ in BlockmatchRound._fields_ if name != "fit_ms"}
        d["fit_ms"] = (float(q.fit_ms[0]), float(q.fit_ms[1]))
        rounds.append(d)
    return {"rounds": int(r.rounds), "empty_range": int(r.empty_range), "lo": np.float32(r.lo), "hi": np.float32(r.hi), "round": rounds}


BLOCKMATCH_METRICS = {"ssd": 0, "ncc": 1}


def refine_field_intensity(fixed, moving, t, field=None, fixed_vox2key=None, moving_vox2key=None, device=0, metric="ssd", **params):
    """sift3d_refine_field_intensity: refine a displacement field (a field dict, None: zero) from the fixed and the moving
    volume (nz, ny, nx) by block matching.  t: the moving -> fixed key transform, 4 x 4 or a match_keys-style dict; vox2key
    4 x 4 (None: identity); params: fields of blockmatch_params.  Returns (field dict, report dict).
    metric: "ssd" (that function) or "ncc" (sift3d_refine_field_intensity_metric with the correlation cost of DESIGN.md section
    7g; the report dict then also holds metric and moving_lo, moving_hi, the range W is quantised with); a number is passed to
    sift3d_refine_field_intensity_metric as it is."""
    f, m = _f32(fixed), _f32(moving)
    fz, fy, fx = f.shape
    mz, my, mx = m.shape
    p = blockmatch_params(**params)
    g = blockmatch_grid(f.shape, fixed_vox2key, **params)
    cap = 3 * g["n"][0] * g["n"][1] * g["n"][2]
    fs, _keep = _field_struct(field) if field is not None else (None, None)
    if field is not None:
        cap = max(cap, 3 * int(np.prod(field["n"])))
    disp = np.zeros(cap, np.float32)
    out = Field()
    out.capacity, out.disp = disp.size, disp.ctypes.data
    rep = BlockmatchReport()
    fv, mv, tm = _m16(fixed_vox2key), _m16(moving_vox2key), _m16(t)
    if metric == "ssd":
        _call("sift3d_refine_field_intensity", int(device), f.ctypes.data, fx, fy, fz, m.ctypes.data, mx, my, mz, _ptr(fv), _ptr(mv),
              tm.ctypes.data, C.byref(fs) if fs is not None else None, C.byref(p), C.byref(out), C.byref(rep))
        return _field_dict(out, disp), _blockmatch_report_dict(rep)
    if isinstance(metric, str) and metric not in BLOCKMATCH_METRICS:
        raise ValueError("no block matching metric %s" % metric)
    mrange = (C.c_float * 2)()
    _call("sift3d_refine_field_intensity_metric", int(device), f.ctypes.data, fx, fy, fz, m.ctypes.data, mx, my, mz, _ptr(fv), _ptr(mv),
          tm.ctypes.data, C.byref(fs) if fs is not None else None, C.byref(p), int(BLOCKMATCH_METRICS.get(metric, metric)), C.byref(out),
          C.byref(rep), mrange)
    d = _blockmatch_report_dict(rep)
    d.update(metric=metric, moving_lo=np.float32(mrange[0]), moving_hi=np.float32(mrange[1]))
    return _field_dict(out, disp), d


# ---- the reverse direction: the inverse field and the Jacobian determinant map (featResample -r, -j), DESIGN.md section 7h ----
INVERT_STATES = ("converged", "not_converged", "diverged")   # SIFT3D_INVERT_STATE of a status word; its low 16 bits are the steps


class InvertParams(C.Structure):
    """sift3d_invert_params"""
    _fields_ = [("spacing", C.c_float), ("radius", C.c_float), ("max_iter", C.c_int32), ("tol", C.c_float), ("max_nodes", C.c_int64)]


class InvertReport(C.Structure):
    """sift3d_invert_report"""
    _fields_ = [("nodes", C.c_int64), ("converged", C.c_int64), ("not_converged", C.c_int64), ("diverged", C.c_int64), ("max_steps", C.c_int32),
                ("rms_residual", C.c_double), ("max_residual", C.c_double), ("max_disp", C.c_double), ("folds", C.c_int64),
                ("kernel_ms", C.c_double)]


def invert_params(**kw):
    """sift3d_invert_defaults, then the given fields (spacing, radius, max_iter, tol, max_nodes)."""
    p = InvertParams()
    host_lib().sift3d_invert_defaults(C.byref(p))
    for k, v in kw.items():
        if k not in dict(InvertParams._fields_):
            raise ValueError("no inversion parameter %s" % k)
        setattr(p, k, v)
    return p


def invert_grid(shape, moving_vox2key=None, **params):
    """sift3d_invert_grid: the inverse grid (dict n, origin, spacing) of a moving volume of shape (nz, ny, nx)"""
    nz, ny, nx = (int(d) for d in shape)
    f = Field()
    if host_lib().sift3d_invert_grid(nx, ny, nz, _ptr(_m16(moving_vox2key)), C.byref(invert_params(**params)), C.byref(f)) != 0:
        raise Sift3DError("sift3d_invert_grid: bad parameters or too many nodes")
    return {"n": tuple(int(x) for x in f.n), "origin": np.array(f.origin, np.float32), "spacing": np.float32(f.spacing)}


def affine_invert(m, double=False):
    """sift3d_affine_invert: the inverse of an affine 4 x 4 in double, rounded to float32 once (double=True: not rounded)"""
    a = _m16(m)
    out = np.zeros(16, np.float64 if double else np.float32)
    if (host_lib().sift3d_affine_invert_d if double else host_lib().sift3d_affine_invert)(a.ctypes.data, out.ctypes.data) != 0:
        raise Sift3DError("sift3d_affine_invert: the matrix is singular or its last row is not 0 0 0 1")
    return out.reshape(4, 4)


def write_matrix(path, m):
    """sift3d_write_matrix: a 4 x 4 in the .trans.txt layout"""
    if host_lib().sift3d_write_matrix(os.fsencode(path), _m16(m).ctypes.data) != 0:
        raise Sift3DError("could not write %s" % path)


def jacobian_factor(out_vox2key=None, src_vox2key=None):
    """sift3d_jacobian_factor: det lin(src_vox2key) / det lin(out_vox2key) as a float (a double)"""
    f = C.c_double(0.0)
    if host_lib().sift3d_jacobian_factor(_ptr(_m16(out_vox2key)), _ptr(_m16(src_vox2key)), C.byref(f)) != 0:
        raise Sift3DError("sift3d_jacobian_factor: a vox2key is singular")
    return f.value


def _grid_struct(grid):
    g = Field()
    g.n[:] = [int(x) for x in grid["n"]]
    g.origin[:] = [float(x) for x in np.asarray(grid["origin"], np.float32)]
    g.spacing = float(grid["spacing"])
    return g


def invert_nodes(m, m_inv, forward, grid, device=0, return_ms=False, **params):
    """sift3d_invert_nodes: field_invert_kernel alone over grid (dict n, origin, spacing).  m, m_inv: 4 x 4; forward: a field dict
    or None.  Returns (u (3, n2, n1, n0) float32, status (n2, n1, n0) uint32, res2 (n2, n1, n0) float64); return_ms=True appends
    kernel_ms."""
    n = tuple(int(x) for x in grid["n"])
    N = max(n[0], 0) * max(n[1], 0) * max(n[2], 0)
    u, status, res2 = np.zeros(3 * max(N, 1), np.float32), np.zeros(max(N, 1), np.uint32), np.zeros(max(N, 1), np.float64)
    fs, _keep = _field_struct(forward) if forward is not None else (None, None)
    g = _grid_struct(grid)
    ms = C.c_double(0.0)
    _call("sift3d_invert_nodes", int(device), _m16(m).ctypes.data, _m16(m_inv).ctypes.data, C.byref(fs) if fs is not None else None,
          C.byref(invert_params(**params)), C.byref(g), u.ctypes.data, status.ctypes.data, res2.ctypes.data, C.byref(ms))
    out = (u[:3 * N].reshape(3, n[2], n[1], n[0]), status[:N].reshape(n[2], n[1], n[0]), res2[:N].reshape(n[2], n[1], n[0]))
    return out + (ms.value,) if return_ms else out


def _invert_report_dict(r):
    return {name: getattr(r, name) for name, _ in InvertReport._fields_}


def invert_field(m, m_inv, forward, grid, device=0, **params):
    """sift3d_invert_field: the inverse field on grid (from invert_grid) and its report.  Returns (field dict, report dict)."""
    n = tuple(int(x) for x in grid["n"])
    disp = np.zeros(3 * max(n[0] * n[1] * n[2], 1), np.float32)
    out = _grid_struct(grid)
    out.capacity, out.disp = disp.size, disp.ctypes.data
    fs, _keep = _field_struct(forward) if forward is not None else (None, None)
    rep = InvertReport()
    _call("sift3d_invert_field", int(device), _m16(m).ctypes.data, _m16(m_inv).ctypes.data, C.byref(fs) if fs is not None else None,
          C.byref(invert_params(**params)), C.byref(out), C.byref(rep))
    return _field_dict(out, disp), _invert_report_dict(rep)


def jacobian_map(out_shape, map, out_vox2key=None, src_vox2key=None, field=None, form=-1, device=0, return_ms=False):
    """sift3d_jacobian_map: det grad of the warp resample_field applies for (map, out_vox2key, src_vox2key, field), on the output
    grid out_shape = (oz, oy, ox).  form 0: six evaluations per voxel, 1: through LDS, -1: the default.  return_ms=True returns
    (J, kernel_ms)."""
    oz, oy, ox = (int(d) for d in out_shape)
    out = np.empty((max(oz, 0), max(oy, 0), max(ox, 0)), np.float32)
    fs, _keep = _field_struct(field) if field is not None else (None, None)
    ms = C.c_double(0.0)
    _call("sift3d_jacobian_map", int(device), ox, oy, oz, _map12(map).ctypes.data, _ptr(_m16(out_vox2key)), _ptr(_m16(src_vox2key)),
          C.byref(fs) if fs is not None else None, out.ctypes.data, int(form), C.byref(ms))
    return (out, ms.value) if return_ms else out


# ---- composition: two alignments chained into one transform and field (featCompose), DESIGN.md section 7i --------------------
COMPOSE_OUTSIDE1, COMPOSE_OUTSIDE2, COMPOSE_ZEROED = 1, 2, 4   # the bits of a status word of sift3d_compose_nodes


class ComposeParams(C.Structure):
    """sift3d_compose_params"""
    _fields_ = [("spacing", C.c_float), ("radius", C.c_float), ("margin", C.c_int32), ("max_nodes", C.c_int64)]


class ComposeReport(C.Structure):
    """sift3d_compose_report"""
    _fields_ = [("nodes", C.c_int64), ("outside1", C.c_int64), ("outside2", C.c_int64), ("zeroed", C.c_int64), ("max_disp", C.c_double),
                ("folds", C.c_int64), ("residual_cells", C.c_int64), ("rms_residual", C.c_double), ("max_residual", C.c_double),
                ("kernel_ms", C.c_double * 2)]


def compose_params(**kw):
    """sift3d_compose_defaults, then the given fields (spacing, radius, margin, max_nodes)."""
    p = ComposeParams()
    host_lib().sift3d_compose_defaults(C.byref(p))
    for k, v in kw.items():
        if k not in dict(ComposeParams._fields_):
            raise ValueError("no composition parameter %s" % k)
        setattr(p, k, v)
    return p


def compose_matrix(m1, m2):
    """sift3d_compose_matrix: M1 M2 in double, rounded to float32 once"""
    out = np.zeros(16, np.float32)
    if host_lib().sift3d_compose_matrix(_m16(m1).ctypes.data, _m16(m2).ctypes.data, out.ctypes.data) != 0:
        raise Sift3DError("sift3d_compose_matrix: a last row is not 0 0 0 1 or an entry is not finite")
    return out.reshape(4, 4)


def _opt_field(field):
    """(a byref of the sift3d_field of a field dict or None, what keeps it alive)"""
    if field is None:
        return None, None
    fs, keep = _field_struct(field)
    return C.byref(fs), (fs, keep)


def compose_grid(shape, a_vox2key=None, field1=None, field2=None, **params):
    """sift3d_compose_grid: the composite grid (dict n, origin, spacing) over image A of shape (nz, ny, nx)"""
    nz, ny, nx = (int(d) for d in shape)
    f = Field()
    (f1, _k1), (f2, _k2) = _opt_field(field1), _opt_field(field2)
    if host_lib().sift3d_compose_grid(nx, ny, nz, _ptr(_m16(a_vox2key)), C.byref(compose_params(**params)), f1, f2, C.byref(f)) != 0:
        raise Sift3DError("sift3d_compose_grid: bad parameters or too many nodes")
    return {"n": tuple(int(x) for x in f.n), "origin": np.array(f.origin, np.float32), "spacing": np.float32(f.spacing)}


def compose_residual(n, status, res2, margin):
    """sift3d_compose_residual: (cells, rms, max) of the cell values res2 over the grid of n = (n0, n1, n2) nodes"""
    nn = (C.c_int64 * 3)(*[int(x) for x in n])
    st, r2 = np.ascontiguousarray(status, np.uint32), np.ascontiguousarray(res2, np.float64)
    if st.size != nn[0] * nn[1] * nn[2] or r2.size != (nn[0] - 1) * (nn[1] - 1) * (nn[2] - 1):
        raise ValueError("status and res2 do not cover the grid")
    rms, big = C.c_double(0.0), C.c_double(0.0)
    cells = host_lib().sift3d_compose_residual(nn, st.ctypes.data, r2.ctypes.data, int(margin), C.byref(rms), C.byref(big))
    return int(cells), rms.value, big.value


def compose_nodes(m1, m2, mc, field1, field2, grid, residual=True, device=0, return_ms=False, **params):
    """sift3d_compose_nodes: field_compose_kernel and (residual=True) compose_residual_kernel alone over grid (dict n, origin,
    spacing).  m1, m2: 4 x 4; mc: the written composite matrix as read back; field1, field2: field dicts or None.  Returns
    (w (3, n2, n1, n0) float32, status (n2, n1, n0) uint32, res2 (n2 - 1, n1 - 1, n0 - 1) float64 or None); return_ms=True appends
    the two kernel times."""
    n = tuple(int(x) for x in grid["n"])
    N = max(n[0], 0) * max(n[1], 0) * max(n[2], 0)
    cn = tuple(max(x - 1, 0) for x in n)
    NC = cn[0] * cn[1] * cn[2]
    w, status = np.zeros(3 * max(N, 1), np.float32), np.zeros(max(N, 1), np.uint32)
    res2 = np.zeros(max(NC, 1), np.float64) if residual else None
    (f1, _k1), (f2, _k2) = _opt_field(field1), _opt_field(field2)
    g = _grid_struct(grid)
    ms = (C.c_double * 2)()
    _call("sift3d_compose_nodes", int(device), _m16(m1).ctypes.data, _m16(m2).ctypes.data, _m16(mc).ctypes.data, f1, f2,
          C.byref(compose_params(**params)), C.byref(g), w.ctypes.data, status.ctypes.data, _ptr(res2), ms)
    out = (w[:3 * N].reshape(3, n[2], n[1], n[0]), status[:N].reshape(n[2], n[1], n[0]),
           res2[:NC].reshape(cn[2], cn[1], cn[0]) if residual else None)
    return out + ((ms[0], ms[1]),) if return_ms else out


def _compose_report_dict(r):
    d = {name: getattr(r, name) for name, _ in ComposeReport._fields_ if name != "kernel_ms"}
    d["kernel_ms"] = (float(r.kernel_ms[0]), float(r.kernel_ms[1]))
    return d


def compose_field(m1, m2, mc, field1, field2, grid, device=0, **params):
    """sift3d_compose_field: the composite field on grid (from compose_grid) and its report.  Returns (field dict, report dict)."""
    n = tuple(int(x) for x in grid["n"])
    disp = np.zeros(3 * max(n[0] * n[1] * n[2], 1), np.float32)
    out = _grid_struct(grid)
    out.capacity, out.disp = disp.size, disp.ctypes.data
    (f1, _k1), (f2, _k2) = _opt_field(field1), _opt_field(field2)
    rep = ComposeReport()
    _call("sift3d_compose_field", int(device), _m16(m1).ctypes.data, _m16(m2).ctypes.data, _m16(mc).ctypes.data, f1, f2,
          C.byref(compose_params(**params)), C.byref(out), C.byref(rep))
    return _field_dict(out, disp), _compose_report_dict(rep)


# ---- multi-atlas label fusion by locally weighted voting (featFuse), DESIGN.md section 7j ----------------------------------
FUSE_MAX_ATLASES, FUSE_U_ONE, FUSE_FALLBACK, FUSE_NONE = 32, 32768, 0x40000000, 0x80000000


class FuseParams(C.Structure):
    """sift3d_fuse_params"""
    _fields_ = [("block", C.c_int32), ("metric", C.c_int32), ("power", C.c_int32), ("fill", C.c_float), ("max_voxels", C.c_int64),
                ("label_interp", C.c_int32)]


class FuseAtlas(C.Structure):
    """sift3d_fuse_atlas"""
    _fields_ = [("image", C.c_void_p), ("labels", C.c_void_p), ("nx", C.c_int64), ("ny", C.c_int64), ("nz", C.c_int64), ("vox2key", C.c_void_p),
                ("moving_to_fixed", C.c_void_p), ("field", C.c_void_p)]


class FuseAtlasReport(C.Structure):
    """sift3d_fuse_atlas_report"""
    _fields_ = [("voters", C.c_int64), ("support", C.c_int64), ("mean_u", C.c_double), ("empty_range", C.c_int32), ("reserved", C.c_int32),
                ("warp_ms", C.c_double), ("weight_ms", C.c_double)]


class FuseReport(C.Structure):
    """sift3d_fuse_report"""
    _fields_ = [("none", C.c_int64), ("fallback", C.c_int64), ("lo", C.c_float), ("hi", C.c_float), ("vote_ms", C.c_double),
                ("atlas", FuseAtlasReport * FUSE_MAX_ATLASES)]


def fuse_params(**kw):
    """sift3d_fuse_defaults, then the given fields (block, metric ("ssd", "ncc" or a number), power, fill, max_voxels, label_interp
    ("nearest", "label" or a number: how the atlases' labels are warped))."""
    p = FuseParams()
    host_lib().sift3d_fuse_defaults(C.byref(p))
    for k, v in kw.items():
        if k not in dict(FuseParams._fields_):
            raise ValueError("no fusion parameter %s" % k)
        setattr(p, k, BLOCKMATCH_METRICS.get(v, v) if k == "metric" else INTERP.get(v, v) if k == "label_interp" else v)
    return p


def fuse_similarity(metric, n, sf, sff, sw, sww, sfw):
    """sift3d_fuse_similarity: u (0 .. 32768) of a patch from its six sums"""
    return int(host_lib().sift3d_fuse_similarity(int(BLOCKMATCH_METRICS.get(metric, metric)), int(n), int(sf), int(sff), int(sw), int(sww), int(sfw)))


def label_overlap(a, b):
    """sift3d_label_overlap of two float32 label volumes: (labels, count_a, count_b, count_both), the labels that occur in either
    volume in ascending order and their three int64 counts; Dice = 2 count_both / (count_a + count_b).  Raises where a voxel is
    neither non-finite nor an integer 0 .. 65535."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        raise ValueError("the label volumes differ in shape")
    ca, cb, cc = (np.zeros(65536, np.int64) for _ in range(3))
    if host_lib().sift3d_label_overlap(a.ctypes.data, b.ctypes.data, a.size, ca.ctypes.data, cb.ctypes.data, cc.ctypes.data) < 0:
        raise Sift3DError("sift3d_label_overlap: a label is neither non-finite nor an integer 0 .. 65535")
    present = np.nonzero((ca > 0) | (cb > 0))[0]
    return present, ca[present], cb[present], cc[present]


def fuse_weights(target, warped, block=2, metric="ssd", w_range=None, device=0, generic=False, return_ms=False):
    """sift3d_fuse_weights: the similarity u of every voxel's patch, uint16 (nz, ny, nx).  target, warped: (nz, ny, nx) float32 on
    one grid; w_range: (lo, hi) warped is quantised with (None: the target's range under "ssd", warped's own under "ncc");
    generic: the kernel's form for any block.  return_ms=True returns (u, kernel_ms)."""
    t, w = _f32(target), _f32(warped)
    if t.shape != w.shape:
        raise ValueError("target and warped differ in shape")
    nz, ny, nx = t.shape
    u = np.zeros(t.shape, np.uint16)
    wr = None if w_range is None else (C.c_float * 2)(float(w_range[0]), float(w_range[1]))
    ms = C.c_double(0.0)
    _call("sift3d_fuse_weights", int(device), t.ctypes.data, w.ctypes.data, nx, ny, nz, int(block), int(BLOCKMATCH_METRICS.get(metric, metric)), wr,
          int(generic), u.ctypes.data, C.byref(ms))
    return (u, ms.value) if return_ms else u


def fuse_vote(u, labels, power=2, device=0, return_ms=False):
    """sift3d_fuse_vote: u: K arrays of uint16, labels: K arrays of float32 of the same shape (not finite: no vote).  Returns the
    words, uint32 of that shape + (2,): label | voters << 16 | FUSE_FALLBACK | FUSE_NONE, and conf.  return_ms=True returns
    (words, kernel_ms)."""
    us = [np.ascontiguousarray(a, np.uint16) for a in u]
    ls = [np.ascontiguousarray(a, np.float32) for a in labels]
    if len(us) != len(ls) or any(a.shape != ls[0].shape for a in us + ls):
        raise ValueError("u and labels differ in number or shape")
    K, shape = len(us), (ls[0].shape if ls else (0,))
    up, lp = (C.c_void_p * max(K, 1))(*[a.ctypes.data for a in us]), (C.c_void_p * max(K, 1))(*[a.ctypes.data for a in ls])
    words = np.zeros(shape + (2,), np.uint32)
    ms = C.c_double(0.0)
    _call("sift3d_fuse_vote", int(device), K, up, lp, int(np.prod(shape)), int(power), words.ctypes.data, C.byref(ms))
    return (words, ms.value) if return_ms else words


def _fuse_report_dict(r, K):
    return {"none": int(r.none), "fallback": int(r.fallback), "lo": np.float32(r.lo), "hi": np.float32(r.hi), "vote_ms": float(r.vote_ms),
            "atlas": [{name: getattr(r.atlas[k], name) for name, _ in FuseAtlasReport._fields_ if name != "reserved"} for k in range(K)]}


def _fuse_stage(entry, target, atlases, target_vox2key, device, search, params):
    """sift3d_fuse_labels or sift3d_fuse_labels_search (entry) on the arguments of fuse_labels"""
    t = _f32(target)
    nz, ny, nx = t.shape
    K = len(atlases)
    arr = (FuseAtlas * max(K, 1))()
    keep = []
    for k, a in enumerate(atlases):
        im, lb = _f32(a["image"]), _f32(a["labels"])
        if im.shape != lb.shape:
            raise ValueError("atlas %d: image and labels differ in shape" % k)
        mv, tm = _m16(a.get("vox2key")), _m16(a["t"])
        fs, disp = _field_struct(a["field"]) if a.get("field") is not None else (None, None)
        keep.append((im, lb, mv, tm, fs, disp))
        arr[k].image, arr[k].labels = im.ctypes.data, lb.ctypes.data
        arr[k].nz, arr[k].ny, arr[k].nx = im.shape
        arr[k].vox2key, arr[k].moving_to_fixed = _ptr(mv), tm.ctypes.data
        arr[k].field = C.addressof(fs) if fs is not None else None
    words = np.zeros((nz, ny, nx, 2), np.uint32)
    rep = FuseReport()
    p = fuse_params(**params)
    if entry == "sift3d_fuse_labels":
        _call(entry, int(device), t.ctypes.data, nx, ny, nz, _ptr(_m16(target_vox2key)), K, arr, C.byref(p), words.ctypes.data, C.byref(rep))
        return words, _fuse_report_dict(rep, K)
    srep = FuseSearchReport()
    _call(entry, int(device), t.ctypes.data, nx, ny, nz, _ptr(_m16(target_vox2key)), K, arr, C.byref(p), int(search), words.ctypes.data, C.byref(rep),
          C.byref(srep))
    out = _fuse_report_dict(rep, K)
    out["search"] = {"radius": int(srep.radius),
                     "atlas": [{name: getattr(srep.atlas[k], name) for name, _ in FuseSearchAtlasReport._fields_} for k in range(K)]}
    return words, out


def fuse_labels(target, atlases, target_vox2key=None, device=0, search=0, **params):
    """sift3d_fuse_labels: the stage.  target: (nz, ny, nx) float32; atlases: dicts with image and labels ((nz, ny, nx) float32 of one
    shape), t (the moving -> fixed key transform, 4 x 4 or a match_keys-style dict) and optionally vox2key (4 x 4) and field (a
    field dict); params: fields of fuse_params.  Returns (words uint32 (nz, ny, nx, 2), report dict).  search = 1 .. 3:
    sift3d_fuse_labels_search, every atlas votes from its best-matching patch within that radius, and the
    report gains "search": the radius and per atlas moved, dist2_sum and search_ms."""
    entry = "sift3d_fuse_labels" if search == 0 else "sift3d_fuse_labels_search"
    return _fuse_stage(entry, target, atlases, target_vox2key, device, search, params)


# ---- the local search of the label fusion (featFuse -s), DESIGN.md section 7k ----------------------------------------------
FUSE_MAX_SEARCH, FUSE_NO_SHIFT = 3, 0xffff


class FuseSearchAtlasReport(C.Structure):
    """sift3d_fuse_search_atlas_report"""
    _fields_ = [("moved", C.c_int64), ("dist2_sum", C.c_int64), ("search_ms", C.c_double)]


class FuseSearchReport(C.Structure):
    """sift3d_fuse_search_report"""
    _fields_ = [("radius", C.c_int32), ("reserved", C.c_int32), ("atlas", FuseSearchAtlasReport * FUSE_MAX_ATLASES)]


def fuse_shift_code(radius, t):
    """sift3d_fuse_shift_code of the shift t = (tx, ty, tz); FUSE_NO_SHIFT where it is none under the radius"""
    return int(host_lib().sift3d_fuse_shift_code(int(radius), int(t[0]), int(t[1]), int(t[2])))


def fuse_shift_of(radius, code):
    """sift3d_fuse_shift_of: (tx, ty, tz), or None for a code that is none under the radius"""
    t = (C.c_int32 * 3)()
    return None if host_lib().sift3d_fuse_shift_of(int(radius), int(code), t) != 0 else (t[0], t[1], t[2])


def fuse_shift_stats(radius, shift):
    """sift3d_fuse_shift_stats over an array of codes: (voters, moved, dist2_sum); raises for a code that is none under the radius"""
    s = np.ascontiguousarray(shift, np.uint16)
    moved, d2 = C.c_int64(0), C.c_int64(0)
    voters = host_lib().sift3d_fuse_shift_stats(int(radius), s.ctypes.data, s.size, C.byref(moved), C.byref(d2))
    if voters < 0:
        raise Sift3DError("sift3d_fuse_shift_stats: a code is none under the radius %d" % radius)
    return int(voters), int(moved.value), int(d2.value)


def fuse_search(target, warped, labels=None, block=2, radius=1, metric="ssd", w_range=None, device=0, generic=False, return_ms=False):
    """sift3d_fuse_search: per voxel the similarity u of warped's best-matching patch within the radius, the code of its shift and
    the label picked there: (u uint16, shift uint16, picked float32 or None), each (nz, ny, nx).  target, warped and the optional
    labels (warped labels, not finite: may not be picked): (nz, ny, nx) float32 on one grid; w_range and generic as for
    fuse_weights.  return_ms=True appends kernel_ms."""
    t, w = _f32(target), _f32(warped)
    lb = None if labels is None else _f32(labels)
    if t.shape != w.shape or (lb is not None and lb.shape != t.shape):
        raise ValueError("target, warped and labels differ in shape")
    nz, ny, nx = t.shape
    u, shift = np.zeros(t.shape, np.uint16), np.zeros(t.shape, np.uint16)
    picked = None if lb is None else np.zeros(t.shape, np.float32)
    wr = None if w_range is None else (C.c_float * 2)(float(w_range[0]), float(w_range[1]))
    ms = C.c_double(0.0)
    _call("sift3d_fuse_search", int(device), t.ctypes.data, w.ctypes.data, _ptr(lb), nx, ny, nz, int(block), int(radius),
          int(BLOCKMATCH_METRICS.get(metric, metric)), wr, int(generic), u.ctypes.data, shift.ctypes.data, _ptr(picked), C.byref(ms))
    return (u, shift, picked, ms.value) if return_ms else (u, shift, picked)


# ---- exact Euclidean distance map and surface distances between label volumes (featFuse -m, featOverlap), DESIGN.md section 7l ----
EDT_MAX_EXTENT, EDT_MAX_SPACING_UM, EDT_MAX_VOXELS, EDT_NONE = 4096, 65535, 1 << 30, 0xffffffffffffffff


class SurfaceParams(C.Structure):
    """sift3d_surface_params"""
    _fields_ = [("first_label", C.c_int32), ("max_labels", C.c_int32), ("device", C.c_int32), ("reserved", C.c_int32)]


class SurfaceRecord(C.Structure):
    """sift3d_surface_record"""
    _fields_ = [("label", C.c_int32), ("reserved", C.c_int32), ("voxels_a", C.c_int64), ("voxels_b", C.c_int64), ("n_a", C.c_int64), ("n_b", C.c_int64),
                ("max_ab", C.c_uint64), ("max_ba", C.c_uint64), ("p95_ab", C.c_uint64), ("p95_ba", C.c_uint64), ("sum_ab", C.c_double),
                ("sum_ba", C.c_double), ("hausdorff_mm", C.c_double), ("hd95_mm", C.c_double), ("assd_mm", C.c_double)]


def surface_params(**kw):
    """sift3d_surface_defaults, then the given fields (first_label, max_labels, device)"""
    p = SurfaceParams()
    host_lib().sift3d_surface_defaults(C.byref(p))
    for k, v in kw.items():
        if k not in dict(SurfaceParams._fields_):
            raise ValueError("no surface distance parameter %s" % k)
        setattr(p, k, v)
    return p


def spacing_um(mm):
    """sift3d_spacing_um: a voxel size in mm as micrometres, or None where it is refused (not finite, or outside 1 .. 65535 um)"""
    um = C.c_uint32(0)
    return None if host_lib().sift3d_spacing_um(float(mm), C.byref(um)) != 0 else int(um.value)


def _surface_record_dict(r):
    return {name: getattr(r, name) for name, _ in SurfaceRecord._fields_ if name != "reserved"}


def surface_stats(list_ab, list_ba):
    """sift3d_surface_stats of the two lists of squared distances (um^2) of one label: a dict of the record's fields but the label
    and its voxel counts.  The lists are copied, not sorted in place."""
    ab, ba = np.array(list_ab, np.uint64).reshape(-1), np.array(list_ba, np.uint64).reshape(-1)
    r = SurfaceRecord()
    host_lib().sift3d_surface_stats(ab.ctypes.data, ab.size, ba.ctypes.data, ba.size, C.byref(r))
    return {k: v for k, v in _surface_record_dict(r).items() if k not in ("label", "voxels_a", "voxels_b")}


def _spacing3(spacing):
    sp = [int(v) for v in spacing]
    if len(sp) != 3 or any(v < 0 or v > 0xffffffff for v in sp):
        raise ValueError("a spacing is three unsigned integers: micrometres along x, y, z")
    return (C.c_uint32 * 3)(*sp)


def distance_map(sites, spacing=(1000, 1000, 1000), device=0, return_ms=False):
    """sift3d_distance_map: sites (nz, ny, nx), non-zero where a site is; spacing: micrometres along x, y, z.  Returns the squared
    distance to the nearest site in um^2, uint64 (nz, ny, nx), EDT_NONE everywhere where there is no site.  return_ms=True returns
    (d2, (total, x, y, z) device ms of the three passes)."""
    s = np.ascontiguousarray(np.asarray(sites) != 0, np.uint8)
    if s.ndim != 3:
        raise ValueError("sites is a volume (nz, ny, nx)")
    nz, ny, nx = s.shape
    d2 = np.zeros(s.shape, np.uint64)
    ms = (C.c_double * 4)()
    _call("sift3d_distance_map", int(device), s.ctypes.data, nx, ny, nz, _spacing3(spacing), d2.ctypes.data, ms)
    return (d2, tuple(ms)) if return_ms else d2


def surface_distances(a, b, spacing=(1000, 1000, 1000), return_ms=False, **params):
    """sift3d_surface_distances of two float32 label volumes (nz, ny, nx) on one grid: a list of dicts, one per label >= first_label
    that either volume has, in ascending order (the fields of sift3d_surface_record).  params: fields of surface_params.
    return_ms=True returns (records, the device ms of the transform kernels)."""
    a, b = _f32(a), _f32(b)
    if a.shape != b.shape or a.ndim != 3:
        raise ValueError("the label volumes are (nz, ny, nx) and of one shape")
    nz, ny, nx = a.shape
    p = surface_params(**params)
    rec = (SurfaceRecord * max(int(p.max_labels), 1))()
    n, ms = C.c_int32(0), C.c_double(0.0)
    _call("sift3d_surface_distances", a.ctypes.data, b.ctypes.data, nx, ny, nz, _spacing3(spacing), C.byref(p), rec, C.byref(n), C.byref(ms))
    out = [_surface_record_dict(rec[k]) for k in range(n.value)]
    return (out, ms.value) if return_ms else out


# ---- connected components of a label volume and island removal (featClean), DESIGN.md section 7m ------------------------------------
CCL_MAX_EXTENT, CCL_MAX_VOXELS, CLEAN_MAX_MIN_VOXELS, CLEAN_MAX_ROUNDS, CCL_STAGES = 4096, 1 << 30, 1 << 24, 16, 6
COMPONENT_DTYPE = np.dtype([("label", "<i4"), ("reserved", "<i4"), ("voxels", "<i8"), ("first", "<i8"), ("box", "<i4", (6,))])   # sift3d_component_record
CLEAN_ROUND_FIELDS = ("components", "small", "resolved", "resolved_voxels", "unresolved", "unresolved_voxels")


class CleanParams(C.Structure):
    """sift3d_clean_params"""
    _fields_ = [("min_voxels", C.c_int32), ("connectivity", C.c_int32), ("rounds", C.c_int32), ("device", C.c_int32)]


class CleanRound(C.Structure):
    """sift3d_clean_round"""
    _fields_ = [(name, C.c_int64) for name in CLEAN_ROUND_FIELDS]


class CleanReport(C.Structure):
    """sift3d_clean_report"""
    _fields_ = [("rounds_run", C.c_int32), ("reserved", C.c_int32), ("round", CleanRound * CLEAN_MAX_ROUNDS), ("total", CleanRound)]


def clean_params(**kw):
    """sift3d_clean_defaults, then the given fields (min_voxels, connectivity, rounds, device)"""
    p = CleanParams()
    host_lib().sift3d_clean_defaults(C.byref(p))
    for k, v in kw.items():
        if k not in dict(CleanParams._fields_):
            raise ValueError("no cleaning parameter %s" % k)
        setattr(p, k, v)
    return p


def clean_check(p):
    """sift3d_clean_check: None, or the text with which the parameters are refused"""
    err = C.create_string_buffer(512)
    return None if host_lib().sift3d_clean_check(C.byref(p), err, len(err)) == 0 else err.value.decode()


def clean_report_dict(rep):
    """a sift3d_clean_report as {"rounds_run", "rounds": [one dict per round run], "total": dict}"""
    row = lambda r: {k: int(getattr(r, k)) for k in CLEAN_ROUND_FIELDS}
    return {"rounds_run": int(rep.rounds_run), "rounds": [row(rep.round[r]) for r in range(rep.rounds_run)], "total": row(rep.total)}


def clean_report_text(rep):
    """sift3d_clean_report_text of a CleanReport"""
    buf = C.create_string_buffer(4096)
    n = host_lib().sift3d_clean_report_text(C.byref(rep), buf, len(buf))
    if n < 0 or n >= len(buf):
        raise Sift3DError("sift3d_clean_report_text -> %d" % n)
    return buf.value.decode()


def label_components(labels, connectivity=6, device=0, max_records=None, return_ms=False):
    """sift3d_label_components of a float32 label volume (nz, ny, nx): (comp, records) -- the component map, uint32 of that shape
    (0: unlabelled), and the records as an array of COMPONENT_DTYPE in key order.  max_records: the room offered for records (None:
    as many as there are components, by calling twice where the first guess is too small); an explicit value that is too small
    raises with the count in the text and in .n_components, the map in .comp.  return_ms=True returns (comp, records, the
    CCL_STAGES device ms: total, label plane, brick pass, border merge, flatten, numbers and records)."""
    v = _f32(labels)
    if v.ndim != 3:
        raise ValueError("labels is a volume (nz, ny, nx)")
    nz, ny, nx = v.shape
    comp = np.zeros(v.shape, np.uint32)
    room = 4096 if max_records is None else int(max_records)
    while True:
        rec = np.zeros(max(room, 1), COMPONENT_DTYPE)
        n, ms = C.c_int64(0), (C.c_double * CCL_STAGES)()
        try:
            _call("sift3d_label_components", int(device), v.ctypes.data, nx, ny, nz, int(connectivity), comp.ctypes.data, rec.ctypes.data, room, C.byref(n), ms)
        except Sift3DError as e:
            if max_records is None and n.value > room:
                room = n.value
                continue
            e.n_components, e.comp = n.value, comp
            raise
        rec = rec[:n.value].copy()
        return (comp, rec, tuple(ms)) if return_ms else (comp, rec)


def clean_labels(labels, return_ms=False, **params):
    """sift3d_clean_labels of a float32 label volume (nz, ny, nx): (out, report) -- the cleaned labels, float32 of that shape, and
    the report as clean_report_dict gives it (its CleanReport under "struct").  params: fields of clean_params.  return_ms=True
    returns (out, report, the device ms of all rounds)."""
    v = _f32(labels)
    if v.ndim != 3:
        raise ValueError("labels is a volume (nz, ny, nx)")
    nz, ny, nx = v.shape
    p = clean_params(**params)
    out = np.zeros(v.shape, np.float32)
    rep, ms = CleanReport(), C.c_double(0.0)
    _call("sift3d_clean_labels", v.ctypes.data, nx, ny, nz, C.byref(p), out.ctypes.data, C.byref(rep), C.byref(ms))
    d = clean_report_dict(rep)
    d["struct"] = rep
    return (out, d, ms.value) if return_ms else (out, d)


# ---- similarity of two images on one grid (featCompare), DESIGN.md section 7o -------------------------------------------------------
SIMILARITY_MAX_BINS, SIMILARITY_MAX_LABELS, SIMILARITY_BINS = 64, 64, (8, 16, 32, 64)
SIMILARITY_SUMS = ("n", "sa", "sb", "saa", "sbb", "sab")
SIMILARITY_MEASURES = ("mi", "nmi", "rho", "rms", "h_a", "h_b", "h_ab")
SIMILARITY_FLUSH = {"slices": 0, "atomics": 1}


class SimilarityParams(C.Structure):
    """sift3d_similarity_params"""
    _fields_ = [("bins", C.c_int32), ("same_scale", C.c_int32), ("max_labels", C.c_int32), ("device", C.c_int32), ("flush", C.c_int32), ("reserved", C.c_int32)]


class SimilarityRecord(C.Structure):
    """sift3d_similarity_record"""
    _fields_ = [("bins", C.c_int32), ("same_scale", C.c_int32), ("empty_range", C.c_int32), ("reserved", C.c_int32), ("a_lo", C.c_float), ("a_hi", C.c_float),
                ("b_lo", C.c_float), ("b_hi", C.c_float), ("excluded", C.c_int64), ("sums", C.c_int64 * len(SIMILARITY_SUMS))] + \
               [(name, C.c_double) for name in SIMILARITY_MEASURES] + [("kernel_ms", C.c_double), ("hist", C.c_int64 * (SIMILARITY_MAX_BINS * SIMILARITY_MAX_BINS))]


class SimilarityLabelRecord(C.Structure):
    """sift3d_similarity_label_record"""
    _fields_ = [("label", C.c_int32), ("reserved", C.c_int32), ("sums", C.c_int64 * len(SIMILARITY_SUMS)), ("rho", C.c_double), ("rms", C.c_double)]


def similarity_params(**kw):
    """sift3d_similarity_defaults, then the given fields (bins, same_scale, max_labels, device, flush: 0 / "slices", 1 / "atomics")"""
    p = SimilarityParams()
    host_lib().sift3d_similarity_defaults(C.byref(p))
    for k, v in kw.items():
        if k not in dict(SimilarityParams._fields_):
            raise ValueError("no similarity parameter %s" % k)
        setattr(p, k, int(SIMILARITY_FLUSH.get(v, v)) if k == "flush" else int(v))
    return p


def similarity_check(p):
    """sift3d_similarity_check: None, or the text with which the parameters are refused"""
    err = C.create_string_buffer(512)
    return None if host_lib().sift3d_similarity_check(C.byref(p), err, len(err)) == 0 else err.value.decode()


def _image_similarity_dict(r, labels):
    bins = int(r.bins)
    d = {"bins": bins, "same_scale": int(r.same_scale), "empty_range": int(r.empty_range), "range_a": (np.float32(r.a_lo), np.float32(r.a_hi)),
         "range_b": (np.float32(r.b_lo), np.float32(r.b_hi)), "excluded": int(r.excluded), "sums": [int(v) for v in r.sums], "n": int(r.sums[0]),
         "hist": np.array(r.hist[:bins * bins], np.int64).reshape(bins, bins), "kernel_ms": float(r.kernel_ms), "struct": r}
    d.update({name: float(getattr(r, name)) for name in SIMILARITY_MEASURES})
    if labels is not None:
        d["labels"] = [{"label": int(l.label), "sums": [int(v) for v in l.sums], "n": int(l.sums[0]), "rho": float(l.rho), "rms": float(l.rms)} for l in labels]
        d["label_structs"] = labels
    return d


def similarity_measures(hist, sums, lo=0.0, hi=1.0, same_scale=False):
    """sift3d_similarity_measures of a joint histogram (bins x bins int64) and its six sums: a dict of mi, nmi, rho, rms, h_a, h_b,
    h_ab; lo, hi: A's range (read under same_scale only)"""
    h = np.ascontiguousarray(hist, np.int64)
    s = np.ascontiguousarray(sums, np.int64).reshape(len(SIMILARITY_SUMS))
    bins = h.shape[0]
    if h.ndim != 2 or h.shape[1] != bins:
        raise ValueError("hist is bins x bins")
    r = SimilarityRecord()
    if host_lib().sift3d_similarity_measures(h.ctypes.data, bins, s.ctypes.data, float(lo), float(hi), int(bool(same_scale)), C.byref(r)) != 0:
        raise Sift3DError("sift3d_similarity_measures: bins = %d is not 8, 16, 32 or 64" % bins)
    return {name: float(getattr(r, name)) for name in SIMILARITY_MEASURES}


def similarity_label_measures(label, sums, lo=0.0, hi=1.0, same_scale=False):
    """sift3d_similarity_label_measures: (rho, rms) of one label's six sums"""
    s = np.ascontiguousarray(sums, np.int64).reshape(len(SIMILARITY_SUMS))
    r = SimilarityLabelRecord()
    host_lib().sift3d_similarity_label_measures(int(label), s.ctypes.data, float(lo), float(hi), int(bool(same_scale)), C.byref(r))
    return float(r.rho), float(r.rms)


def similarity_report_text(result):
    """sift3d_similarity_report_text of what image_similarity returned"""
    lab = result.get("label_structs")
    args = (C.byref(result["struct"]), None if lab is None else C.byref(lab), 0 if lab is None else len(result["labels"]))
    need = host_lib().sift3d_similarity_report_text(*args, None, 0)
    if need < 0:
        raise Sift3DError("sift3d_similarity_report_text -> %d" % need)
    buf = C.create_string_buffer(need + 1)
    if host_lib().sift3d_similarity_report_text(*args, buf, len(buf)) != need:
        raise Sift3DError("sift3d_similarity_report_text: the length changed")
    return buf.value.decode()


def joint_histogram(a, b, a_range, b_range, bins=64, device=0, return_ms=False):
    """sift3d_joint_histogram of two float32 volumes (nz, ny, nx) quantised with the given (lo, hi) ranges: (hist int64 bins x bins,
    the six sums as Python integers, excluded).  return_ms=True appends kernel_ms."""
    a, b = _f32(a), _f32(b)
    if a.shape != b.shape or a.ndim != 3:
        raise ValueError("the images are (nz, ny, nx) and of one shape")
    nz, ny, nx = a.shape
    bins = int(bins)
    hist, sums = np.zeros((max(bins, 0), max(bins, 0)), np.int64), np.zeros(len(SIMILARITY_SUMS), np.int64)
    ar, br = (C.c_float * 2)(*[float(v) for v in a_range]), (C.c_float * 2)(*[float(v) for v in b_range])
    excluded, ms = C.c_int64(0), C.c_double(0.0)
    _call("sift3d_joint_histogram", int(device), a.ctypes.data, b.ctypes.data, nx, ny, nz, ar, br, bins, hist.ctypes.data, sums.ctypes.data, C.byref(excluded),
          C.byref(ms))
    out = (hist, [int(v) for v in sums], int(excluded.value))
    return out + (ms.value,) if return_ms else out


def image_similarity(a, b, labels=None, **params):
    """sift3d_image_similarity of two float32 volumes (nz, ny, nx) on one grid: a dict of the record's fields (hist as int64 bins x
    bins, sums as Python integers, n, range_a, range_b, the measures, kernel_ms; the structures under "struct" and
    "label_structs") and, with labels (a float32 label volume of that shape), "labels": one dict per label.  params: fields of
    similarity_params."""
    a, b = _f32(a), _f32(b)
    lb = None if labels is None else _f32(labels)
    if a.shape != b.shape or a.ndim != 3 or (lb is not None and lb.shape != a.shape):
        raise ValueError("the images and the labels are (nz, ny, nx) and of one shape")
    nz, ny, nx = a.shape
    p = similarity_params(**params)
    rec = SimilarityRecord()
    lrec = None if lb is None else (SimilarityLabelRecord * SIMILARITY_MAX_LABELS)()
    n = C.c_int32(0)
    _call("sift3d_image_similarity", a.ctypes.data, b.ctypes.data, _ptr(lb), nx, ny, nz, C.byref(p), C.byref(rec), lrec, C.byref(n))
    return _image_similarity_dict(rec, None if lb is None else (SimilarityLabelRecord * n.value)(*lrec[:n.value]))


# ---- affine registration by mutual information (featRegister), DESIGN.md section 7q -------------------------------------------------
REGISTER_MAX_MAPS, REGISTER_MAX_LEVELS, REGISTER_THETA = 32, 4, 12
REGISTER_METRICS = {"mi": 0, "nmi": 1}
REGISTER_FORMS = {"default": -1, "by_brick": 0, "by_map": 1, "by_brick_plane": 2, "by_map_plane": 3}


class RegisterParams(C.Structure):
    """sift3d_register_params"""
    _fields_ = [("dof", C.c_int32), ("metric", C.c_int32), ("bins", C.c_int32), ("n_levels", C.c_int32), ("stride", C.c_int32 * REGISTER_MAX_LEVELS),
                ("max_iterations", C.c_int32), ("device", C.c_int32), ("form", C.c_int32), ("reserved", C.c_int32),
                ("first_step", C.c_double * REGISTER_MAX_LEVELS), ("last_step", C.c_double * REGISTER_MAX_LEVELS), ("min_overlap", C.c_double)]


class RegisterLevel(C.Structure):
    """sift3d_register_level"""
    _fields_ = [("stride", C.c_int32), ("iterations", C.c_int32), ("evaluations", C.c_int32), ("stop", C.c_int32), ("n_lattice", C.c_int64),
                ("score_in", C.c_double), ("score_out", C.c_double), ("last_step", C.c_double), ("device_ms", C.c_double)]


class RegisterReport(C.Structure):
    """sift3d_register_report"""
    _fields_ = [("dof", C.c_int32), ("metric", C.c_int32), ("bins", C.c_int32), ("n_levels", C.c_int32), ("stop", C.c_int32), ("reserved", C.c_int32),
                ("h", C.c_double), ("rho", C.c_double), ("theta", C.c_double * REGISTER_THETA), ("result", C.c_float * 16), ("map", C.c_float * 12),
                ("reserved2", C.c_float * 4), ("level", RegisterLevel * REGISTER_MAX_LEVELS), ("outside_before", C.c_int64), ("outside_after", C.c_int64),
                ("before", SimilarityRecord), ("after", SimilarityRecord)]


def register_params(**kw):
    """sift3d_register_defaults, then the given fields: dof, metric (0 / "mi", 1 / "nmi"), bins, max_iterations, device, min_overlap, form
    (a key of REGISTER_FORMS or its number), and levels = [(stride, first_step, last_step), ...] with the steps in multiples of h"""
    p = RegisterParams()
    host_lib().sift3d_register_defaults(C.byref(p))
    for k, v in kw.items():
        if k == "levels":
            p.n_levels = len(v)
            for l, (s, a, b) in enumerate(v[:REGISTER_MAX_LEVELS]):
                p.stride[l], p.first_step[l], p.last_step[l] = int(s), float(a), float(b)
        elif k == "min_overlap":
            p.min_overlap = float(v)
        elif k in ("dof", "bins", "max_iterations", "device", "n_levels"):
            setattr(p, k, int(v))
        elif k == "metric":
            p.metric = int(REGISTER_METRICS.get(v, v))
        elif k == "form":
            p.form = int(REGISTER_FORMS.get(v, v))
        else:
            raise ValueError("no registration parameter %s" % k)
    return p


def register_check(p):
    """sift3d_register_check: None, or the text with which the parameters are refused"""
    err = C.create_string_buffer(512)
    return None if host_lib().sift3d_register_check(C.byref(p), err, len(err)) == 0 else err.value.decode()


def _theta(theta):
    t = np.ascontiguousarray(theta, np.float64)
    if t.size != REGISTER_THETA:
        raise ValueError("theta is 12 numbers: t, r, s, g")
    return t.reshape(REGISTER_THETA)


def register_map(theta, shape, fixed_vox2key=None, moving_vox2key=None, initial=None):
    """sift3d_register_map: the 3 x 4 float32 map fixed voxel -> moving voxel of theta for a fixed image of shape (nz, ny, nx)"""
    t, (nz, ny, nx) = _theta(theta), (int(d) for d in shape)
    fv, mv, m0 = _m16(fixed_vox2key), _m16(moving_vox2key), _m16(initial)
    out = np.zeros(12, np.float32)
    if host_lib().sift3d_register_map(t.ctypes.data, nx, ny, nz, _ptr(fv), _ptr(mv), _ptr(m0), out.ctypes.data) != 0:
        raise Sift3DError("sift3d_register_map: a matrix is singular, not finite or its last row is not 0 0 0 1")
    return out.reshape(3, 4)


def register_result(theta, shape, fixed_vox2key=None, initial=None):
    """sift3d_register_result: the 4 x 4 float32 moving -> fixed matrix M1 = inv(D(theta)) . M0"""
    t, (nz, ny, nx) = _theta(theta), (int(d) for d in shape)
    fv, m0 = _m16(fixed_vox2key), _m16(initial)
    out = np.zeros(16, np.float32)
    if host_lib().sift3d_register_result(t.ctypes.data, nx, ny, nz, _ptr(fv), _ptr(m0), out.ctypes.data) != 0:
        raise Sift3DError("sift3d_register_result: a matrix is singular, not finite or its last row is not 0 0 0 1")
    return out.reshape(4, 4)


def register_candidates(theta, dof, u, rho):
    """sift3d_register_candidates: (2 active parameters) x 12 float64, + before -"""
    t, out = _theta(theta), np.zeros((2 * REGISTER_THETA, REGISTER_THETA), np.float64)
    n = host_lib().sift3d_register_candidates(t.ctypes.data, int(dof), float(u), float(rho), out.ctypes.data)
    if n < 0:
        raise Sift3DError("sift3d_register_candidates: dof = %d is not 3, 6, 7, 9 or 12" % int(dof))
    return out[:n].copy()


def register_lattice(shape, stride, fixed_vox2key=None):
    """sift3d_register_lattice of a fixed image of shape (nz, ny, nx): (N, points per axis (x, y, z), h, rho)"""
    nz, ny, nx = (int(d) for d in shape)
    fv, n, h, rho = _m16(fixed_vox2key), (C.c_int64 * 3)(), C.c_double(0), C.c_double(0)
    N = host_lib().sift3d_register_lattice(nx, ny, nz, int(stride), _ptr(fv), n, C.byref(h), C.byref(rho))
    if N < 0:
        raise Sift3DError("sift3d_register_lattice: an extent below 1, a stride other than 1, 2, 4, 8 or a degenerate vox2key")
    return int(N), tuple(int(v) for v in n), h.value, rho.value


def warp_histogram(fixed, moving, maps, fixed_range, moving_range, stride=1, bins=64, form="default", device=0, return_ms=False):
    """sift3d_warp_histogram: the joint histograms of fixed (nz, ny, nx) and moving (mz, my, mx) under K maps (K x 3 x 4, fixed voxel ->
    moving voxel) on the lattice of the stride: (hist int64 K x bins x bins, sums K lists of six Python integers, excluded K, outside K).
    return_ms=True appends kernel_ms."""
    f, m = _f32(fixed), _f32(moving)
    if f.ndim != 3 or m.ndim != 3:
        raise ValueError("the images are (nz, ny, nx)")
    a = np.ascontiguousarray(maps, np.float32)
    if a.size % 12:
        raise ValueError("a map is 3 x 4 floats")
    a = a.reshape(-1, 12)
    K, bins = len(a), int(bins)
    (nz, ny, nx), (mz, my, mx) = f.shape, m.shape
    hist, sums = np.zeros((K, max(bins, 0), max(bins, 0)), np.int64), np.zeros((K, len(SIMILARITY_SUMS)), np.int64)
    excluded, outside, ms = np.zeros(K, np.int64), np.zeros(K, np.int64), C.c_double(0.0)
    fr, mr = (C.c_float * 2)(*[float(v) for v in fixed_range]), (C.c_float * 2)(*[float(v) for v in moving_range])
    _call("sift3d_warp_histogram", int(device), f.ctypes.data, nx, ny, nz, m.ctypes.data, mx, my, mz, a.ctypes.data, K, int(stride), fr, mr, bins,
          int(REGISTER_FORMS.get(form, form)), hist.ctypes.data, sums.ctypes.data, excluded.ctypes.data, outside.ctypes.data, C.byref(ms))
    out = (hist, [[int(v) for v in row] for row in sums], [int(v) for v in excluded], [int(v) for v in outside])
    return out + (ms.value,) if return_ms else out


def _register_report_dict(r):
    d = {"dof": int(r.dof), "metric": int(r.metric), "bins": int(r.bins), "stop": int(r.stop), "h": float(r.h), "rho": float(r.rho),
         "theta": np.array(r.theta[:], np.float64), "result": np.array(r.result[:], np.float32).reshape(4, 4), "map": np.array(r.map[:], np.float32).reshape(3, 4),
         "levels": [{k: (float if k in ("score_in", "score_out", "last_step", "device_ms") else int)(getattr(v, k)) for k, _ in RegisterLevel._fields_}
                    for v in r.level[:r.n_levels]],
         "outside_before": int(r.outside_before), "outside_after": int(r.outside_after), "before": _image_similarity_dict(r.before, None),
         "after": _image_similarity_dict(r.after, None), "struct": r}
    return d


def register_affine(fixed, moving, fixed_vox2key=None, moving_vox2key=None, initial=None, **params):
    """sift3d_register_affine: the affine alignment of moving (mz, my, mx) to fixed (nz, ny, nx) by mutual information.  A dict: theta
    (12 float64), result (M1, 4 x 4 float32, moving keys -> fixed keys: write_matrix's input), map, levels (one dict per level), stop,
    before and after (image_similarity's dicts on the whole lattice under theta = 0 and theta*), outside_before, outside_after.
    params: fields of register_params."""
    f, m = _f32(fixed), _f32(moving)
    if f.ndim != 3 or m.ndim != 3:
        raise ValueError("the images are (nz, ny, nx)")
    (nz, ny, nx), (mz, my, mx) = f.shape, m.shape
    fv, mv, m0 = _m16(fixed_vox2key), _m16(moving_vox2key), _m16(initial)
    p, rep = register_params(**params), RegisterReport()
    _call("sift3d_register_affine", f.ctypes.data, nx, ny, nz, m.ctypes.data, mx, my, mz, _ptr(fv), _ptr(mv), _ptr(m0), C.byref(p), C.byref(rep))
    return _register_report_dict(rep)


def register_report_text(report):
    """sift3d_register_report_text of what register_affine returned (or of a RegisterReport)"""
    r = report["struct"] if isinstance(report, dict) else report
    need = host_lib().sift3d_register_report_text(C.byref(r), None, 0)
    if need < 0:
        raise Sift3DError("sift3d_register_report_text -> %d" % need)
    buf = C.create_string_buffer(need + 1)
    if host_lib().sift3d_register_report_text(C.byref(r), buf, len(buf)) != need:
        raise Sift3DError("sift3d_register_report_text: the length changed")
    return buf.value.decode()


# ---- a template from up to 32 warped images (featAverage), DESIGN.md section 7r -----------------------------------------------------
AVERAGE_MAX_IMAGES, AVERAGE_MAX_TRIM = 32, 15
AVERAGE_FORMS = {"default": -1, "column": 0}
AVERAGE_MODES = {"mean": 0, "median": AVERAGE_MAX_TRIM}


class AverageParams(C.Structure):
    """sift3d_average_params"""
    _fields_ = [("trim", C.c_int32), ("min_count", C.c_int32), ("fill", C.c_float), ("device", C.c_int32), ("max_voxels", C.c_int64), ("form", C.c_int32),
                ("reserved", C.c_int32)]


class AverageImage(C.Structure):
    """sift3d_average_image"""
    _fields_ = [("image", C.c_void_p), ("nx", C.c_int64), ("ny", C.c_int64), ("nz", C.c_int64), ("vox2key", C.c_void_p), ("moving_to_fixed", C.c_void_p),
                ("field", C.c_void_p)]


class AverageImageReport(C.Structure):
    """sift3d_average_image_report"""
    _fields_ = [("contributing", C.c_int64), ("upload_ms", C.c_double)]


class AverageReport(C.Structure):
    """sift3d_average_report"""
    _fields_ = [("images", C.c_int32), ("trim", C.c_int32), ("min_count", C.c_int32), ("reserved", C.c_int32), ("voxels", C.c_int64), ("none", C.c_int64),
                ("below", C.c_int64), ("count", C.c_int64 * (AVERAGE_MAX_IMAGES + 1)), ("kernel_ms", C.c_double), ("wall_ms", C.c_double),
                ("image", AverageImageReport * AVERAGE_MAX_IMAGES)]


def average_params(**kw):
    """sift3d_average_defaults, then the given fields: trim (0 .. 15, or "mean" / "median"), min_count, fill, device, max_voxels, form (a
    key of AVERAGE_FORMS or its number)"""
    p = AverageParams()
    host_lib().sift3d_average_defaults(C.byref(p))
    for k, v in kw.items():
        if k == "trim":
            p.trim = int(AVERAGE_MODES.get(v, v))
        elif k == "form":
            p.form = int(AVERAGE_FORMS.get(v, v))
        elif k == "fill":
            p.fill = float(v)
        elif k in ("min_count", "device", "max_voxels"):
            setattr(p, k, int(v))
        else:
            raise ValueError("no averaging parameter %s" % k)
    return p


def average_check(p, K):
    """sift3d_average_check: None, or the text with which the parameters are refused for K images"""
    err = C.create_string_buffer(512)
    return None if host_lib().sift3d_average_check(C.byref(p), int(K), err, len(err)) == 0 else err.value.decode()


def _average_report_dict(r):
    K = int(r.images)
    return {"images": K, "trim": int(r.trim), "min_count": int(r.min_count), "voxels": int(r.voxels), "none": int(r.none), "below": int(r.below),
            "count": [int(v) for v in r.count[:K + 1]], "kernel_ms": float(r.kernel_ms), "wall_ms": float(r.wall_ms),
            "image": [{"contributing": int(r.image[k].contributing), "upload_ms": float(r.image[k].upload_ms)} for k in range(K)], "struct": r}


def average_counts(mask, K, trim=0, min_count=1):
    """sift3d_average_counts: the report's counts (a dict as average_warped's report, the times 0) from a mask plane"""
    m = np.ascontiguousarray(mask, np.uint32)
    rep = AverageReport()
    if host_lib().sift3d_average_counts(m.ctypes.data, m.size, int(K), int(trim), int(min_count), C.byref(rep)) != 0:
        raise Sift3DError("sift3d_average_counts: K outside 1 .. 32, or the mask holds a bit at or above K")
    return _average_report_dict(rep)


def average_report_text(report):
    """sift3d_average_report_text of what average_warped returned as its report (or of an AverageReport)"""
    r = report["struct"] if isinstance(report, dict) else report
    need = host_lib().sift3d_average_report_text(C.byref(r), None, 0)
    if need < 0:
        raise Sift3DError("sift3d_average_report_text -> %d" % need)
    buf = C.create_string_buffer(need + 1)
    if host_lib().sift3d_average_report_text(C.byref(r), buf, len(buf)) != need:
        raise Sift3DError("sift3d_average_report_text: the length changed")
    return buf.value.decode()


def mean_field(fields):
    """sift3d_mean_field: the node-wise mean of field dicts on one node grid, a field dict.  Raises where a grid differs."""
    K = len(fields)
    arr, keep = (Field * max(K, 1))(), []
    for k, d in enumerate(fields):
        f, disp = _field_struct(d)
        keep.append(disp)
        arr[k] = f
    out, err = Field(), C.create_string_buffer(512)
    rc = host_lib().sift3d_mean_field(K, arr, C.byref(out), err, len(err))
    if rc == -4:
        disp = np.zeros(3 * int(out.n[0]) * int(out.n[1]) * int(out.n[2]), np.float32)
        out.capacity, out.disp = disp.size, disp.ctypes.data
        rc = host_lib().sift3d_mean_field(K, arr, C.byref(out), err, len(err))
    if rc != 0:
        e = Sift3DError("sift3d_mean_field -> %d: %s" % (rc, err.value.decode(errors="replace")))
        e.code = rc
        raise e
    return _field_dict(out, disp)


def average_warped(shape, images, grid_vox2key=None, **params):
    """sift3d_average_warped: the template of K images on the grid of shape (nz, ny, nx).  images: dicts with image ((nz, ny, nx) float32)
    and optionally t (the image's moving -> fixed key transform against the grid, 4 x 4; None: identity), vox2key (4 x 4) and field (a
    field dict); params: fields of average_params.  Returns (avg float32, var float32, mask uint32, report dict), the planes (nz, ny, nx)."""
    nz, ny, nx = (int(d) for d in shape)
    K = len(images)
    arr, keep = (AverageImage * max(K, 1))(), []
    for k, a in enumerate(images):
        im = _f32(a["image"])
        if im.ndim != 3:
            raise ValueError("image %d is not (nz, ny, nx)" % k)
        mv, tm = _m16(a.get("vox2key")), _m16(a.get("t"))
        fs, disp = _field_struct(a["field"]) if a.get("field") is not None else (None, None)
        keep.append((im, mv, tm, fs, disp))
        arr[k].image = im.ctypes.data
        arr[k].nz, arr[k].ny, arr[k].nx = im.shape
        arr[k].vox2key, arr[k].moving_to_fixed = _ptr(mv), _ptr(tm)
        arr[k].field = C.addressof(fs) if fs is not None else None
    avg, var, mask = (np.zeros((max(nz, 0), max(ny, 0), max(nx, 0)), t) for t in (np.float32, np.float32, np.uint32))
    p, rep = average_params(**params), AverageReport()
    _call("sift3d_average_warped", nx, ny, nz, _ptr(_m16(grid_vox2key)), K, arr, C.byref(p), avg.ctypes.data, var.ctypes.data, mask.ctypes.data, C.byref(rep))
    return avg, var, mask, _average_report_dict(rep)


# ---- intensity matching of a registered image (featNormalize), DESIGN.md section 7s -------------------------------------------------
NORMALIZE_BINS, NORMALIZE_MAX_KNOTS = 1024, 257
NORMALIZE_MODES = {"linear": 0, "hist": 1}
NORMALIZE_COUNTS = ("masked", "outside", "excluded")


class NormalizeParams(C.Structure):
    """sift3d_normalize_params"""
    _fields_ = [("mode", C.c_int32), ("knots", C.c_int32), ("device", C.c_int32), ("reserved", C.c_int32)]


class Transfer(C.Structure):
    """sift3d_transfer"""
    _fields_ = [("mode", C.c_int32), ("m", C.c_int32), ("a_lo", C.c_float), ("a_hi", C.c_float), ("b_lo", C.c_float), ("b_hi", C.c_float), ("wa", C.c_double),
                ("tail", C.c_double), ("xb", C.c_double * NORMALIZE_MAX_KNOTS), ("xa", C.c_double * NORMALIZE_MAX_KNOTS), ("slope", C.c_double * NORMALIZE_MAX_KNOTS)]


class NormalizeReport(C.Structure):
    """sift3d_normalize_report"""
    _fields_ = [("mode", C.c_int32), ("knots", C.c_int32), ("reference_voxels", C.c_int64), ("image_voxels", C.c_int64), ("counts", C.c_int64 * 3),
                ("sums", C.c_int64 * 6), ("hist_ms", C.c_double), ("apply_ms", C.c_double), ("wall_ms", C.c_double), ("table", Transfer)]


def normalize_params(**kw):
    """sift3d_normalize_defaults, then the given fields: mode ("linear", "hist" or its number), knots, device"""
    p = NormalizeParams()
    host_lib().sift3d_normalize_defaults(C.byref(p))
    for k, v in kw.items():
        if k == "mode":
            p.mode = int(NORMALIZE_MODES.get(v, v))
        elif k in ("knots", "device"):
            setattr(p, k, int(v))
        else:
            raise ValueError("no normalisation parameter %s" % k)
    return p


def normalize_check(p):
    """sift3d_normalize_check: None, or the text with which the parameters are refused"""
    err = C.create_string_buffer(512)
    return None if host_lib().sift3d_normalize_check(C.byref(p), err, len(err)) == 0 else err.value.decode()


def _transfer_dict(t):
    m = int(t.m)
    return {"mode": int(t.mode), "m": m, "a_range": (np.float32(t.a_lo), np.float32(t.a_hi)), "b_range": (np.float32(t.b_lo), np.float32(t.b_hi)), "wa": float(t.wa),
            "tail": float(t.tail), "xb": np.array(t.xb[:m], np.float64), "xa": np.array(t.xa[:m], np.float64), "slope": np.array(t.slope[:max(m - 1, 0)], np.float64),
            "struct": t}


def transfer_struct(d):
    """a Transfer from a table dict (its struct, or its fields: mode, a_range, b_range, wa, tail, xb, xa, slope)"""
    if isinstance(d, Transfer):
        return d
    if d.get("struct") is not None:
        return d["struct"]
    t = Transfer()
    t.mode, t.m = int(d.get("mode", 0)), len(d["xb"])
    (t.a_lo, t.a_hi), (t.b_lo, t.b_hi) = d["a_range"], d["b_range"]
    t.wa, t.tail = float(d["wa"]), float(d["tail"])
    for k in range(min(t.m, NORMALIZE_MAX_KNOTS)):
        t.xb[k], t.xa[k] = float(d["xb"][k]), float(d["xa"][k])
        if k < len(d["slope"]):
            t.slope[k] = float(d["slope"][k])
    return t


def normalize_transfer(mode, hist_a, hist_b, sums, a_range, b_range, knots=64):
    """sift3d_normalize_transfer: the table dict (mode, m, a_range, b_range, wa, tail, xb, xa, slope) of two histograms (1024 int64 each)
    and the six sums; raises Sift3DError with the refusal's text"""
    ha, hb, s = (np.ascontiguousarray(v, np.int64) for v in (hist_a, hist_b, sums))
    if ha.size != NORMALIZE_BINS or hb.size != NORMALIZE_BINS or s.size != 6:
        raise ValueError("two histograms of 1024 words and six sums")
    ar, br = (C.c_float * 2)(*[float(v) for v in a_range]), (C.c_float * 2)(*[float(v) for v in b_range])
    t, err = Transfer(), C.create_string_buffer(512)
    rc = host_lib().sift3d_normalize_transfer(int(NORMALIZE_MODES.get(mode, mode)), int(knots), ha.ctypes.data, hb.ctypes.data, s.ctypes.data, ar, br, C.byref(t), err, len(err))
    if rc != 0:
        e = Sift3DError("sift3d_normalize_transfer -> %d: %s" % (rc, err.value.decode(errors="replace")))
        e.code = rc
        raise e
    return _transfer_dict(t)


def transfer_check(table):
    """sift3d_transfer_check: None, or the text with which the table is refused"""
    err = C.create_string_buffer(512)
    return None if host_lib().sift3d_transfer_check(C.byref(transfer_struct(table)), err, len(err)) == 0 else err.value.decode()


def _normalize_image(a):
    """(AverageImage, what it points to) of an image dict: image and optionally t, vox2key, field, as average_warped takes them"""
    im = _f32(a["image"])
    if im.ndim != 3:
        raise ValueError("the image is not (nz, ny, nx)")
    mv, tm = _m16(a.get("vox2key")), _m16(a.get("t"))
    fs, disp = _field_struct(a["field"]) if a.get("field") is not None else (None, None)
    s = AverageImage()
    s.image = im.ctypes.data
    s.nz, s.ny, s.nx = im.shape
    s.vox2key, s.moving_to_fixed = _ptr(mv), _ptr(tm)
    s.field = C.addressof(fs) if fs is not None else None
    return s, (im, mv, tm, fs, disp)


def _reference(reference, mask):
    r = _f32(reference)
    if r.ndim != 3:
        raise ValueError("the reference is not (nz, ny, nx)")
    k = None if mask is None else _f32(mask)
    if k is not None and k.shape != r.shape:
        raise ValueError("the mask is on the reference's grid")
    return r, k


def overlap_histograms(reference, image, ref_range, image_range, ref_vox2key=None, mask=None, device=0, return_ms=False):
    """sift3d_overlap_histograms: (hist_a int64 1024, hist_b int64 1024, sums: six Python integers, counts: a dict masked, outside,
    excluded) of the reference (nz, ny, nx) and an image dict (image, t, vox2key, field) with the ranges given.  return_ms=True appends kernel_ms."""
    r, k = _reference(reference, mask)
    s, keep = _normalize_image(image)
    nz, ny, nx = r.shape
    ha, hb, sums, counts, ms = np.zeros(NORMALIZE_BINS, np.int64), np.zeros(NORMALIZE_BINS, np.int64), np.zeros(6, np.int64), np.zeros(3, np.int64), C.c_double(0.0)
    rr, ir = (C.c_float * 2)(*[float(v) for v in ref_range]), (C.c_float * 2)(*[float(v) for v in image_range])
    _call("sift3d_overlap_histograms", int(device), r.ctypes.data, nx, ny, nz, _ptr(_m16(ref_vox2key)), None if k is None else k.ctypes.data, C.addressof(s), rr, ir,
          ha.ctypes.data, hb.ctypes.data, sums.ctypes.data, counts.ctypes.data, C.byref(ms))
    out = (ha, hb, [int(v) for v in sums], dict(zip(NORMALIZE_COUNTS, (int(v) for v in counts))))
    return out + (ms.value,) if return_ms else out


def apply_transfer(image, table, device=0, return_ms=False):
    """sift3d_apply_transfer: the table (normalize_transfer's dict, or a Transfer) applied to every voxel of image; float32 of its shape"""
    v = _f32(image)
    out, ms = np.empty(v.shape, np.float32), C.c_double(0.0)
    _call("sift3d_apply_transfer", int(device), v.ctypes.data, v.size, C.byref(transfer_struct(table)), out.ctypes.data, C.byref(ms))
    return (out, ms.value) if return_ms else out


def _normalize_report_dict(r):
    return {"mode": int(r.mode), "knots": int(r.knots), "reference_voxels": int(r.reference_voxels), "image_voxels": int(r.image_voxels),
            "counts": dict(zip(NORMALIZE_COUNTS, (int(v) for v in r.counts))), "sums": [int(v) for v in r.sums], "hist_ms": float(r.hist_ms),
            "apply_ms": float(r.apply_ms), "wall_ms": float(r.wall_ms), "table": _transfer_dict(r.table) if r.table.m >= 2 else None, "struct": r}


def normalize_intensity(reference, image, ref_vox2key=None, mask=None, **params):
    """sift3d_normalize_intensity: the image dict (image, t, vox2key, field) on its own grid on the reference's intensity scale: (out
    float32 of the image's shape, report dict).  params: fields of normalize_params.  A refusal raises Sift3DError with .report, the
    counts as far as they were taken."""
    r, k = _reference(reference, mask)
    s, keep = _normalize_image(image)
    nz, ny, nx = r.shape
    out, p, rep = np.empty(keep[0].shape, np.float32), normalize_params(**params), NormalizeReport()
    try:
        _call("sift3d_normalize_intensity", r.ctypes.data, nx, ny, nz, _ptr(_m16(ref_vox2key)), None if k is None else k.ctypes.data, C.addressof(s), C.byref(p),
              out.ctypes.data, C.byref(rep))
    except Sift3DError as e:
        e.report = _normalize_report_dict(rep)
        raise
    return out, _normalize_report_dict(rep)


def normalize_report_text(report):
    """sift3d_normalize_report_text of what normalize_intensity returned as its report (or of a NormalizeReport)"""
    r = report["struct"] if isinstance(report, dict) else report
    need = host_lib().sift3d_normalize_report_text(C.byref(r), None, 0)
    if need < 0:
        raise Sift3DError("sift3d_normalize_report_text -> %d" % need)
    buf = C.create_string_buffer(need + 1)
    if host_lib().sift3d_normalize_report_text(C.byref(r), buf, len(buf)) != need:
        raise Sift3DError("sift3d_normalize_report_text: the length changed")
    return buf.value.decode()


def _map12(m):
    a = np.ascontiguousarray(m, np.float32)
    if a.size != 12:
        raise ValueError("a resampling map is 3 x 4 floats")
    return a.reshape(12)


def resample_affine(vol, out_shape, map, interp="linear", fill=0.0, device=0, return_ms=False):
    """sift3d_resample_affine: vol (nz, ny, nx) float32 resampled onto an output of out_shape = (oz, oy, ox) through the
    3 x 4 map that takes an output voxel index (i, j, k) to a source voxel position.  interp "linear", "nearest" or "label" (label-aware linear, for label maps); output
    voxels that map outside the source get fill.  return_ms=True returns (out, kernel_ms)."""
    v = _f32(vol)
    nz, ny, nx = v.shape
    oz, oy, ox = (int(d) for d in out_shape)
    out = np.empty((oz, oy, ox), np.float32)
    m = _map12(map)
    ms = C.c_double(0.0)
    _call("sift3d_resample_affine", int(device), v.ctypes.data, nx, ny, nz, out.ctypes.data, ox, oy, oz, m.ctypes.data, INTERP[interp],
          float(fill), C.byref(ms))
    return (out, ms.value) if return_ms else out


def resample_map(moving_to_fixed, fixed_vox2key=None, moving_vox2key=None):
    """sift3d_resample_map: the 3 x 4 map that puts the moving image on the fixed grid, inv(moving_vox2key) .
    inv(moving_to_fixed) . fixed_vox2key in double, rounded to float32 once (4 x 4 inputs; None = identity)."""
    ms = [None if a is None else np.ascontiguousarray(a, np.float32).reshape(16) for a in (moving_to_fixed, fixed_vox2key, moving_vox2key)]
    if ms[0] is None:
        raise ValueError("moving_to_fixed is required")
    out = np.zeros(12, np.float32)
    if host_lib().sift3d_resample_map(*[None if a is None else a.ctypes.data for a in ms], out.ctypes.data) != 0:
        raise Sift3DError("sift3d_resample_map: a matrix is singular or its last row is not 0 0 0 1")
    return out.reshape(3, 4)


def key_vox2key(voxel=(1.0, 1.0, 1.0), world=None):
    """sift3d_key_vox2key: the 4 x 4 float32 map from an image's voxel indices to the key coordinates featExtract writes
    for it -- x + 0.5 in voxel units (world None), world . (x + 0.5 f) under -w / -ws (world: the qto_xyz / sto_xyz used,
    f = min(voxel) / voxel)."""
    v = np.ascontiguousarray(voxel, np.float32).reshape(3)
    w = None if world is None else np.ascontiguousarray(world, np.float32).reshape(16)
    m = np.zeros(16, np.float32)
    host_lib().sift3d_key_vox2key(v.ctypes.data, None if w is None else w.ctypes.data, m.ctypes.data)
    return m.reshape(4, 4)


def similarity_matrix(d):
    """sift3d_similarity_matrix: the 4 x 4 float32 matrix WriteMatrix prints for a match_keys-style dict, before %f."""
    t, _keep = _similarity_struct(d)
    m = np.zeros(16, np.float32)
    host_lib().sift3d_similarity_matrix(C.byref(t), m.ctypes.data)
    return m.reshape(4, 4)


def read_similarity(path):
    """sift3d_read_similarity: the 4 x 4 float32 matrix of a .trans.txt file."""
    m = np.zeros(16, np.float32)
    if host_lib().sift3d_read_similarity(os.fsencode(path), m.ctypes.data) != 0:
        raise Sift3DError("could not read a 4 x 4 similarity with last row 0 0 0 1 from %s" % path)
    return m.reshape(4, 4)


def match_votes(first, labels, n_labels, nn_idx, nn_dist2):
    """sift3d_match_votes: (votes, counts), each n_images x n_labels."""
    first = np.ascontiguousarray(first, np.int64)
    labels = np.ascontiguousarray(labels, np.int32)
    nn_idx = np.ascontiguousarray(nn_idx, np.int32)
    nn_dist2 = np.ascontiguousarray(nn_dist2, np.int32)
    n_img, k = len(first) - 1, nn_idx.shape[1]
    votes = np.zeros((n_img, n_labels), np.float32)
    counts = np.zeros((n_img, n_labels), np.int32)
    rc = host_lib().sift3d_match_votes(None, first.ctypes.data, n_img, labels.ctypes.data, int(n_labels), nn_idx.ctypes.data,
                                       nn_dist2.ctypes.data, k, votes.ctypes.data, counts.ctypes.data)
    if rc != 0:
        raise Sift3DError("sift3d_match_votes -> %d" % rc)
    return votes, counts


LIBM_CURRENT, LIBM_GCC5 = 0, 1   # sift3d_set_libm_variant


def set_libm_variant(which):
    """Process-wide: which build of the reference the Gaussian taps follow (include/sift3d.h); returns the previous setting."""
    r = hip_lib().sift3d_set_libm_variant(int(which))
    if r < 0:
        raise Sift3DError("sift3d_set_libm_variant(%r) -> %d" % (which, r))
    return r


def gauss_taps(sigma, min_value=0.01):
    t = np.zeros(129, np.float32)
    n = hip_lib().sift3d_gauss_taps(float(sigma), float(min_value), t.ctypes.data)
    if n < 0:
        raise Sift3DError("sift3d_gauss_taps(%r, %r) -> %d" % (sigma, min_value, n))
    return t[:n].copy()


def synth_blobs(nx, ny, nz, seed=12345):
    """Deterministic blob-field volume, shape (nz, ny, nx) float32."""
    v = np.empty((nz, ny, nx), np.float32)
    host_lib().sift3d_synth_blobs(v.ctypes.data, nx, ny, nz, seed)
    return v


def synth_blobs_slices(nx, ny, nz, z0, z1, seed=12345):
    """Planes [z0, z1) of synth_blobs(nx, ny, nz, seed), without making the rest: shape (z1 - z0, ny, nx)."""
    z0, z1 = max(0, int(z0)), min(int(nz), int(z1))
    v = np.empty((max(0, z1 - z0), ny, nx), np.float32)
    if z1 > z0:
        host_lib().sift3d_synth_blobs_slices(v.ctypes.data, nx, ny, nz, seed, z0, z1)
    return v


class _NiftiMinImage(C.Structure):
    """nifti_min_image (csrc/nifti_min.h)"""
    _fields_ = [("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int), ("nt", C.c_int), ("dx", C.c_float), ("dy", C.c_float),
                ("dz", C.c_float), ("datatype", C.c_int), ("qform_code", C.c_int), ("sform_code", C.c_int),
                ("qto_xyz", C.c_float * 16), ("sto_xyz", C.c_float * 16), ("data", C.POINTER(C.c_float))]


def nifti_fast_inflate(on):
    """csrc/nifti_min.h: 0 = gzip'ed files through zlib only; 1 (default) = through libdeflate where the system has it."""
    host_lib().nifti_min_fast_inflate(int(bool(on)))


def nifti_fast_inflate_count():
    return int(host_lib().nifti_min_fast_inflate_count())


def read_nifti(path):
    """nifti_min_read: (volume float32 of shape (nt*nz, ny, nx), header dict).  Raises Sift3DError with the reader's code."""
    img = _NiftiMinImage()
    rc = host_lib().nifti_min_read(os.fsencode(path), C.byref(img))
    if rc != 0:
        e = Sift3DError("nifti_min_read(%s) -> %d" % (path, rc))
        e.code = rc
        raise e
    try:
        n = img.nx * img.ny * img.nz * img.nt
        vol = np.ctypeslib.as_array(img.data, shape=(n,)).copy().reshape(img.nt * img.nz, img.ny, img.nx)
        hdr = {"dims": (img.nx, img.ny, img.nz, img.nt), "voxel": (img.dx, img.dy, img.dz), "datatype": img.datatype,
               "qform_code": img.qform_code, "sform_code": img.sform_code,
               "qto_xyz": np.array(img.qto_xyz, np.float32).reshape(4, 4), "sto_xyz": np.array(img.sto_xyz, np.float32).reshape(4, 4)}
    finally:
        host_lib().nifti_min_free(C.byref(img))
    return vol, hdr


def write_nifti(path, vol, voxel=(1.0, 1.0, 1.0), qform=None, sform=None):
    """float32 .nii writer.  qform = (quatern_b, c, d, qoffset_x, y, z, qfac), sform = 12 floats (srow_x, y, z)."""
    vol = np.ascontiguousarray(vol, np.float32)
    nz, ny, nx = vol.shape
    q = None if qform is None else np.ascontiguousarray(qform, np.float32).reshape(7)
    s = None if sform is None else np.ascontiguousarray(sform, np.float32).reshape(12)
    rc = host_lib().nifti_min_write_f32_ex(os.fsencode(path), vol.ctypes.data, nx, ny, nz, *[float(v) for v in voxel],
                                           None if q is None else q.ctypes.data, None if s is None else s.ctypes.data)
    if rc != 0:
        raise Sift3DError("could not write %s" % path)


def write_key(path, feats, eig_thres=140.0, comments=()):
    feats = np.ascontiguousarray(feats, FEATURE_DTYPE)
    arr = (C.c_char_p * max(1, len(comments)))(*[c.encode() for c in comments])
    rc = host_lib().sift3d_write_key(os.fsencode(path), feats.ctypes.data, len(feats), float(eig_thres), len(comments),
                                     C.cast(arr, C.c_void_p))
    if rc != 0:
        raise Sift3DError("could not write %s" % path)


def write_key_bin(path, feats, eig_thres=140.0):
    """msFeature3DVectorOutputBin: header lines as text, then fixed-size binary records."""
    feats = np.ascontiguousarray(feats, FEATURE_DTYPE)
    if host_lib().sift3d_write_key_bin(os.fsencode(path), feats.ctypes.data, len(feats), float(eig_thres)) != 0:
        raise Sift3DError("could not write %s" % path)


def world_transform(feats, m44):
    """sift3d_world_transform (featExtract.cpp:436-538): records to world coordinates through a 4 x 4 voxel-to-mm matrix."""
    out = np.ascontiguousarray(feats, FEATURE_DTYPE).copy()
    m = np.ascontiguousarray(m44, np.float32).reshape(4, 4)
    host_lib().sift3d_world_transform(out.ctypes.data, len(out), m.ctypes.data)
    return out


def write_pgm(path, slice_yx):
    """output_float + GenericImage::WriteToFile: an x-y slice of floats as the reference's image.pgm."""
    a = _f32(slice_yx)
    if a.ndim != 2 or host_lib().sift3d_write_pgm(os.fsencode(path), a.ctypes.data, a.shape[0], a.shape[1]) != 0:
        raise Sift3DError("could not write %s" % path)


def read_key(path):
    """msFeature3DVectorInputText: the records of a text .key file as a FEATURE_DTYPE array."""
    L = host_lib()
    ptr, n = C.c_void_p(), C.c_int64(0)
    rc = L.sift3d_read_key(os.fsencode(path), C.byref(ptr), C.byref(n))
    if rc != 0:
        raise Sift3DError("could not read %s (%d)" % (path, rc))
    out = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n.value * FEATURE_DTYPE.itemsize,)).view(FEATURE_DTYPE).copy()
    L.free_ptr(ptr)
    return out


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


class Context:
    """Device-resident pyramid for volumes of up to nx*ny*nz voxels on one HIP device."""

    def __init__(self, nx, ny, nz, device=0, slab=False):
        """slab=True: sift3d_create_slab -- a context for the Z-slab building blocks, without level buffers of its own."""
        self._L = hip_lib()
        if self._L.sift3d_device_count() <= 0:
            raise Sift3DError("no HIP device visible and there is no CPU fallback")
        make = self._L.sift3d_create_slab if slab else self._L.sift3d_create
        self._h = make(int(device), int(nx), int(ny), int(nz))
        if not self._h:
            raise Sift3DError("sift3d_create%s(device=%d, %d x %d x %d) failed" % ("_slab" if slab else "", device, nx, ny, nz))
        self.device = device
        self._shape = None   # (nz, ny, nx) of the volume last set, after its resize

    def set_tuning(self, knob, value):
        """sift3d_set_tuning: TUNE_* knobs (tests and A/B timing; no knob changes a result)."""
        self._chk(self._L.sift3d_set_tuning(self._h, int(knob), int(value)), "sift3d_set_tuning")

    def host_buffer_grows(self):
        """sift3d_host_buffer_grows: runs on this context that outgrew their pinned record buffers."""
        return int(self._L.sift3d_host_buffer_grows(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._L.sift3d_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def _chk(self, rc, what):
        if rc != 0:
            raise Sift3DError("%s -> %d: %s" % (what, rc, self._L.sift3d_last_error(self._h).decode()))

    # ---- operator level (host arrays shaped (nz, ny, nx)) ----
    def gauss_blur(self, vol, sigma, min_value=0.01):
        vol = _f32(vol)
        nz, ny, nx = vol.shape
        out = np.empty_like(vol)
        self._chk(self._L.sift3d_gauss_blur(self._h, vol.ctypes.data, out.ctypes.data, nx, ny, nz, float(sigma),
                                            float(min_value)), "sift3d_gauss_blur")
        return out

    def dog(self, a, b):
        a, b = _f32(a), _f32(b)
        out = np.empty_like(a)
        self._chk(self._L.sift3d_dog(self._h, a.ctypes.data, b.ctypes.data, out.ctypes.data, a.size), "sift3d_dog")
        return out

    def subsample2(self, vol):
        vol = _f32(vol)
        nz, ny, nx = vol.shape
        out = np.empty((nz // 2, ny // 2, nx // 2), np.float32)
        self._chk(self._L.sift3d_subsample2(self._h, vol.ctypes.data, nx, ny, nz, out.ctypes.data), "sift3d_subsample2")
        return out

    def double_size(self, vol):
        vol = _f32(vol)
        nz, ny, nx = vol.shape
        out = np.empty((2 * nz, 2 * ny, 2 * nx), np.float32)
        self._chk(self._L.sift3d_double_size(self._h, vol.ctypes.data, nx, ny, nz, out.ctypes.data), "sift3d_double_size")
        return out

    def halve_size(self, vol):
        vol = _f32(vol)
        nz, ny, nx = vol.shape
        out = np.empty((nz // 2, ny // 2, nx // 2), np.float32)
        self._chk(self._L.sift3d_halve_size(self._h, vol.ctypes.data, nx, ny, nz, out.ctypes.data), "sift3d_halve_size")
        return out

    def selftest_lds_add(self, a, b):
        """(a + b on the vector ALU, a + b through ds_add_f32), both computed on the device."""
        a, b = _f32(a).ravel(), _f32(b).ravel()
        valu, lds = np.empty_like(a), np.empty_like(a)
        self._chk(self._L.sift3d_selftest_lds_add(self._h, a.ctypes.data, b.ctypes.data, a.size, valu.ctypes.data,
                                                  lds.ctypes.data), "sift3d_selftest_lds_add")
        return valu, lds

    def extrema(self, d_prev, d_cur, d_next=None, capacity=None):
        """Returns (minima, maxima) structured arrays in raster order."""
        d_prev, d_cur = _f32(d_prev), _f32(d_cur)
        nz, ny, nx = d_cur.shape
        d_next = None if d_next is None else _f32(d_next)
        cap = int(capacity) if capacity is not None else d_cur.size // 8 + 1024
        mins = np.zeros(cap, EXTREMUM_DTYPE)
        maxs = np.zeros(cap, EXTREMUM_DTYPE)
        nmin, nmax = C.c_int64(0), C.c_int64(0)
        rc = self._L.sift3d_extrema(self._h, d_prev.ctypes.data, d_cur.ctypes.data,
                                    None if d_next is None else d_next.ctypes.data, nx, ny, nz, mins.ctypes.data, cap,
                                    C.byref(nmin), maxs.ctypes.data, cap, C.byref(nmax))
        self._chk(rc, "sift3d_extrema")
        return mins[:nmin.value].copy(), maxs[:nmax.value].copy()

    # ---- pipeline level ----
    def set_volume(self, vol, resize=0):
        """resize: +1 / -1 = the -2+ / -2- options (doubled / halved on the device after the upload)."""
        vol = _f32(vol)
        nz, ny, nx = vol.shape
        self._chk(self._L.sift3d_set_volume_resized(self._h, vol.ctypes.data, nx, ny, nz, int(resize)), "sift3d_set_volume_resized")
        self._shape = self._resized((nz, ny, nx), resize)

    def reserve(self, n_extrema):
        self._chk(self._L.sift3d_reserve(self._h, int(n_extrema)), "sift3d_reserve")

    def set_volume_in_runs(self, vol, runs, resize=0):
        """sift3d_set_volume_begin / _planes / _end: the volume handed over in the given runs of planes [(z0, n), ...]."""
        vol = _f32(vol)
        nz, ny, nx = vol.shape
        self._chk(self._L.sift3d_set_volume_begin(self._h, nx, ny, nz, int(resize)), "sift3d_set_volume_begin")
        for z0, n in runs:
            part = vol[z0:z0 + n]
            self._chk(self._L.sift3d_set_volume_planes(self._h, part.ctypes.data, int(z0), int(n)), "sift3d_set_volume_planes")
        self._chk(self._L.sift3d_set_volume_end(self._h), "sift3d_set_volume_end")
        self._shape = self._resized((nz, ny, nx), resize)

    def set_volume_dev(self, dev_ptr, nx, ny, nz):
        self._chk(self._L.sift3d_set_volume_dev(self._h, C.c_void_p(int(dev_ptr)), nx, ny, nz), "sift3d_set_volume_dev")
        self._shape = (int(nz), int(ny), int(nx))

    @staticmethod
    def _resized(shape, resize):
        return tuple(2 * d if resize > 0 else d // 2 if resize < 0 else d for d in shape)

    # ---- the resident pyramid of the last detect / extract (tests) ----
    def _slice(self, entry, octave, level, z, shape_yx):
        out = np.empty(shape_yx, np.float32)
        nx, ny = C.c_int64(0), C.c_int64(0)
        self._chk(getattr(self._L, entry)(self._h, int(octave), int(level), int(z), out.ctypes.data, C.byref(nx), C.byref(ny)), entry)
        assert (ny.value, nx.value) == tuple(shape_yx), (entry, octave, (ny.value, nx.value), shape_yx)
        return out

    def level_slice(self, octave, level, z, shape_yx):
        """sift3d_get_level_slice: slice z of Gaussian level 0..4 of an octave, (ny_o, nx_o) float32."""
        return self._slice("sift3d_get_level_slice", octave, level, z, shape_yx)

    def dog_slice(self, octave, level, z, shape_yx):
        """sift3d_get_dog_slice: slice z of DoG level 0..4 of an octave; raises Sift3DError ("... not stored ...") for a level
        the last run did not store."""
        return self._slice("sift3d_get_dog_slice", octave, level, z, shape_yx)

    def pyramid(self):
        """The resident pyramid as the last detect / extract left it, assembled slice by slice: one dict per octave of that run,
        {"L": [L_0..L_4], "D": [D_0..D_4]}, each a (nz_o, ny_o, nx_o) float32 array -- or None for a DoG level the run did not
        store (dog_slice).  Any other refusal raises."""
        out = []
        shape = self._shape
        for o in range(int(self.timings()["n_octaves"])):
            assert min(shape) > 2, (o, shape)
            lv = {"L": [], "D": []}
            for j in range(5):
                lv["L"].append(np.stack([self.level_slice(o, j, z, shape[1:]) for z in range(shape[0])]))
                try:
                    lv["D"].append(np.stack([self.dog_slice(o, j, z, shape[1:]) for z in range(shape[0])]))
                except Sift3DError as e:
                    if "not stored" not in str(e):
                        raise
                    lv["D"].append(None)
            out.append(lv)
            shape = tuple(d // 2 for d in shape)
        return out

    def detect(self, initial_image_scale=1.0):
        out, n = C.c_void_p(), C.c_int64(0)
        self._chk(self._L.sift3d_detect(self._h, float(initial_image_scale), C.byref(out), C.byref(n)), "sift3d_detect")
        try:
            buf = (C.c_char * (n.value * CANDIDATE_DTYPE.itemsize)).from_address(out.value) if n.value else b""
            return np.frombuffer(buf, CANDIDATE_DTYPE, n.value).copy()
        finally:
            self._L.sift3d_free(out)

    def extract(self, initial_image_scale=1.0, desc_mode=DESC_SIFT, eig_thres=140.0, size_factor=1.0, copy=True):
        """Full extraction -> structured array of records.  copy=False returns a view of the context's
        pinned download buffer, valid until the next call on this context."""
        out, n = C.c_void_p(), C.c_int64(0)
        self._chk(self._L.sift3d_extract_view(self._h, float(initial_image_scale), int(desc_mode), float(eig_thres),
                                              float(size_factor), C.byref(out), C.byref(n)), "sift3d_extract_view")
        if n.value == 0:
            return np.zeros(0, FEATURE_DTYPE)
        buf = (C.c_char * (n.value * FEATURE_DTYPE.itemsize)).from_address(out.value)
        a = np.frombuffer(buf, FEATURE_DTYPE, n.value)
        return a.copy() if copy else a

    # ---- device-pointer forms (bench) ----
    def gauss_blur_dog_dev(self, d_in, d_out, d_dog, nx, ny, nz, sigma, min_value=0.01):
        self._chk(self._L.sift3d_gauss_blur_dog_dev(self._h, C.c_void_p(int(d_in)), C.c_void_p(int(d_out)) if d_out else None,
                                                    C.c_void_p(int(d_dog)) if d_dog else None, nx, ny, nz, float(sigma),
                                                    float(min_value)), "sift3d_gauss_blur_dog_dev")

    def gauss_blur_dog_half_dev(self, d_in, d_out, d_dog, d_half, nx, ny, nz, sigma, min_value=0.01):
        """sift3d_gauss_blur_dog_half_dev: level, DoG and the half-size volume; returns True when one launch made all three."""
        one = C.c_int(0)
        self._chk(self._L.sift3d_gauss_blur_dog_half_dev(self._h, C.c_void_p(int(d_in)), C.c_void_p(int(d_out)),
                                                         C.c_void_p(int(d_dog)) if d_dog else None, C.c_void_p(int(d_half)), nx, ny, nz,
                                                         float(sigma), float(min_value), C.byref(one)), "sift3d_gauss_blur_dog_half_dev")
        return bool(one.value)

    def gauss_blur_dev(self, d_in, d_out, nx, ny, nz, sigma, min_value=0.01):
        self._chk(self._L.sift3d_gauss_blur_dev(self._h, C.c_void_p(int(d_in)), C.c_void_p(int(d_out)), nx, ny, nz,
                                                float(sigma), float(min_value)), "sift3d_gauss_blur_dev")

    def blur_window_supported(self, nx, ny, sigma, min_value=0.01):
        return bool(self._L.sift3d_blur_window_supported(nx, ny, float(sigma), float(min_value)))

    def gauss_blur_dog_window_dev(self, d_in, d_out, d_dog, nx, ny, nz, z_lo, z_hi, sigma, min_value=0.01):
        """sift3d_gauss_blur_dog_window_dev: only the output planes [z_lo, z_hi) are produced."""
        self._chk(self._L.sift3d_gauss_blur_dog_window_dev(self._h, C.c_void_p(int(d_in)), C.c_void_p(int(d_out)) if d_out else None,
                                                           C.c_void_p(int(d_dog)) if d_dog else None, nx, ny, nz, int(z_lo), int(z_hi),
                                                           float(sigma), float(min_value)), "sift3d_gauss_blur_dog_window_dev")

    def dog_dev(self, d_a, d_b, d_out, n):
        self._chk(self._L.sift3d_dog_dev(self._h, C.c_void_p(int(d_a)), C.c_void_p(int(d_b)), C.c_void_p(int(d_out)), n),
                  "sift3d_dog_dev")

    def resample_affine_dev(self, d_src, src_shape, d_dst, out_shape, map, interp="linear", fill=0.0):
        """sift3d_resample_affine_dev on device buffers; shapes as (nz, ny, nx)."""
        nz, ny, nx = (int(d) for d in src_shape)
        oz, oy, ox = (int(d) for d in out_shape)
        m = _map12(map)
        self._chk(self._L.sift3d_resample_affine_dev(self._h, C.c_void_p(int(d_src)), nx, ny, nz, C.c_void_p(int(d_dst)), ox, oy, oz,
                                                     m.ctypes.data, INTERP[interp], float(fill)), "sift3d_resample_affine_dev")

    def subsample2_dev(self, d_in, nx, ny, nz, d_out):
        self._chk(self._L.sift3d_subsample2_dev(self._h, C.c_void_p(int(d_in)), nx, ny, nz, C.c_void_p(int(d_out))),
                  "sift3d_subsample2_dev")

    # ---- Z-slab building blocks ----
    def candidates_reset(self):
        self._chk(self._L.sift3d_candidates_reset(self._h), "sift3d_candidates_reset")

    def extrema_append_dev(self, d_prev, d_cur, d_next, nx, ny, nz_local, level_id, z_lo, z_hi):
        self._chk(self._L.sift3d_extrema_append_dev(self._h, C.c_void_p(int(d_prev)), C.c_void_p(int(d_cur)),
                                                    C.c_void_p(int(d_next)), nx, ny, nz_local, int(level_id), int(z_lo),
                                                    int(z_hi)), "sift3d_extrema_append_dev")

    def lazy_levels_supported(self, nx, ny, nz_local, next_sigma):
        return bool(self._L.sift3d_lazy_levels_supported(nx, ny, nz_local, float(next_sigma)))

    def extrema_append_lazy_dev(self, d_prev, g_prev_a, g_prev_b, d_cur, d_next, g_next, next_sigma, nx, ny, nz_local, level_id,
                                z_lo, z_hi):
        """Like extrema_append_dev with a neighbour level given as Gaussian levels instead of a stored DoG volume (0 = not
        given): the level below as g_prev_a - g_prev_b, the level above as g_next - blur(g_next, next_sigma)."""
        vp = lambda v: C.c_void_p(int(v)) if v else None
        self._chk(self._L.sift3d_extrema_append_lazy_dev(self._h, vp(d_prev), vp(g_prev_a), vp(g_prev_b), vp(d_cur), vp(d_next),
                                                         vp(g_next), float(next_sigma), nx, ny, nz_local, int(level_id), int(z_lo),
                                                         int(z_hi)), "sift3d_extrema_append_lazy_dev")

    @staticmethod
    def _level_array(levels):
        arr = (LevelDesc * len(levels))()
        for i, lv in enumerate(levels):
            arr[i] = LevelDesc(int(lv["img"]), int(lv["dogc"]), lv["nx"], lv["ny"], lv["nz_local"], lv["nz_global"],
                               lv["z_offset"], lv["sigma_h"], lv["sigma_c"], lv["sigma_l"], lv["octave_factor"])
        return arr

    def candidates_dev(self, levels):
        arr = self._level_array(levels)
        out, n = C.c_void_p(), C.c_int64(0)
        self._chk(self._L.sift3d_candidates_dev(self._h, arr, len(levels), C.byref(out), C.byref(n)), "sift3d_candidates_dev")
        try:
            buf = (C.c_char * (n.value * CANDIDATE_DTYPE.itemsize)).from_address(out.value) if n.value else b""
            return np.frombuffer(buf, CANDIDATE_DTYPE, n.value).copy()
        finally:
            self._L.sift3d_free(out)

    def describe_dev(self, levels, desc_mode=DESC_SIFT, eig_thres=140.0, size_factor=1.0, copy=True):
        """Returns (records, group); group = level_id*2 + is_max per record.  copy=False returns views of the
        context's pinned download buffers, valid until the next call on this context."""
        arr = self._level_array(levels)
        view, grp, n = C.c_void_p(), C.c_void_p(), C.c_int64(0)
        self._chk(self._L.sift3d_describe_dev(self._h, arr, len(levels), int(desc_mode), float(eig_thres), float(size_factor),
                                              C.byref(view), C.byref(grp), C.byref(n)), "sift3d_describe_dev")
        if n.value == 0:
            return np.zeros(0, FEATURE_DTYPE), np.zeros(0, np.int32)
        rb = (C.c_char * (n.value * FEATURE_DTYPE.itemsize)).from_address(view.value)
        gb = (C.c_char * (n.value * 4)).from_address(grp.value)
        recs, grp = np.frombuffer(rb, FEATURE_DTYPE, n.value), np.frombuffer(gb, np.int32, n.value)
        return (recs.copy(), grp.copy()) if copy else (recs, grp)

    def describe_dev_counts(self, levels, desc_mode=DESC_SIFT, eig_thres=140.0, size_factor=1.0):
        """First half of describe_dev for a caller that places several contexts' records in one list (include/sift3d.h): this
        context's records per group (GROUPS int32, a copy) and their sum.  describe_dev_place must follow."""
        arr = self._level_array(levels)
        cnt, n = C.c_void_p(), C.c_int64(0)
        self._chk(self._L.sift3d_describe_dev_counts(self._h, arr, len(levels), int(desc_mode), float(eig_thres), float(size_factor),
                                                     C.byref(cnt), C.byref(n)), "sift3d_describe_dev_counts")
        return np.frombuffer((C.c_char * (GROUPS * 4)).from_address(cnt.value), np.int32, GROUPS).copy(), n.value

    def describe_dev_place(self, list_address, shift):
        """Second half: the descriptor kernel stores record i of group g at list[i + shift[g]] (list_address: registered host memory,
        host_register).  Returns this context's record count -- or, with list_address None (the list turned out too small), what
        describe_dev(copy=False) returns: views of the context's own buffers."""
        n, own, grp = C.c_int64(0), C.c_void_p(), C.c_void_p()
        sh = np.ascontiguousarray(shift, np.int32) if shift is not None else None
        self._chk(self._L.sift3d_describe_dev_place(self._h, C.c_void_p(int(list_address)) if list_address else None,
                                                    sh.ctypes.data_as(C.c_void_p) if sh is not None else None, C.byref(own), C.byref(grp),
                                                    C.byref(n)), "sift3d_describe_dev_place")
        if list_address:
            return n.value
        if n.value == 0:
            return np.zeros(0, FEATURE_DTYPE), np.zeros(0, np.int32)
        rb = (C.c_char * (n.value * FEATURE_DTYPE.itemsize)).from_address(own.value)
        gb = (C.c_char * (n.value * 4)).from_address(grp.value)
        return np.frombuffer(rb, FEATURE_DTYPE, n.value), np.frombuffer(gb, np.int32, n.value)

    def set_max_octaves(self, n):
        """0 = the reference's stop rule (default); n > 0 = at most n octaves."""
        self._chk(self._L.sift3d_set_max_octaves(self._h, int(n)), "sift3d_set_max_octaves")

    def sync(self):
        self._chk(self._L.sift3d_sync(self._h), "sift3d_sync")

    def set_stream(self, hip_stream):
        self._chk(self._L.sift3d_set_stream(self._h, C.c_void_p(int(hip_stream)) if hip_stream else None), "sift3d_set_stream")

    def enable_timing(self, on=True):
        """False / 0 off, True / 1 every launch, 2 only the blur launches on the full-size volume, 3 every launch with the
        extrema kept on the main stream (each launch timed alone)."""
        self._chk(self._L.sift3d_enable_timing(self._h, int(on)), "sift3d_enable_timing")

    def launch_log(self):
        """Per-launch records (stage, ntaps, nvox, alg_bytes, ms) of the last pipeline/blur call."""
        n = C.c_int64(0)
        self._L.sift3d_get_launch_log(self._h, None, 0, C.byref(n))
        out = np.zeros(max(1, n.value), LAUNCH_DTYPE)
        self._chk(self._L.sift3d_get_launch_log(self._h, out.ctypes.data, len(out), C.byref(n)), "sift3d_get_launch_log")
        return out[:n.value]

    def timings(self):
        t = _Timings()
        self._chk(self._L.sift3d_get_timings(self._h, C.byref(t)), "sift3d_get_timings")
        d = {"total_ms": t.total_ms, "n_octaves": t.n_octaves, "n_extrema": t.n_extrema,
             "n_keypoints": t.n_keypoints, "n_records": t.n_records, "stages": {}}
        for i, s in enumerate(STAGES):
            d["stages"][s] = {"ms": t.ms[i], "launches": t.launches[i], "alg_bytes": t.alg_bytes[i]}
        return d
