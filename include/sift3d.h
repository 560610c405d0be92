/*
 * sift3d.h -- C-ABI of the MI355X-native 3D SIFT extraction path.
 *
 * Drop-in boundary for the accelerator back-end of CarluerJB/3D_SIFT_CUDA's
 * featExtract.  Plain C types only.  Each entry point names the reference
 * interface it replaces; R/ stands for
 * /root/reference/3dsift_cleanup-softVote_App_Weight_SoftMax/.
 *
 * Conventions (differences from the reference are deliberate and listed in
 * INTEGRATION.md): every function returns SIFT3D_OK (0) or a negative
 * sift3d_status instead of calling exit() like gpuErrchk
 * (R/cuda_common/SIFT_cuda_Tools.cuh:13-21); sizes are int64_t; volumes are
 * dense float32, x fastest, index (z*ny + y)*nx + x (FEATUREIO,
 * R/src_common/FeatureIO.h:21-33); the caller owns every buffer it passes
 * in; arrays the library returns are released with sift3d_free().
 * Results are those of the reference's CPU path (-d omitted): pass order
 * x,y,z, zero borders, separate multiply/add in ascending tap order.
 *
 * There is no CPU fallback: without a usable HIP device sift3d_create()
 * returns NULL and sift3d_device_count() returns 0.
 *
 * THE CALLS THAT MATTER to a maintainer of the reference (everything else in
 * this header serves tests, measurements, several GPUs, or the matcher):
 *   lifecycle     sift3d_device_count, sift3d_create, sift3d_destroy,
 *                 sift3d_last_error, sift3d_free
 *   the four accelerator wrappers of R/cuda_common/SIFT_cuda_Tools.cuh
 *                 sift3d_gauss_blur   <- blur_3d_simpleborders_CUDA_Row_Col_Shared_mem
 *                 sift3d_dog          <- fioCudaMultSum
 *                 sift3d_subsample2   <- SubSampleInterpolateCuda
 *                 sift3d_extrema      <- detectExtrema4D_test_cuda
 *   the pipeline  sift3d_set_volume (or _resized for -2+ / -2-), sift3d_extract
 *                 <- msGeneratePyramidDOG3D_efficient + the descriptor loop
 *   output        sift3d_write_key (csrc/keyfile.h, libsift3d_host.so) <- msFeature3DVectorOutputText
 * INTEGRATION.md shows the reference-side edit for each.  Section index:
 * operator level; pipeline level; tuning; timing; Z-slab building blocks and
 * sift3d_extract_zslab (several GPUs, beyond the reference); host helpers
 * (.key, NIfTI, world coordinates); matcher; guided re-matching (featMatchMultiple -a -e); resampling (featResample).
 * Development hooks and the one hardware self-test are in sift3d_dev.h, not here.
 */
#ifndef SIFT3D_H
#define SIFT3D_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Layout version of the structures this header passes by pointer (sift3d_zslab_stats, sift3d_timings, sift3d_feature, ...).
 * The library writes WHOLE structures through the caller's pointers, so a binding compiled against another layout would be
 * overrun: a binding checks sift3d_abi_version() == SIFT3D_ABI_VERSION once, when it loads the library (the in-tree ctypes
 * mirror and featExtract do).  7: sift3d_fuse_params gained label_interp, sift3d_interp gained SIFT3D_INTERP_LABEL; 6: the tuning enum gained SIFT3D_TUNE_FUSED_STAGGER, sift3d_set_libm_variant (round 6); 5: sift3d_zslab_stats gained comm_sets, resident_volume, merge_ms, halo_bytes_subsample, enqueue_ms (round 5); 4: transport,
 * transport_fell_back, rccl_version (round 4). */
#define SIFT3D_ABI_VERSION 7
int sift3d_abi_version(void);

#define SIFT3D_DESC_LEN 64
#define SIFT3D_INFO_MIN0MAX1 0x00000010u /* R/src_common/MultiScale.h:28 */
#define SIFT3D_INFO_REORIENT 0x00000020u /* R/src_common/MultiScale.h:30 */

typedef enum {
    SIFT3D_OK = 0,
    SIFT3D_ERR_ARG = -1,      /* bad argument / shape */
    SIFT3D_ERR_DEVICE = -2,   /* HIP runtime error (sift3d_last_error has the text) */
    SIFT3D_ERR_MEMORY = -3,   /* host or device allocation failed */
    SIFT3D_ERR_CAPACITY = -4, /* caller-provided output array too small (counts are still exact) */
    SIFT3D_ERR_COMM = -5      /* a halo copy between slabs (sift3d_extract_zslab) failed */
} sift3d_status;

/* Descriptor selected by -b / -br / -bn (/root/reference/README.md:26-34;
 * alternatives at R/src_common/MultiScale.cpp:1037-1045). */
typedef enum { SIFT3D_DESC_SIFT = 0, SIFT3D_DESC_BRIEF = 1, SIFT3D_DESC_RRIEF = 2, SIFT3D_DESC_NRRIEF = 3 } sift3d_desc_mode;

/* LOCATION_VALUE_XYZ, R/src_common/LocationValue.h:41-47 */
typedef struct {
    int32_t x, y, z;
    float value;
} sift3d_extremum;

/* What msFeature3DVectorOutputText prints per record
 * (R/src_common/MultiScale.h:386-474): Feature3DInfo without the patch. */
typedef struct {
    float x, y, z, scale;
    float ori[9];
    float eigs[3];
    uint32_t info;
    float desc[SIFT3D_DESC_LEN];
} sift3d_feature;

/* One validated scale-space extremum before the per-keypoint stage. */
typedef struct {
    int32_t octave, level; /* level 1..3: DoG index inside the octave */
    int32_t is_max;
    int32_t x, y, z;
    float value, h_value, l_value; /* DoG at the extremum, one level below, one above */
} sift3d_candidate;

typedef struct sift3d_ctx sift3d_ctx;

/* ---- devices and contexts --------------------------------------------------
 * get_num_device()/check_best_device(), R/featExtract/featExtract.cpp:238-270;
 * the device-buffer life cycle buried in fioAllocate/fioDelete/fioCopy
 * (R/src_common/FeatureIO.cpp:384-387,527-530,1857-1860). */
int sift3d_device_count(void);
/* Allocates the device-resident pyramid for volumes of up to nx*ny*nz voxels on
 * HIP device `device` (0-based, as cudaSetDevice receives it in the reference).
 * NULL on failure. */
sift3d_ctx *sift3d_create(int device, int64_t nx, int64_t ny, int64_t nz);
/* A context for the Z-slab building blocks below only: the caller owns every level buffer, so none is allocated here
 * (a twelfth of the memory of sift3d_create).  nz_local: the most slices of an nx * ny volume any one call will be handed
 * (slab + halos).  The *_dev operators, sift3d_candidates_reset / _extrema_append*_dev / _candidates_dev / _describe_dev
 * work; entry points that use the context's own pyramid (host-pointer operators, sift3d_set_volume*, sift3d_detect,
 * sift3d_extract*) return SIFT3D_ERR_ARG. */
sift3d_ctx *sift3d_create_slab(int device, int64_t nx, int64_t ny, int64_t nz_local);
void sift3d_destroy(sift3d_ctx *ctx);
const char *sift3d_last_error(const sift3d_ctx *ctx);
/* Optional: run on a caller-owned hipStream_t (e.g. one of torch's); NULL = the
 * context's own stream.  Ordering of device buffers handed to the *_dev entry
 * points: while the context runs on its own stream, every *_dev call is fenced
 * against the legacy default stream in both directions with events (it waits for
 * what the default stream has queued, and the default stream waits for what the
 * call queued), so a caller that works on the default stream -- as the reference
 * does, and as torch does unless told otherwise -- needs no synchronisation of
 * its own.  A caller that produces or consumes on another stream passes that
 * stream here; the context then runs on it and the fences are skipped. */
int sift3d_set_stream(sift3d_ctx *ctx, void *hip_stream);
int sift3d_sync(sift3d_ctx *ctx);
void sift3d_free(void *p);

/* ---- Gaussian taps (host) ---------------------------------------------------
 * calculate_gaussian_filter_size + generate_gaussian_filter1d
 * (R/src_common/GaussianMask.cpp:12-57,241-265) and the normalisation of
 * gb3d_blur3d_interleave (R/src_common/GaussBlur3D.cpp:1190-1201).
 * Returns the (odd) tap count, or a negative status; taps must hold 129 floats. */
int sift3d_gauss_taps(float sigma, float min_value, float *taps);
/* Which build of the reference the taps follow.  GaussianMask.cpp calls exp() on a float.  A current g++ (libstdc++ >= 6:
 * <math.h> brings the C++ overloads) makes that expf() and forms the tap's product with the scale in float -- the reference
 * as it compiles today, the default here and what the oracle follows.  The toolchain of the CPU binary the reference
 * repository ships (R/bin/Linux/featExtract, GCC 5.4) made it the C exp(double), with the product formed in double and
 * rounded once (its disassembly at 0x451c87, 0x451d0e, 0x4523b7-0x4523ca).  The two differ by one or two units in the last
 * place of a tap, which every later stage carries into the last printed digits of a record.  With SIFT3D_LIBM_GCC5 the
 * extraction reproduces that binary's .key files byte for byte (tests/test_gpu_parity.py::
 * test_cli_reproduces_the_shipped_binary).  Process-wide (sift3d_gauss_taps takes no context); contexts keep the taps of
 * their patch filters from creation, so choose before sift3d_create.  Returns the previous setting, or SIFT3D_ERR_ARG. */
#define SIFT3D_LIBM_CURRENT 0
#define SIFT3D_LIBM_GCC5 1
int sift3d_set_libm_variant(int which);
int sift3d_get_libm_variant(void);

/* ---- operator level: the reference's four accelerator entry points ---------
 * Host-pointer forms copy in, run on the device and copy the result back
 * (what every reference wrapper does); *_dev forms take device pointers and
 * stay asynchronous on the context's stream. */

/* gb3d_blur3d -> blur_3d_simpleborders_CUDA_Row_Col_Shared_mem
 * (R/cuda_common/SIFT_cuda_Tools.cuh:69-76, called from
 * R/src_common/GaussBlur3D.cpp:1240-1245); the input is NOT clobbered. */
int sift3d_gauss_blur(sift3d_ctx *ctx, const float *in, float *out, int64_t nx, int64_t ny, int64_t nz, float sigma,
                      float min_value);
int sift3d_gauss_blur_dev(sift3d_ctx *ctx, const float *d_in, float *d_out, int64_t nx, int64_t ny, int64_t nz,
                          float sigma, float min_value);
/* Fused form used by the pyramid: out = blur(in), dog = in - out.  d_out may be NULL when only the DoG is wanted
 * (the pyramid does that for its sixth level); d_dog may be NULL. */
int sift3d_gauss_blur_dog_dev(sift3d_ctx *ctx, const float *d_in, float *d_out, float *d_dog, int64_t nx, int64_t ny,
                              int64_t nz, float sigma, float min_value);
/* The same plus what the next octave starts from: d_half = the 2 x 2 x 2 mean of the blurred volume, a dense
 * (nx / 2) x (ny / 2) x (nz / 2) array (fioSubSampleInterpolate, R/src_common/FeatureIO.cpp:1474-1554, called on level 3 of
 * every octave at R/src_common/MultiScale.cpp:409-413).  Where the shape allows (an 11-tap filter -- the pyramid's level 3 --
 * on at least 2^22 voxels, nx a multiple of 8) the blur launch writes it from the planes it holds in registers and
 * *in_one_launch (optional) is 1; otherwise a subsample launch follows and it is 0.  The bytes are the same either way. */
int sift3d_gauss_blur_dog_half_dev(sift3d_ctx *ctx, const float *d_in, float *d_out, float *d_dog, float *d_half, int64_t nx,
                                   int64_t ny, int64_t nz, float sigma, float min_value, int *in_one_launch);
/* The same restricted to the output planes [z_lo, z_hi) of the volume: planes outside the window are not written, the
 * input is read as far as the filter reaches (zeros beyond the volume).  A Z-slab rank filters its two boundary bands
 * with it first, hands them to the halo exchange, and filters the interior while they travel.
 * Only the one-launch form of the blur has a window: sift3d_blur_window_supported says whether this row length and
 * filter take it (rows of whole 16-byte vectors, a plane below 2^29 voxels, at most 17 taps). */
int sift3d_blur_window_supported(int64_t nx, int64_t ny, float sigma, float min_value);
int sift3d_gauss_blur_dog_window_dev(sift3d_ctx *ctx, const float *d_in, float *d_out, float *d_dog, int64_t nx, int64_t ny,
                                     int64_t nz, int64_t z_lo, int64_t z_hi, float sigma, float min_value);
/* fioMultSum_interleave(a, b, out, -1.0f) -> fioCudaMultSum
 * (SIFT_cuda_Tools.cuh:213-217, R/src_common/FeatureIO.cpp:1941-1943) */
int sift3d_dog(sift3d_ctx *ctx, const float *a, const float *b, float *out, int64_t n);
int sift3d_dog_dev(sift3d_ctx *ctx, const float *d_a, const float *d_b, float *d_out, int64_t n);
/* Subsample_interleave -> SubSampleInterpolateCuda (SIFT_cuda_Tools.cuh:202-205,
 * R/src_common/FeatureIO.cpp:1556-1564): out is (nx/2)*(ny/2)*(nz/2). */
int sift3d_subsample2(sift3d_ctx *ctx, const float *in, int64_t nx, int64_t ny, int64_t nz, float *out);
int sift3d_subsample2_dev(sift3d_ctx *ctx, const float *d_in, int64_t nx, int64_t ny, int64_t nz, float *d_out);
/* detectExtrema4D_test_interleave -> detectExtrema4D_test_cuda
 * (SIFT_cuda_Tools.cuh:32-38, R/src_common/MultiScale.cpp:1523-1546): strict
 * extrema of d_cur over its 26 neighbours and centre+26 of d_prev; when d_next
 * is not NULL also centre+26 of d_next (the reference's later validation,
 * MultiScale.cpp:425-453).  Lists come back in raster z,y,x order, minima and
 * maxima separately, as the CPU scan produces them.  *n_min / *n_max always
 * receive the exact counts. */
int sift3d_extrema(sift3d_ctx *ctx, const float *d_prev, const float *d_cur, const float *d_next, int64_t nx, int64_t ny,
                   int64_t nz, sift3d_extremum *minima, int64_t cap_min, int64_t *n_min, sift3d_extremum *maxima,
                   int64_t cap_max, int64_t *n_max);
/* fioDoubleSize (R/src_common/FeatureIO.cpp:2452-2548), out is 2nx*2ny*2nz; and
 * fioSubSample2DCenterPixel (:1670-1714), out is (nx/2)*(ny/2)*(nz/2): the -2+ / -2- options. */
int sift3d_double_size(sift3d_ctx *ctx, const float *in, int64_t nx, int64_t ny, int64_t nz, float *out);
int sift3d_halve_size(sift3d_ctx *ctx, const float *in, int64_t nx, int64_t ny, int64_t nz, float *out);

/* ---- pipeline level: msGeneratePyramidDOG3D_efficient + the descriptor loop --
 * (R/src_common/MultiScale.cpp:236-570, R/featExtract/featExtract.cpp:409,474-505).
 * Everything stays on the device between the upload of the volume and the
 * download of the records. */
/* Input semantics: any float32 values.  NaN compares false as in the reference (a NaN neighbour refutes an extremum), and
 * +-inf and magnitudes near FLT_MAX follow IEEE arithmetic through the pyramid.  Every sift3d_set_volume* scans the volume once:
 * one that holds a NaN, an infinity or |v| > FLT_MAX / 4 takes the element-wise first extrema pass; the
 * records of volumes with infinities or overflowing values are not defined by the reference past the candidates. */
int sift3d_set_volume(sift3d_ctx *ctx, const float *vol, int64_t nx, int64_t ny, int64_t nz);
int sift3d_set_volume_dev(sift3d_ctx *ctx, const float *d_vol, int64_t nx, int64_t ny, int64_t nz);
/* The -2+ / -2- options without a round trip through the host (R/featExtract/featExtract.cpp:409-421 calls
 * fioDoubleSize / fioSubSample2DCenterPixel on the host image): upload vol (nx*ny*nz), resize it on the device
 * (resize = +1: doubled to 2nx*2ny*2nz, -1: halved to (nx/2)*(ny/2)*(nz/2), 0: as it is) and make the result the
 * context's volume.  The context must have been created for the larger of the two sizes. */
int sift3d_set_volume_resized(sift3d_ctx *ctx, const float *vol, int64_t nx, int64_t ny, int64_t nz, int resize);
/* The same volume arriving in runs of whole z planes (round 5; the reference reads the whole file and then copies the whole
 * volume, blocking, once per octave: fioCopy, R/src_common/FeatureIO.cpp:1841-1863): sift3d_set_volume_begin names the shape
 * that will arrive and the resize; sift3d_set_volume_planes queues planes [z0, z0 + n) (host memory, nx*ny*n floats) on the
 * context's stream and returns -- every plane exactly once, in any order; the caller keeps a run of planes unchanged until
 * sift3d_set_volume_end, which runs the resize if one was asked for and returns when the volume is resident.  featExtract
 * uploads what it has read while the rest of a .nii.gz is still being inflated. */
int sift3d_set_volume_begin(sift3d_ctx *ctx, int64_t nx, int64_t ny, int64_t nz, int resize);
int sift3d_set_volume_planes(sift3d_ctx *ctx, const float *planes, int64_t z0, int64_t n);
int sift3d_set_volume_end(sift3d_ctx *ctx);
/* Optional: make room now for a run that will find about n_extrema validated extrema (the per-keypoint buffers and the
 * pinned record buffers are otherwise made inside the first extraction, once their size is known: about 25 ms of a 512^3
 * extraction that a process which extracts once -- the command line -- can spend beside its file read instead).  Blob fields
 * yield one extremum per 3 000 voxels.  A run that finds more grows the buffers as before; results never depend on it. */
int sift3d_reserve(sift3d_ctx *ctx, int64_t n_extrema);
/* Scale-space + detection only: validated extrema of every octave/level in the
 * reference's order.  *out is malloc'ed (sift3d_free). */
int sift3d_detect(sift3d_ctx *ctx, float initial_image_scale, sift3d_candidate **out, int64_t *n_out);
/* Full extraction.  initial_image_scale: 1, or 0.5 after -2+; size_factor: what
 * featExtract.cpp:423-427 applies to x,y,z,scale (0.5 for -2+, 2 for -2-);
 * eig_thres: 140 in featExtract.cpp:297.  *out is malloc'ed (sift3d_free). */
int sift3d_extract(sift3d_ctx *ctx, float initial_image_scale, int desc_mode, float eig_thres, float size_factor,
                   sift3d_feature **out, int64_t *n_out);
/* One z-slice of Gaussian level `level` (0..4) of octave `octave` as the last sift3d_detect / sift3d_extract left it, copied
 * to the host as a dense nx_o * ny_o array (out must hold the octave's plane; *nx_out / *ny_out, which may be NULL, receive
 * its size).  For the reference's debug output ./image.pgm: the middle slice of octave 0's first blurred level
 * (R/src_common/MultiScale.cpp:373-384), which the featExtract command line of this build writes as the reference does. */
int sift3d_get_level_slice(sift3d_ctx *ctx, int octave, int level, int64_t z, float *out, int64_t *nx_out, int64_t *ny_out);
/* The same for DoG level `level` (0..4; D_k = L_k - L_{k+1}) of the last sift3d_detect / sift3d_extract.  A level that run did
 * not store in full is refused with a message that says "not stored": D_0 and D_4 of an octave whose neighbour levels were
 * evaluated around the candidates only (SIFT3D_TUNE_LAZY_LEVELS), and every level while no run has followed the last
 * sift3d_set_volume.  For tests, which hold the resident pyramid to the oracle's level by level. */
int sift3d_get_dog_slice(sift3d_ctx *ctx, int octave, int level, int64_t z, float *out, int64_t *nx_out, int64_t *ny_out);
/* Beyond the reference: stop the pyramid after n octaves.  n = 0 restores the reference's only
 * rule -- halve until a dimension is <= 2 (R/src_common/MultiScale.cpp:337,359-360) -- which is also the default; the
 * command line has no such option and never sets it.  Records are ordered octave-major, so a limited run returns
 * exactly the leading records of the unlimited one. */
int sift3d_set_max_octaves(sift3d_ctx *ctx, int n);
/* Implementation choices a caller may override (tests exercise both sides of each; none is needed for normal use, and
 * none changes a result -- every combination returns the same bytes).  No environment variable is read anywhere in the
 * library. */
typedef enum {
    SIFT3D_TUNE_BLUR_FUSED = 0, /* one fused x+y+z+DoG launch per level: 1 where it pays (default), 0 never, 2 wherever the shape allows */
    SIFT3D_TUNE_FUSED_CHUNKS,   /* z chunks of the fused launch: 0 = cost model (default), n >= 1 forced */
    SIFT3D_TUNE_FUSED_ROWS,     /* rows per thread of the fused launch: 0 = by filter and size (default), 1 or 2 forced */
    SIFT3D_TUNE_LAZY_LEVELS,    /* 1 (default): D0, D4 and L5 of an octave are evaluated around the candidates only; 0: stored and
                                 * filtered in full, as the reference's schedule does (MultiScale.cpp:405-413) */
    SIFT3D_TUNE_TINY_OCTAVE,    /* 1 (default): an octave of at most 4096 voxels is built by one workgroup in one launch; 0: level by level */
    SIFT3D_TUNE_SAMPLER_CAP,    /* workgroups of a CU that may sample a patch at a time in the descriptor kernel: 4 (default); 0: no limit */
    SIFT3D_TUNE_KP_CHUNKS,      /* the per-keypoint stage in n chunks, the keypoint kernel of chunk i+1 on one stream beside the
                                 * descriptor kernel of chunk i on another: 0 (default) or 1 = one launch of each, one after the other
                                 * (the overlap does not pay), up to 16; any value but 0 also switches
                                 * SIFT3D_TUNE_SPLIT_TAIL's schedule off */
    SIFT3D_TUNE_BANDS_FIRST,    /* Z-slab drivers: 1 (default) a rank filters the two boundary bands of a level first and the interior
                                 * while they travel to its neighbours; 0: the level in one piece, then the exchange (round 2) */
    SIFT3D_TUNE_HOST_RECORDS,   /* records per candidate the pinned download buffers are first sized for: 5 (default; blob fields yield
                                 * 4.2), 1..12; a run that yields more grows them (sift3d_host_buffer_grows counts) */
    SIFT3D_TUNE_FUSED_TILE,     /* (x, y) tile of the fused launch's two-rows-per-thread mapping: 0 = by measurement (default), 1 = 64 x 32,
                                 * 2 = 128 x 16 */
    SIFT3D_TUNE_FUSED_SUB,      /* 1 (default): the launch that makes level 3 of an octave also writes the next octave's level 0 (the
                                 * 2 x 2 x 2 mean) where the shape allows; 0: a subsample launch of its own, as before round 4 */
    SIFT3D_TUNE_SPLIT_TAIL,     /* 1 (default): the extrema of octaves 0 and 1 are sorted and their keypoint kernel started while the coarser
                                 * octaves are still being built; 0: one sort and one keypoint launch behind the whole pyramid; 2 (tests): as 1 with room
                                 * for eight extrema of the coarser octaves only, so that the fall-back to the schedule of 0 runs */
    SIFT3D_TUNE_DESC_SEGMENT,   /* descriptor kernel: the record list is dealt to the XCDs in contiguous eighths of segments of 8 n records:
                                 * 32 (default: 256 records a segment, all XCDs in the same part of the list at a time); 0: eighths of the
                                 * whole list (rounds 2 - 3); 1: round-robin */
    SIFT3D_TUNE_FUSED_ORDER,    /* fused blur: which workgroup takes which tile.  Workgroup b of a launch goes to XCD b mod 8.  0: by measurement;
                                 * 1: XCD x walks the x-th eighth of the tiles in (x, y, chunk) order -- whole rows of tiles per XCD (rounds 1 - 4);
                                 * 2: workgroup b takes tile b; 3: column strips -- XCD x owns the tiles of column x mod tiles_x, so that a
                                 * tile's y neighbours share its L2 and an XCD always reads the same byte columns of every row */
    SIFT3D_TUNE_FUSED_STAGGER,  /* fused blur, two-rows-per-thread mapping, 7 - 13 taps: the second-dispatched half of a workgroup's wavefronts
                                 * runs half a step behind the first (z pass and stores of a plane at the start of the next step), each
                                 * (half, role) pair of wavefronts running its own straight-line copy of the march.  0: by measurement
                                 * (default: from 11 taps up); 1: off (the kernel of rounds 2 - 5); 2: on */
    SIFT3D_TUNE_DESC_ORDER,     /* descriptor kernel: which lane samples which patch voxel.  1 (default): in image order -- a counting sort by
                                 * the image row (z, y cell) a sample reads hands the four lanes of a quad samples of one row
                                 * (csrc/sample_order.h); 0: in patch order, fast patch axis closest to x */
    SIFT3D_TUNE_COUNT
} sift3d_tuning;
int sift3d_set_tuning(sift3d_ctx *ctx, int knob, int value);
/* how often a run on this context found its pinned record buffers too small and grew them (see SIFT3D_TUNE_HOST_RECORDS) */
int64_t sift3d_host_buffer_grows(const sift3d_ctx *ctx);

/* Same, without the final host copy: *view points at the context's pinned download buffer and stays
 * valid until the next call on this context (or sift3d_destroy).  Do not free it.  The memory is the caller's to read AND
 * to modify in place until then (featExtract applies the -w transform there); the next run overwrites it. */
int sift3d_extract_view(sift3d_ctx *ctx, float initial_image_scale, int desc_mode, float eig_thres, float size_factor,
                        const sift3d_feature **view, int64_t *n_out);

/* ---- Z-slab building blocks (multi-GPU) --------------------------------------
 * The reference has no multi-GPU code; this is the surface the Z-slab driver
 * (3d_sift_cuda_amd/zslab.py: one process per GPU, halo exchange with
 * torch.distributed = RCCL over xGMI) needs on top of the *_dev operators.
 * The caller owns the level buffers (device memory): each holds nz_local
 * slices of a level whose whole volume has nz_global slices, starting at
 * global slice z_offset (slab + halos).  Geometry is always computed in
 * whole-volume coordinates, so records are those of the undivided volume. */
typedef struct {
    const float *img;  /* Gaussian level L_k (device), nx*ny*nz_local */
    const float *dogc; /* DoG level k (device), same shape */
    int64_t nx, ny, nz_local, nz_global, z_offset;
    float sigma_h, sigma_c, sigma_l; /* sigmas of levels k-1, k, k+1 (MultiScale.cpp:463) */
    float octave_factor;             /* 2^octave (MultiScale.cpp:531-543) */
} sift3d_level_desc;
/* Forget the extrema collected so far (also restarts the launch log). */
int sift3d_candidates_reset(sift3d_ctx *ctx);
/* Queue one extrema pass over device buffers of nz_local slices and keep the
 * extrema whose local z lies in [z_lo, z_hi) (and in 1..nz_local-2): a slab
 * keeps its own slices, the halo slices are the neighbour's.  level_id =
 * octave*3 + (DoG level - 1) orders the output. Asynchronous. */
int sift3d_extrema_append_dev(sift3d_ctx *ctx, const float *d_prev, const float *d_cur, const float *d_next, int64_t nx,
                              int64_t ny, int64_t nz_local, int level_id, int64_t z_lo, int64_t z_hi);
/* The same pass when a neighbour level is not stored as a DoG volume -- what the single-device pipeline does for the
 * first and last detection level of an octave:
 *   d_prev == NULL: the level below is g_prev_a - g_prev_b, the two Gaussian levels it is the difference of, read at the
 *                   27 positions around an extremum (as the reference's validateDifferencePeak3D reads a level it never
 *                   materialises, R/src_common/MultiScale.cpp:1135-1223);
 *   d_next == NULL: the level above is g_next - blur(g_next, next_sigma), and that blur is evaluated only at the 27
 *                   positions around each extremum that passed everything else, from the (2R+3)^3 block of g_next around
 *                   it -- g_next must therefore be valid R+1 = 9 slices beyond the slices [z_lo, z_hi) (rows and planes
 *                   outside the buffer read as zero, i.e. as the border of the whole volume).
 * sift3d_lazy_levels_supported: 1 when this shape can take that form (rows of whole 16-byte vectors, a plane below
 * 2^29 voxels, the 17-tap filter of the pyramid's last level); otherwise store the levels and use sift3d_extrema_append_dev.
 * A pure function of its arguments. */
int sift3d_lazy_levels_supported(int64_t nx, int64_t ny, int64_t nz_local, float next_sigma);
int sift3d_extrema_append_lazy_dev(sift3d_ctx *ctx, const float *d_prev, const float *g_prev_a, const float *g_prev_b,
                                   const float *d_cur, const float *d_next, const float *g_next, float next_sigma, int64_t nx,
                                   int64_t ny, int64_t nz_local, int level_id, int64_t z_lo, int64_t z_hi);
/* Sort what was collected and return it with whole-volume coordinates (malloc'ed, sift3d_free). */
int sift3d_candidates_dev(sift3d_ctx *ctx, const sift3d_level_desc *levels, int n_levels, sift3d_candidate **out,
                          int64_t *n_out);
/* Sort what was collected and run the per-keypoint stage on it.  levels[id]
 * describes level_id == id.  *view / *group_view (level_id*2 + is_max per
 * record) point at pinned buffers owned by the context, valid until the next
 * call. */
int sift3d_describe_dev(sift3d_ctx *ctx, const sift3d_level_desc *levels, int n_levels, int desc_mode, float eig_thres,
                        float size_factor, const sift3d_feature **view, const int32_t **group_view, int64_t *n_out);

/* sift3d_describe_dev in two halves (round 5), for a caller that places the records of SEVERAL contexts -- the ranks of a Z-slab run,
 * one process each -- in ONE list, so that nothing is gathered or merged afterwards.  A context's records come out sorted by group
 * (level_id*2 + is_max; SIFT3D_GROUPS of them), and the single-device order is, group by group, one run per rank in rank order; so:
 *   sift3d_describe_dev_counts  sorts, runs the keypoint kernel and returns this context's records per group (*group_counts: SIFT3D_GROUPS
 *                               words owned by the context) and their sum;
 *   the caller                  exchanges the counts between the ranks and lays the runs out: shift[g] = (records of groups < g of all ranks)
 *                               + (records of group g of lower ranks) - (this rank's own records of groups < g);
 *   sift3d_describe_dev_place   runs the descriptor kernel, which stores this context's record i (of group g) at list[i + shift[g]], and
 *                               waits for it.  list: host memory the device can write -- e.g. a shared-memory segment that every rank's
 *                               process maps and has passed to sift3d_host_register; the per-record group words stay in the context
 *                               (*group_view).  list == NULL (it turned out too small): the records go to the context's own pinned
 *                               buffers, *own_view, exactly as after sift3d_describe_dev.
 * sift3d_host_register / _unregister: hipHostRegister (portable, mapped) / hipHostUnregister on the caller's pages. */
#define SIFT3D_GROUPS 193
int sift3d_describe_dev_counts(sift3d_ctx *ctx, const sift3d_level_desc *levels, int n_levels, int desc_mode, float eig_thres,
                               float size_factor, const int32_t **group_counts, int64_t *n_records);
int sift3d_describe_dev_place(sift3d_ctx *ctx, sift3d_feature *list, const int32_t *shift, const sift3d_feature **own_view,
                              const int32_t **group_view, int64_t *n_out);
int sift3d_host_register(void *p, int64_t bytes);
int sift3d_host_unregister(void *p);

/* ---- Z-slab extraction from C: one process, several devices ---------------------
 * The whole volume (host memory) is cut into one Z-slab per entry of `devices` (the same partitioning, halo widths and
 * exchange schedule as the per-process driver above), each slab on its own device, halos moved between the devices with
 * hipMemcpyPeerAsync -- xGMI between the GPUs of a node -- queued behind events, so the host never waits inside the pyramid
 * (one host thread per device queues its launches).
 * The records come back merged in the single-GPU order and are the single-GPU records bit for bit.  A device may be listed
 * more than once (the slab logic rehearsed on one GPU).  A volume too thin to shard (a slab must be 32 slices thick) runs
 * whole on devices[0].  SIFT3D_ERR_COMM: a halo copy or its ordering failed; *err (err_len bytes, may be NULL) gets the text.
 * *out is malloc'ed (sift3d_free). */
typedef struct {
    int32_t n_ranks, sharded_octaves; /* n_ranks: the slabs (the octaves below the sharded ones have a rank of their own on devices[0], not counted) */
    int64_t exchanges;            /* halo copies queued on the critical path + deferred batches */
    int64_t halo_bytes_critical;  /* the 8-slice halo every level needs before the next blur (9 of L4), all ranks */
    int64_t halo_bytes_deferred;  /* the rest of the L1..L3 patch halos, copied beside L4 / L5 / extrema */
    int64_t gather_bytes;         /* the first unsharded octave assembled on devices[0] */
    int64_t n_extrema, n_keypoints, n_records;
    double wall_ms;               /* host wall time of the extraction: upload of the slabs, pyramid, per-keypoint stage, download, merge */
    int64_t halo_bytes_hidden;    /* the part of halo_bytes_critical issued bands-first: copied while the receiver filters its interior */
    int32_t transport;            /* what moved the slices between ranks: SIFT3D_TRANSPORT_PEER_COPY or SIFT3D_TRANSPORT_RCCL */
    int32_t transport_fell_back;  /* 1: RCCL was asked for, but a device is listed more than once (not something RCCL ranks can
                                   * be): peer copies were used */
    int32_t rccl_version;         /* ncclGetVersion() of the library that was loaded (0 with peer copies) */
    int32_t comm_sets;            /* RCCL communicator sets in use: 2, or 1 with SIFT3D_ZSLAB_SERIAL_CHANNELS (0 with peer copies) */
    int32_t resident_volume;      /* 1: the input slices were on the devices already (sift3d_zslab_extract_resident): no upload in wall_ms */
    int32_t list_grown;           /* 1: the merged list had to be replaced by a larger one AFTER the slabs' records were in it (the coarse octaves'
                                   * records did not fit behind them): the slabs' part was copied over.  Rare; tests force it */
    double merge_ms;              /* host time spent on the merged order (part of wall_ms).  Round 5: the ranks' descriptor kernels store their
                                   * records straight into their places in ONE pinned list, so this is the per-group offset table and its
                                   * upload (microseconds) plus, when the list has to grow, its allocation -- there is no merge left */
    int64_t halo_bytes_subsample; /* the part of halo_bytes_deferred the next octave waits for: the eight slices of L3 beyond +- 8 that the
                                   * subsample reads (first deferred step); the rest is waited for before the per-keypoint stage only */
    double enqueue_ms;            /* host time from the start of the call until the last rank's pyramid, extrema passes and count request are
                                   * queued (before its first host wait).  One host thread per rank since the second half of round 5 */
} sift3d_zslab_stats;
/* How a block of slices travels from one rank's device to another's (sift3d_zslab_set_tuning(h, SIFT3D_ZSLAB_TRANSPORT, v),
 * sift3d_extract_zslab_over): peer copies -- hipMemcpyPeerAsync on the receiver's stream behind the sender's event, the
 * default -- or RCCL: ncclSend / ncclRecv on the ranks' halo streams inside one ncclGroupStart / ncclGroupEnd per exchange
 * step, one communicator set for the halos a launch waits for and one for the deferred patch halos.  RCCL is loaded at run
 * time (librccl.so.1; sift3d_zslab_set_transport_library names another build, NULL restores the default); a failure to load
 * it or to create the communicators is SIFT3D_ERR_COMM with the reason in err.  NEITHER transport has moved a byte between
 * two GPUs yet (one-GPU development box). */
#define SIFT3D_ZSLAB_TRANSPORT 1000
#define SIFT3D_TRANSPORT_PEER_COPY 0
#define SIFT3D_TRANSPORT_RCCL 1
/* sift3d_zslab_set_tuning(h, SIFT3D_ZSLAB_SERIAL_CHANNELS, 1): RCCL with ONE communicator set -- the deferred patch halos go
 * through the communicators of the per-level halos and queue behind them (RCCL orders a communicator's operations).  Slower
 * by design (the deferred slices in front of the next level's 8); it exists as the fallback to try in the same lease if two
 * communicators per device ever stall each other on real links.  Results are the same bytes. */
#define SIFT3D_ZSLAB_SERIAL_CHANNELS 1001
/* sift3d_zslab_set_tuning(h, SIFT3D_ZSLAB_DUPLICATE_RANKS, 1): a device listed more than once is handed to ncclCommInitAll as
 * it is instead of falling back to peer copies.  Real RCCL refuses such a list (SIFT3D_ERR_COMM); the rehearsal library of
 * tests/rccl_shim (given to sift3d_zslab_set_transport_library) accepts it, which is how the RCCL half of the exchange --
 * group pairing, stream order, the two communicator sets -- runs with 2 .. 8 ranks on a one-GPU box. */
#define SIFT3D_ZSLAB_DUPLICATE_RANKS 1002
/* sift3d_zslab_set_tuning(h, SIFT3D_ZSLAB_POISON_HALO, 1) (tests): every halo slice of L1..L3 that the exchange does NOT fetch is
 * filled with NaN before the per-keypoint stage -- a patch that reached further than the driver's bound would show in the records.
 * 1 + k: the NaN start k slices earlier, inside what was fetched (never inside what the pyramid itself reads): the smallest k that
 * changes a record is the margin the bound has on that volume. */
#define SIFT3D_ZSLAB_POISON_HALO 1003
/* sift3d_zslab_set_tuning(h, SIFT3D_ZSLAB_PATCH_WAIT, v): when a rank waits for the halo slices of L1..L3 that only patches read.
 * 0 (default): before its per-keypoint stage -- they have every later octave to arrive in; 1: at the end of their own octave, with
 * the subsample's slices (rounds 2 - 4).  Same bytes either way. */
#define SIFT3D_ZSLAB_PATCH_WAIT 1004
/* sift3d_zslab_set_tuning(h, SIFT3D_ZSLAB_LIST_ROOM, n) (tests): a newly allocated merged list has room for n records behind the slabs'
 * (the octaves that are not sharded append theirs there); -1 (default): an eighth of the slabs' records + 4096.  0 forces the growth
 * path whenever those octaves have a record.  The handle's list is dropped by the call. */
#define SIFT3D_ZSLAB_LIST_ROOM 1005
void sift3d_zslab_set_transport_library(const char *path);
int sift3d_extract_zslab(const int *devices, int n_devices, const float *vol, int64_t nx, int64_t ny, int64_t nz,
                         float initial_image_scale, int desc_mode, float eig_thres, float size_factor, sift3d_feature **out,
                         int64_t *n_out, sift3d_zslab_stats *stats, char *err, int64_t err_len);
/* sift3d_extract_zslab with the transport named (SIFT3D_TRANSPORT_*); sift3d_extract_zslab uses peer copies */
int sift3d_extract_zslab_over(int transport, const int *devices, int n_devices, const float *vol, int64_t nx, int64_t ny, int64_t nz,
                              float initial_image_scale, int desc_mode, float eig_thres, float size_factor, sift3d_feature **out,
                              int64_t *n_out, sift3d_zslab_stats *stats, char *err, int64_t err_len);
/* The same with the contexts, streams and events of the slabs kept between volumes of one shape: create once, extract any
 * number of volumes (the level buffers of a run come from one arena per slab, sized after the first run), destroy.
 * sift3d_extract_zslab is create + extract + destroy; creating the contexts dominates its wall time. */
typedef struct sift3d_zslab sift3d_zslab;
sift3d_zslab *sift3d_zslab_create(const int *devices, int n_devices, int64_t nx, int64_t ny, int64_t nz, char *err, int64_t err_len);
int sift3d_zslab_extract(sift3d_zslab *h, const float *vol, float initial_image_scale, int desc_mode, float eig_thres,
                         float size_factor, sift3d_feature **out, int64_t *n_out, sift3d_zslab_stats *stats, char *err,
                         int64_t err_len);
void sift3d_zslab_destroy(sift3d_zslab *h);
/* The resident form (round 5) -- what sift3d_set_volume + sift3d_extract_view are to one device: sift3d_zslab_set_volume
 * cuts the host volume into the ranks' input slices (slab +- 16) and uploads them once; sift3d_zslab_extract_resident then
 * runs any number of extractions from HBM.  *view is the handle's own host buffer with the merged records (single-GPU order,
 * single-GPU bytes), valid until the handle's next call; do not free it.  stats->wall_ms then holds no upload. */
/* (Both extraction forms: the ranks' records are placed in the merged order by the descriptor kernels themselves -- a rank's
 * records are sorted by (level, is_max) group already, so once every rank's records per group are known, a 193-word read-back
 * beside the record total each rank waits for anyway, a record's merged position is its own position plus a per-group shift.) */
int sift3d_zslab_set_volume(sift3d_zslab *h, const float *vol, char *err, int64_t err_len);
int sift3d_zslab_extract_resident(sift3d_zslab *h, float initial_image_scale, int desc_mode, float eig_thres, float size_factor,
                                  const sift3d_feature **view, int64_t *n_out, sift3d_zslab_stats *stats, char *err, int64_t err_len);
/* sift3d_set_tuning on every slab's context (and the driver's own use of SIFT3D_TUNE_LAZY_LEVELS) */
int sift3d_zslab_set_tuning(sift3d_zslab *h, int knob, int value);

/* ---- matcher: exact nearest neighbours of 64-component descriptors ------------------
 * The search step of featMatchMultiple (R/feat_common/featMatchUtilities.cpp:1612: flann_find_nearest_neighbors_index over
 * a kd-tree forest built at :1559 with 8 trees, 64 checks -- approximate and randomised; FLANN is not part of
 * /root/reference), done exactly on the matrix cores: squared Euclidean distances from an int8 Gram matrix.
 * db / queries: n x 64 components, each 0..127 (the rank descriptors of a .key file are 0..63).  For every query the k
 * (1..32) nearest database vectors, ascending by (distance, database index): idx and dist2 hold n_q x k entries (-1 /
 * INT32_MAX past the end of a database smaller than k).  A vector that is in both sets finds itself at distance 0, as in
 * the reference, whose vote stage drops the hits inside the query's own image.  repeats > 1 runs the search that many times
 * and reports the mean device time of the runs after the first in *kernel_ms (may be NULL); with repeats == 1 the figure
 * is the one run end to end on the device's clock, including the read-back that validates the bytes.  n_db and n_q at most
 * 2^31 - 4096 (32-bit row indices, the last tile padded). */
int sift3d_knn64(int device, const int8_t *db, int64_t n_db, const int8_t *queries, int64_t n_q, int k, int32_t *idx,
                 int32_t *dist2, int repeats, double *kernel_ms, char *err, int64_t err_len);

/* ---- matcher, alignment path: ratio matching and Hough similarity (featMatchMultiple -a) ------------------------------
 * matchAllToOne -> MatchKeys -> determine_similarity_transform_hough (R/featMatchMultiple/featMatchMultiple.cpp:148-390,
 * R/feat_common/featMatchUtilities.cpp:336-428, 816-1250) with the descriptor distance DistSqrPCs(.., 64) restored; the
 * deliberate differences are listed in DESIGN.md section 8.  The fixed image's records are the database, the moving
 * image's records the queries; the transform maps moving coordinates to fixed ones. */

/* msComputeNearestNeighborDistanceRatioInfo: for every query record the reference's in-order scan of ALL database records
 * (n_db >= 2), with compatible_features at its defaults between the candidate and the current best.  Per query: i1 / d1
 * the best database index and its squared distance, i2 / d2 the second; the reference's ratio is (float)d1 / (float)d2.
 * Descriptors as sift3d_match_descriptors takes them (whole numbers 0..127, else SIFT3D_ERR_ARG).  *kernel_ms (may be
 * NULL): device time of the search kernel. */
int sift3d_match_ratio(int device, const sift3d_feature *db, int64_t n_db, const sift3d_feature *q, int64_t n_q, int32_t *i1, int32_t *d1,
                       int32_t *i2, int32_t *d2, double *kernel_ms, char *err, int64_t err_len);

/* determine_similarity_transform_hough on M given correspondences (pfProb all ones): p0 / s0 / o0 the moving side (3, 1
 * and 9 floats per match, frames row-major), p1 / s1 / o1 the fixed side.  counts (M entries, may be NULL): inliers of each
 * one-match hypothesis, -1 where two of its three points coincide (skipped).  *winner: the first hypothesis with the most
 * inliers (at least one), or -1; rot / *scale its transform and flags (M entries, may be NULL) its inlier flags (zeros
 * when there is no winner).  The winner's transform is computed on the device and checked bit for bit against the host. */
int sift3d_hough_similarity(int device, const float *p0, const float *p1, const float *s0, const float *s1, const float *o0, const float *o1,
                            int32_t m, int32_t *counts, int32_t *winner, float *rot, float *scale, int32_t *flags, char *err,
                            int64_t err_len);

/* The result of MatchKeys for one moving image: x_fixed = scale * rot (x_moving - center0) + center1 = scale * rot x_moving
 * + trans.  The identity (scale 1, rot I, trans 0, center1 = center0) when there are fewer than 2 fixed records, no moving
 * record, at most 3 matches or no winning hypothesis.  inliers: the match count when there are at most 3 matches, else
 * the winner's inlier count (0 without a winner). */
typedef struct {
    float scale;
    float rot[9];      /* row-major */
    float trans[3];
    float center0[3];  /* bounding-box centre of the moving records (getMinMaxDim) */
    float center1[3];  /* center0 mapped by the winning hypothesis */
    int32_t n_matches; /* min(moving records, max_matches) when there are at least 2 fixed records, else 0 */
    int32_t inliers;
    int32_t winner;    /* index into the sorted matches, or -1 */
    int32_t capacity;  /* entries the caller's arrays below hold (0: they are not filled) */
    int32_t *moving_idx; /* per match, sorted by (ratio, moving index) ascending with NaN ratios last: */
    int32_t *fixed_idx;
    int32_t *inlier;   /* 1: inlier of the winner */
    int32_t *dist2;    /* squared descriptor distance of the match */
} sift3d_similarity;

/* MatchKeys (featMatchUtilities.cpp:1028-1250): ratio search, the matches sorted by ratio and cut at max_matches (the
 * reference's iMaxMatches is 3000), the Hough, the transform.  out->capacity and the four arrays are the caller's; the
 * arrays are filled when capacity >= n_matches (else SIFT3D_ERR_CAPACITY, with everything else filled in). */
int sift3d_match_keys(int device, const sift3d_feature *fixed, int64_t n_fixed, const sift3d_feature *moving, int64_t n_moving,
                      int32_t max_matches, sift3d_similarity *out, char *err, int64_t err_len);

/* Host helpers of this path (also in libsift3d_host.so; no GPU needed).
 * The closed float interval [lo, hi] of ratios r with fabsf(logf(r)) < (float)t, from this host's logf: compatible_features'
 * scale test as a comparison the device can make.  Returns 0, or -1 if logf is not monotonic within 2^16 floats of an end. */
int sift3d_log_ratio_interval(double t, float *lo, float *hi);
/* TransformSimilarity::Invert (R/feat_common/featMatchUtilities.h:213-226): the inverse transform in scale / rot / trans. */
void sift3d_similarity_invert(const sift3d_similarity *in, sift3d_similarity *out);
/* TransformSimilarity::WriteMatrix: the 4 x 4 text matrix of a .trans.txt file.  Returns 0 or -1. */
int sift3d_write_similarity(const char *path, const sift3d_similarity *t);
/* The three match files of matchAllToOne (featMatchMultiple.cpp:297-358) for one moving image: <base>.matches.info.txt,
 * .matches.img1.txt and .matches.img2.txt.  fixed_name / moving_name: the key file names as given (the headers name them
 * with the extension replaced by .hdr).  Every fixed record g gets the moving record of its last inlier (in match order);
 * t's arrays must hold its n_matches entries.  Returns 0 or -1. */
int sift3d_write_alignment_matches(const char *base, const char *fixed_name, const char *moving_name, const sift3d_feature *fixed,
                                   int64_t n_fixed, const sift3d_feature *moving, int64_t n_moving, const sift3d_similarity *t);

/* ---- guided re-matching: refine an alignment over many pairs (featMatchMultiple -a -e; beyond the reference) ----------
 * The reference names this step (MatchKeys' bExpand, matchAllToOne's bExpandedMatching: "try to find some additional
 * correspondences (inliers of inliers)") and always leaves it off.  DESIGN.md section 7d states the contract;
 * tests/refine_oracle.c restates the search.
 *
 * sift3d_guided_search: for every moving record m the best and second-best fixed records f, ordered by (squared descriptor
 * distance over the 64 rank components, fixed index), among those that pass, in float and in this order:
 *   - the line flags are equal (AM_INFO_LINE of the info words);
 *   - r = f.scale / (m.scale * t->scale) lies in the interval sift3d_log_ratio_interval(0.4054651) gives (NaN, 0 and
 *     infinite ratios fail);
 *   - with q = t->scale * t->rot (x_m - t->center0) + t->center1 (similarity_transform_3point's order), the squared distance
 *     ((dx * dx + dy * dy) + dz * dz) from f to q is below radius * radius (a NaN position fails).
 * i1 / d1, i2 / d2: n_moving entries each, -1 / INT32_MAX where there is no candidate.  visited (may be NULL): candidates
 * the spatial index made the query examine.  The index is a uniform grid of cell edge radius * (1 + 2^-10) over the
 * fixed records' finite bounding box, records with a non-finite position in no cell; it only skips records.  Descriptors
 * as sift3d_match_descriptors takes them.  *kernel_ms (may be NULL): device time of the search kernel. */
int sift3d_guided_search(int device, const sift3d_feature *fixed, int64_t n_fixed, const sift3d_feature *moving, int64_t n_moving,
                         const sift3d_similarity *t, float radius, int32_t *i1, int32_t *d1, int32_t *i2, int32_t *d2, int32_t *visited,
                         double *kernel_ms, char *err, int64_t err_len);

/* A least-squares similarity over n point pairs, p_moving -> p_fixed (3 floats each): Umeyama (1991) in double with
 * det R = +1, the 3 x 3 SVD by one-sided Jacobi sweeps, rounded to float once.  Fills out->scale, rot, trans and center1 =
 * the fit applied to out->center0 (the caller's), so am_sim_point and sift3d_similarity_matrix describe the same map;
 * nothing else of *out is touched.  Returns 0, or -1 for fewer than 3 pairs, a non-finite coordinate, or centred points of
 * rank < 2 (collinear). */
int sift3d_fit_similarity(const float *p_moving, const float *p_fixed, int64_t n, sift3d_similarity *out);

typedef struct {
    int32_t max_rounds;     /* 3 */
    float min_radius;       /* 1.0 key units */
    float max_radius;       /* 16.0 */
    int32_t ratio_num;      /* 4: accept when i2 == -1 or ratio_num * d2 > ratio_den * d1 (int64, squared distances) */
    int32_t ratio_den;      /* 5 */
    float stop_shift;       /* 0.01: stop when the moving box's eight corners move by less */
    int64_t index_cells_max; /* 2^26: dense cell-start table up to this many cells, sorted cell keys above */
} sift3d_refine_params;
void sift3d_refine_defaults(sift3d_refine_params *p);
/* sift3d_guided_search with the index form of p->index_cells_max (the only field it reads; NULL: defaults). */
int sift3d_guided_search_params(int device, const sift3d_feature *fixed, int64_t n_fixed, const sift3d_feature *moving, int64_t n_moving,
                                const sift3d_similarity *t, float radius, const sift3d_refine_params *p, int32_t *i1, int32_t *d1, int32_t *i2,
                                int32_t *d2, int32_t *visited, double *kernel_ms, char *err, int64_t err_len);

#define SIFT3D_REFINE_MAX_ROUNDS 16
typedef enum {
    SIFT3D_REFINE_STOP_ROUNDS = 0,    /* max_rounds rounds ran */
    SIFT3D_REFINE_STOP_CONVERGED = 1, /* the corners moved by less than stop_shift */
    SIFT3D_REFINE_STOP_FIT = 2,       /* a fit was refused (too few or collinear pairs): the previous transform is kept */
    SIFT3D_REFINE_STOP_NONE = 3       /* nothing to refine (no fixed or no moving record) */
} sift3d_refine_stop;
typedef struct {
    float radius;      /* the search radius of the round */
    int64_t visited;   /* candidates examined, summed over the queries */
    int32_t accepted;  /* pairs accepted by the ratio test, one per fixed record */
    int32_t kept;      /* pairs kept by the trim (0 when the round's fit was refused) */
    double rms;        /* RMS residual of the kept pairs under the round's transform */
    double shift;      /* largest move of the eight corners against the round before */
    double kernel_ms;  /* device time of the round's search kernel */
} sift3d_refine_round;
typedef struct {
    int32_t rounds;    /* rounds run (a refused round counts) */
    int32_t stop;      /* sift3d_refine_stop */
    sift3d_refine_round round[SIFT3D_REFINE_MAX_ROUNDS];
} sift3d_refine_report;

/* The refinement loop, every choice in double on the host: predict, search (the fixed set and its
 * index stay on the device across rounds), accept by the ratio test, keep one pair per fixed record (least (d1, moving
 * index)), fit, trim to residuals <= 3 x the lower median, refit.  init: sift3d_match_keys' result with its arrays (the
 * Hough inliers set round 0's radius, 3 x their RMS residual clamped to [min_radius, max_radius]).  p NULL: defaults.
 * out: scale / rot / trans / center0 / center1 of the refined map; its arrays (capacity n_moving) hold the kept pairs by
 * moving index with inlier = 1, n_matches = inliers = their count, winner = -1.  rep (may be NULL): per round. */
int sift3d_refine_similarity(int device, const sift3d_feature *fixed, int64_t n_fixed, const sift3d_feature *moving, int64_t n_moving,
                             const sift3d_similarity *init, const sift3d_refine_params *p, sift3d_similarity *out, sift3d_refine_report *rep,
                             char *err, int64_t err_len);

/* ---- resampling: the moving image on the fixed image's grid (featResample; beyond the reference) ----------------------
 * DESIGN.md section 7c states the arithmetic; tests/resample_oracle.c restates it.  Volumes are dense float32, x fastest.
 * map: 3 x 4 row-major, output voxel index (i, j, k) -> source voxel position
 *   q_r = ((map[4r] * i + map[4r + 1] * j) + map[4r + 2] * k) + map[4r + 3]  (i, j, k as floats, no fused multiply-add).
 * A sample is taken where 0 <= q <= n - 1 on every axis (a NaN position fails); every other output voxel gets fill.
 * Linear: trilinear over the eight corners, x then y then z, each step (1 - w) * a + w * b -- a NaN or infinite corner of
 * weight 0 still reaches the result.  Nearest: the voxel min(floorf(q + 0.5f), n - 1).  Source extents 1 .. 2^24, output
 * extents 1 .. 2^31 - 1 with at most 2^40 voxels; 64-bit indices throughout.
 * Label (label-aware linear, for label maps; DESIGN.md section 7n, restated by tests/label_interp_oracle.c): linear's f = floorf(q),
 * w = q - f, i0, i1 = min(i0 + 1, n - 1) and u = 1.0f - w.  Corner c = a + 2b + 4d (a, b, d in {0, 1} along x, y, z) has the value
 * L_c = src[(z_d ny + y_b) nx + x_a] and the weight W_c = (X_a * Y_b) * Z_d, X_0 = ux, X_1 = wx and likewise Y and Z (float
 * multiplies in that association).  Two corners are of one class when their values compare equal with == (-0 and 0 are one
 * class); all non-finite corners (NaN, +-inf) together are the unlabelled class.  A class' score is ((..((t_0 + t_1) + t_2) ..) +
 * t_7) in float, t_c = W_c for its corners and 0.0f for the others.  The largest score wins; at equal scores a labelled class
 * beats the unlabelled one, and among labelled classes the smaller value wins.  The result is the value of the winner's
 * lowest-numbered corner with its bits (-0 survives), a quiet NaN where the unlabelled class wins.  It follows that a corner of
 * weight 0 decides nothing (unlike linear, a NaN corner of weight 0 does not reach the result), that the identity map returns the
 * source's bits on every finite voxel, and that the result is always a value the source holds, or NaN, or fill.  The mode is
 * defined on any float volume: the resampler makes no integer check.  Extents as above. */
typedef enum { SIFT3D_INTERP_LINEAR = 0, SIFT3D_INTERP_NEAREST = 1, SIFT3D_INTERP_LABEL = 2 } sift3d_interp;
/* Host arrays in and out, on `device`.  *kernel_ms (may be NULL): device time of the resampling kernel. */
int sift3d_resample_affine(int device, const float *src, int64_t nx, int64_t ny, int64_t nz, float *dst, int64_t ox, int64_t oy,
                           int64_t oz, const float map[12], int interp, float fill, double *kernel_ms, char *err, int64_t err_len);
/* Device buffers, on the context's stream and ordered like every other *_dev entry point (any context, a slab one too). */
int sift3d_resample_affine_dev(sift3d_ctx *ctx, const float *d_src, int64_t nx, int64_t ny, int64_t nz, float *d_dst, int64_t ox,
                               int64_t oy, int64_t oz, const float map[12], int interp, float fill);
/* Host helpers (also in libsift3d_host.so).  The 4 x 4 row-major matrix WriteMatrix prints for t, before its %f rounding:
 * x_fixed_key = m . x_moving_key. */
void sift3d_similarity_matrix(const sift3d_similarity *t, float m[16]);
/* Parses a .trans.txt (sixteen numbers, nothing after them).  Returns 0, or -1 when the file cannot be read, holds
 * another count of numbers, or its last row is not 0 0 0 1. */
int sift3d_read_similarity(const char *path, float m[16]);
/* The map of sift3d_resample_affine that puts the moving image on the fixed grid: A = inv(moving_vox2key) .
 * inv(moving_to_fixed) . fixed_vox2key, in double, rounded to float once.  vox2key: voxel index -> key coordinates (the
 * identity for keys in voxel units; qto_xyz / sto_xyz of the image for featExtract -w / -ws); NULL means identity.
 * Returns 0, or -1 when a matrix's last row is not 0 0 0 1 or a matrix is singular. */
int sift3d_resample_map(const float moving_to_fixed[16], const float fixed_vox2key[16], const float moving_vox2key[16], float map[12]);
/* vox2key of an image whose keys featExtract wrote: the records of a blob centred on voxel x sit at x + 0.5 (voxel units,
 * world == NULL), or at world . (x + 0.5 f) under -w / -ws, world = that image's qto_xyz / sto_xyz (row-major 4 x 4) and
 * f = min(voxel) / voxel per axis (the isotropic resampling of -w).  voxel: the image's voxel sizes (used with world only).
 * Keys of -2+ / -2- extractions follow neither form. */
void sift3d_key_vox2key(const float voxel[3], const float world[16], float m[16]);

/* ---- nonrigid alignment: a keypoint displacement field (featMatchMultiple -a -e -u, featResample -u; beyond the reference) ---
 * DESIGN.md section 7e states the contract; tests/field_oracle.c restates the fit and the warp.  T is the refined similarity
 * (moving key -> fixed key, the .trans.txt).  The field is backward: at a fixed key position y the moving key position is
 * phi(y) = T^-1(y) + v(y).  v lives on a node grid in fixed key space, its values in moving key units.  Node (a, b, c) sits at
 * (origin[0] + (float)a * spacing, origin[1] + (float)b * spacing, origin[2] + (float)c * spacing), computed in float.
 * Everything outside the grid has v = 0; the grid reaches the support radius past every sample, so its border is 0. */
typedef struct {
    int64_t n[3];      /* nodes per axis, 2 .. 2^24 each */
    float origin[3];   /* key position of node (0, 0, 0) */
    float spacing;     /* h */
    int64_t capacity;  /* floats disp holds (0: not filled); at least 3 n0 n1 n2 to be filled */
    float *disp;       /* component-major: disp[comp * N + (c * n1 + b) * n0 + a], N = n0 n1 n2 */
} sift3d_field;

typedef struct {
    float spacing;           /* h: 4 key units */
    float radius;            /* R, the support radius of the triweight kernel: 20 */
    float lambda;            /* pseudo-weight of zero displacement at every node: 0.1 */
    float search_radius;     /* sift3d_refine_field's guided search radius: 8; must exceed the largest displacement to capture */
    float min_tol;           /* the trim keeps e <= max(min_tol, 3 x the lower median of e): 1.0 */
    int32_t ratio_num;       /* 4: accept when i2 == -1 or ratio_num * d2 > ratio_den * d1 (sift3d_refine_similarity's rule) */
    int32_t ratio_den;       /* 5 */
    int64_t max_nodes;       /* 2^26: grids with more nodes are refused */
    int64_t index_cells_max; /* 2^26: the guided search's index form (sift3d_refine_params) */
} sift3d_field_params;
void sift3d_field_defaults(sift3d_field_params *p);

/* Samples |v_c| above this bound are refused: with at most 2^31 samples of weight <= 1 no int64 sum can overflow
 * (2^31 * (2^7 * 2^24 + 1) < 2^63). */
#define SIFT3D_FIELD_MAX_DISP 128.0f

/* The grid of a sample set (y: n key positions, 3 floats each; samples with a non-finite component are skipped): per axis
 * o = (float)(min y - R) in double (min and max 0 where no sample is finite), n = floor((max - min + 2R) / h) + 2.  Fills
 * f->n, origin and spacing; nothing else.  SIFT3D_ERR_ARG for bad parameters (h, R > 0 and finite, lambda >= 0) or a grid
 * of more than p->max_nodes nodes or more than 2^24 along an axis.  The grid of a superset is at least as large on every
 * axis: the fixed records' positions give a capacity for any pairing of them. */
int sift3d_field_size(const float *y, int64_t n, const sift3d_field_params *p, sift3d_field *f);

/* The samples of accepted pairs (fixed position p_fixed[i], moving position p_moving[i], 3 floats each): y_i = p_fixed[i],
 * v_i = p_moving[i] - T^-1(p_fixed[i]) with T^-1(y) = center0 + rot^T (y - center1) / scale in double (rows summed
 * ((r0 d0 + r1 d1) + r2 d2)), rounded to float once. */
void sift3d_field_samples(const sift3d_similarity *t, const float *p_fixed, const float *p_moving, int64_t n, float *y, float *v);

/* One fit on the GPU (field_fit_kernel) over the grid of sift3d_field_size.  At node P and for every finite sample:
 * dx = y.x - P.x (float), d2 = ((dx dx + dy dy) + dz dz); only d2 < R R counts: t = 1 - d2 / (R R), w = (t t) t;
 * W += rint(w 2^24), V_c += rint((w v_c) 2^24) in int64, so the sums are exact and order-free; the node's value is
 * (float)((double)V_c / ((double)W + lambda 2^24)), 0 where that denominator is 0.  f->capacity < 3N: SIFT3D_ERR_CAPACITY
 * with the grid filled in.  A finite |v_c| > SIFT3D_FIELD_MAX_DISP: SIFT3D_ERR_ARG.  *kernel_ms (may be NULL): device time. */
int sift3d_fit_field(int device, const float *y, const float *v, int64_t n, const sift3d_field_params *p, sift3d_field *f, double *kernel_ms,
                     char *err, int64_t err_len);

typedef struct {
    int32_t accepted;  /* pairs the ratio test accepted, one per fixed record: the samples of the first pass */
    int32_t kept;      /* samples the trim kept: the second pass */
    double rms_before; /* RMS of e_i = |v_i - v(y_i)| over the accepted samples under the first pass */
    double rms_after;  /* RMS of e_i over the kept samples under the second pass */
    double max_disp;   /* largest |v| over the nodes of the result */
    int64_t folds;     /* nodes where det grad phi <= 0 (sift3d_field_folds) */
    double search_ms;  /* device time of the guided search kernel */
    double fit_ms[2];  /* device time of the fit kernel, first and second pass */
} sift3d_field_report;

/* Search, accept, fit, trim, refit: one sift3d_guided_search at t with p->search_radius; the accept rule of
 * sift3d_refine_similarity (ratio test, the least (d1, moving index) per fixed record); the samples of sift3d_field_samples;
 * a fit over them on their grid; e_i = |v_i - v(y_i)| (sift3d_field_eval, double norm); keep e_i <= max(min_tol, 3 x the
 * lower median); a second fit over the kept samples on the same grid.  t: the refined similarity (its arrays are not read).
 * out: capacity as sift3d_fit_field (SIFT3D_ERR_CAPACITY with the grid filled in).  p NULL: defaults.  rep may be NULL. */
int sift3d_refine_field(int device, const sift3d_feature *fixed, int64_t n_fixed, const sift3d_feature *moving, int64_t n_moving,
                        const sift3d_similarity *t, const sift3d_field_params *p, sift3d_field *out, sift3d_field_report *rep, char *err,
                        int64_t err_len);

/* sift3d_resample_affine through T and a field (field_warp_kernel).  Per output voxel p: q = map p (section 7c's order);
 * kappa = C p in the same order, C the first three rows of fixed_vox2key; g = (kappa - origin) / spacing per axis (float
 * divide); where 0 <= g <= n - 1 on every axis, v = the trilinear interpolation of the nodes (section 7c's floor, weights, clamp
 * and x -> y -> z order, per component), else v = 0 and q is left as it is; q_r += ((K[r][0] v0 + K[r][1] v1) + K[r][2] v2),
 * K the linear part of inv(moving_vox2key) (sift3d_field_warp_terms); then section 7c's inside test, gather and fill.  A zero
 * field gives the bytes of sift3d_resample_affine.  vox2key NULL: identity.  *kernel_ms (may be NULL): device time. */
int sift3d_resample_field(int device, const float *src, int64_t nx, int64_t ny, int64_t nz, float *dst, int64_t ox, int64_t oy, int64_t oz,
                          const float map[12], const float fixed_vox2key[16], const float moving_vox2key[16], const sift3d_field *field, int interp,
                          float fill, double *kernel_ms, char *err, int64_t err_len);

/* Host helpers (also in libsift3d_host.so).
 * C (3 x 4, the first rows of fixed_vox2key) and K (3 x 3, the linear part of inv(moving_vox2key) in double, rounded to float
 * once) of sift3d_resample_field.  Returns 0, or -1 when a last row is not 0 0 0 1 or moving_vox2key is singular. */
int sift3d_field_warp_terms(const float fixed_vox2key[16], const float moving_vox2key[16], float c[12], float k[9]);
/* v at n key positions y (3 floats each) into out (3 floats each): the interpolation of sift3d_resample_field, 0 outside. */
void sift3d_field_eval(const sift3d_field *f, const float *y, int64_t n, float *out);
/* Nodes where det grad phi <= 0: grad phi = rot^T / scale + grad v, grad v by central differences in double over 2h with
 * v = 0 past the grid; *max_disp (may be NULL): the largest |v| over the nodes, in double. */
int64_t sift3d_field_folds(const sift3d_similarity *t, const sift3d_field *f, double *max_disp);
/* <moving>.field.nii: NIfTI-1 float32, dim (5, n0, n1, n2, 1, 3), intent_code 1006 (DISPVECT), pixdim h, qform and sform
 * (codes 2, aligned) mapping node index -> key position (diagonal h, offset origin), descrip naming the convention.
 * sift3d_write_field returns 0 or -1.
 * sift3d_read_field accepts exactly what the writer writes: SIFT3D_ERR_ARG for anything else (another datatype, dim[5] != 3,
 * a rotated or non-uniform matrix, a short file), SIFT3D_ERR_CAPACITY (the grid filled in) when f->capacity < 3N. */
int sift3d_write_field(const char *path, const sift3d_field *f);
int sift3d_read_field(const char *path, sift3d_field *f);

/* ---- intensity refinement of the displacement field by block matching (featResample -i; beyond the reference) -------------
 * DESIGN.md section 7f states the contract; tests/blockmatch_oracle.c restates the block search as a serial brute force.
 *
 * The block search.  F (fixed) and W (the moving image already warped onto the fixed grid) are nx ny nz floats, x fastest.
 * Both are quantised with one affine map fixed from F alone: lo, hi = the least and the largest finite value of F
 * (sift3d_blockmatch_range; hi > lo is required); q(v) = -1 where v is not finite, else t = (((double)v - lo) / (hi - lo)) * 1023
 * in double, q = 0 for t <= 0, 1023 for t >= 1023, else rint(t) (ties to even).  The quantisation step is (hi - lo) / 1023.
 * A lattice node (a, b, c) sits at voxel p = first + stride (a, b, c) and has index (c n1 + b) n0 + a.  For every integer shift
 * s in [-r, r]^3: cost(s) = sum over u in [-b, b]^3 of (qF(p + u) - qW(p + u + s))^2, an exact integer below 2^32.  The argmin
 * is the shift of the least (cost, |s|^2, s_z, s_y, s_x) in that order.  A node is flagged where any voxel of p + [-b, b]^3 in
 * F or of p + [-(b + r), b + r]^3 in W lies outside the volume or has q = -1; a flagged node's other words are 0.  Per node 16
 * 32-bit words:
 *   [0..2] argmin shift x, y, z (int32)   [3] flag   [4] cost(argmin)   [5] cost(0)
 *   [6..11] cost at argmin - x, + x, - y, + y, - z, + z (0xffffffff where that shift is outside the search cube)
 *   [12] sum of qF over the block   [13] sum of qF^2 over the block   [14], [15] 0 */
#define SIFT3D_BLOCKMATCH_WORDS 16
#define SIFT3D_BLOCKMATCH_MAX_B 6 /* 13^3 * 1023^2 < 2^32 */
#define SIFT3D_BLOCKMATCH_MAX_R 6
#define SIFT3D_BLOCKMATCH_NONE 0xffffffffu
#define SIFT3D_BLOCKMATCH_MAX_ROUNDS 8

typedef struct {
    int32_t stride;          /* node spacing in fixed voxels: 4 */
    int32_t block;           /* b, the block's half-width: 4 (a 9^3 block); 1 .. SIFT3D_BLOCKMATCH_MAX_B */
    int32_t search;          /* r, the search half-width: 3; 1 .. SIFT3D_BLOCKMATCH_MAX_R */
    int32_t rounds;          /* 2; 0 .. SIFT3D_BLOCKMATCH_MAX_ROUNDS (0 returns the input field) */
    float variance_quantile; /* 0.25: a node needs a block variance above this quantile of the unflagged nodes' */
    float cost_fraction;     /* 0.8: a nonzero argmin needs cost(argmin) < cost_fraction * cost(0) */
    float spacing;           /* h of the output grid: 4 key units */
    float radius;            /* R of the fit (sift3d_field_params): 20 */
    float lambda;            /* 0.1 */
    float min_tol;           /* 1.0 */
    int64_t max_nodes;       /* 2^26: larger lattices and output grids are refused */
} sift3d_blockmatch_params;
void sift3d_blockmatch_defaults(sift3d_blockmatch_params *p);

typedef struct {
    int64_t nodes, flagged;                             /* lattice nodes; flagged by the kernel */
    int64_t gated_variance, gated_border, gated_cost;   /* unflagged nodes the gates dropped, each counted at its first failing gate */
    int64_t samples, kept;                              /* into the first fit; into the second, after the trim */
    double rms_before, rms_after;                       /* RMS of e_i = |v_i - v(y_i)| under the first and the second fit */
    double max_disp;                                    /* largest |v| over the nodes of the round's field */
    int64_t folds;                                      /* nodes where det (L + grad v) <= 0 (sift3d_blockmatch_folds) */
    double warp_ms, match_ms, fit_ms[2];                /* device time: field_warp_kernel, quantisation + block_match_kernel, the fits */
} sift3d_blockmatch_round;

typedef struct {
    int32_t rounds;       /* rounds that produced a field */
    int32_t empty_range;  /* 1: F has no two distinct finite values, nothing was matched and the input field came back */
    float lo, hi;         /* the quantisation range */
    sift3d_blockmatch_round round[SIFT3D_BLOCKMATCH_MAX_ROUNDS];
} sift3d_blockmatch_report;

/* The block search alone on the GPU (bm_quantize_kernel, block_match_kernel): F, W host arrays, out SIFT3D_BLOCKMATCH_WORDS words
 * per node.  generic: 0 the specialised kernel where one exists (b = 4, r = 3 or 4); 1 the kernel's form for any b, r; 2 the
 * specialised form with one multiply-add per instruction (same words from all three).  SIFT3D_ERR_ARG
 * with text: extents outside 1 .. 2^27 - 1, b, r or stride out of range, counts < 1 or more than 2^27 nodes, no finite range. */
int sift3d_block_match(int device, const float *f, const float *w, int64_t nx, int64_t ny, int64_t nz, const int64_t first[3], int64_t stride,
                       const int64_t count[3], int32_t b, int32_t r, int32_t generic, uint32_t *out, double *kernel_ms, char *err,
                       int64_t err_len);

/* Refine a displacement field from the images.  fixed (fx fy fz) and moving (mx my mz): host volumes; vox2key as
 * sift3d_resample_field (NULL: identity); moving_to_fixed: T as the 4 x 4 of the .trans.txt; in: the field to start from
 * (NULL: v = 0).  The output grid is sift3d_blockmatch_grid's: it covers the fixed volume's box.  Per round: W = the moving
 * volume warped through T and the current field onto the fixed grid (field_warp_kernel, linear, fill NaN); the block search
 * over sift3d_blockmatch_lattice; the gates and samples of sift3d_blockmatch_samples (the current field read through
 * sift3d_field_eval); a fit on the output grid, the trim of sift3d_refine_field, a second fit.  The round's field replaces the
 * current one.  A round without samples ends the call.  With no completed round (rounds = 0, an empty range, no sample) out
 * receives the input field as it is, grid included (a zero field on the output grid for in == NULL).  out->capacity must hold
 * the larger of the two grids (SIFT3D_ERR_CAPACITY with the output grid filled in).  SIFT3D_ERR_ARG with text: extents the warp
 * refuses, parameters out of range, a block + search window wider than the volume, a lattice or grid above max_nodes. */
int sift3d_refine_field_intensity(int device, const float *fixed, int64_t fx, int64_t fy, int64_t fz, const float *moving, int64_t mx,
                                  int64_t my, int64_t mz, const float fixed_vox2key[16], const float moving_vox2key[16],
                                  const float moving_to_fixed[16], const sift3d_field *in, const sift3d_blockmatch_params *p, sift3d_field *out,
                                  sift3d_blockmatch_report *rep, char *err, int64_t err_len);

/* ---- the correlation cost of the block search (featResample -i -c; tests/blockmatch_ncc_oracle.c) ----
 * The sum of squared differences above needs both images on one intensity scale.  The second cost is the zero-mean normalised
 * cross-correlation of the two blocks, which no gain, offset or slowly varying bias of the moving image changes.
 * Quantisation: F as above.  W is quantised with the range of the MOVING volume's finite values (sift3d_blockmatch_range on the
 * moving image, fixed once for all rounds: a trilinear warp cannot leave it); same 10-bit map, same -1 for non-finite values,
 * same flags.  A moving volume without two distinct finite values is an empty range exactly like F's.
 * Per node, N = (2b + 1)^3, and shift s, in exact integers (int64; the raw sums stay below 2^32 for b <= 6, |A| and the V's
 * below 2^43):
 *   Sf = sum qF, Sff = sum qF^2 over the block (words [12], [13]);  Sw(s) = sum qW, Sww(s) = sum qW^2, Sfw(s) = sum qF qW over
 *   the block shifted by s;  A(s) = N Sfw - Sf Sw,  Vf = N Sff - Sf^2,  Vw(s) = N Sww - Sw^2
 * then in IEEE double, each integer converted exactly, one operation at a time, no contraction:
 *   rho2(s) = A > 0 and Vf > 0 and Vw > 0 ? ((double)A * (double)A) / ((double)Vf * (double)Vw) : 0
 *   cost(s) = (uint32) rint((1 - (rho2 > 1 ? 1 : rho2)) * 2^31)     0 .. 2^31; anticorrelated, flat F or flat W block: 2^31
 * (A^2 <= Vf Vw holds in the integers; the comparison only catches a quotient that rounds above 1.)  cost(s) is a 32-bit integer
 * again and takes the place of the SSD everywhere: the argmin order (cost, |s|^2, s_z, s_y, s_x), the sixteen words (words
 * [4] .. [11] hold these costs), the flags, sift3d_blockmatch_samples with its gates and parabola step, the fit, the trim and
 * the report are those stated above. */
#define SIFT3D_BLOCKMATCH_SSD 0
#define SIFT3D_BLOCKMATCH_NCC 1
/* sift3d_block_match under the correlation cost: F quantised with F's range, W with W's own.  generic: 0 the register form of
 * the kernel where one exists (b = 4, r = 3 or 4), anything else its form for any b, r (same words).  Refuses what
 * sift3d_block_match refuses, and a W without two distinct finite values. */
int sift3d_block_match_ncc(int device, const float *f, const float *w, int64_t nx, int64_t ny, int64_t nz, const int64_t first[3],
                           int64_t stride, const int64_t count[3], int32_t b, int32_t r, int32_t generic, uint32_t *out, double *kernel_ms,
                           char *err, int64_t err_len);
/* sift3d_refine_field_intensity under a chosen cost: metric SIFT3D_BLOCKMATCH_SSD is that function itself, bit for bit (it calls
 * this one); SIFT3D_BLOCKMATCH_NCC runs the same stage on the correlation cost.  moving_range (may be NULL) receives lo, hi of
 * W's quantisation under NCC and 0, 0 under SSD; rep->lo, rep->hi stay F's range and rep->empty_range is set where either range
 * is empty.  Any other metric: SIFT3D_ERR_ARG with text. */
int sift3d_refine_field_intensity_metric(int device, const float *fixed, int64_t fx, int64_t fy, int64_t fz, const float *moving, int64_t mx,
                                         int64_t my, int64_t mz, const float fixed_vox2key[16], const float moving_vox2key[16],
                                         const float moving_to_fixed[16], const sift3d_field *in, const sift3d_blockmatch_params *p,
                                         int32_t metric, sift3d_field *out, sift3d_blockmatch_report *rep, float moving_range[2], char *err,
                                         int64_t err_len);

/* Host helpers (also in libsift3d_host.so).
 * lo, hi of the quantisation; returns 1, or 0 where F has no two distinct finite values. */
int sift3d_blockmatch_range(const float *f, int64_t n, float *lo, float *hi);
/* The lattice of a volume: first = b + r on every axis, count = floor((n - 1 - 2 (b + r)) / stride) + 1, so that no node's
 * window leaves the volume.  Returns 0, or -1 where 2 (b + r) + 1 exceeds an extent or a parameter is out of range. */
int sift3d_blockmatch_lattice(int64_t nx, int64_t ny, int64_t nz, const sift3d_blockmatch_params *p, int64_t first[3], int64_t count[3]);
/* The output grid: sift3d_field_size (p's spacing, radius, max_nodes) over the key positions of the eight corner voxels
 * (0 or n - 1 per axis), each ((c0 x + c1 y) + c2 z) + c3 in float.  Fills n, origin, spacing. */
int sift3d_blockmatch_grid(int64_t nx, int64_t ny, int64_t nz, const float fixed_vox2key[16], const sift3d_blockmatch_params *p, sift3d_field *f);
/* Gates and samples from the kernel's words, all exact.  With N = (2b + 1)^3, a node's variance is N [13] - [12]^2 (int64).
 * In this order a node is dropped when it is flagged; when its variance is not above the threshold (the ascending variances
 * of the unflagged nodes at index floor(q m), m their count, q = variance_quantile); when |s| = r on an axis; when s != 0 and
 * not (double)cost(s) < (double)cost_fraction * (double)cost(0).  counts[4] receives those four tallies.  Per axis the sub-voxel
 * step is d = 0.5 (c- - c+) / (c- - 2 c0 + c+) in double where that denominator is positive, else 0.  With C the fixed vox2key,
 * D = s + d in double and L the inverse of moving_to_fixed's linear part (adjugate, double): y = (float)(C p), k = C (p + D) in
 * double, v = (float)((double)v_in((float)k) + L (C_linear D)), rows summed ((a0 + a1) + a2), v_in by sift3d_field_eval
 * (0 for in == NULL).  y, v: room for 3 floats per node.  Returns the number of samples, or -1 for bad arguments. */
int64_t sift3d_blockmatch_samples(const uint32_t *words, int64_t nx, int64_t ny, int64_t nz, const sift3d_blockmatch_params *p,
                                  const float fixed_vox2key[16], const float moving_to_fixed[16], const sift3d_field *in, float *y, float *v,
                                  int64_t counts[4]);
/* sift3d_field_folds for a 4 x 4 T: nodes where det (L + grad v) <= 0, L the inverse of T's linear part */
int64_t sift3d_blockmatch_folds(const float moving_to_fixed[16], const sift3d_field *f, double *max_disp);

/* ---- the reverse direction: the inverse field and the Jacobian determinant map (featResample -r, -j; beyond the reference) ---
 * DESIGN.md section 7h states the contract; tests/invert_oracle.c restates it.  M is the forward 4 x 4 (moving key -> fixed
 * key), phi(y) = inv(M) y + v(y) the forward map (v read through the sift3d_field_eval contract, 0 outside its grid and for a
 * NULL field).  M' is inv(M) as a reader gets it back from its .trans.txt (sift3d_affine_invert, sift3d_write_matrix,
 * sift3d_read_similarity).  The inverse field u lives on a node grid in MOVING key space, its values in FIXED key units:
 * psi(z) = inv(M') z + u(z) solves phi(psi(z)) = z, so (M', u) is an ordinary .trans.txt + .field.nii pair with the roles of
 * the two images swapped.  With P = inv(M'), Q = inv(M) (sift3d_affine_invert_d) and A the linear part of M, per node z (its
 * float position widened to double), everything in double unless said:
 *   b_r = ((P[r][0] z0 + P[r][1] z1) + P[r][2] z2) + P[r][3];  u = 0;  k = 0
 *   loop:  y = b + u;  v = sift3d_field_eval at (float)y
 *          r_c = ((((Q[c][0] y0 + Q[c][1] y1) + Q[c][2] y2) + Q[c][3]) + (double)v_c) - z_c;  rr = (r0 r0 + r1 r1) + r2 r2
 *          rr <= (double)tol (double)tol: converged, stop.  k == max_iter: not converged, stop (u stays).
 *          u_c = u_c - ((A[c][0] r0 + A[c][1] r1) + A[c][2] r2);  k = k + 1
 *          a component of u outside [-SIFT3D_FIELD_MAX_DISP, SIFT3D_FIELD_MAX_DISP] or NaN: u = 0, diverged, stop.
 * The node's value is (float)u, its status word k | state << 16 and its residual the last rr. */
#define SIFT3D_INVERT_CONVERGED 0u
#define SIFT3D_INVERT_NOT_CONVERGED 1u
#define SIFT3D_INVERT_DIVERGED 2u
#define SIFT3D_INVERT_STEPS(w) ((w) & 0xffffu)
#define SIFT3D_INVERT_STATE(w) ((w) >> 16)
#define SIFT3D_INVERT_MAX_ITER 65535

typedef struct {
    float spacing;     /* h of the inverse grid: 4 key units (featResample passes the forward field's) */
    float radius;      /* R: the grid reaches R past the moving volume's box: 20 */
    int32_t max_iter;  /* 30; 1 .. SIFT3D_INVERT_MAX_ITER */
    float tol;         /* 1e-3 key units; >= 0 (0: every node with a nonzero residual runs to max_iter) */
    int64_t max_nodes; /* 2^26: larger grids are refused */
} sift3d_invert_params;
void sift3d_invert_defaults(sift3d_invert_params *p);

typedef struct {
    int64_t nodes, converged, not_converged, diverged;
    int32_t max_steps;                  /* the most steps any node used */
    double rms_residual, max_residual;  /* of |r| over the converged nodes, summed in node order */
    double max_disp;                    /* largest |u| over the nodes */
    int64_t folds;                      /* sift3d_blockmatch_folds(M', u) */
    double kernel_ms;                   /* device time of field_invert_kernel */
} sift3d_invert_report;

/* The inverse grid: sift3d_field_size (p's spacing, radius, max_nodes) over the key positions of the moving volume's eight
 * corner voxels, as sift3d_blockmatch_grid does for the fixed volume.  p NULL: defaults.  Fills n, origin, spacing. */
int sift3d_invert_grid(int64_t nx, int64_t ny, int64_t nz, const float moving_vox2key[16], const sift3d_invert_params *p, sift3d_field *f);
/* field_invert_kernel alone on the GPU over the grid in `grid` (n, origin, spacing; its disp is not used): u (3 N floats,
 * component-major), status (N words) and res2 (N doubles, may be NULL) are host arrays.  forward NULL: v = 0.  SIFT3D_ERR_ARG with
 * text: a singular matrix or a last row other than 0 0 0 1, max_iter or tol out of range, a grid with an axis outside
 * 1 .. 2^24 or more than max_nodes nodes, a forward field sift3d_resample_field would refuse. */
int sift3d_invert_nodes(int device, const float m[16], const float m_inv[16], const sift3d_field *forward, const sift3d_invert_params *p,
                        const sift3d_field *grid, float *u, uint32_t *status, double *res2, double *kernel_ms, char *err, int64_t err_len);
/* The stage: sift3d_invert_nodes over out's grid (the caller sets out->n, origin and spacing, from sift3d_invert_grid) into
 * out->disp, and the report.  out->capacity < 3 N or no out->disp: SIFT3D_ERR_CAPACITY, the grid left filled in.  Nodes that did
 * not converge keep their last iterate, diverged nodes get 0; both are counted, neither is an error.  rep may be NULL. */
int sift3d_invert_field(int device, const float m[16], const float m_inv[16], const sift3d_field *forward, const sift3d_invert_params *p,
                        sift3d_field *out, sift3d_invert_report *rep, char *err, int64_t err_len);
/* The Jacobian determinant of a warp on its output grid (jacobian_map_kernel): with q(p) the output voxel -> source voxel map
 * sift3d_resample_field applies for (map, out_vox2key, src_vox2key, field) -- its position arithmetic, for any p -- per voxel p
 *   D[r][a] = (q_r(p + e_a) - q_r(p - e_a)) * 0.5f in float;  det D in double in sift3d_blockmatch_folds' order;
 *   J(p) = (float)(det D * factor),  factor = det lin(src_vox2key) / det lin(out_vox2key) in double (sift3d_jacobian_factor).
 * That is det grad phi in key units: the physical volume ratio under -w, the voxel-count ratio with voxel keys.  J <= 0 is a
 * fold; a NaN node gives NaN.  field NULL: the affine map alone.  out: ox oy oz floats (host).  form 0: six evaluations of q per
 * voxel; 1: the workgroup's brick and a one-voxel halo evaluated once into LDS; -1: the default.  Same
 * numbers from both.  Extents as sift3d_resample_field's output. */
int sift3d_jacobian_map(int device, int64_t ox, int64_t oy, int64_t oz, const float map[12], const float out_vox2key[16],
                        const float src_vox2key[16], const sift3d_field *field, float *out, int form, double *kernel_ms, char *err,
                        int64_t err_len);
/* Host helpers (also in libsift3d_host.so).
 * The inverse of an affine 4 x 4 (last row 0 0 0 1): the adjugate of the 3 x 3 part over its determinant, then
 * t'_r = -((o[r][0] t0 + o[r][1] t1) + o[r][2] t2), in double; sift3d_affine_invert rounds to float once.  0, or -1 for a last
 * row other than 0 0 0 1 or a singular or non-finite matrix. */
int sift3d_affine_invert_d(const float m[16], double out[16]);
int sift3d_affine_invert(const float m[16], float out[16]);
/* m in the .trans.txt layout (%f, tabs, the last row as 0.0 0.0 0.0 1.0), so that sift3d_read_similarity reads it back */
int sift3d_write_matrix(const char *path, const float m[16]);
/* det lin(src_vox2key) / det lin(out_vox2key) in double (NULL: identity); 0, or -1 where one of them is 0 or not finite */
int sift3d_jacobian_factor(const float out_vox2key[16], const float src_vox2key[16], double *factor);

/* ---- composition: two alignments chained into one transform and field (featCompose; beyond the reference) -------------------
 * DESIGN.md section 7i states the contract; tests/compose_oracle.c restates it.  Pair 1 registers moving B to fixed A: M1 is its
 * .trans.txt (B key -> A key), v1 an optional field on a grid in A key space with values in B key units, phi1(y) = inv(M1) y +
 * v1(y), A key -> B key.  Pair 2 registers moving C to fixed B: M2 is C key -> B key, v2 an optional field on a grid in B key space
 * with values in C key units, phi2(s) = inv(M2) s + v2(s).  The composite Phi = phi2 o phi1, A key -> C key, is the pair of "C
 * moving, A fixed".  Its matrix is Mc = M1 M2 (sift3d_compose_matrix).  Mc' is Mc as a reader gets it back (sift3d_write_matrix,
 * sift3d_read_similarity), and the composite field w(y) = Phi(y) - inv(Mc') y lives on a node grid in A key space with values in C
 * key units, so the %f rounding of the matrix is absorbed by w and (Mc', w) is an ordinary .trans.txt + .field.nii pair.
 * With P1 = inv(M1), P2 = inv(M2), Pc = inv(Mc') (sift3d_affine_invert_d), per node y (its float position origin + (float)index h,
 * widened to double), everything in double unless said:
 *   a_r = ((P1[r][0] y0 + P1[r][1] y1) + P1[r][2] y2) + P1[r][3]
 *   v1  = field 1 at y: sift3d_field_eval's float arithmetic (g = (y - o) / h, inside where 0 <= g <= n - 1, floor, weights, the
 *         upper index clamped, x then y then z, each step (1 - w) a + w b); 0 outside its grid and for no field
 *   s_r = a_r + (double)v1_r
 *   b_r = ((P2[r][0] s0 + P2[r][1] s1) + P2[r][2] s2) + P2[r][3]
 *   v2  = field 2 at ((float)s0, (float)s1, (float)s2), same arithmetic; 0 outside and for no field
 *   t_r = b_r + (double)v2_r
 *   c_r = ((Pc[r][0] y0 + Pc[r][1] y1) + Pc[r][2] y2) + Pc[r][3]
 *   w_r = t_r - c_r
 * The node's value is (float)w.  Its status word: SIFT3D_COMPOSE_OUTSIDE1 where field 1 is given and y is outside its grid,
 * SIFT3D_COMPOSE_OUTSIDE2 where field 2 is given and s is outside its grid, SIFT3D_COMPOSE_ZEROED where a component of w is not
 * within +-SIFT3D_FIELD_MAX_DISP (NaN included): the node is then written as 0.  A NaN node of v1 or v2 zeroes exactly the
 * composite nodes whose gather reads it, weight 0 included.
 * The interpolation residual, per cell (n - 1 cells per axis): z = origin + ((float)index + 0.5f) h in float, widened; t(z) and
 * c(z) as above; wt = the composite nodes just written, interpolated at z with the same float arithmetic;
 * e_r = t_r - (c_r + (double)wt_r); the cell's value is the double (e0 e0 + e1 e1) + e2 e2. */
#define SIFT3D_COMPOSE_OUTSIDE1 1u
#define SIFT3D_COMPOSE_OUTSIDE2 2u
#define SIFT3D_COMPOSE_ZEROED 4u

typedef struct {
    float spacing;     /* h of the composite grid; 0: field 1's spacing, else field 2's, else 4 key units */
    float radius;      /* R: the grid reaches R past image A's box: 20 */
    int32_t margin;    /* cells from the grid's border that the residual's figures leave out; -1: ceil(radius / the grid's spacing) */
    int64_t max_nodes; /* 2^26: larger grids are refused */
} sift3d_compose_params;
void sift3d_compose_defaults(sift3d_compose_params *p);

typedef struct {
    int64_t nodes;                      /* of the composite grid */
    int64_t outside1, outside2, zeroed; /* nodes with SIFT3D_COMPOSE_OUTSIDE1, _OUTSIDE2, _ZEROED set */
    double max_disp;                    /* largest |w| over the nodes */
    int64_t folds;                      /* sift3d_blockmatch_folds(Mc', w) */
    int64_t residual_cells;             /* cells the residual's figures cover */
    double rms_residual, max_residual;  /* of |e| over those cells, summed in index order (sift3d_compose_residual) */
    double kernel_ms[2];                /* device time of field_compose_kernel and of compose_residual_kernel */
} sift3d_compose_report;

/* field_compose_kernel, and compose_residual_kernel where res2 is given, alone on the GPU over the grid in `grid` (n, origin,
 * spacing; its disp is not used): w (3 N floats, component-major) and status (N words) are host arrays; res2 (may be NULL)
 * receives the (n0 - 1)(n1 - 1)(n2 - 1) cell values, x fastest, and needs 2 nodes per axis.  mc: Mc' as read back.  field1, field2
 * NULL: v = 0.  kernel_ms (may be NULL): the two device times.  p NULL: defaults; only max_nodes is read.  SIFT3D_ERR_ARG with
 * text: a singular matrix or a last row other than 0 0 0 1, a grid with an axis outside 1 .. 2^24 (2 .. 2^24 with res2) or more
 * than max_nodes nodes, a field sift3d_resample_field would refuse. */
int sift3d_compose_nodes(int device, const float m1[16], const float m2[16], const float mc[16], const sift3d_field *field1,
                         const sift3d_field *field2, const sift3d_compose_params *p, const sift3d_field *grid, float *w, uint32_t *status,
                         double *res2, double kernel_ms[2], char *err, int64_t err_len);
/* The stage: sift3d_compose_nodes with the residual over out's grid (the caller sets out->n, origin and spacing, from
 * sift3d_compose_grid) into out->disp, and the report.  out->capacity < 3 N or no out->disp: SIFT3D_ERR_CAPACITY, the grid left
 * filled in.  Zeroed nodes are counted, not an error.  rep may be NULL. */
int sift3d_compose_field(int device, const float m1[16], const float m2[16], const float mc[16], const sift3d_field *field1,
                         const sift3d_field *field2, const sift3d_compose_params *p, sift3d_field *out, sift3d_compose_report *rep, char *err,
                         int64_t err_len);
/* Host helpers (also in libsift3d_host.so).
 * Mc = M1 M2: the floats widened to double, each entry ((a0 b0 + a1 b1) + a2 b2), plus a3 in the translation column, the last
 * row 0 0 0 1, rounded to float once.  0, or -1 for a last row other than 0 0 0 1 or a non-finite entry. */
int sift3d_compose_matrix(const float m1[16], const float m2[16], float out[16]);
/* h of the composite grid: p->spacing where it is not 0 (p NULL: 0), else field 1's, else field 2's, else 4 */
float sift3d_compose_spacing(const sift3d_compose_params *p, const sift3d_field *field1, const sift3d_field *field2);
/* The composite grid: sift3d_blockmatch_grid's rule (sift3d_compose_spacing, p's radius and max_nodes) over image A's eight corner
 * voxels.  p NULL: defaults.  Fills n, origin, spacing. */
int sift3d_compose_grid(int64_t nx, int64_t ny, int64_t nz, const float a_vox2key[16], const sift3d_compose_params *p, const sift3d_field *field1,
                        const sift3d_field *field2, sift3d_field *f);
/* The residual's figures from the cell values res2 and the status words of a grid of n nodes: over the cells at least `margin`
 * cells from the border on every axis (index margin .. n - 2 - margin) none of whose eight corner nodes is SIFT3D_COMPOSE_ZEROED,
 * in index order: their count (returned), *rms = sqrt(sum / count) and *max = sqrt of the largest value; 0 for no cell. */
int64_t sift3d_compose_residual(const int64_t n[3], const uint32_t *status, const double *res2, int64_t margin, double *rms, double *max);

/* ---- multi-atlas label fusion by locally weighted voting (featFuse; beyond the reference) -----------------------------------
 * DESIGN.md section 7j states the contract; tests/fuse_oracle.c restates it as a serial brute force.
 *
 * The target T (nx ny nz floats, x fastest, extents 1 .. 2^24) is the fixed image; each of K atlases (1 .. SIFT3D_FUSE_MAX_ATLASES)
 * is a moving one with an intensity volume, a label volume of the same extents, its moving_to_fixed 4 x 4 and an optional field:
 * featResample's roles.  Atlas label voxels are non-finite (unlabelled) or integers 0 .. 65535; anything else is SIFT3D_ERR_ARG.
 * Warp: W_k = the atlas intensities through sift3d_resample_field's arithmetic (sift3d_resample_affine's without a field), linear,
 * fill NaN; M_k = the atlas labels through the same map, nearest (label_interp SIFT3D_INTERP_LABEL: label-aware linear, section 7n;
 * its result is a label the atlas holds or NaN, so everything after the warp is the same), fill NaN.
 * Quantisation: section 7f's q (-1: not finite).  T with T's range (sift3d_blockmatch_range; an empty range refuses the call);
 * W_k with T's range under SIFT3D_BLOCKMATCH_SSD and with the range of atlas k's own intensity volume under SIFT3D_BLOCKMATCH_NCC
 * (an empty one gives that atlas u = 0 everywhere).
 * Patch sums, per voxel x and atlas k, half-width b (1 .. SIFT3D_BLOCKMATCH_MAX_B): over the u in [-b, b]^3 with x + u inside the
 * volume, qT(x + u) >= 0 and qW(x + u) >= 0: n = their count, Sf = sum qT, Sff = sum qT^2, Sw = sum qW, Sww = sum qW^2,
 * Sfw = sum qT qW; each below 2^32.  Border patches are clipped, not flagged.
 * Similarity u_k(x) in 0 .. 32768, 0 where n = 0 (sift3d_fuse_similarity):
 *   SSD: D = Sff - 2 Sfw + Sww (int64, >= 0); u = (n 2^15) / (D + n), unsigned 64-bit division: one quantisation step^2 per voxel
 *        regularises, D = 0 gives 32768.
 *   NCC: A = n Sfw - Sf Sw, Vf = n Sff - Sf^2, Vw = n Sww - Sw^2; c = section 7g's cost (its sequence of double operations, n in
 *        place of N); u = (2^31 - c) >> 16.
 * Weight: w = 1 (power 0: majority voting), u (power 1) or u u <= 2^30 (power 2).
 * Vote: atlas k votes at x iff M_k(x) is finite.  S(l) = sum of w_k over the voters with M_k(x) = l (uint64).  If power > 0 and every
 * voter's w is 0, every voter weighs 1 and SIFT3D_FUSE_FALLBACK is set.  The fused label is the l of the largest S(l), ties to the
 * smallest l; conf = (S(win) 65535) / sum over l of S(l), integer division.  No voter: label 0, conf 0, SIFT3D_FUSE_NONE.
 * Two 32-bit words per voxel: [0] label in bits 0 - 15, the number of voters in bits 16 - 21, the two flags; [1] conf. */
#define SIFT3D_FUSE_MAX_ATLASES 32
#define SIFT3D_FUSE_U_ONE 32768
#define SIFT3D_FUSE_FALLBACK 0x40000000u /* bit 30 */
#define SIFT3D_FUSE_NONE 0x80000000u     /* bit 31 */

typedef struct {
    int32_t block;      /* b, the patch half-width: 2; 1 .. SIFT3D_BLOCKMATCH_MAX_B */
    int32_t metric;     /* SIFT3D_BLOCKMATCH_SSD */
    int32_t power;      /* 2; 0, 1 or 2 */
    float fill;         /* 0: the value featFuse writes where no atlas votes (the words do not depend on it) */
    int64_t max_voxels; /* 2^28: above max_voxels target voxels times atlases the stage is refused */
    int32_t label_interp; /* SIFT3D_INTERP_NEAREST: how M_k is warped; or SIFT3D_INTERP_LABEL.  Anything else is SIFT3D_ERR_ARG */
} sift3d_fuse_params;
void sift3d_fuse_defaults(sift3d_fuse_params *p);

typedef struct {
    const float *image, *labels;  /* nx ny nz floats each, x fastest */
    int64_t nx, ny, nz;           /* 1 .. 2^24 */
    const float *vox2key;         /* 16 floats; NULL: identity */
    const float *moving_to_fixed; /* 16 floats: the atlas' .trans.txt */
    const sift3d_field *field;    /* NULL: none */
} sift3d_fuse_atlas;

typedef struct {
    int64_t voters;      /* voxels where the atlas votes */
    int64_t support;     /* voxels where it votes for the fused label */
    double mean_u;       /* (double)(sum of u over its voters) / voters; 0 for no voter or power 0 */
    int32_t empty_range; /* 1: NCC and the atlas' intensities have no two distinct finite values */
    int32_t reserved;
    double warp_ms, weight_ms; /* device time: the atlas' uploads and its two warps; quantisation + fuse_weight_kernel */
} sift3d_fuse_atlas_report;

typedef struct {
    int64_t none, fallback; /* voxels with SIFT3D_FUSE_NONE, with SIFT3D_FUSE_FALLBACK */
    float lo, hi;           /* T's quantisation range */
    double vote_ms;         /* device time: fuse_vote_kernel */
    sift3d_fuse_atlas_report atlas[SIFT3D_FUSE_MAX_ATLASES];
} sift3d_fuse_report;

/* fuse_weight_kernel alone: T and W (already on T's grid) host arrays, u one uint16 per voxel.  w_range: lo, hi that W is quantised
 * with; NULL: T's range under SSD, W's own under NCC.  A w_range without hi > lo gives u = 0 everywhere.  generic: 0 the kernel's
 * form with b at compile time where one exists (b = 2), anything else its form for any b (same u).  SIFT3D_ERR_ARG with text: extents
 * outside 1 .. 2^24, b outside 1 .. 6, an unknown metric, a T without two distinct finite values. */
int sift3d_fuse_weights(int device, const float *t, const float *w, int64_t nx, int64_t ny, int64_t nz, int32_t b, int32_t metric,
                        const float w_range[2], int32_t generic, uint16_t *u, double *kernel_ms, char *err, int64_t err_len);
/* fuse_label_kernel and fuse_vote_kernel alone: u[k], labels[k]: n values each of atlas k (u <= 32768; labels as the atlas labels
 * above, not finite: no vote); words: 2 n.  SIFT3D_ERR_ARG with text: K outside 1 .. 32, a power outside 0 .. 2, a u above 32768, a
 * label that is neither non-finite nor an integer 0 .. 65535 (the text names the atlas and the first such voxel). */
int sift3d_fuse_vote(int device, int32_t K, const uint16_t *const *u, const float *const *labels, int64_t n, int32_t power, uint32_t *words,
                     double *kernel_ms, char *err, int64_t err_len);
/* The stage.  T is quantised once and stays on the device; the atlases stream through one at a time (warp, quantise, weigh, warp the
 * labels); the u and label planes stay for the vote, 4 bytes per voxel and atlas.  Power 0 launches no weight kernel and warps no
 * intensities.  p NULL: defaults.  words: 2 nx ny nz; rep may be NULL.  SIFT3D_ERR_ARG with text: what the above refuse, a matrix
 * that sift3d_resample_map refuses, a field that sift3d_resample_field refuses, nx ny nz K above max_voxels, a label_interp that is
 * neither SIFT3D_INTERP_NEAREST nor SIFT3D_INTERP_LABEL (on the host, before any launch). */
int sift3d_fuse_labels(int device, const float *target, int64_t nx, int64_t ny, int64_t nz, const float target_vox2key[16], int32_t K,
                       const sift3d_fuse_atlas *atlases, const sift3d_fuse_params *p, uint32_t *words, sift3d_fuse_report *rep, char *err,
                       int64_t err_len);

/* Host helpers (also in libsift3d_host.so).
 * u from the six sums under a metric, as stated above; 0 for n <= 0 or an unknown metric. */
uint32_t sift3d_fuse_similarity(int32_t metric, int64_t n, int64_t sf, int64_t sff, int64_t sw, int64_t sww, int64_t sfw);
/* The label domain: a finite voxel of a label volume is an integer 0 .. SIFT3D_LABEL_COUNT - 1 */
#define SIFT3D_LABEL_COUNT 65536
/* The first voxel of a label volume that is neither non-finite nor an integer 0 .. 65535, or -1 for none */
int64_t sift3d_fuse_check_labels(const float *labels, int64_t n);
/* The overlap of two label volumes in exact counts: per label l, count_a[l] and count_b[l] voxels of that label (non-finite voxels
 * have none) and count_both[l] where both have it; each array holds SIFT3D_LABEL_COUNT counts.  Dice(l) = 2 count_both / (count_a + count_b).
 * Returns the number of labels that occur in either volume, or -1 where sift3d_fuse_check_labels refuses one of them. */
int64_t sift3d_label_overlap(const float *a, const float *b, int64_t n, int64_t *count_a, int64_t *count_b, int64_t *count_both);

/* ---- the local search of the label fusion (featFuse -s; beyond the reference) ------------------------------------------------
 * DESIGN.md section 7k states the contract; tests/fuse_search_oracle.c restates it as a serial brute force.
 *
 * Section 7j lets atlas k vote at voxel x with the label it carries at x.  With a search radius r (0 .. SIFT3D_FUSE_MAX_SEARCH,
 * b + r <= SIFT3D_BLOCKMATCH_MAX_B) it votes with the label and the weight of its best-matching nearby patch.  Inputs as above: qT and
 * qW_k on the target grid (-1: not finite), M_k the warped labels, the half-width b.
 * Candidates at x: the shifts t in [-r, r]^3 where x + t lies inside the volume and M_k(x + t) is finite (without labels, as
 * sift3d_fuse_search may be called: every shift inside the volume).
 * Sums per candidate: over the v in [-b, b]^3 where x + v and x + t + v lie inside the volume, qT(x + v) >= 0 and
 * qW(x + t + v) >= 0: the six integers above with qW taken at x + t + v; the same bounds.
 * Similarity: u(x, t) = sift3d_fuse_similarity(metric, the six sums).
 * Choice: t* is the candidate of the largest u; ties go to the smallest |t|^2, then the smallest tz, then ty, then tx.  A flat region
 * keeps t = 0, r = 0 is the rule above exactly, and a candidate with u = 0 is still a candidate.
 * Result per voxel and atlas: u* = u(x, t*); the picked label M_k(x + t*); the shift code
 * ((tz + r)(2r + 1) + (ty + r))(2r + 1) + (tx + r) as a uint16.  No candidate: the atlas does not vote at x, u = 0xffff, the picked
 * label is NaN and the code SIFT3D_FUSE_NO_SHIFT.
 * Vote: as above, over the K planes of u* and picked labels. */
#define SIFT3D_FUSE_MAX_SEARCH 3
#define SIFT3D_FUSE_NO_SHIFT 0xffffu

typedef struct {
    int64_t moved;     /* voters with t* != 0 */
    int64_t dist2_sum; /* sum of |t*|^2 over the voters, exact */
    double search_ms;  /* device time: fuse_search_kernel */
} sift3d_fuse_search_atlas_report;

typedef struct {
    int32_t radius; /* the search the stage ran with */
    int32_t reserved;
    sift3d_fuse_search_atlas_report atlas[SIFT3D_FUSE_MAX_ATLASES];
} sift3d_fuse_search_report;

/* fuse_search_kernel alone: T, W and the optional warped labels (on T's grid) host arrays; u and shift one uint16 per voxel; picked
 * one float per voxel (NaN: no vote), which feeds sift3d_fuse_vote as it is.  labels NULL: every shift inside the volume is a
 * candidate, picked is not written and may be NULL.  w_range as for sift3d_fuse_weights; a W without a range counts as not finite
 * everywhere (u = 0, every tie to the smallest shift).  generic: 0 the kernel's form with b and r at compile time where one exists
 * (b = 2, r = 1 .. 3), anything else its form for any b, r (same words).  SIFT3D_ERR_ARG with text: what sift3d_fuse_weights
 * refuses, r outside 0 .. 3, b + r above 6, a label that sift3d_fuse_vote would refuse. */
int sift3d_fuse_search(int device, const float *t, const float *w, const float *labels, int64_t nx, int64_t ny, int64_t nz, int32_t b, int32_t r,
                       int32_t metric, const float w_range[2], int32_t generic, uint16_t *u, uint16_t *shift, float *picked, double *kernel_ms,
                       char *err, int64_t err_len);
/* The stage with a search radius.  search 0: the words and the report of sift3d_fuse_labels.  search 1 .. 3: every atlas streams
 * through as there, and after its labels are warped fuse_search_kernel writes its u* plane and its picked labels, which
 * fuse_label_kernel turns into its label plane; the vote is unchanged.  rep's voters, support and mean_u are those of the chosen
 * planes, its weight_ms the quantisation plus the search kernel.  srep (may be NULL): per atlas moved, dist2_sum and search_ms.  An
 * atlas whose range is empty under NCC has nothing to search by and votes as with search 0.  The planes stay at 4 bytes per voxel and
 * atlas; the picked labels (4 bytes per voxel) and the shift plane (2 bytes per voxel) are one atlas' at a time, the shift plane
 * kept only until that atlas' counts are taken.  SIFT3D_ERR_ARG with text: what sift3d_fuse_labels refuses, a search outside
 * 0 .. 3, block + search above 6, a search with power 0 (without weights there is nothing to search by). */
int sift3d_fuse_labels_search(int device, const float *target, int64_t nx, int64_t ny, int64_t nz, const float target_vox2key[16], int32_t K,
                              const sift3d_fuse_atlas *atlases, const sift3d_fuse_params *p, int32_t search, uint32_t *words, sift3d_fuse_report *rep,
                              sift3d_fuse_search_report *srep, char *err, int64_t err_len);
/* Host helpers (also in libsift3d_host.so).
 * The code of the shift (tx, ty, tz) under the radius r; SIFT3D_FUSE_NO_SHIFT for r outside 0 .. 3 or a component outside -r .. r. */
uint16_t sift3d_fuse_shift_code(int32_t r, int32_t tx, int32_t ty, int32_t tz);
/* The way back: t = (tx, ty, tz); -1 for a code that is none under r (SIFT3D_FUSE_NO_SHIFT among them), else 0. */
int sift3d_fuse_shift_of(int32_t r, uint32_t code, int32_t t[3]);
/* Over a plane of n codes: the voters (codes other than SIFT3D_FUSE_NO_SHIFT; returned), those with a shift other than 0 and the sum
 * of |t|^2; -1 for a code that is none under r. */
int64_t sift3d_fuse_shift_stats(int32_t r, const uint16_t *shift, int64_t n, int64_t *moved, int64_t *dist2_sum);

/* ---- exact Euclidean distance map and surface distances between label volumes (featFuse -m, featOverlap; beyond the reference) ----
 * DESIGN.md section 7l states the contract; tests/edt_oracle.c restates it as a serial brute force.
 *
 * Distance map.  sites: nx ny nz uint8 flags (x fastest, non-zero: a site); spacing_um: three integers, micrometres per voxel along
 * x, y, z.  Extents 1 .. SIFT3D_EDT_MAX_EXTENT each and at most 2^30 voxels in all; spacings 1 .. SIFT3D_EDT_MAX_SPACING_UM.
 *   D2(x) = min over the sites s of (sx (x0 - s0))^2 + (sy (x1 - s1))^2 + (sz (x2 - s2))^2, in um^2, one uint64 per voxel;
 * SIFT3D_EDT_NONE everywhere where there is no site.  The largest value is 3 (4095 * 65535)^2 < 2^58: every term is an exact integer
 * and a minimum has no order, so the 64 bits do not depend on how they are found.
 * Surface of the label l in a label volume (labels as in the fusion: non-finite is unlabelled, else an integer 0 .. 65535): the
 * voxels that carry l and have a face neighbour that lies outside the volume or does not carry l.
 * Surface distances of l between the volumes A and B on one grid: the list A->B holds, per surface voxel of l in A, the D2 of the
 * map whose sites are the surface voxels of l in B; B->A likewise; n_a and n_b elements.  Each list is sorted ascending; then
 *   max = the last element, p95 = the element at index (95 n + 99) / 100 - 1, sum = the sum of sqrt((double)d2) in ascending order,
 *   hausdorff_mm = sqrt((double)max(max_ab, max_ba)) / 1000, hd95_mm = sqrt((double)max(p95_ab, p95_ba)) / 1000,
 *   assd_mm = (sum_ab + sum_ba) / (double)(n_a + n_b) / 1000.
 * A label that one of the volumes lacks (n_a = 0 or n_b = 0) has no distances: its integer fields are SIFT3D_EDT_NONE and its sums
 * and derived values NaN. */
#define SIFT3D_EDT_MAX_EXTENT 4096
#define SIFT3D_EDT_MAX_SPACING_UM 65535u
#define SIFT3D_EDT_MAX_VOXELS ((int64_t)1 << 30)
#define SIFT3D_EDT_NONE UINT64_MAX

typedef struct {
    int32_t first_label; /* 1: the labels below are skipped (1 skips the background, 0 includes it) */
    int32_t max_labels;  /* 64: with more labels to evaluate the stage is refused */
    int32_t device;      /* 0 */
    int32_t reserved;
} sift3d_surface_params;

typedef struct {
    int32_t label;
    int32_t reserved;
    int64_t voxels_a, voxels_b;               /* voxels that carry the label */
    int64_t n_a, n_b;                         /* of them surface voxels */
    uint64_t max_ab, max_ba, p95_ab, p95_ba;  /* um^2 */
    double sum_ab, sum_ba;                    /* um */
    double hausdorff_mm, hd95_mm, assd_mm;
} sift3d_surface_record;

/* The transform alone on host arrays: d2 one uint64 per voxel.  kernel_ms (may be NULL): four values, the device time of the three
 * passes together and of the x, y and z pass.  SIFT3D_ERR_ARG with text naming the argument: an extent outside 1 .. 4096, more than
 * 2^30 voxels, a spacing outside 1 .. 65535; all checked before anything is allocated. */
int sift3d_distance_map(int device, const uint8_t *sites, int64_t nx, int64_t ny, int64_t nz, const uint32_t spacing_um[3], uint64_t *d2,
                        double kernel_ms[4], char *err, int64_t err_len);
/* The stage: the labels >= first_label that occur in a or b, in ascending order, one record each; records holds max_labels of them,
 * *n_records how many were written.  The label planes are made once per volume; per label one launch marks both surfaces, then one
 * transform and one gather per direction, and sift3d_surface_stats makes the record.  p NULL: defaults.  kernel_ms (may be NULL):
 * the device time of the transform kernels.  SIFT3D_ERR_ARG with text: what sift3d_distance_map refuses, a voxel that
 * sift3d_fuse_check_labels refuses (the volume and the voxel), more than max_labels labels (the count; nothing is dropped). */
int sift3d_surface_distances(const float *a, const float *b, int64_t nx, int64_t ny, int64_t nz, const uint32_t spacing_um[3],
                             const sift3d_surface_params *p, sift3d_surface_record *records, int32_t *n_records, double *kernel_ms, char *err,
                             int64_t err_len);
/* Host helpers (also in libsift3d_host.so). */
void sift3d_surface_defaults(sift3d_surface_params *p);
/* A voxel size in mm as micrometres: lroundf(mm * 1000); -1 for a value that is not finite or a result outside 1 .. 65535, else 0. */
int sift3d_spacing_um(float mm, uint32_t *um);
/* The two lists of one label into rec's n_a, n_b, integer and derived fields, as stated above; sorts the lists in place.  With
 * n_a = 0 or n_b = 0 the lists are not read and may be NULL.  rec's label and voxel counts are left as they are. */
void sift3d_surface_stats(uint64_t *list_ab, int64_t n_a, uint64_t *list_ba, int64_t n_b, sift3d_surface_record *rec);

/* ---- connected components of a label volume and island removal (featClean; beyond the reference) ------------------------------
 * DESIGN.md section 7m states the contract; tests/ccl_oracle.c restates it as a serial flood fill.  Everything is integers, minima
 * and counts: no result depends on tiling, launch order or the order atomics arrive in.
 *
 * Labels as in the fusion: a non-finite voxel is unlabelled, any other an integer 0 .. 65535 (0 is a label like any other: its
 * components are the holes and the background).  Extents 1 .. SIFT3D_CCL_MAX_EXTENT each, at most 2^30 voxels.  connectivity: 6
 * (faces) or 26 (faces, edges and corners).
 * Components: two voxels are joined if they carry the same label and are neighbours under the connectivity; a component is a class
 * of the transitive closure; unlabelled voxels belong to none.  A component's key is the smallest linear index (x fastest) of its
 * voxels; components are numbered 1 .. n in ascending key order.  The map holds per voxel its component's number, 0 where the voxel
 * is unlabelled.  The record of component k is records[k - 1].
 * Cleaning, one round on the round's input L: a component with voxels < min_voxels is small, every other kept.  For every voxel x
 * of a small component C and every face neighbour y of x (faces only, under both connectivities) that lies inside the volume and
 * belongs to a kept component, votes[label(y)] grows by one.  C takes the label of the most votes, ties to the smaller label;
 * without a vote C is unresolved and keeps its label.  Every decision reads L; the round's output is L with the voxels of resolved
 * components rewritten as (float)label, every other voxel keeping its 32 bits.  Rounds repeat on the previous output until one
 * resolves nothing or `rounds` have run; the round that resolves nothing is counted and reported.  min_voxels = 1 returns the input
 * bit for bit. */
#define SIFT3D_CCL_MAX_EXTENT 4096
#define SIFT3D_CCL_MAX_VOXELS ((int64_t)1 << 30)
#define SIFT3D_CLEAN_MAX_MIN_VOXELS (1 << 24)
#define SIFT3D_CLEAN_MAX_ROUNDS 16
#define SIFT3D_CLEAN_VOTE_BYTES ((int64_t)1 << 30) /* the budget of the vote table: small components x labels present x 4 bytes */
/* kernel_ms of sift3d_label_components: total, label plane, brick pass, border merge, flatten, numbers and records */
#define SIFT3D_CCL_STAGES 6

typedef struct {
    int32_t label;
    int32_t reserved;
    int64_t voxels;
    int64_t first;  /* the key: the smallest linear index of the component's voxels */
    int32_t box[6]; /* min x, max x, min y, max y, min z, max z, inclusive */
} sift3d_component_record;

typedef struct {
    int32_t min_voxels;   /* 8: components below it are small; 1 .. 2^24 */
    int32_t connectivity; /* 6; or 26 */
    int32_t rounds;       /* 4; 1 .. 16 */
    int32_t device;       /* 0 */
} sift3d_clean_params;

typedef struct {
    int64_t components;        /* of the round's input */
    int64_t small;             /* of them below min_voxels: resolved + unresolved */
    int64_t resolved;          /* small components that took a neighbour's label */
    int64_t resolved_voxels;   /* the voxels rewritten */
    int64_t unresolved;        /* small components without a vote */
    int64_t unresolved_voxels;
} sift3d_clean_round;

typedef struct {
    int32_t rounds_run;
    int32_t reserved;
    sift3d_clean_round round[SIFT3D_CLEAN_MAX_ROUNDS];
    /* components: those of the input; resolved and resolved_voxels: summed over the rounds; small, unresolved and
     * unresolved_voxels: the last round's */
    sift3d_clean_round total;
} sift3d_clean_report;

/* The components of a label volume on host arrays.  comp (may be NULL): one uint32 per voxel.  records (may be NULL: only the map
 * and the count are wanted): room for max_records.  *n_components is always set once the volume has been labelled, and comp filled;
 * with records given and n_components > max_records the call returns SIFT3D_ERR_ARG with the count in the text and writes no record,
 * so that the caller can come back with room.  kernel_ms (may be NULL): SIFT3D_CCL_STAGES values of device time.  SIFT3D_ERR_ARG
 * with text, checked before anything is allocated: an extent outside 1 .. 4096, more than 2^30 voxels, a connectivity other than 6
 * or 26; then a voxel that sift3d_fuse_check_labels refuses, named. */
int sift3d_label_components(int device, const float *labels, int64_t nx, int64_t ny, int64_t nz, int32_t connectivity, uint32_t *comp,
                            sift3d_component_record *records, int64_t max_records, int64_t *n_components, double *kernel_ms, char *err,
                            int64_t err_len);
/* The cleaning on host arrays: out one float per voxel (may be labels itself).  p NULL: defaults.  report and kernel_ms (the device
 * time of all rounds, each from its first launch to its last) may be NULL.  The device holds 22.125 bytes per voxel (the labels 4,
 * the label plane 2.125, the parent, root and flag planes 12, the small indices 4; sift3d_label_components holds the first 18.125
 * and 48 bytes per record) plus the vote table.  SIFT3D_ERR_ARG with text: what sift3d_label_components refuses, what
 * sift3d_clean_check refuses, a vote table above
 * SIFT3D_CLEAN_VOTE_BYTES (the small components, the labels and the bytes in the text). */
int sift3d_clean_labels(const float *labels, int64_t nx, int64_t ny, int64_t nz, const sift3d_clean_params *p, float *out,
                        sift3d_clean_report *report, double *kernel_ms, char *err, int64_t err_len);
/* Host helpers (also in libsift3d_host.so). */
void sift3d_clean_defaults(sift3d_clean_params *p);
/* 0, or -1 and into err which extent is outside 1 .. 4096 or that the volume has more than 2^30 voxels */
int sift3d_ccl_check_extents(int64_t nx, int64_t ny, int64_t nz, char *err, int64_t err_len);
/* 0, or -1 and into err which of min_voxels, connectivity and rounds is refused, with its value and its range */
int sift3d_clean_check(const sift3d_clean_params *p, char *err, int64_t err_len);
/* The report as text: one commented header line, one line per round, one total line.  Returns the length the whole text needs
 * (without the terminating 0), as snprintf does; buf holds at most len - 1 characters of it.  4096 bytes hold every report. */
int64_t sift3d_clean_report_text(const sift3d_clean_report *rep, char *buf, int64_t len);

/* ---- similarity of two images on one grid (featCompare; beyond the reference) ---------------------------------------------------
 * DESIGN.md section 7o states the contract; tests/similarity_oracle.c restates it serially.  The GPU makes counts and integer sums
 * only, so no result depends on tiling, launch order or the order atomics arrive in; every derived value is host arithmetic.
 *
 * Inputs: A and B are nx ny nz floats, x fastest; extents 1 .. 4096 each, at most 2^30 voxels; bins one of 8, 16, 32, 64.
 * Quantisation: section 7f's q (above: -1 for a non-finite value, else 0 .. 1023, in double, ties to even).  A with A's range
 * (sift3d_blockmatch_range); B with B's own range, or with A's under same_scale.  An image that needs a range and has no two
 * distinct finite values is no error: empty_range is 1 for A, 2 for B (never under same_scale, where B needs none), 3 for both;
 * then no voxel counts (n = 0, excluded = nx ny nz), the histogram is zero, every derived value is NaN and nothing is launched.
 * A voxel counts when qA >= 0 and qB >= 0; excluded is the number of the others.
 * Joint histogram: hist[i bins + j], int64, is the number of counted voxels with qA >> s = i and qB >> s = j, s = 10 - log2 bins.
 * Sums over the counted voxels, int64 each (below 2^51): [0] n, [1] Sa = sum qA, [2] Sb, [3] Saa = sum qA^2, [4] Sbb, [5] Sab.
 * Per label (optional third volume L of section 7j's labels: non-finite is unlabelled, else an integer 0 .. 65535): for every
 * label that occurs on a counted voxel, in ascending order, the same six sums over the counted voxels that carry it.  A counted
 * voxel with a non-finite L is in no label's row and stays in the whole-image numbers.  More than max_labels such labels refuse
 * the call.  There is no histogram per label.
 * Derived values (sift3d_similarity_measures; one sequence of double operations, built without contraction):
 *   D = Saa - 2 Sab + Sbb;  rms = sqrt((double)D / (double)n) * (((double)hi - (double)lo) / 1023.0) under same_scale (lo, hi: A's
 *   range), else NaN;
 *   rho: C = n Sab - Sa Sb, Va = n Saa - Sa^2, Vb = n Sbb - Sb^2, each exact in 128-bit integers and converted to double once;
 *   rho = (double)C / (sqrt(Va) * sqrt(Vb)), NaN unless Va > 0 and Vb > 0;
 *   H(c) = log((double)n) - S / (double)n, S the left-to-right sum of (double)c * log((double)c) over the cells c > 0 in ascending
 *   index order: h_a over the row sums, h_b over the column sums, h_ab over the bins^2 cells in row-major order;
 *   mi = (h_a + h_b) - h_ab;  nmi = (h_a + h_b) / h_ab, NaN unless h_ab > 0;  n = 0: NaN throughout.
 *   Per label: n, rho and rms from that label's sums, by the same text. */
#define SIFT3D_SIMILARITY_MAX_BINS 64
#define SIFT3D_SIMILARITY_MAX_LABELS 64
#define SIFT3D_SIMILARITY_SUMS 6

typedef struct {
    int32_t bins;       /* 64; or 8, 16, 32 */
    int32_t same_scale; /* 0; 1: B is quantised with A's range and rms is given */
    int32_t max_labels; /* 64; 1 .. SIFT3D_SIMILARITY_MAX_LABELS */
    int32_t device;     /* 0 */
    int32_t flush;      /* 1: 64-bit global atomic adds of the workgroups' non-zero cells; 0: the workgroups' histograms as slices in
                           global memory, summed by a second kernel.  Both are exact; DESIGN.md section 7o has their times */
    int32_t reserved;
} sift3d_similarity_params;

typedef struct {
    int32_t bins, same_scale;
    int32_t empty_range; /* 0; 1: A has no range; 2: B; 3: both */
    int32_t reserved;
    float a_lo, a_hi, b_lo, b_hi; /* the ranges the images were quantised with (b: a's under same_scale) */
    int64_t excluded;
    int64_t sums[SIFT3D_SIMILARITY_SUMS]; /* n, Sa, Sb, Saa, Sbb, Sab */
    double mi, nmi, rho, rms, h_a, h_b, h_ab;
    double kernel_ms; /* device time of the launches */
    int64_t hist[SIFT3D_SIMILARITY_MAX_BINS * SIFT3D_SIMILARITY_MAX_BINS]; /* the first bins^2 words */
} sift3d_similarity_record;

typedef struct {
    int32_t label;
    int32_t reserved;
    int64_t sums[SIFT3D_SIMILARITY_SUMS];
    double rho, rms;
} sift3d_similarity_label_record;

/* The kernel alone on host arrays, with the ranges the caller passes (lo, hi each: finite, hi > lo): hist bins^2 int64, sums
 * SIFT3D_SIMILARITY_SUMS int64, *excluded; kernel_ms may be NULL.  SIFT3D_ERR_ARG with text naming the argument, before anything
 * is allocated: a null pointer, an extent outside 1 .. 4096, more than 2^30 voxels, bins other than 8, 16, 32, 64, a range that
 * is not finite or has hi <= lo. */
int sift3d_joint_histogram(int device, const float *a, const float *b, int64_t nx, int64_t ny, int64_t nz, const float a_range[2],
                           const float b_range[2], int32_t bins, int64_t *hist, int64_t *sums, int64_t *excluded, double *kernel_ms, char *err,
                           int64_t err_len);
/* The stage: takes the ranges, checks the labels, launches and computes the derived values.  labels may be NULL; with labels,
 * label_records has room for p->max_labels records and *n_labels is how many were written.  p NULL: defaults.  SIFT3D_ERR_ARG with
 * text, before anything is allocated: what sift3d_joint_histogram refuses, what sift3d_similarity_check refuses, a voxel of labels
 * that sift3d_fuse_check_labels refuses (the voxel in the text), more than max_labels labels on counted voxels (the count in the
 * text; nothing is dropped). */
int sift3d_image_similarity(const float *a, const float *b, const float *labels, int64_t nx, int64_t ny, int64_t nz,
                            const sift3d_similarity_params *p, sift3d_similarity_record *record, sift3d_similarity_label_record *label_records,
                            int32_t *n_labels, char *err, int64_t err_len);
/* Host helpers (also in libsift3d_host.so). */
void sift3d_similarity_defaults(sift3d_similarity_params *p);
/* 0, or -1 and into err which of bins, same_scale, max_labels and flush is refused, with its value */
int sift3d_similarity_check(const sift3d_similarity_params *p, char *err, int64_t err_len);
/* The derived values of a histogram (bins^2 int64; may be record->hist) and its sums into record's bins, same_scale, sums, mi, nmi,
 * rho, rms, h_a, h_b and h_ab; lo, hi: A's range (read under same_scale only).  Nothing else of record is touched.  -1 for a null
 * pointer or bins other than 8, 16, 32, 64, else 0. */
int sift3d_similarity_measures(const int64_t *hist, int32_t bins, const int64_t *sums, float lo, float hi, int32_t same_scale,
                               sift3d_similarity_record *record);
/* rho and rms of one label's sums into rec, by the same text; rec's label and sums are set from the arguments */
void sift3d_similarity_label_measures(int32_t label, const int64_t *sums, float lo, float hi, int32_t same_scale,
                                      sift3d_similarity_label_record *rec);
/* The report as text: "# range_a lo hi", "# range_b lo hi", "# same_scale 0|1", "# voxels counted excluded", the line
 * "mi nmi rho rms h_a h_b h_ab" and, with n_labels >= 0 and label_records given, "# label n rho rms" and one line per label.  A NaN
 * is written as nan.  Returns the length the whole text needs (without the terminating 0), as snprintf does; buf holds at most
 * len - 1 characters of it.  8192 bytes hold every report. */
int64_t sift3d_similarity_report_text(const sift3d_similarity_record *record, const sift3d_similarity_label_record *label_records,
                                      int32_t n_labels, char *buf, int64_t len);

/* ---- affine registration by mutual information (featRegister; beyond the reference) ---------------------------------------------
 * DESIGN.md section 7q states the contract; tests/register_oracle.c restates it serially.  The GPU makes counts and integer sums
 * only; every score and every matrix is host arithmetic in double (register_host.c, similarity_host.c).
 *
 * The kernel's contract (sift3d_warp_histogram).  F: nx ny nz floats, M: mx my mz floats, x fastest; every extent 1 .. 4096, at
 * most 2^30 voxels each; bins 8, 16, 32 or 64; stride s 1, 2, 4 or 8; K = 1 .. SIFT3D_REGISTER_MAX_MAPS maps of 12 floats each,
 * fixed voxel -> moving voxel, exactly the map of sift3d_resample_affine; two ranges (lo, hi), finite with hi > lo.
 * Lattice: the fixed voxels (a s, b s, c s) with a s < nx, b s < ny, c s < nz; N is their number.
 * Per lattice voxel p and map k: q = map p in section 7c's order; v = the linear sample of M at q with fill = NaN (all eight
 * corners read and weighed, so a non-finite corner of weight 0 reaches v); qA = q(F[p]) with F's range, qB = q(v) with M's range
 * (section 7f's q).  The voxel counts when qA >= 0 and qB >= 0.
 * Per map: hist[i bins + j] (int64) and the six sums of the section above over the counted voxels; excluded = N - n; outside = the
 * lattice voxels whose q fails the sampler's inside test 0 <= q <= extent - 1 (a NaN q included), so outside <= excluded.
 *
 * The transform family.  theta = (t[3], r[3], s[3], g[3]), 12 doubles, acts in fixed key space about c = fixed_vox2key .
 * ((nx - 1) / 2, (ny - 1) / 2, (nz - 1) / 2):  D(y) = c + L (y - c) + t,  L = (R(r) . G(g)) . diag(exp s), R Rodrigues' formula on
 * the rotation vector r (the identity at |r| = 0: a = sqrt((r0 r0 + r1 r1) + r2 r2), R = I + (sin a / a) K + ((1 - cos a) / (a a))
 * (K K), K the cross-product matrix of r), G unit upper triangular with g = (g_xy, g_xz, g_yz).  The map of theta is A =
 * inv(moving_vox2key) . (inv(M0) . (D . fixed_vox2key)), with the inverses as sift3d_resample_map takes them, rounded to float
 * once; M0 is the initial moving -> fixed matrix (NULL: identity).  The result is M1 = inv(D) . M0, rounded to float once, a
 * moving -> fixed matrix like M0: sift3d_write_matrix writes it and featResample, featFuse and featCompose read it.
 * dof: 3 = t; 6 = t, r; 7 = t, r and one scale shared by s0 = s1 = s2; 9 = t, r, s; 12 = all.
 * Units: h = the fixed image's smallest voxel edge in key units (the least column norm of fixed_vox2key's 3 x 3 part); rho = half
 * the largest key-space edge (n - 1) |column| of the fixed volume (h / 2 for a single voxel).  A step u moves t by u and r, s, g
 * by u / rho.
 * Search: up to SIFT3D_REGISTER_MAX_LEVELS levels of (stride, first step, last step), steps in multiples of h.  One iteration
 * scores, in ONE launch, theta + step and then theta - step for every active parameter in the order t, r, s, g (2 dof maps).  The
 * score is mi or nmi of sift3d_similarity_measures from the map's integers.  A candidate is admissible when its score is not NaN
 * and (double)n >= min_overlap (double)N.  The best admissible candidate (greatest score, ties to the lowest index) is moved to
 * when its score is strictly greater than the current one; otherwise the step is halved.  A level ends when the step falls below
 * its last step, or after max_iterations iterations (recorded in stop).  The next level re-scores theta on its own lattice first.
 * No smoothing and no pyramid: a level is a lattice stride and nothing else. */
#define SIFT3D_REGISTER_MAX_MAPS 32
#define SIFT3D_REGISTER_MAX_LEVELS 4
#define SIFT3D_REGISTER_THETA 12
#define SIFT3D_REGISTER_METRIC_MI 0
#define SIFT3D_REGISTER_METRIC_NMI 1
/* sift3d_warp_histogram's form: SIFT3D_REGISTER_FORM_DEFAULT, or a sum of the bits below.  Every form gives the same integers */
#define SIFT3D_REGISTER_FORM_DEFAULT (-1)
#define SIFT3D_REGISTER_FORM_BY_MAP 1 /* workgroups ordered by map; without it the maps of one brick run side by side on one XCD */
#define SIFT3D_REGISTER_FORM_PLANE 2  /* F quantised once into an int16 lattice plane; without it F is read and quantised per map */

typedef struct {
    int32_t dof;            /* 12; or 3, 6, 7, 9 */
    int32_t metric;         /* SIFT3D_REGISTER_METRIC_NMI; or _MI */
    int32_t bins;           /* 32; or 8, 16, 64 */
    int32_t n_levels;       /* 3; 1 .. SIFT3D_REGISTER_MAX_LEVELS */
    int32_t stride[SIFT3D_REGISTER_MAX_LEVELS];    /* 4, 2, 1; each 1, 2, 4 or 8 */
    int32_t max_iterations; /* 200, per level; at least 1 */
    int32_t device;         /* 0 */
    int32_t form;           /* SIFT3D_REGISTER_FORM_DEFAULT */
    int32_t reserved;
    double first_step[SIFT3D_REGISTER_MAX_LEVELS]; /* 4, 1, 1/4: multiples of h; finite, > 0 */
    double last_step[SIFT3D_REGISTER_MAX_LEVELS];  /* 1, 1/4, 1/16: > 0 and <= first_step */
    double min_overlap;     /* 0.25; 0 .. 1 */
} sift3d_register_params;

typedef struct {
    int32_t stride, iterations, evaluations;
    int32_t stop;           /* 0: the step fell below the last step; 1: max_iterations */
    int64_t n_lattice;      /* N */
    double score_in, score_out, last_step /* key units */, device_ms;
} sift3d_register_level;

typedef struct {
    int32_t dof, metric, bins, n_levels;
    int32_t stop;           /* 0, or 1 where a level stopped at max_iterations */
    int32_t reserved;
    double h, rho;
    double theta[SIFT3D_REGISTER_THETA]; /* theta* */
    float result[16];       /* M1 */
    float map[12];          /* A(theta*) */
    float reserved2[4];
    sift3d_register_level level[SIFT3D_REGISTER_MAX_LEVELS];
    int64_t outside_before, outside_after;
    sift3d_similarity_record before, after; /* the whole lattice (stride 1) under theta = 0 and under theta*, one K = 2 launch */
} sift3d_register_report;

/* K joint histograms under K maps, host arrays in and out: hist n_maps bins^2 int64, sums n_maps SIFT3D_SIMILARITY_SUMS int64,
 * excluded and outside n_maps int64 each; kernel_ms may be NULL.  SIFT3D_ERR_ARG with text naming the argument, before anything is
 * allocated: a null pointer, an extent outside 1 .. 4096 or more than 2^30 voxels (either image), bins, stride, n_maps, a range,
 * a form that is neither the default nor a sum of its bits. */
int sift3d_warp_histogram(int device, const float *fixed, int64_t nx, int64_t ny, int64_t nz, const float *moving, int64_t mx, int64_t my,
                          int64_t mz, const float *maps, int32_t n_maps, int32_t stride, const float fixed_range[2], const float moving_range[2],
                          int32_t bins, int32_t form, int64_t *hist, int64_t *sums, int64_t *excluded, int64_t *outside, double *kernel_ms, char *err,
                          int64_t err_len);
/* The search.  vox2key, initial: 4 x 4 row-major, NULL: identity; p NULL: defaults.  Each image's range is its own
 * (sift3d_blockmatch_range).  SIFT3D_ERR_ARG with text, before anything is allocated: a null pointer, extents, what
 * sift3d_register_check refuses, a matrix sift3d_register_map refuses at theta = 0, an image without two distinct finite values;
 * and, before anything further is allocated, a start that is inadmissible at the first level (n and N in the text). */
int sift3d_register_affine(const float *fixed, int64_t nx, int64_t ny, int64_t nz, const float *moving, int64_t mx, int64_t my, int64_t mz,
                           const float fixed_vox2key[16], const float moving_vox2key[16], const float initial[16], const sift3d_register_params *p,
                           sift3d_register_report *report, char *err, int64_t err_len);
/* Host helpers (also in libsift3d_host.so). */
void sift3d_register_defaults(sift3d_register_params *p);
/* 0, or -1 and into err which field is refused, with its value */
int sift3d_register_check(const sift3d_register_params *p, char *err, int64_t err_len);
/* A(theta) into map; 0, or -1 where a matrix's last row is not 0 0 0 1, a matrix is singular or an entry of the map is not finite */
int sift3d_register_map(const double theta[SIFT3D_REGISTER_THETA], int64_t nx, int64_t ny, int64_t nz, const float fixed_vox2key[16],
                        const float moving_vox2key[16], const float initial[16], float map[12]);
/* M1(theta) into result; 0 or -1 likewise */
int sift3d_register_result(const double theta[SIFT3D_REGISTER_THETA], int64_t nx, int64_t ny, int64_t nz, const float fixed_vox2key[16],
                           const float initial[16], float result[16]);
/* The candidates of one iteration around theta at step u (key units): 2 active parameters x SIFT3D_REGISTER_THETA doubles into
 * cand, + before -.  Returns their number, or -1 for a dof other than 3, 6, 7, 9, 12. */
int sift3d_register_candidates(const double theta[SIFT3D_REGISTER_THETA], int32_t dof, double u, double rho, double *cand);
/* The lattice of a stride: the points per axis into n, h and rho of the fixed image (each may be NULL); returns N, or -1 for an
 * extent below 1, a stride other than 1, 2, 4, 8 or a vox2key whose 3 x 3 part has a column that is zero or not finite */
int64_t sift3d_register_lattice(int64_t nx, int64_t ny, int64_t nz, int32_t stride, const float fixed_vox2key[16], int64_t n[3], double *h,
                                double *rho);
/* The report as text: a header, one line per level, theta*, M1 and the two records' "n excluded outside mi nmi rho".  Returns the
 * length the whole text needs, as snprintf does; buf holds at most len - 1 characters of it.  4096 bytes hold every report. */
int64_t sift3d_register_report_text(const sift3d_register_report *report, char *buf, int64_t len);

/* ---- a template from up to 32 warped images (featAverage; beyond the reference) ---------------------------------------------------
 * DESIGN.md section 7r states the contract; tests/average_oracle.c restates it serially.  One launch samples all K images at every
 * voxel of the output grid and writes three planes; no warped volume is written.
 *
 * The output grid: nx ny nz voxels (each extent 1 .. 2^24, at most 2^40 voxels, x fastest) with grid_vox2key (NULL: identity).  Image
 * k is a moving image in featResample's roles: its map is sift3d_resample_map(moving_to_fixed, grid_vox2key, vox2key), its field
 * terms sift3d_field_warp_terms(grid_vox2key, vox2key).
 * Per grid voxel x and image k, v_k is the image sampled linearly with fill NaN: with a field sift3d_resample_field's arithmetic,
 * without one sift3d_resample_affine's, bit for bit.  Image k contributes iff v_k is finite; n is the number of contributors and
 * mask has bit k set iff image k contributes.
 * Mean and variance, in double: S = sum of (double)v_k over the contributors in image order; m = S / (double)n; V = sum of
 * ((double)v_k - m)^2 in image order; var = (float)(V / (double)(n - 1)), 0 for n = 1.  No square root is taken.  Every sum starts
 * from +0.
 * Average: trim = 0: avg = (float)m.  trim = t > 0: the contributors are ranked by value, equal values (-0 == 0) by image index:
 * rank_k = #{j : v_j < v_k, or v_j == v_k and j < k}; t_eff = min(t, (n - 1) / 2) (integer division); avg = (float)(the sum of
 * (double)v over the ranks t_eff .. n - 1 - t_eff, added in rank order, / (double)(n - 2 t_eff)).  t = 15 is the median for every
 * n <= 32: the middle value for odd n, the mean of the middle two for even n.
 * Short voxels: where n < min_count, avg and var are fill; mask is kept. */
#define SIFT3D_AVERAGE_MAX_IMAGES 32
#define SIFT3D_AVERAGE_MAX_TRIM 15
#define SIFT3D_AVERAGE_FORM_DEFAULT (-1)
#define SIFT3D_AVERAGE_FORM_COLUMN 0 /* the one form built: a lane keeps its K samples in its own LDS column */

typedef struct {
    int32_t trim;       /* 0; 0 .. SIFT3D_AVERAGE_MAX_TRIM */
    int32_t min_count;  /* 1; 1 .. K */
    float fill;         /* NaN */
    int32_t device;     /* 0 */
    int64_t max_voxels; /* 2^32: the sum of all source voxels; a call above it is refused */
    int32_t form;       /* SIFT3D_AVERAGE_FORM_DEFAULT */
    int32_t reserved;
} sift3d_average_params;

typedef struct {
    const float *image;           /* nx ny nz floats, x fastest */
    int64_t nx, ny, nz;           /* 1 .. 2^24 */
    const float *vox2key;         /* 16 floats; NULL: identity */
    const float *moving_to_fixed; /* 16 floats: the image's .trans.txt against the grid; NULL: identity */
    const sift3d_field *field;    /* NULL: none */
} sift3d_average_image;

typedef struct {
    int64_t contributing; /* grid voxels where the image contributes (from mask, exact) */
    double upload_ms;     /* device time of the image's copy (and its field's) to the device */
} sift3d_average_image_report;

typedef struct {
    int32_t images, trim, min_count, reserved;
    int64_t voxels;                                  /* nx ny nz */
    int64_t none;                                    /* voxels with n = 0 */
    int64_t below;                                   /* voxels with n < min_count (those with n = 0 included) */
    int64_t count[SIFT3D_AVERAGE_MAX_IMAGES + 1];    /* count[n]: voxels with n contributors */
    double kernel_ms, wall_ms;                       /* device time of the launch; host time of the whole call */
    sift3d_average_image_report image[SIFT3D_AVERAGE_MAX_IMAGES];
} sift3d_average_report;

/* The stage.  Every image goes to the device once and stays for the one launch.  avg, var: nx ny nz floats; mask: nx ny nz uint32;
 * p NULL: defaults; report may be NULL.  SIFT3D_ERR_ARG with text naming the argument and the image, before anything is allocated: a
 * null pointer, K outside 1 .. 32, a grid extent outside 1 .. 2^24 or more than 2^40 grid voxels, what sift3d_average_check refuses,
 * an image extent outside 1 .. 2^24, a field that sift3d_resample_field refuses, a matrix that sift3d_resample_map refuses, source
 * voxels above max_voxels. */
int sift3d_average_warped(int64_t nx, int64_t ny, int64_t nz, const float grid_vox2key[16], int32_t K, const sift3d_average_image *images,
                          const sift3d_average_params *p, float *avg, float *var, uint32_t *mask, sift3d_average_report *report, char *err,
                          int64_t err_len);
/* Host helpers (also in libsift3d_host.so). */
void sift3d_average_defaults(sift3d_average_params *p);
/* 0, or -1 and into err which field is refused, with its value: trim, min_count (against K), max_voxels, form */
int sift3d_average_check(const sift3d_average_params *p, int32_t K, char *err, int64_t err_len);
/* The report's counts from the mask plane (n words): images, trim, min_count, voxels, none, below, count[] and every image's
 * contributing; the times are left as they are.  0, or -1 for a null pointer, K outside 1 .. 32 or a mask with a bit at or above K */
int sift3d_average_counts(const uint32_t *mask, int64_t n, int32_t K, int32_t trim, int32_t min_count, sift3d_average_report *report);
/* The report as text: "# images K trim t min_count c", "# voxels N none a below b", "# image contributing upload_ms" and one line per
 * image, "# n voxels" and one line per n = 0 .. K, "# kernel_ms wall_ms" and their line.  Returns the length the whole text needs, as
 * snprintf does, or -1 for a null report or images outside 1 .. 32; buf holds at most len - 1 characters of it.  4096 bytes hold every report. */
int64_t sift3d_average_report_text(const sift3d_average_report *report, char *buf, int64_t len);
/* The node-wise mean of K fields on one grid: out->disp[i] = (float)((sum of (double)fields[k].disp[i] in image order) / (double)K).
 * Fills out->n, origin and spacing from fields[0].  SIFT3D_ERR_ARG with text: K outside 1 .. 32, a null pointer, a field whose disp holds
 * fewer than 3 n0 n1 n2 floats, a field whose n, origin bits or spacing bits differ from those of the first (the text names it);
 * SIFT3D_ERR_CAPACITY with the grid filled in where out->capacity < 3 n0 n1 n2. */
int sift3d_mean_field(int32_t K, const sift3d_field *fields, sift3d_field *out, char *err, int64_t err_len);

/* ---- intensity matching of a registered image (featNormalize; beyond the reference) -----------------------------------------------
 * DESIGN.md section 7s states the contract; tests/normalize_oracle.c restates it serially.  The GPU makes two histograms, integer sums
 * and counts over the reference grid, then applies a transfer table to every voxel of the image; the table is host arithmetic in
 * double (normalize_host.c, built without contraction), so every word of every result is held to the oracle by equality of bits.
 *
 * Inputs: R, the reference, nx ny nz floats with ref_vox2key; B, the image, a sift3d_average_image (its extents, vox2key,
 * moving_to_fixed and field; NULL: identity or none) in featResample's moving role against R; an optional mask M of nx ny nz floats.
 * Every extent 1 .. 4096, at most 2^30 voxels per volume.
 * Ranges: (alo, ahi) = sift3d_blockmatch_range of R, (blo, bhi) of B, each over its whole volume.
 * Per reference voxel x: a = R[x]; b = B sampled linearly with fill NaN at x's position, with a field sift3d_resample_field's
 * arithmetic, without one sift3d_resample_affine's, bit for bit; qa = q(a; alo, ahi), qb = q(b; blo, bhi), section 7f's q.
 * Classes, exclusive, tested in this order: masked (M given and M[x] not finite or == 0); outside (x's position fails the sampler's
 * inside test 0 <= q <= extent - 1, a NaN position included); excluded (qa < 0 or qb < 0); counted.
 * The GPU returns hist_a[1024] and hist_b[1024] (int64: the counted voxels by qa and by qb), the six sums n, Sa, Sb, Saa, Sbb, Sab of
 * the similarity section over the counted voxels, and counts[3] = masked, outside, excluded.
 *
 * The transfer table: m >= 2 knots, xb strictly increasing, xa non-decreasing, slope[k] = (xa[k+1] - xa[k]) / (xb[k+1] - xb[k]) for
 * k < m - 1, tail = (xa[m-1] - xa[0]) / (xb[m-1] - xb[0]), all doubles in quantiser units; both ranges; wa = ((double)ahi -
 * (double)alo) / 1023.0.
 * linear: Va = n Saa - Sa^2, Vb = n Sbb - Sb^2, exact in 128-bit integers, converted to double once; ma = (double)Sa / (double)n,
 * mb = (double)Sb / (double)n; g = sqrt(Va) / sqrt(Vb); xb = {0, 1023}, xa = {ma + (0 - mb) g, ma + (1023 - mb) g}.  Refused unless
 * n >= 2, Va > 0 and Vb > 0.
 * hist (Q knots asked for, 2 .. 256): for j = 0 .. Q, r_j = (j (n - 1)) / Q (integer division); in a histogram h with running sums
 * cum_i (cum_-1 = 0), i the smallest bin with cum_i > r_j: x_j = ((double)i - 0.5) + ((double)(r_j - cum_(i-1)) + 0.5) / (double)h_i;
 * xa_j from hist_a, xb_j from hist_b.  Knot 0 is kept, knot j iff xb_j > the xb of the last kept knot.  Refused when n < 2, when fewer
 * than two knots are kept, or when the first and last kept xa are equal.
 * Applying it to a voxel v of B: a non-finite v keeps its bits; else u = (((double)v - blo) / (bhi - blo)) 1023, unrounded and
 * unclamped; u < xb[0]: y = xa[0] + (u - xb[0]) tail; u >= xb[m-1]: y = xa[m-1] + (u - xb[m-1]) tail; else, k the largest index
 * with xb[k] <= u, y = fmin(xa[k] + (u - xb[k]) slope[k], xa[k+1]); out = (float)((double)alo + y wa). */
#define SIFT3D_NORMALIZE_BINS 1024
#define SIFT3D_NORMALIZE_MAX_KNOTS 257 /* Q + 1 at Q = 256 */
#define SIFT3D_NORMALIZE_COUNTS 3      /* masked, outside, excluded */
#define SIFT3D_NORMALIZE_LINEAR 0
#define SIFT3D_NORMALIZE_HIST 1

typedef struct {
    int32_t mode;   /* SIFT3D_NORMALIZE_LINEAR; or _HIST */
    int32_t knots;  /* Q: 64; 2 .. 256; read under _HIST only */
    int32_t device; /* 0 */
    int32_t reserved;
} sift3d_normalize_params;

typedef struct {
    int32_t mode;
    int32_t m;                    /* the kept knots, 2 .. SIFT3D_NORMALIZE_MAX_KNOTS */
    float a_lo, a_hi, b_lo, b_hi; /* the reference's range and the image's */
    double wa, tail;
    double xb[SIFT3D_NORMALIZE_MAX_KNOTS], xa[SIFT3D_NORMALIZE_MAX_KNOTS];
    double slope[SIFT3D_NORMALIZE_MAX_KNOTS]; /* slope[m - 1 ..] = 0: not read */
} sift3d_transfer;

typedef struct {
    int32_t mode, knots;                     /* as asked for */
    int64_t reference_voxels, image_voxels;  /* nx ny nz; mx my mz */
    int64_t counts[SIFT3D_NORMALIZE_COUNTS]; /* masked, outside, excluded */
    int64_t sums[SIFT3D_SIMILARITY_SUMS];    /* n, Sa, Sb, Saa, Sbb, Sab */
    double hist_ms, apply_ms, wall_ms;       /* device time of either launch; host time of the whole call */
    sift3d_transfer table;
} sift3d_normalize_report;

/* The first kernel alone on host arrays, with the ranges the caller passes (lo, hi each: finite, hi > lo).  mask may be NULL;
 * hist_a, hist_b: 1024 int64 each; sums: SIFT3D_SIMILARITY_SUMS int64; counts: SIFT3D_NORMALIZE_COUNTS int64; kernel_ms may be NULL.
 * SIFT3D_ERR_ARG with text naming the argument, before anything is allocated: a null pointer, an extent outside 1 .. 4096 or more than
 * 2^30 voxels (either volume), a range, a matrix that sift3d_resample_map refuses, a field that sift3d_resample_field refuses. */
int sift3d_overlap_histograms(int device, const float *reference, int64_t nx, int64_t ny, int64_t nz, const float ref_vox2key[16], const float *mask,
                              const sift3d_average_image *image, const float ref_range[2], const float image_range[2], int64_t *hist_a, int64_t *hist_b,
                              int64_t *sums, int64_t *counts, double *kernel_ms, char *err, int64_t err_len);
/* The second kernel alone: out[i] = the table applied to image[i], n voxels (1 .. 2^30), host arrays.  SIFT3D_ERR_ARG with text: a null
 * pointer, n, a table that sift3d_transfer_check refuses. */
int sift3d_apply_transfer(int device, const float *image, int64_t n, const sift3d_transfer *table, float *out, double *kernel_ms, char *err,
                          int64_t err_len);
/* The stage: the ranges, one upload per volume, the histogram launch, the table, the apply launch.  out: mx my mz floats, the image on
 * its own grid on the reference's intensity scale; p NULL: defaults; report may be NULL.  SIFT3D_ERR_ARG with text, before anything is
 * allocated: what sift3d_overlap_histograms refuses, what sift3d_normalize_check refuses, an image without two distinct finite values;
 * and after the histogram launch what sift3d_normalize_transfer refuses (the counts are in the report then). */
int sift3d_normalize_intensity(const float *reference, int64_t nx, int64_t ny, int64_t nz, const float ref_vox2key[16], const float *mask,
                               const sift3d_average_image *image, const sift3d_normalize_params *p, float *out, sift3d_normalize_report *report,
                               char *err, int64_t err_len);
/* Host helpers (also in libsift3d_host.so). */
void sift3d_normalize_defaults(sift3d_normalize_params *p);
/* 0, or -1 and into err which field is refused, with its value: mode, knots (under _HIST) */
int sift3d_normalize_check(const sift3d_normalize_params *p, char *err, int64_t err_len);
/* The table from the histograms (1024 int64 each), the sums and both ranges (lo, hi).  0, or -1 with the refusal's text in err: a null
 * pointer, a mode or Q that sift3d_normalize_check refuses, a range that is not finite or has hi <= lo, sums[0] other than the total of
 * either histogram or a negative word, and the refusals of the two modes above. */
int sift3d_normalize_transfer(int32_t mode, int32_t knots, const int64_t *hist_a, const int64_t *hist_b, const int64_t *sums, const float a_range[2],
                              const float b_range[2], sift3d_transfer *table, char *err, int64_t err_len);
/* 0, or -1 with text: m outside 2 .. 257, xb not strictly increasing, xa decreasing, a value that is not finite, a range */
int sift3d_transfer_check(const sift3d_transfer *table, char *err, int64_t err_len);
/* The report as text: "# mode linear|hist knots Q kept m", "# range_reference lo hi", "# range_image lo hi", "# reference_voxels N counted
 * n masked a outside b excluded c", "# image_voxels N", "# knot xb xa slope" and one line per kept knot (%.17g), "# tail wa" and their
 * line, "# hist_ms apply_ms wall_ms" and their line.  Returns the length the whole text needs, as snprintf does, or -1 for a null report
 * or a table with m outside 2 .. 257; buf holds at most len - 1 characters of it.  32768 bytes hold every report. */
int64_t sift3d_normalize_report_text(const sift3d_normalize_report *report, char *buf, int64_t len);

/* ---- measurement ------------------------------------------------------------
 * Device time per stage of the last sift3d_detect/sift3d_extract call, from
 * HIP events recorded on the stream the kernels ran on. */
typedef enum {
    SIFT3D_STAGE_BLUR_X = 0, /* separable pass along x */
    SIFT3D_STAGE_BLUR_Y,     /* pass along y */
    SIFT3D_STAGE_BLUR_Z_DOG, /* pass along z with fused DoG store */
    SIFT3D_STAGE_SUBSAMPLE,
    SIFT3D_STAGE_EXTREMA,
    SIFT3D_STAGE_KEYPOINT,   /* refinement, patch, orientation frames */
    SIFT3D_STAGE_DESCRIPTOR,
    SIFT3D_STAGE_BLUR_FUSED, /* x, y, z passes and the DoG store in one kernel */
    SIFT3D_STAGE_OCTAVE_TINY, /* all five levels and DoGs of an octave of at most 4096 voxels in one workgroup */
    SIFT3D_STAGE_COUNT
} sift3d_stage;
typedef struct {
    double ms[SIFT3D_STAGE_COUNT];        /* summed kernel time */
    int64_t launches[SIFT3D_STAGE_COUNT];
    double alg_bytes[SIFT3D_STAGE_COUNT]; /* algorithmic bytes moved */
    int64_t n_octaves, n_extrema, n_keypoints, n_records;
    double total_ms;                      /* first kernel to last, on the stream */
} sift3d_timings;
/* on: 0 off; 1 every launch bracketed by two events (full per-stage breakdown; costs about 1 ms per 512^3 run);
 * 2 only the blur launches on the full-size volume (the dominant kernels: what a benchmark can leave on);
 * 3 as 1, with the extrema passes kept on the main stream instead of running beside the coarser octaves' blurs: slower
 *   overall, but every launch is then timed alone (exclusive kernel times). */
int sift3d_enable_timing(sift3d_ctx *ctx, int on);
int sift3d_get_timings(const sift3d_ctx *ctx, sift3d_timings *t);
/* Per-launch log of the same call (needs timing enabled): one entry per kernel
 * launch in issue order, so a bench can group by kernel instantiation
 * (stage + tap count) and compare with a rocprofv3 kernel trace. */
typedef struct {
    int32_t stage;  /* sift3d_stage */
    int32_t ntaps;  /* Gaussian tap count of a blur launch, else 0 */
    int64_t nvox;   /* voxels (or keypoints / records) the launch covered */
    double alg_bytes;
    double ms;
    double start_ms; /* when the launch began, counted from the first timed launch of the call (a timeline across the streams) */
} sift3d_launch_record;
int sift3d_get_launch_log(const sift3d_ctx *ctx, sift3d_launch_record *out, int64_t cap, int64_t *n);

/* Development hooks (make DEV=1 builds only) and the one hardware self-test the product library carries are declared in
 * include/sift3d_dev.h: they are not part of the boundary a caller of the reference binds. */

#ifdef __cplusplus
}
#endif
#endif
