"""One table of operator-level blur cases that runs every blur kernel the library builds ("Blur ledger").

The library builds 94 forms of blur_fused_ring_kernel (kernels_blur_fused.hip, chosen by blur_plan.h), 16 of blur_x_kernel<R, VEC>
and 64 of blur_col_kernel<R, VEC, DOG, FULL> (kernels_volume.hip), and sends filters of more than 17 taps to
blur_axis_generic_kernel.  The pyramid launches a handful of them; a caller of the public entry points reaches all.  CASES holds,
for each of them, an operator-level call that runs it, at the smallest shapes that still have partial tiles.  tests/
test_blur_ledger.py (CPU) holds the table to reach every built kernel and names the cases behind each; tests/
test_gpu_blur_ledger.py runs every case against the oracle, bit for bit.  Plain data: no GPU import here.

Not in the table: the one-tap filter (sigma <= 0.3).  blur_dev copies the input and clears the DoG there, where the oracle, like
the reference, filters: out = 0 + 1 * v makes +0.0 of -0.0, and in - out is -0.0 there and NaN at NaN and +-inf voxels
(tests/test_blur_ledger.py pins that on the CPU).  The change that sent one tap through the generic kernel, and its GPU cases,
were taken out again: a GPU run of the suite on that build ended in an illegal memory access whose cause was not found.

Shapes are (nx, ny, nz), volumes (nz, ny, nx) float32, as everywhere in the suite.
"""
import collections
import itertools

import numpy as np

# one filter per half-width R = 1 .. 8 (3 .. 17 taps): test_gpu_parity.SIGMAS, with 0.5 for the 3 taps
SIGMA_OF_R = {1: 0.5, 2: 0.95, 3: 1.2262736558914185, 4: 1.5198684930801392, 5: 1.9465880393981934, 6: 2.452547311782837,
              7: 2.75, 8: 3.0900158882141113}
GENERIC_SIGMAS = (4.5, 7.0)          # more than 17 taps: blur_axis_generic_kernel
ONE_TAP_SIGMAS = (0.0, 0.2, 0.3)     # one tap: no case here (see above); the CPU pin of the oracle's one-tap filter uses them

# the entry point of a case and the outputs it asks for
LEVEL, DOG, BOTH = "gauss_blur_dev", "gauss_blur_dog_dev:dog", "gauss_blur_dog_dev:level+dog"
OUTPUT_SETS = (LEVEL, DOG, BOTH)
HALF = "gauss_blur_dog_half_dev"     # level + DoG + the half-size volume
HOST = "gauss_blur"                  # the host-array entry point, level only

# has_out, has_dog of an entry
OUTPUTS = {LEVEL: (True, False), DOG: (False, True), BOTH: (True, True), HALF: (True, True), HOST: (True, False)}

FAMILIES = ("fused 1-row", "fused 2-row", "three-pass VEC 4", "three-pass VEC 1", "generic")


class Case(collections.namedtuple("Case", "family entry dims sigma knob_items fused nonfinite")):
    """entry: one of the above.  dims: (nx, ny, nz).  knob_items: sorted ((TUNE_* name without the prefix, value), ...), every
    other knob at its default.  fused: whether the fused launch must be what runs.  nonfinite: the input also holds two NaN, a
    +inf and a -inf voxel."""
    __slots__ = ()

    def __new__(cls, family, entry, dims, sigma, knobs, fused, nonfinite):
        return super().__new__(cls, family, entry, tuple(dims), float(sigma), tuple(sorted(dict(knobs).items())), fused, nonfinite)

    @property
    def knobs(self):
        return dict(self.knob_items)


FUSED_SHAPE_OF_TILE = {1: (72, 40, 12),    # 64 x 32 tile: two tile columns, a partial tile in x and in y
                       2: (136, 24, 12)}   # 128 x 16 tile: the same
THIN_OF_TILE = {1: (72, 20, 2),            # thinner than the 3-tap filter and than every prefetch depth
                2: (136, 12, 2)}
THREE_PASS_SHAPES = ((20, 20, 20),         # VEC 4 on both column passes; every axis >= 2 * 8 + 2: FULL for every R
                     (20, 3, 3),           # VEC 4; short axes for every R
                     (19, 21, 23),         # VEC 1; FULL
                     (19, 3, 3),           # VEC 1; short
                     (18, 6, 5))           # y pass VEC 1, z pass VEC 4 (X * Y = 108); FULL / short switches inside the R range
GENERIC_SHAPES = ((40, 24, 20), (19, 21, 23))
DEFAULT_FUSED = (64, 64, 64)               # 2^18 voxels: a 3-tap blur with every knob untouched takes the fused launch
DEFAULT_THREE_PASS = (64, 64, 63)          # one plane fewer: it does not


def _fused_family(rows):
    return "fused 1-row" if rows == 1 else "fused 2-row"


def _three_pass_family(dims):
    return "three-pass VEC 4" if dims[0] % 4 == 0 else "three-pass VEC 1"


def _build():
    cases = []
    # ---- fused, forced on: every filter, output set, thread mapping, tile and stagger; the tile knob picks the shape ----
    for R, entry, rows, tile, stagger in itertools.product(range(1, 9), OUTPUT_SETS, (1, 2), (1, 2), (1, 2)):
        knobs = {"BLUR_FUSED": 2, "FUSED_ROWS": rows, "FUSED_TILE": tile, "FUSED_STAGGER": stagger}
        cases.append(Case(_fused_family(rows), entry, FUSED_SHAPE_OF_TILE[tile], SIGMA_OF_R[R], knobs, True, False))
    # the launch that carries the half-size volume: 11 taps, both outputs, two rows per thread
    for tile, stagger in itertools.product((1, 2), (1, 2)):
        knobs = {"BLUR_FUSED": 2, "FUSED_ROWS": 2, "FUSED_TILE": tile, "FUSED_STAGGER": stagger, "FUSED_SUB": 1}
        cases.append(Case("fused 2-row", HALF, FUSED_SHAPE_OF_TILE[tile], SIGMA_OF_R[5], knobs, True, False))
    # the 3-tap forms once more: a volume thinner than the filter and the prefetch, and three z chunks
    for entry, (rows, tile) in itertools.product(OUTPUT_SETS, ((1, 1), (2, 1), (2, 2))):   # one row per thread has the one tile
        knobs = {"BLUR_FUSED": 2, "FUSED_ROWS": rows, "FUSED_TILE": tile, "FUSED_STAGGER": 1}
        cases.append(Case(_fused_family(rows), entry, THIN_OF_TILE[tile], SIGMA_OF_R[1], knobs, True, False))
        cases.append(Case(_fused_family(rows), entry, FUSED_SHAPE_OF_TILE[tile], SIGMA_OF_R[1], dict(knobs, FUSED_CHUNKS=3), True, False))
    # ---- fused by default: what sift3d_gauss_blur(vol, 0.5) runs on 2^18 voxels and one plane below ----
    cases.append(Case("fused 1-row", HOST, DEFAULT_FUSED, SIGMA_OF_R[1], {}, True, False))
    cases.append(Case("three-pass VEC 4", HOST, DEFAULT_THREE_PASS, SIGMA_OF_R[1], {}, False, False))
    # ---- three passes, default knobs, all below 2^18 voxels ----
    for dims, R, entry in itertools.product(THREE_PASS_SHAPES, range(1, 9), OUTPUT_SETS):
        cases.append(Case(_three_pass_family(dims), entry, dims, SIGMA_OF_R[R], {}, False, False))
    # ---- the generic kernel with its DoG branch ----
    for dims, sigma, entry in itertools.product(GENERIC_SHAPES, GENERIC_SIGMAS, (BOTH, DOG)):
        cases.append(Case("generic", entry, dims, sigma, {}, False, False))
    # ---- one case per family again, with NaN and +-inf voxels in the input ----
    fused = {"BLUR_FUSED": 2, "FUSED_TILE": 1, "FUSED_STAGGER": 2}
    cases.append(Case("fused 1-row", BOTH, FUSED_SHAPE_OF_TILE[1], SIGMA_OF_R[1], dict(fused, FUSED_ROWS=1), True, True))
    cases.append(Case("fused 2-row", BOTH, FUSED_SHAPE_OF_TILE[1], SIGMA_OF_R[3], dict(fused, FUSED_ROWS=2), True, True))
    cases.append(Case("three-pass VEC 4", BOTH, (20, 20, 20), SIGMA_OF_R[2], {}, False, True))
    cases.append(Case("three-pass VEC 1", BOTH, (19, 21, 23), SIGMA_OF_R[7], {}, False, True))
    cases.append(Case("generic", BOTH, (40, 24, 20), 4.5, {}, False, True))
    return tuple(cases)


CASES = _build()
N_FORCED_FUSED = 196   # the first block above: 8 filters x 3 output sets x 2 mappings x 2 tiles x 2 staggers + 4 with the carry


# the pipeline with a first blur of 3 taps (initial_image_scale 0.33: sigma 0.514): (dims, seed of synth_blobs), the seeds chosen
# on the CPU (tests/test_blur_ledger.py holds each to at least 20 candidates in the oracle)
PIPELINE_SCALE = 0.33
PIPELINE_CASES = (((64, 64, 64), 12345),   # 2^18 voxels: the first blur is the fused 3-tap level-only launch
                  ((61, 56, 48), 777))     # below 2^18: three passes, on rows padded to whole vectors

EXTREMES = (0, -0.0, 1e-38, -1e-38, 1e30, -1e30, 1e-45, 3.0)   # the row test_blur_random_noise_and_extremes plants


def nonfinite_voxels(dims):
    """[((z, y, x), value)]: two NaN, one +inf and one -inf, each at least one voxel away from every face"""
    nx, ny, nz = dims
    at = ((nz // 2, ny // 2, nx // 2), (nz // 3, ny // 3, nx // 3), (nz // 2 + 1, ny // 4, 2 * nx // 3), (nz // 4, 2 * ny // 3, nx // 4))
    assert len(set(at)) == 4 and all(1 <= p < n - 1 for zyx in at for p, n in zip(zyx, (nz, ny, nx))), dims
    return list(zip(at, (np.nan, np.nan, np.inf, -np.inf)))


_volumes = {}


def volume(dims, nonfinite=False):
    """The input of every case of a shape: white noise of sigma 1000 with EXTREMES planted in the first row (signed zeros,
    subnormals, magnitudes that cancel), read-only and made once per shape."""
    key = (tuple(dims), bool(nonfinite))
    if key not in _volumes:
        nx, ny, nz = dims
        rng = np.random.default_rng(nx * 1000003 + ny * 1009 + nz)
        vol = (rng.standard_normal((nz, ny, nx)) * 1000).astype(np.float32)
        vol[0, 0, :8] = EXTREMES
        if nonfinite:
            for zyx, v in nonfinite_voxels(dims):
                vol[zyx] = v
        vol.setflags(write=False)
        _volumes[key] = vol
    return _volumes[key]


def describe(case):
    """one line that names a case in a failure message"""
    return "%s %s %dx%dx%d sigma=%r%s%s" % (case.family, case.entry, case.dims[0], case.dims[1], case.dims[2], case.sigma,
                                              "".join(" %s=%d" % kv for kv in sorted(case.knobs.items())), " nonfinite" if case.nonfinite else "")
