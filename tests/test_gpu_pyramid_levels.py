"""GPU suite: every stored level of the resident pyramid against the oracle's, bit for bit, through the C-ABI.

The pipeline tests judge the pyramid by the candidates and records that come out of it, and past octave 1 the volumes the suite
uses hold next to none (DESIGN.md section 9 has the counts).  Here the volumes themselves are read back after a run
(sift3d_get_level_slice, sift3d_get_dog_slice) and compared with pyramid_cases.oracle_pyramid: every Gaussian level L_0..L_4 and
every stored DoG level D_0..D_4 of every octave.  No tolerance: the kernels repeat the reference's float operations in its
order.  A NaN matches only where the oracle has one.

Every run goes through sift3d_detect and then through sift3d_extract (split tail, three streams); the levels read back after
the second must be the bytes read back after the first.
"""
import numpy as np
import pytest

import image_like as il
import pyramid_cases as pc

pytestmark = pytest.mark.gpu

BIG = (128, 128, 128)   # the context's size, and the volume that goes first where stale floats are wanted
_cache = {}


def case(built, oracle, kind, dims, seed, scale=1.0):
    """(volume, oracle pyramid) of a case, made once per session"""
    key = (kind, dims, seed, scale)
    if key not in _cache:
        if kind == "blobs":
            vol = pc.blobs_offset(built, dims, seed)
        elif kind == "signed":
            vol = pc.signed_blobs(dims, seed)
        else:
            vol = il.make(kind, built.synth_blobs(*dims, seed=seed), seed)
        _cache[key] = (vol, pc.oracle_pyramid(oracle, vol, scale))
    return _cache[key]


def make_stale(built, ctx):
    """a larger, strongly offset volume through the context: stale floats in every pad column and buffer tail of what follows"""
    ctx.set_volume(pc.blobs_offset(built, BIG, 3, 500.0))
    assert len(ctx.extract()) > 0


def _same_bytes(a, b):
    for o, (p, q) in enumerate(zip(a, b)):
        for kind in ("L", "D"):
            for j in range(5):
                u, v = p[kind][j], q[kind][j]
                assert (u is None) == (v is None), (o, kind, j)
                assert u is None or u.tobytes() == v.tobytes(), ("after extract", o, kind, j)
    assert len(a) == len(b)


def run_and_compare(built, ctx, vol, want, dims, what, scale=1.0, every_level=False, tiny=None):
    """vol through detect, then extract, on ctx; the resident pyramid against `want`.  every_level: nothing may be missing
    (TUNE_LAZY_LEVELS 0); otherwise only D_0 and D_4 of octaves the octave_tiny stage did not build.  tiny: how many octave_tiny
    launches the run must show (None: as many as the shape has octaves of at most 4096 voxels).  Returns the launch log and the
    stage tallies of the detect run."""
    ctx.enable_timing(True)
    ctx.set_volume(vol)
    ctx.detect(initial_image_scale=scale)
    log, st = ctx.launch_log(), ctx.timings()["stages"]
    got = ctx.pyramid()
    lines, missing = pc.compare_levels(got, want, what)
    print("%s: %d octaves, not stored: %s" % (what, len(got), missing))
    for ln in lines:
        print(ln)
    assert len(got) == len(want) == len(pc.octave_shapes(dims))
    assert not lines, "\n".join(lines)
    shapes = pc.octave_shapes(dims)
    tiny_nvox = log[log["stage"] == built.STAGES.index("octave_tiny")]["nvox"].tolist()
    assert len(tiny_nvox) == st["octave_tiny"]["launches"] == (pc.tiny_octaves(dims) if tiny is None else tiny), (what, tiny_nvox)
    by_tiny = [o for o, (x, y, z) in enumerate(shapes) if x * y * z in tiny_nvox]
    assert len(by_tiny) == len(tiny_nvox) and all(np.prod(shapes[o]) <= pc.TINY_VOX for o in by_tiny)
    if every_level:
        assert not missing, (what, missing)
    else:
        assert all(kind == "D" and j in (0, 4) and o not in by_tiny for o, kind, j in missing), (what, missing, by_tiny)
    ctx.extract(initial_image_scale=scale)
    _same_bytes(got, ctx.pyramid())
    return log, st


@pytest.mark.parametrize("dims", [(72, 72, 72), (100, 100, 100), (168, 40, 36), (67, 45, 38)])
@pytest.mark.parametrize("kind", ["blobs", "signed"])
def test_pitched_coarse_octaves_after_a_larger_volume(built, oracle, dims, kind):
    """72 -> 36 -> 18 (pitch 20) -> 9 (12) -> 4; 100 -> 50 (52) -> 25 (28) -> 12 -> 6 -> 3 (4); 168 -> 84 -> 42 (44) -> 21 (24)
    -> 10 (12) -> 5 (8); 67 odd everywhere.  The context has held a larger volume offset by 500: a pad column or a buffer tail that
    the pipeline leaves as it finds it, and that a blur then reads as the zero border, changes the logical columns next to it."""
    vol, want = case(built, oracle, kind, dims, 21)
    with built.Context(*BIG) as ctx:
        make_stale(built, ctx)
        run_and_compare(built, ctx, vol, want, dims, "%s %s after 128^3 + 500" % (kind, dims))


TINY_SHAPES = [(16, 16, 16), (17, 16, 16), (15, 13, 14), (20, 12, 9), (3, 3, 400), (5, 40, 20)]


@pytest.mark.parametrize("dims", TINY_SHAPES)
@pytest.mark.parametrize("first", [True, False])
def test_single_workgroup_octaves_from_octave_0(built, oracle, dims, first):
    """Volumes whose octave 0 (or, at 17 x 16 x 16, octave 1) is built whole by one workgroup: five levels, five DoG levels, the
    last of them in the small buffer of its own, pitched rows (15, 13 -> 16; 20 -> 10 -> pitch 12; 3 -> 4; 5 -> 8), as the first
    volume of a context and after a larger one."""
    vol, want = case(built, oracle, "signed", dims, 7)
    with built.Context(*BIG) as ctx:
        if not first:
            make_stale(built, ctx)
        run_and_compare(built, ctx, vol, want, dims, "signed %s %s" % (dims, "first" if first else "after 128^3 + 500"))
    vol, want = case(built, oracle, "blobs", dims, 7)
    with built.Context(*dims) as ctx:
        run_and_compare(built, ctx, vol, want, dims, "blobs %s in a context of its size" % (dims,))


@pytest.mark.parametrize("dims", [(88, 61, 47), (104, 96, 81)])
def test_forced_fused_blur_on_coarse_octaves_carries_the_subsample(built, oracle, dims):
    """TUNE_BLUR_FUSED 2 with two rows per thread puts the fused kernel on every octave it supports, so coarse octaves of odd
    sizes hand their half-size volume to the next octave from the level-3 launch (TUNE_FUSED_SUB 1) or from the subsample kernel
    (0): the same levels either way, the oracle's."""
    vol, want = case(built, oracle, "signed", dims, 13)
    subs = {}
    for sub in (1, 0):
        with built.Context(*dims) as ctx:
            ctx.set_tuning(built.TUNE_BLUR_FUSED, 2)
            ctx.set_tuning(built.TUNE_FUSED_ROWS, 2)
            ctx.set_tuning(built.TUNE_FUSED_SUB, sub)
            log, st = run_and_compare(built, ctx, vol, want, dims, "signed %s fused, FUSED_SUB %d" % (dims, sub))
        fused = log[log["stage"] == built.STAGES.index("blur_fused")]
        assert len(fused) > 5 and (fused["nvox"] < fused["nvox"].max()).any(), fused["nvox"].tolist()   # coarse octaves too
        subs[sub] = st["subsample"]["launches"]
    assert subs[1] < subs[0], subs


KNOBS = {"default": ([], 1.0), "lazy_0": ([("TUNE_LAZY_LEVELS", 0)], 0.5), "tiny_0": ([("TUNE_TINY_OCTAVE", 0)], 2.0),
         "fused_0": ([("TUNE_BLUR_FUSED", 0)], 1.0), "fused_2": ([("TUNE_BLUR_FUSED", 2)], 1.0), "split_0": ([("TUNE_SPLIT_TAIL", 0)], 1.0),
         "lazy_0_tiny_0": ([("TUNE_LAZY_LEVELS", 0), ("TUNE_TINY_OCTAVE", 0)], 1.0)}


@pytest.mark.parametrize("dims", [(72, 72, 72), (67, 45, 38), (16, 16, 16)])
@pytest.mark.parametrize("knobs", sorted(KNOBS))
def test_knobs_change_no_level(built, oracle, dims, knobs):
    """Each choice between two ways of making a level: the stored levels are the oracle's on both sides of it.  With
    TUNE_LAZY_LEVELS 0 every level of every octave is stored and compared; with TUNE_TINY_OCTAVE 0 no octave_tiny launch may
    appear.  lazy_0 runs at initial_image_scale 0.5, tiny_0 at 2.0 (another first blur)."""
    settings, scale = KNOBS[knobs]
    vol, want = case(built, oracle, "signed", dims, 5, scale)
    with built.Context(*BIG) as ctx:
        make_stale(built, ctx)
        for name, value in settings:
            ctx.set_tuning(getattr(built, name), value)
        run_and_compare(built, ctx, vol, want, dims, "signed %s %s" % (dims, knobs), scale=scale,
                        every_level=("TUNE_LAZY_LEVELS", 0) in settings, tiny=0 if ("TUNE_TINY_OCTAVE", 0) in settings else None)


@pytest.mark.parametrize("kind", ["nan_slab", "nan_voxels"])
def test_nan_spreads_through_the_coarse_octaves_as_in_the_oracle(built, oracle, kind):
    """Three NaN planes at the y = 0 face (and, second case, two isolated NaN voxels): each blur widens them, each subsample
    halves them, until the coarse octaves hold nothing else.  Where the oracle's level has a NaN the resident one has, and
    nowhere else."""
    dims = (67, 45, 38)
    vol, want = case(built, oracle, kind, dims, 5)
    assert all(np.isnan(G[0]).any() for G, _ in want[:3]) and not np.isnan(want[0][0][4]).all()
    with built.Context(*BIG) as ctx:
        make_stale(built, ctx)
        run_and_compare(built, ctx, vol, want, dims, "%s %s" % (kind, dims))
    with built.Context(*dims) as ctx:
        ctx.set_tuning(built.TUNE_LAZY_LEVELS, 0)
        run_and_compare(built, ctx, vol, want, dims, "%s %s, every level stored" % (kind, dims), every_level=True)


def test_dog_readback_refuses_what_is_not_there(built):
    dims = (40, 36, 33)
    vol = built.synth_blobs(*dims, seed=2)
    plane = (36, 40)

    def refused(ctx, text, *a):
        with pytest.raises(built.Sift3DError) as e:
            ctx.dog_slice(*a)
        assert text in str(e.value), str(e.value)

    with built.Context(*dims) as ctx:
        refused(ctx, "not stored", 0, 1, 0, plane)           # no volume, no run
        ctx.set_volume(vol)
        refused(ctx, "not stored", 0, 1, 0, plane)           # a volume, no run
        ctx.detect()
        assert ctx.dog_slice(0, 1, 0, plane).shape == plane
        refused(ctx, "octave 0 not stored", 0, 0, 0, plane)  # a lazy octave: D_0 and D_4
        refused(ctx, "octave 0 not stored", 0, 4, 0, plane)
        assert ctx.dog_slice(2, 4, 0, (9, 10)).shape == (9, 10)   # 10 x 9 x 8: one workgroup's, D_4 in the small buffer
        for octave, level in ((-1, 1), (4, 1), (0, -1), (0, 5)):
            refused(ctx, "no DoG level", octave, level, 0, plane)
        refused(ctx, "outside 0..32", 0, 1, 33, plane)
        refused(ctx, "outside 0..32", 0, 1, -1, plane)
        refused(ctx, "outside 0..15", 1, 1, 16, (18, 20))
        ctx.set_max_octaves(2)
        ctx.detect()
        refused(ctx, "no DoG level", 2, 1, 0, (9, 10))       # the last run stopped after two octaves
        ctx.set_max_octaves(0)
        ctx.set_volume(vol)
        refused(ctx, "not stored", 0, 1, 0, plane)           # a new volume: the levels are the last one's
        ctx.extract()
        assert ctx.dog_slice(0, 2, 32, plane).shape == plane
        ctx.gauss_blur(vol, 1.5)                             # operator-level calls use the level buffers as scratch
        refused(ctx, "not stored", 0, 1, 0, plane)
    with built.Context(*dims, slab=True) as ctx:
        refused(ctx, "needs a full context", 0, 1, 0, plane)
