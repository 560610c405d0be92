"""GPU suite on image-like volumes (tests/image_like.py): quantized, piecewise-constant, high-dynamic-range, NaN-masked and
+-inf inputs, stage by stage against the oracle.

Bar: the operators bit for bit (a NaN matches a NaN), extrema and candidate lists exact, and records as in
test_gpu_parity.py -- info and desc exact, every float field bit-identical -- except that a record field may be NaN where,
and only where, the oracle's is NaN at the same field.  The +-inf, near-FLT_MAX and denormal-scaled classes are compared up
to the candidates only: past the detection the reference converts non-finite coordinates to int, which has no defined
result (an UndefinedBehaviorSanitizer build of the oracle flags those conversions for exactly these classes).
"""
import struct
import subprocess

import numpy as np
import pytest

import _oracle
import image_like as il

pytestmark = pytest.mark.gpu

REC_SHAPE = (96, 104, 112)     # (nz, ny, nx): NaN masks leave a few hundred records at this size
OP_SHAPES = [(40, 48, 64), (19, 21, 33)]
SIG0 = 1.5198684930801392


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_floats(got, want):
    """bit for bit, except that any NaN matches any NaN"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape
    gn, wn = np.isnan(got), np.isnan(want)
    assert (gn == wn).all(), "NaN at different places: %d vs %d" % (gn.sum(), wn.sum())
    assert (bits(got)[~gn] == bits(want)[~wn]).all()


def vol_of(pkg, name, shape, seed=11):
    nz, ny, nx = shape
    return il.make(name, pkg.synth_blobs(nx, ny, nz, seed=seed), seed=seed)


def same_lists(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for f in ("x", "y", "z"):
        assert (got[f] == want[f]).all()
    assert (bits(got["value"]) == bits(want["value"])).all()


def same_candidates(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for f in ("octave", "level", "is_max", "x", "y", "z"):
        assert (got[f] == want[f]).all(), f
    for f in ("value", "h_value", "l_value"):
        assert (bits(got[f]) == bits(want[f])).all(), f


def compare_records_nan_aware(got, want):
    """_compare_records of test_gpu_parity.py, bit-identical floats, with NaN accepted only where the oracle has NaN."""
    assert len(got) == len(want), (len(got), len(want))
    assert (got["info"] == want["info"]).all()
    for f in ("desc", "x", "y", "z", "scale", "ori", "eigs"):
        same_floats(got[f], want[f])


@pytest.mark.parametrize("shape", OP_SHAPES)
@pytest.mark.parametrize("name", sorted(il.CLASSES))
def test_blur_dog_subsample_bit_exact(built, oracle, shape, name):
    vol = vol_of(built, name, shape)
    nz, ny, nx = shape
    with np.errstate(all="ignore"):
        want_b = oracle.blur(vol, SIG0)
        want_b2 = oracle.blur(want_b, 1.2262736558914185)
        want_d = oracle.dog(want_b, want_b2)
        want_s = oracle.subsample(want_b2)
    with built.Context(nx, ny, nz) as ctx:
        b = ctx.gauss_blur(vol, SIG0)
        b2 = ctx.gauss_blur(want_b, 1.2262736558914185)
        d = ctx.dog(want_b, want_b2)
        s = ctx.subsample2(want_b2)
    same_floats(b, want_b)
    same_floats(b2, want_b2)
    same_floats(d, want_d)
    same_floats(s, want_s)


TRIPLES = il.dog_triples((12, 11, 16), seed=5)       # rows of whole 16-byte vectors: the first pass + validate kernels
TRIPLES_ODD = il.dog_triples((12, 11, 13), seed=6)   # and rows that are not: the element-wise kernel


@pytest.mark.parametrize("name", sorted(TRIPLES))
def test_extrema_lists_on_ties_nan_and_inf(built, oracle, name):
    """sift3d_extrema against the oracle on partial plateaus, signed zeros and NaN / +-inf in d_prev, d_cur or d_next."""
    for trip in (TRIPLES[name], TRIPLES_ODD[name]):
        Dp, Dc, Dn = trip
        nz, ny, nx = Dc.shape
        with built.Context(nx, ny, nz) as ctx:
            mins, maxs = ctx.extrema(Dp, Dc, Dn, capacity=Dc.size)
            omin, omax = oracle.detect3(Dp, Dc, Dn)
            same_lists(mins, omin)
            same_lists(maxs, omax)
            mins, maxs = ctx.extrema(Dp, Dc, None, capacity=Dc.size)
            omin, omax = oracle.detect(Dp, Dc)
            same_lists(mins, omin)
            same_lists(maxs, omax)


@pytest.mark.parametrize("shape", [(40, 36, 44), (40, 36, 43), (24, 40, 256)])
@pytest.mark.parametrize("name", sorted(il.CLASSES))
def test_extrema_lists_on_image_like_levels(built, oracle, shape, name):
    """The oracle's own DoG levels of each class (NaN borders, plateaus, infinities) through sift3d_extrema: the march
    (X = 256: chunks of planes), the plane-per-block form (X = 44) and the element-wise kernel (X = 43)."""
    vol = vol_of(built, name, shape)
    nz, ny, nx = shape
    with np.errstate(all="ignore"):
        G, D = oracle.octave_levels(oracle.blur(vol, SIG0))
    with built.Context(nx, ny, nz) as ctx:
        for l in (1, 2, 3):
            mins, maxs = ctx.extrema(D[l - 1], D[l], D[l + 1])
            omin, omax = oracle.detect3(D[l - 1], D[l], D[l + 1])
            same_lists(mins, omin)
            same_lists(maxs, omax)


def _candidates_and_records(built, oracle, vol, modes, eigs=(140.0,), knobs=()):
    nz, ny, nx = vol.shape
    with built.Context(nx, ny, nz) as ctx:
        for k, v in knobs:
            ctx.set_tuning(k, v)
        ctx.set_volume(vol)
        cand = ctx.detect()
        recs = {(m, e): ctx.extract(desc_mode=m, eig_thres=e) for m in modes for e in eigs}
    return cand, recs


@pytest.mark.parametrize("name", sorted(il.CLASSES))
def test_candidates_on_image_like(built, oracle, name):
    vol = vol_of(built, name, REC_SHAPE)
    cand, _ = _candidates_and_records(built, oracle, vol, ())
    want = oracle.candidates(vol)
    same_candidates(cand, want)
    if name not in ("near_max",):
        assert len(want) > 5


@pytest.mark.parametrize("eig", [140.0, 0.0, -1.0, 1e30])
@pytest.mark.parametrize("name", il.RECORD_CLASSES)
def test_records_on_image_like(built, oracle, name, eig):
    """desc modes 0-3; eig_thres < 0 sends every candidate (degenerate and NaN patches included) through orientation and
    descriptor code, 0 and 1e30 the two ends of the eigenvalue test."""
    vol = vol_of(built, name, REC_SHAPE)
    _, recs = _candidates_and_records(built, oracle, vol, (0, 1, 2, 3), (eig,))
    for m in (0, 1, 2, 3):
        want, _ = oracle.extract(vol, desc_mode=m, eig_thres=eig)
        compare_records_nan_aware(recs[(m, eig)], want)
        if eig in (140.0, -1.0):
            assert len(want) > 5


KNOBS = [[], [("TUNE_BLUR_FUSED", 0)], [("TUNE_BLUR_FUSED", 1)], [("TUNE_BLUR_FUSED", 2)], [("TUNE_LAZY_LEVELS", 0)],
         [("TUNE_TINY_OCTAVE", 0)], [("TUNE_SPLIT_TAIL", 0)], [("TUNE_SPLIT_TAIL", 1)], [("TUNE_SPLIT_TAIL", 2)]]


@pytest.mark.parametrize("name", ["u8", "i16", "steps", "nan_voxels", "nan_slab", "nan_box", "inf_voxels"])
def test_every_extrema_path_by_knobs(built, oracle, name):
    """Every knob setting that changes which kernels run gives the oracle's candidates (and, for classes with a defined
    reference output, the oracle's records)."""
    vol = vol_of(built, name, REC_SHAPE)
    want = oracle.candidates(vol)
    want_r = oracle.extract(vol)[0] if name in il.RECORD_CLASSES else None
    for knobs in KNOBS:
        cand, recs = _candidates_and_records(built, oracle, vol, (0,) if want_r is not None else (),
                                             knobs=[(getattr(built, k), v) for k, v in knobs])
        same_candidates(cand, want)
        if want_r is not None:
            compare_records_nan_aware(recs[(0, 140.0)], want_r)


@pytest.mark.parametrize("name", ["u8", "nan_voxels", "nan_box"])
def test_fused_blur_shape_on_image_like(built, oracle, name):
    """168 x 164 x 160 (> 2^22 voxels): the fused blur and the march run on the first octave."""
    vol = vol_of(built, name, (160, 164, 168))
    cand, recs = _candidates_and_records(built, oracle, vol, (0,))
    same_candidates(cand, oracle.candidates(vol))
    compare_records_nan_aware(recs[(0, 140.0)], oracle.extract(vol)[0])


@pytest.mark.parametrize("shape", [(27, 29, 33), (21, 23, 18), (31, 17, 45)])
@pytest.mark.parametrize("name", ["u8", "phantom", "nan_voxels", "nan_slab", "inf_voxels"])
def test_small_odd_shapes_on_image_like(built, oracle, shape, name):
    """Small odd shapes through the element-wise extrema kernel: candidates and records of octave 0 (0 to 12 candidates a
    volume) and at most one candidate of octave 1.  The octaves one workgroup builds whole (octave 1 on) contribute nothing
    else to these lists; their levels are compared in test_gpu_pyramid_levels.py::test_single_workgroup_octaves_from_octave_0."""
    vol = vol_of(built, name, shape)
    cand, recs = _candidates_and_records(built, oracle, vol, (0, 3) if name in il.RECORD_CLASSES else (), (-1.0,))
    same_candidates(cand, oracle.candidates(vol))
    if name in il.RECORD_CLASSES:
        for m in (0, 3):
            compare_records_nan_aware(recs[(m, -1.0)], oracle.extract(vol, desc_mode=m, eig_thres=-1.0)[0])


def _write_int16_nifti(built, path, vol_i16):
    """NIfTI-1 with datatype INT16: the float32 writer's header with the datatype, bitpix and data replaced."""
    built.write_nifti(path, vol_i16.astype(np.float32))
    raw = bytearray(open(path, "rb").read())
    off = int(struct.unpack_from("<f", raw, 108)[0])
    struct.pack_into("<hh", raw, 70, 4, 16)
    open(path, "wb").write(bytes(raw[:off]) + np.ascontiguousarray(vol_i16, "<i2").tobytes())


def test_cli_on_nan_background_and_int16(built, oracle, tmp_path):
    """featExtract -d0 on a float32 NIfTI with a NaN background and on an int16 NIfTI: the .key is byte-identical to the
    oracle CLI's."""
    shape = (64, 72, 80)
    cases = []
    f = str(tmp_path / "nan.nii")
    built.write_nifti(f, vol_of(built, "nan_slab", shape))
    cases.append(f)
    g = str(tmp_path / "i16.nii")
    _write_int16_nifti(built, g, vol_of(built, "i16", shape).astype(np.int16))
    cases.append(g)
    for nii in cases:
        for flag in (None, "-bn"):
            k1, k2 = str(tmp_path / "gpu.key"), str(tmp_path / "cpu.key")
            r = subprocess.run([built.FEATEXTRACT, "-d0"] + ([flag] if flag else []) + [nii, k1], capture_output=True, text=True)
            assert r.returncode == 0, r.stdout + r.stderr
            r = subprocess.run([_oracle.CLI] + ([flag] if flag else []) + [nii, k2], capture_output=True, text=True)
            assert r.returncode == 0, r.stdout + r.stderr
            a, b = open(k1, "rb").read(), open(k2, "rb").read()
            assert a == b and len(a.splitlines()) > 8, (nii, flag)


def test_zslab_nan_masked_matches_single_gpu(built):
    """One NaN-masked volume through the one-process Z-slab driver on devices [0, 0]: the single-GPU bytes (every rank
    takes the element-wise first pass, also the one whose own slices are finite)."""
    vol = vol_of(built, "nan_slab", (160, 72, 96))
    vol[:40] = np.nan   # the first rank's slices: NaN only there
    nz, ny, nx = vol.shape
    with built.Context(nx, ny, nz) as ctx:
        ctx.set_volume(vol)
        want = ctx.extract()
    got, st = built.extract_zslab(vol, [0, 0])
    assert st["n_ranks"] == 2 and len(want) > 20
    assert got.tobytes() == want.tobytes()
