"""The oracle on image-like volumes (tests/image_like.py): quantized, piecewise-constant, high-dynamic-range, NaN-masked and
+-inf inputs.  These pin the oracle's NaN and tie semantics against a plain numpy restatement of the reference's
comparisons, so the GPU parity tests on the same classes (tests/test_gpu_image_like.py) compare with a checker whose
semantics are known, and hold the OpenMP build to the serial bytes on the new classes."""
import ctypes as C

import numpy as np
import pytest

import _oracle
import image_like as il


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _as_list(ext):
    return [(int(e["z"]), int(e["y"]), int(e["x"])) for e in ext]


def _check_values(ext, Dc):
    """every listed value is the level's own value at the voxel, bit for bit"""
    for e in ext:
        assert bits(np.float32(e["value"])) == bits(Dc[e["z"], e["y"], e["x"]])


TRIPLES = il.dog_triples((12, 11, 13), seed=5)


@pytest.mark.parametrize("name", sorted(TRIPLES))
def test_oracle_detect3_matches_numpy_restatement(oracle, name):
    """o3_detect3 (26 + 27 + 27 strict comparisons) against shifted-array all(v < c) / all(v > c), NaN comparing false."""
    Dp, Dc, Dn = TRIPLES[name]
    mins, maxs = oracle.detect3(Dp, Dc, Dn)
    want_min, want_max = il.np_extrema(Dp, Dc, Dn)
    assert _as_list(mins) == want_min and _as_list(maxs) == want_max
    _check_values(mins, Dc)
    _check_values(maxs, Dc)


@pytest.mark.parametrize("name", sorted(TRIPLES))
def test_oracle_detect_and_validate_match_numpy_restatement(oracle, name):
    """o3_detect (26 in the own level, 27 in the level below) and then o3_validate_peak / _valley against the level above
    given as G1 - G2 (G2 = 0, so G1 - G2 is the level itself): the two-step form gives the one-step lists."""
    Dp, Dc, Dn = TRIPLES[name]
    mins, maxs = oracle.detect(Dp, Dc)
    want_min, want_max = il.np_extrema(Dp, Dc, None)
    assert _as_list(mins) == want_min and _as_list(maxs) == want_max
    L = oracle.L
    for fn in (L.o3_validate_peak, L.o3_validate_valley):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64]
    nz, ny, nx = Dc.shape
    G1 = np.ascontiguousarray(Dn, np.float32)
    G2 = np.zeros_like(G1)
    keep = lambda ext, fn: [ext[i] for i in range(len(ext))
                            if fn(ext[i:i + 1].ctypes.data, G1.ctypes.data, G2.ctypes.data, nx, ny, nz)]
    vmin = keep(mins, L.o3_validate_valley)
    vmax = keep(maxs, L.o3_validate_peak)
    want_min, want_max = il.np_extrema(Dp, Dc, Dn)
    assert _as_list(vmin) == want_min and _as_list(vmax) == want_max


def test_triples_exercise_the_edge_cases(oracle):
    """The triples are not vacuous: the tied and partly tied ones have extrema to lose, and the plateau voxels planted in
    partial_plateau are refused (a tie with one of the 26 / with the level above)."""
    mins, maxs = oracle.detect3(*TRIPLES["ties"])
    assert len(mins) + len(maxs) > 0
    mins, maxs = oracle.detect3(*TRIPLES["partial_plateau"])
    assert (4, 4, 4) not in _as_list(maxs) and (4, 4, 5) not in _as_list(maxs)
    assert (4, 9, 4) not in _as_list(mins) and (9, 4, 4) not in _as_list(mins)
    assert sum(map(len, oracle.detect3(*TRIPLES["signed_zero"]))) == 0   # -0 == +0: a tie, never an extremum
    for tag in ("nan", "inf", "ninf"):
        for lvl in ("prev", "cur", "next"):
            Dp, Dc, Dn = TRIPLES["%s_%s" % (tag, lvl)]
            assert not (np.isfinite(Dp).all() and np.isfinite(Dc).all() and np.isfinite(Dn).all())


def test_nan_neighbour_refuses_an_extremum(oracle):
    """The case the max / min form of the GPU's first pass gets wrong: a clear peak with ONE NaN among its 26 (or its 27 in
    either neighbour level) is no extremum, in the oracle as in the reference; without the NaN it is one."""
    shape = (7, 7, 7)
    Dp = np.zeros(shape, np.float32); Dc = np.zeros(shape, np.float32); Dn = np.zeros(shape, np.float32)
    Dc[3, 3, 3] = 5.0
    Dc[1, 5, 5] = -5.0
    assert oracle.detect3(Dp, Dc, Dn)[1]["x"].tolist() == [3]
    for lvl, (z, y, x) in ((1, (2, 3, 4)), (1, (4, 4, 4)), (0, (3, 3, 3)), (2, (2, 2, 2))):
        t = [Dp.copy(), Dc.copy(), Dn.copy()]
        t[lvl][z, y, x] = np.nan
        mins, maxs = oracle.detect3(*t)
        assert len(maxs) == 0, (lvl, z, y, x)
        assert il.np_extrema(*t)[1] == []
    # a NaN centre is neither (the valley planted at (1, 5, 5) stays the one minimum)
    t = [Dp.copy(), Dc.copy(), Dn.copy()]
    t[1][3, 3, 3] = np.nan
    mins, maxs = oracle.detect3(*t)
    assert len(maxs) == 0 and _as_list(mins) == [(1, 5, 5)]
    # an infinite centre over finite neighbours is a maximum; beside another +inf it is not (inf < inf is false)
    t = [Dp.copy(), Dc.copy(), Dn.copy()]
    t[1][3, 3, 3] = np.inf
    assert len(oracle.detect3(*t)[1]) == 1
    t[2][3, 3, 4] = np.inf
    assert len(oracle.detect3(*t)[1]) == 0


CLASS_SHAPE = (40, 36, 44)   # (nz, ny, nx)


@pytest.mark.parametrize("name", sorted(il.CLASSES))
def test_oracle_octave_extrema_match_numpy_on_image_like_levels(oracle, pkg, name):
    """The DoG levels the oracle itself makes from each class (plateaus, NaN borders, infinities, overflow) through its
    detect3, against the numpy restatement: the three detection levels of octave 0."""
    nz, ny, nx = CLASS_SHAPE
    vol = il.make(name, pkg.synth_blobs(nx, ny, nz, seed=21), seed=2)
    with np.errstate(all="ignore"):
        G, D = oracle.octave_levels(oracle.blur(vol, 1.5198684930801392))
    seen = 0
    for l in (1, 2, 3):
        mins, maxs = oracle.detect3(D[l - 1], D[l], D[l + 1])
        want_min, want_max = il.np_extrema(D[l - 1], D[l], D[l + 1])
        assert _as_list(mins) == want_min and _as_list(maxs) == want_max, l
        seen += len(mins) + len(maxs)
    if name in il.NAN_CLASSES:
        assert np.isnan(D).any() and (~np.isnan(D)).any()   # a NaN border exists in the levels the test ran on
    if name not in ("nan_box", "nan_sphere"):
        assert seen > 0


def test_classes_are_deterministic_and_of_their_kind(pkg):
    nz, ny, nx = CLASS_SHAPE
    b = pkg.synth_blobs(nx, ny, nz, seed=21)
    for name in il.CLASSES:
        a, c = il.make(name, b, seed=2), il.make(name, b, seed=2)
        assert a.dtype == np.float32 and a.shape == (nz, ny, nx)
        assert a.tobytes() == c.tobytes(), name
    u8 = il.make("u8", b)
    assert u8.min() == 0 and u8.max() == 255 and (u8 == np.round(u8)).all()
    i16 = il.make("i16", b)
    assert i16.min() == -1024 and (i16 == -1024).mean() > 0.1 and (i16 == np.round(i16)).all()
    assert len(np.unique(il.make("phantom", b))) < 32 and len(np.unique(il.make("steps", b))) < 64
    for name in il.NAN_CLASSES:
        v = il.make(name, b)
        assert np.isnan(v).any() and np.isfinite(v).any() and not np.isinf(v).any()
    assert np.isposinf(il.make("inf_voxels", b)).any() and np.isneginf(il.make("inf_voxels", b)).any()
    assert np.abs(il.make("near_max", b)).max() > 2.5e38


@pytest.mark.parametrize("name", ["u8", "i16", "nan_sphere", "nan_voxels"])
def test_openmp_build_is_byte_identical_on_image_like(oracle, pkg, name):
    """The check of test_oracle_pins.py::test_openmp_build_is_byte_identical on quantized and NaN-masked volumes: the same
    bytes for the blur (NaN payloads included), the candidate lists in the same order, and the records."""
    omp = _oracle.load_omp()
    vol = il.make(name, pkg.synth_blobs(112, 104, 96, seed=17), seed=1)
    assert (bits(omp.blur(vol, 3.0900158882141113)) == bits(oracle.blur(vol, 3.0900158882141113))).all()
    a, b = oracle.candidates(vol), omp.candidates(vol)
    assert len(a) == len(b) and len(a) > 0 and a.tobytes() == b.tobytes()
    for mode in (0, 3):
        ra, _ = oracle.extract(vol, desc_mode=mode)
        rb, _ = omp.extract(vol, desc_mode=mode)
        assert len(ra) == len(rb) and ra.tobytes() == rb.tobytes()


def test_oracle_rank_rule_with_nan_and_signed_zero(oracle):
    """o3_rank (the reference's stable insertion sort) on descriptors with NaN values and signed zeros, against the rule the
    descriptor kernel restates: a NaN keeps its own index, and the values between two NaNs are ranked among themselves,
    ties (-0 == +0 included) by index."""
    rng = np.random.default_rng(0)

    def rule(v):
        nans = np.isnan(v)
        out = np.arange(64)
        for l in range(64):
            if nans[l]:
                continue
            lo = max([j + 1 for j in range(l) if nans[j]], default=0)
            hi = min([j for j in range(l + 1, 64) if nans[j]], default=64)
            out[l] = lo + sum(1 for j in range(lo, hi) if v[j] < v[l] or (v[j] == v[l] and j < l))
        return out

    for t in range(200):
        v = np.round(rng.normal(0, 2, 64)).astype(np.float32)
        v[rng.random(64) < (0.0, 0.05, 0.3, 1.0)[t % 4]] = np.nan
        if t % 5 == 0:
            v[::3] = -0.0
        pc = v.copy()
        oracle.L.o3_rank(pc.ctypes.data)
        assert (pc.astype(np.int64) == rule(v)).all(), t
