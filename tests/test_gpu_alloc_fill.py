"""GPU suite: no result may depend on what an allocation held ("The allocator's fill hook").

Every device and pinned host block of the library comes from csrc/alloc_fill.hip (tests/test_alloc_ledger.py keeps it so), and
sift3d_selftest_alloc_fill makes that allocator fill each block, and each piece a slab rank cuts from its reused arena, with one
byte before the library sees it.  A young process mostly gets zero pages, so a missing or short clear passes every other test; here
each entry point runs its smallest case that reaches every buffer of the call under the fill bytes 0xFF and 0x55 and is held to
its CPU ORACLE -- never to an unpoisoned GPU run -- with the family's own helpers and exactness.  Two bytes, because all-ones is
what the code itself uses for "none" (EDT_NONE, index -1, a NaN label), while 0x55 is a large finite float (1.46e13), a positive
int and a valid uint16 label.  After every poisoned call `fill()` asserts from the hook's counters that blocks were filled: a case
that allocates nothing under the hook fails instead of passing for nothing.  The oracle's answer is computed once per case
(`once`) and shared by both bytes."""
import numpy as np
import pytest

import align_cases as ac
from blockmatch_cases import BlockOracle, cpu_refine_intensity, lattice_numpy, same_field, same_report
from blockmatch_ncc_cases import NccOracle
from ccl_cases import CclOracle, pattern, planted, same_bits, same_records
from compose_cases import ComposeOracle
from edt_cases import NONE as EDT_NONE, EdtOracle, blocky_pair, oracle_records, sites
from field_cases import FieldOracle, sample_set
from fuse_cases import FuseOracle, leg, pair as fuse_pair, same_report as same_fuse_report, scenario
from fuse_search_cases import FuseSearchOracle, block_labels, fuse_planes, same_search_report, shifted_pair, warped_planes
from invert_cases import CONVERGED, DIVERGED, NOT_CONVERGED, InvertOracle, forward_field, oblique, state, written_inverse
from refine_cases import RefineOracle, interval, noisy_case
from resample_cases import ResampleOracle, about_centre, rot, special_volume
from test_gpu_align import _hough_case, _same as same_similarity
from test_gpu_blockmatch import pair as ssd_pair
from test_gpu_blockmatch_ncc import pair as ncc_pair
from test_gpu_ccl import same_report as same_clean_report
from test_gpu_compose import M1, M2, check_compose, setup as compose_setup
from test_gpu_edt import same_records as same_surface_records
from test_gpu_fuse import votes
from test_gpu_fuse_search import same_search
from test_gpu_invert import check_invert, check_jacobian, grids as invert_grids
from test_gpu_match_scale import TILE, PLAN_TILES, library_plan, plan_segments
from test_gpu_parity import _compare_records, _same_lists, vol_of
from test_gpu_refine import _same_refine, _sets, _transform
from test_gpu_resample import _same as same_resampled
from test_match import clustered

pytestmark = pytest.mark.gpu

FILLS = [pytest.param(0xFF, id="ff"), pytest.param(0x55, id="55")]


@pytest.fixture(params=FILLS)
def fill(built, request):
    """every allocation of the library inside the test holds the byte; fill() after a call asserts that the call's blocks were filled"""
    with built.alloc_fill(request.param) as stats:
        def filled():
            blocks, nbytes = stats()
            assert blocks > 0 and nbytes > 0, "nothing was allocated under the fill: the case checks nothing"
            return blocks, nbytes
        filled.byte = request.param
        yield filled


@pytest.fixture(scope="module")
def once():
    """once(key, make): the oracle's answer of a case, computed the first time and handed unchanged to both fill bytes"""
    memo = {}

    def get(key, make):
        if key not in memo:
            memo[key] = make()
        return memo[key]
    return get


def oracle_fixture(cls, name):
    @pytest.fixture(scope="module")
    def make(tmp_path_factory):
        return cls(tmp_path_factory.mktemp(name))
    return make


oc = oracle_fixture(CclOracle, "ccl_oracle")
ed = oracle_fixture(EdtOracle, "edt_oracle")
fz = oracle_fixture(FuseOracle, "fuse_oracle")
fs = oracle_fixture(FuseSearchOracle, "fuse_search_oracle")
ro = oracle_fixture(ResampleOracle, "resample_oracle")
fo = oracle_fixture(FieldOracle, "field_oracle")
bo = oracle_fixture(BlockOracle, "blockmatch_oracle")
no = oracle_fixture(NccOracle, "blockmatch_ncc_oracle")
io = oracle_fixture(InvertOracle, "invert_oracle")
co = oracle_fixture(ComposeOracle, "compose_oracle")
aorc = oracle_fixture(ac.AlignOracle, "align_oracle")
rorc = oracle_fixture(RefineOracle, "refine_oracle")


# ---- the switch ------------------------------------------------------------------------------------------------------------------------
def test_the_setter_proves_itself_and_counts(built):
    """sift3d_selftest_alloc_fill: its own 4 KiB probe holds the byte (else the wrapper raises) and is not counted; a call's blocks are
    counted once and the counters start again with every read; off means off"""
    v = pattern((5, 9, 33), "blocky")
    with built.alloc_fill(0xA7) as stats:
        assert stats() == (0, 0)
        built.label_components(v, 6)
        blocks, nbytes = stats()
        assert blocks >= 7 and nbytes >= 8 * v.size     # the seven buffers of the component pass; its labels and parents alone are 8 bytes a voxel
        assert stats() == (0, 0)
    built.label_components(v, 6)
    with built.alloc_fill(0x00) as stats:               # 0 is a byte like any other
        assert stats() == (0, 0)
    for bad in (-2, 256):
        assert built.hip_lib().sift3d_selftest_alloc_fill(bad, None) != 0
    with pytest.raises(ValueError):
        with built.alloc_fill(-1):
            pass


# ---- components and cleaning (ccl_api.hip) ---------------------------------------------------------------------------------------------
# (11, 19, 70): several bricks each way; (5, 9, 33): 1485 voxels, no multiple of 64 -- the last word of the `valid` bit plane reaches past n
@pytest.mark.parametrize("shape", [(11, 19, 70), (5, 9, 33)])
def test_components_under_the_fill(built, oc, once, fill, shape):
    v = pattern(shape, "random5")
    assert v.size % 64 != 0
    for conn in (6, 26):
        want_comp, want_rec = once(("label", shape, conn), lambda: oc.label(v, conn))
        comp, rec = built.label_components(v, conn)
        fill()
        assert np.array_equal(comp, want_comp), (conn, int((comp != want_comp).sum()))
        same_records(rec, want_rec)
    assert len(want_rec) > 50


@pytest.mark.parametrize("shape", [(11, 19, 70), (5, 9, 33)])
def test_cleaning_under_the_fill(built, oc, once, fill, shape):
    """min_voxels 8, rounds 4 on five random labels: under 6 all four rounds run (6207, 1161, 19 and 0 small components at 11 x 19 x
    70).  The vote table is allocated by the first round that has small components, regrown only by a round that has more of them
    than any before, and cleared by each round over the bytes that round reads; d_size and d_counts are cleared per round too"""
    v = pattern(shape, "random5")
    for conn in (6, 26):
        want, want_rep = once(("clean", shape, conn), lambda: oc.clean(v, 8, conn, 4))
        out, rep = built.clean_labels(v, min_voxels=8, connectivity=conn, rounds=4)
        fill()
        same_bits(out, want)
        same_clean_report(rep, want_rep)
    assert want_rep["rounds_run"] >= 2 and want_rep["total"]["resolved"] > 0


@pytest.mark.parametrize("name", ["nested", "walled_nan"])
def test_planted_cleaning_under_the_fill(built, oc, once, fill, name):
    v, kw = planted()[name]
    want, want_rep = once(("planted", name), lambda: oc.clean(v, **kw))
    out, rep = built.clean_labels(v, **kw)
    fill()
    same_bits(out, want)
    same_clean_report(rep, want_rep)


# ---- distance map and surface distances (edt_api.hip) ----------------------------------------------------------------------------------
SPACING = (700, 1300, 3000)


@pytest.mark.parametrize("name", ["none", "random1"])
@pytest.mark.parametrize("shape", [(11, 19, 70), (3, 5, 65)])
def test_distance_map_under_the_fill(built, ed, once, fill, shape, name):
    s = sites(shape, name)
    want = once(("map", shape, name), lambda: ed.map(s, SPACING))
    got = built.distance_map(s, SPACING)
    fill()
    assert got.dtype == np.uint64 and np.array_equal(got, want), int((got != want).sum())
    assert (got == EDT_NONE).all() if name == "none" else (got == 0).sum() == s.sum()


def test_surface_distances_under_the_fill(built, ed, once, fill):
    """first_label 0: five labels in turn through one d_cnt, one cursor and one pair of lists; then labels that one volume lacks"""
    a, b = blocky_pair()
    want = once("surface", lambda: oracle_records(built, ed, a, b, SPACING, first_label=0))
    got = built.surface_distances(a, b, SPACING, first_label=0)
    fill()
    same_surface_records(got, want)
    assert [r["label"] for r in got] == [0, 1, 2, 7, 65535]
    a, b = blocky_pair(seed=6)
    a[a == 7] = 9
    b[2:5, 3:9, 10:30] = 12
    want = once("surface, one-sided", lambda: oracle_records(built, ed, a, b, (1000, 2000, 500)))
    got = built.surface_distances(a, b, (1000, 2000, 500))
    fill()
    same_surface_records(got, want)
    assert sorted(r["label"] for r in got) == [1, 2, 7, 9, 12, 65535]


# ---- fusion (fuse_api.hip) -------------------------------------------------------------------------------------------------------------
W_RANGE = (np.float32(-900.0), np.float32(1300.0))


@pytest.mark.parametrize("metric", ["ssd", "ncc"])
def test_fuse_weights_under_the_fill(built, fz, once, fill, metric):
    T, W = fuse_pair((5, 9, 33), 9, holes=True)
    for rng in (None, W_RANGE):
        want = once(("weights", metric, rng is None), lambda: fz.weights(T, W, 2, metric, w_range=rng))
        got = built.fuse_weights(T, W, block=2, metric=metric, w_range=rng)
        fill()
        assert got.dtype == np.uint16 and np.array_equal(got, want)
    assert want.max() > 0


@pytest.mark.parametrize("metric", ["ssd", "ncc"])
def test_fuse_search_under_the_fill(built, fs, once, fill, metric):
    """W quantised with its own or the target's range, with a given range, and -- a W of NaN alone under the correlation -- with none:
    the one conditional fill of the file"""
    shape = (5, 9, 33)
    T, W = shifted_pair(shape, 9, (-1, 1, 2), holes=True)
    labels = block_labels(shape, 4)
    nan = np.full(shape, np.nan, np.float32)
    for key, w, lab, rng in (("own", W, labels, None), ("given", W, labels, W_RANGE), ("no labels", W, None, None), ("nan", nan, labels, None)):
        want = once(("search", metric, key), lambda: fs.search(T, w, lab, 2, 2, metric, w_range=rng))
        got = built.fuse_search(T, w, lab, block=2, radius=2, metric=metric, w_range=rng)
        fill()
        same_search(got, want)


def test_fuse_vote_under_the_fill(built, fz, once, fill):
    u, labels = votes(3, 3001, 3)
    for power in (0, 2):
        want = once(("vote", power), lambda: fz.vote(u, labels, power))
        got = built.fuse_vote(u, labels, power=power)
        fill()
        assert np.array_equal(got, want)


@pytest.fixture(scope="module")
def fuse_scen(built, ro, tmp_path_factory):
    return scenario(built, ro, tmp_path_factory.mktemp("fuse_scenario"))


@pytest.fixture(scope="module")
def fuse_planes_of(built, fs, ro, fo, fuse_scen):
    """the scenario's warped planes by the resampling and field oracles, once"""
    memo = {}

    def get(metric):
        if metric not in memo:
            memo[metric] = warped_planes(built, fs, ro, fo, fuse_scen["target"], leg(fuse_scen, metric), fuse_scen["vox2key"], metric)
        return memo[metric]
    return get


@pytest.mark.parametrize("search", [0, 2])
def test_fuse_stage_under_the_fill(built, fs, once, fill, fuse_scen, fuse_planes_of, search):
    """the five-atlas scenario (40^3, the family's smallest) under the correlation: the stage's restatement on the oracles' planes"""
    want, want_rep = once(("stage", search), lambda: fuse_planes(fs, *fuse_planes_of("ncc"), block=2, metric="ncc", power=2, search=search))
    words, rep = built.fuse_labels(fuse_scen["target"], leg(fuse_scen, "ncc"), fuse_scen["vox2key"], search=search, metric="ncc", power=2)
    fill()
    assert np.array_equal(words, want)
    same_fuse_report(rep, want_rep)
    if search:
        same_search_report(rep, want_rep)
        assert sum(a["moved"] for a in want_rep["search"]["atlas"]) > 0


# ---- block matching (blockmatch_api.hip) -----------------------------------------------------------------------------------------------
# (b, r) = (4, 3): the form with b and r at compile time; (6, 4): the form for any b, r.  37 x 21 x 50: no multiple of the brick
@pytest.mark.parametrize("kind", ["random", "constant"])
@pytest.mark.parametrize("b,r,stride", [(4, 3, 4), (6, 4, 7)])
def test_block_match_under_the_fill(built, bo, no, once, fill, kind, b, r, stride):
    shape = (50, 21, 37)
    first, count = lattice_numpy(shape, stride, b, r)
    for metric, oracle, make, match in (("ssd", bo, ssd_pair, built.block_match), ("ncc", no, ncc_pair, built.block_match_ncc)):
        F, W = make(kind, shape, 3)
        want = once(("match", metric, kind, b, r), lambda: oracle.match(F, W, first, stride, count, b, r))
        got = match(F, W, first, stride, count, b, r)
        fill()
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (metric, np.argwhere((got != want).any(-1))[:5])


def test_intensity_refinement_under_the_fill(built, bo, fo, once, fill):
    """one round of sift3d_refine_field_intensity (d_words, d_nodes) on a smooth pair moved by up to two voxels, from no field"""
    V, M = ssd_pair("smooth", (40, 44, 48), 11)
    T4 = np.eye(4, dtype=np.float32)
    want, want_rep = once("intensity", lambda: cpu_refine_intensity(built, bo, fo, V, M, T4, None, None, None, rounds=1))
    got, rep = built.refine_field_intensity(V, M, T4, None, None, None, rounds=1)
    fill()
    same_report(rep, want_rep)
    same_field(got, want)
    assert want_rep["rounds"] == 1 and want_rep["round"][0]["kept"] > 20


# ---- field fit and warp (field_api.hip) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,R", [("clustered", 200, 4.0), ("random", 3, 20.0), ("random", 0, 20.0)])
def test_field_fit_under_the_fill(built, fo, once, fill, kind, n, R):
    """six clusters at radius = spacing leave most cells of the sample index and most nodes without a sample; three samples; none"""
    y, v = sample_set(kind, 17 + n, n)
    got = built.fit_field(y, v, spacing=4.0, radius=R, lam=0.1)
    fill()
    want = once(("fit", kind, n), lambda: fo.fit(y, v, got, R, 0.1))
    assert got["n"] == want["n"] and got["disp"].tobytes() == want["disp"].tobytes()
    if n == 200:
        assert (want["disp"] == 0).all(0).mean() > 0.5 and (want["disp"] != 0).any()


@pytest.mark.parametrize("interp", ["linear", "nearest"])
def test_field_warp_under_the_fill(built, fo, once, fill, interp):
    shape, out_shape = (37, 5, 129), (34, 2, 126)
    rng = np.random.default_rng(sum(shape))
    vol = special_volume(shape, 1)
    A = about_centre(rot((1, 2, 3), 17.0), shape, out_shape, shift=(0.5, -0.75, 1.0))
    fv = built.key_vox2key((1.0, 1.0, 1.0))
    n = tuple(int(x) for x in (np.array(out_shape[::-1]) // 4 + 4))
    disp = rng.uniform(-3, 3, (3,) + n[::-1]).astype(np.float32)
    disp.reshape(-1)[rng.choice(disp.size, disp.size // 30, replace=False)] = np.nan
    field = {"n": n, "origin": np.array([-6.0, -5.5, -7.25], np.float32), "spacing": np.float32(4.0), "disp": disp}
    Cm, K = built.field_warp_terms(fv, fv)
    want = once(("warp", interp), lambda: fo.warp(vol, out_shape, A, Cm, K, field, interp, np.nan))
    got = built.resample_field(vol, out_shape, A, field, fv, fv, interp, np.nan)
    fill()
    assert np.array_equal(got, want, equal_nan=True) and np.isfinite(want).any()


# ---- inversion and Jacobian (invert_api.hip) -------------------------------------------------------------------------------------------
def test_inversion_under_the_fill(built, io, fill, tmp_path):
    """the rough field at spacing 1 (test_invert_kernel_cpu_cases' "random") with a few NaN nodes: its nodes stop converged, not
    converged and diverged, and d_status and d_res are read back whole"""
    m = oblique()
    m_inv = written_inverse(built, m, tmp_path)
    fwd, inv = invert_grids(built, m, 1.0)
    field = forward_field("random", fwd, seed=3, amp=6.0)
    field["disp"] = field["disp"].copy()
    rng = np.random.default_rng(1)
    for c in range(3):
        field["disp"][c][tuple(rng.integers(1, n - 1, 5) for n in fwd["n"][::-1])] = np.nan
    _, st, _ = check_invert(built, io, m, m_inv, field, inv)
    fill()
    s = state(st)
    assert (s == CONVERGED).any() and (s == NOT_CONVERGED).any() and (s == DIVERGED).any()
    check_invert(built, io, m, m_inv, None, inv)    # without a forward field: no node buffer
    fill()


@pytest.mark.parametrize("kind", ["nan", "none"])
def test_jacobian_under_the_fill(built, io, fill, kind):
    """both forms (and the library's own choice) at 37 x 5 x 129: rows cut in x"""
    shape = (129, 5, 37)
    A = built.resample_map(oblique(), None, None)
    field = None
    if kind == "nan":
        corners = np.array([[x, y, z] for x in (0, shape[2] - 1) for y in (0, shape[1] - 1) for z in (0, shape[0] - 1)], np.float32)
        grid = built.field_size(corners, spacing=4.0, radius=3.0)
        field = forward_field("random", grid, seed=2, amp=1.5)
        rng = np.random.default_rng(3)
        for c in range(3):
            field["disp"][c][tuple(rng.integers(0, n, 4) for n in grid["n"][::-1])] = np.nan
    J = check_jacobian(built, io, shape, A, None, None, field)
    fill()
    assert np.isfinite(J).any() and (kind == "none" or np.isnan(J).any())


# ---- composition (compose_api.hip) -----------------------------------------------------------------------------------------------------
def test_composition_under_the_fill(built, co, fill, tmp_path):
    """check_compose runs the node kernel with the residual (d_w4, d_res) and without; a cut grid with random fields, and none"""
    mr, _, g1, g2 = compose_setup(built, tmp_path, 4.0)
    f1, f2 = forward_field("random", g1, seed=1, amp=1.0), forward_field("random", g2, seed=2, amp=1.0)
    grid = {"n": (9, 7, 5), "origin": np.array([3.25, 1.5, 7.0], np.float32), "spacing": np.float32(2.5)}
    w, st, r2 = check_compose(built, co, M1, M2, mr, f1, f2, grid)
    fill()
    assert (w != 0).all() and (r2 > 0).all()
    check_compose(built, co, M1, M2, mr, None, None, grid)
    fill()


# ---- ratio matching and Hough (align_api.hip) ------------------------------------------------------------------------------------------
def test_ratio_and_hough_under_the_fill(built, aorc, once, fill):
    """record sets from 512 true pairs: the ratio search, the Hough transform of 512 correspondences (d_counts, d_flags, d_hyp), the
    whole of MatchKeys; and correspondences whose scales are all zero, where every hypothesis is degenerate and none wins"""
    fixed, moving, *_ = ac.recovery_case(11, n=512)
    want = once("ratio", lambda: aorc.ratio(fixed, moving))
    got = built.match_ratio(fixed, moving)[:4]
    fill()
    for g, w, name in zip(got, want[:4], ("i1", "d1", "i2", "d2")):
        assert (g == w).all(), name
    want = once("keys", lambda: aorc.match_keys(fixed, moving))
    same_similarity(built.match_keys(fixed, moving), want)
    fill()
    assert want["winner"] >= 0 and want["inliers"] > 100
    args = _hough_case(512, 512)
    none = args[:2] + (np.zeros_like(args[2]),) + args[3:]
    for key, a in (("hough", args), ("hough, no winner", none)):
        want = once(key, lambda: aorc.hough(*a))
        got = built.hough_similarity(*a)
        fill()
        assert (got["counts"] == want["counts"]).all() and got["winner"] == want["winner"] and (got["flags"] == want["flags"]).all()
        assert got["rot"].tobytes() == want["rot"].tobytes() and got["scale"].tobytes() == want["scale"].tobytes()
        assert (want["winner"] >= 0) == (key == "hough") and ((want["counts"] == -1).all() == (key != "hough"))


# ---- guided search and refinement (refine_api.hip) -------------------------------------------------------------------------------------
def test_guided_search_under_the_fill(built, rorc, once, fill):
    f, m = _sets("clustered", 3)
    t = _transform(3)
    lo, hi = interval()
    want = once("guided", lambda: rorc.search(f, m, t, 4.0, lo, hi))
    for cells_max in (None, 1):                          # the dense cell table and the sorted keys
        got = built.guided_search(f, m, t, 4.0, index_cells_max=cells_max)
        fill()
        for name, g, w in zip(("i1", "d1", "i2", "d2"), got[:4], want):
            assert np.array_equal(g, w), (name, cells_max)
        assert (got[4] >= 0).all() and (got[4][want[2] >= 0] >= 2).all()
    assert (want[2] >= 0).sum() > len(m) // 4


def test_refinement_under_the_fill(built, aorc, rorc, once, fill):
    """the loop from the oracle's Hough transform, at the one radius the loop starts from"""
    f, m, *_ = noisy_case(4, n=600)
    init = once("refine init", lambda: aorc.match_keys(f, m))
    got, rep = built.refine_similarity(f, m, init)
    fill()
    want = _same_refine(built, got, rep, f, m, init, rorc)
    assert want["rounds"] >= 1


# ---- resampling (resample_api.hip) -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["linear", "nearest"])
def test_resampling_under_the_fill(built, ro, once, fill, mode):
    """130 x 67 x 33 onto 141 x 70 x 40: rows of 141, no multiple of 4, so the last store of a row is a cut one"""
    src, out = (33, 67, 130), (40, 70, 141)
    vol = special_volume(src, 11)
    A = about_centre(1.1 * rot((-3, 1, 0.5), 47.0), src, out, (-0.4, 0.25, 0.0))
    want = once(("resample", mode), lambda: ro.resample(vol, out, A, mode, -7.0))
    got = built.resample_affine(vol, out, A, mode, -7.0)
    fill()
    same_resampled(got, want)
    assert (want == -7.0).any() and (want != -7.0).any()


# ---- knn (match_api.hip) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 17])
def test_knn_under_the_fill(built, oracle, once, fill, k):
    """100 queries over the last database with one segment and the first with two (sift3d_knn_plan): the partial lists of the
    segments (d_pd, d_pi) and their merge"""
    below = TILE * (PLAN_TILES * 2 - 1)
    pool = once("knn pool", lambda: clustered(np.random.default_rng(600), below + 1, 53, 4))
    q = once("knn queries", lambda: np.concatenate([pool[np.random.default_rng(601).integers(0, below, 50)], clustered(np.random.default_rng(602), 50, 53, 4)]))
    for n_db, segments in ((below, 1), (below + 1, 2)):
        assert plan_segments(n_db, len(q)) == segments == library_plan(built, n_db, len(q))
        wi, wd = once(("knn", n_db, k), lambda: oracle.knn64(pool[:n_db], q, k))
        gi, gd, _ = built.knn64(pool[:n_db], q, k)
        fill()
        assert np.array_equal(gi, wi) and np.array_equal(gd, wd), (n_db, k)


# ---- the pipeline context (api_context.hip, api_pipeline.hip, api_ops.hip, kernels_extrema.hip) ------------------------------------------
@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("dims,seed,scale", [((50, 47, 45), 8, 0.5), ((64, 64, 64), 12345, 1.0)])
def test_fresh_context_extracts_under_the_fill(built, oracle, once, fill, dims, seed, scale, mode):
    """a context created under the fill: sift3d_create clears the level buffers and the sampler tokens and leaves T[], the lists and
    the counter words as they come; (50, 47, 45) has pitched rows whose pad columns are read as zeros"""
    vol = vol_of(built, dims, seed)
    want = once(("extract", dims, mode), lambda: oracle.extract(vol, init_scale=scale, desc_mode=mode)[0])
    with built.Context(*dims) as ctx:
        fill()
        ctx.set_volume(vol)
        got = ctx.extract(initial_image_scale=scale, desc_mode=mode)
        again = ctx.extract(initial_image_scale=scale, desc_mode=mode)
    fill()                                               # the per-keypoint buffers are allocated by the first extraction
    assert len(want) > 5 and _compare_records(got, want), "float fields are within 1e-4 but not bit-identical"
    assert again.tobytes() == got.tobytes()


def test_dense_noise_regrows_the_lists_under_the_fill(built, oracle, once, fill):
    """test_extrema_dense_noise_grows_capacity's white noise at 144^3.  Extrema among the 53 voxels of two levels are 2 / 54 of the
    142^3 interior voxels, 106 000 +- 330, and the candidate lists of a 144^3 context hold 144^3 / 32 + 8192 = 101 504: the lists
    are regrown (at 128^3 the two numbers are 74 088 and 73 728, within a standard deviation and a half: not a size to rely on),
    and before that the own-level list overflows its segments and the launches are replayed.  With three levels nothing regrows."""
    n = 144
    rng = np.random.default_rng(3)
    D = [rng.standard_normal((n, n, n)).astype(np.float32) for _ in range(3)]
    want2 = once("noise 2", lambda: oracle.detect(D[0], D[1]))
    want3 = once("noise 3", lambda: oracle.detect3(D[0], D[1], D[2]))
    assert len(want2[0]) + len(want2[1]) > n ** 3 // 32 + 8192 > len(want3[0]) + len(want3[1])
    with built.Context(n, n, n) as ctx:
        blocks0, _ = fill()
        mins, maxs = ctx.extrema(D[0], D[1], None, capacity=n ** 3 // 16)
        blocks1, _ = fill()
        assert blocks1 >= 5                              # two key lists, two value lists and the sort's scratch, allocated anew
        _same_lists(mins, want2[0])
        _same_lists(maxs, want2[1])
        mins, maxs = ctx.extrema(D[0], D[1], D[2], capacity=n ** 3 // 16)
        _same_lists(mins, want3[0])
        _same_lists(maxs, want3[1])


@pytest.mark.parametrize("knob,values", [("TUNE_TINY_OCTAVE", (0, 1)), ("TUNE_LAZY_LEVELS", (0, 1)), ("TUNE_BLUR_FUSED", (0, 2))])
def test_knobs_on_both_sides_under_the_fill(built, oracle, once, fill, knob, values):
    """one volume, a fresh context per setting: the single-workgroup octave kernel or the passes, levels evaluated around the extrema
    or stored, the one-launch blur wherever it takes the shape or nowhere (the pass intermediates T[] are never cleared)"""
    dims = (88, 61, 47)
    vol = vol_of(built, dims, 13)
    want = once("knobs", lambda: oracle.extract(vol)[0])
    assert len(want) > 20
    for value in values:
        with built.Context(*dims) as ctx:
            ctx.set_tuning(getattr(built, knob), value)
            ctx.set_volume(vol)
            got = ctx.extract()
        fill()
        assert _compare_records(got, want), (knob, value)


# ---- the slab driver (zslab_driver.hip) ------------------------------------------------------------------------------------------------
def test_slab_driver_twice_through_one_handle_under_the_fill(built, fill):
    """the first run allocates beside the arena, the second cuts its pieces from the arena the first one sized -- filled like new
    blocks.  Against the single-device bytes, which test_fresh_context_extracts_under_the_fill ties to the oracle."""
    dims = (96, 80, 160)
    vol = vol_of(built, dims, 7)
    with built.Context(*dims) as ctx:
        ctx.set_volume(vol)
        want = ctx.extract()
    fill()
    assert len(want) > 50
    with built.ZSlab(dims[0], dims[1], dims[2], [0, 0]) as h:
        fill()
        for run in range(2):
            got, st = h.extract(vol)
            _, nbytes = fill()
            assert got.tobytes() == want.tobytes(), run
            assert st["n_ranks"] == 2 and st["sharded_octaves"] >= 1
            assert nbytes > 4 * vol.size                 # the level buffers of both ranks: more than the volume itself
