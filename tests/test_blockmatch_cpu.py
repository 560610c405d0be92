"""CPU suite: the intensity refinement of DESIGN.md section 7f without a GPU -- the block search oracle against a numpy
restatement (at b = 6 also where the costs pass 2^31), planted translations, ties, flags, the quantiser at half-way values and
over the widest and the narrowest range; the host helpers (range, lattice, grid, gates, sub-voxel step, samples, folds)
against hand-made words; and the nonrigid scenario of section 7e refined on the CPU."""
import numpy as np
import pytest

from blockmatch_cases import (NONE, SUM_MAX_B6, WORDS, BlockOracle, cpu_refine_intensity, ends_lattice, ends_pair, half_way_values, lattice3, lattice_numpy,
                              match_numpy, probe_read, quantiser_probe, quantize_numpy, scenario_score, scenario_setup, shifts, stripes, volume)
from field_cases import FieldOracle


@pytest.fixture(scope="module")
def bo(tmp_path_factory):
    return BlockOracle(tmp_path_factory.mktemp("blockmatch_oracle"))


@pytest.fixture(scope="module")
def fo(tmp_path_factory):
    return FieldOracle(tmp_path_factory.mktemp("field_oracle"))


ENDS = ["speckled", "straddling", "solid", "bright"]   # blockmatch_cases.ends_pair: volumes of 0 and 1 alone, at the ends of the integer sums


@pytest.mark.parametrize("kind", ["random", "smooth", "constant"] + ENDS)
@pytest.mark.parametrize("b,r,stride", [(1, 1, 1), (1, 3, 4), (4, 1, 5), (4, 3, 1), (4, 3, 4), (4, 3, 5), (6, 1, 1), (6, 4, 3)])
def test_oracle_equals_numpy(built, bo, kind, b, r, stride):
    """The int64 restatement cannot wrap, so it settles what the words are where the sums pass 2^31: at b = 6 on the volumes of 0
    and 1 alone, on 26 x 27 x 29 (the 21^3 window of (6, 4) does not fit the smaller volume)."""
    shape = (19, 17, 24) if b < 6 else (26, 27, 29)   # (nz, ny, nx)
    if kind in ENDS:
        F, W = ends_pair(kind, shape, 11)
    else:
        F = volume(kind, shape, 11)
        W = np.roll(F, (1, 0, -1), (0, 1, 2)) + (0 if kind == "constant" else np.random.default_rng(2).normal(0, 1.0, shape).astype(np.float32))
    lo, hi = bo.range(F)
    assert (lo, hi) == built.blockmatch_range(F) == (F.min(), F.max())
    qf, qw = bo.quantize(F, lo, hi), bo.quantize(W, lo, hi)
    assert (qf == quantize_numpy(F, lo, hi)).all() and (qw == quantize_numpy(W, lo, hi)).all()
    assert qf.min() == 0 and qf.max() == 1023 and qw.min() >= 0 and qw.max() <= 1023
    if kind in ENDS:
        assert set(np.unique(qf)) == {0, 1023} and set(np.unique(qw)) == {0, 1023}
    first, count = lattice_numpy(shape, stride, b, r)
    assert (first, count) == built.blockmatch_lattice(shape, stride=stride, block=b, search=r)
    # one node more on every side: those leave the volume and are flagged
    first, count = tuple(f - stride for f in first), tuple(c + 2 for c in count)
    got, want = bo.match_q(qf, qw, first, stride, count, b, r), match_numpy(qf, qw, first, stride, count, b, r)
    assert got.tobytes() == want.tobytes()
    inner = got[1:-1, 1:-1, 1:-1]
    assert (inner[..., 3] == 0).all() and (got[..., 3] != 0).sum() == got[..., 3].size - inner[..., 3].size
    assert (got[got[..., 3] != 0] == np.eye(WORDS, dtype=np.uint32)[3]).all()
    # the ends: what test_gpu_integer_ends.py relies on, asserted on the oracle's words
    top = (2 * b + 1) ** 3 * 1023 ** 2
    if kind == "speckled":
        print("speckled b %d r %d: least cost %d .. %d of at most %d" % (b, r, inner[..., 4].min(), inner[..., 4].max(), top))
        assert len(np.unique(inner[..., 4])) > 1                  # the costs vary from node to node
        if b == 6:
            assert inner[..., 4].min() >= 2 ** 31 and top == SUM_MAX_B6 < 2 ** 32
    if kind == "straddling" and b == 6:   # within one node, costs below and beyond 2^31: a signed compare of two costs or keys would show
        both = (inner[..., 4] < 2 ** 31) & (np.where(inner[..., 5:12] == NONE, 0, inner[..., 5:12]).max(-1) >= 2 ** 31)
        print("straddling b %d r %d: least cost %d .. %d, a cost on either side of 2^31 at %.3f of the nodes" % (b, r, inner[..., 4].min(), inner[..., 4].max(), both.mean()))
        assert both.mean() > 0.25           # the record shows 8 of the (2r + 1)^3 costs: a quarter of the nodes is plenty
    if kind == "bright":
        print("bright b %d r %d: Sf2 %d .. %d" % (b, r, inner[..., 13].min(), inner[..., 13].max()))
        if b == 6:
            assert inner[..., 13].min() >= 2 ** 31
    if kind == "solid":   # where no window reaches W's corner voxel every cost is the largest there is, and the zero shift wins
        f1, c1 = ends_lattice(kind, shape, stride, b, r)
        w = bo.match_q(qf, qw, f1, stride, c1, b, r)
        assert (w[..., 3] == 0).all() and (shifts(w) == 0).all() and (w[..., 4:12] == top).all()
        assert (w[..., 12:14] == 0).all() and w.tobytes() == match_numpy(qf, qw, f1, stride, c1, b, r).tobytes()


@pytest.mark.parametrize("b,r", [(1, 1), (4, 3), (6, 1)])
def test_ties_between_unit_shifts_go_to_the_least_z_then_y_then_x(bo, b, r):
    """the checkerboard against its complement: the six unit shifts all cost 0, the zero shift the most, and s_z = -1 wins (least z
    first); stripes along one axis: only -1 and +1 along it tie, and -1 wins.  Every node's window lies inside the volume, so
    there is no face here at which -1 could be missing: the fusion search has those (test_fuse_search_cpu.py)."""
    shape = (17, 18, 19)
    first, count = lattice_numpy(shape, 1, b, r)
    top = (2 * b + 1) ** 3 * 1023 ** 2
    F, W = lattice3(shape)
    w = bo.match(F, W, first, 1, count, b, r)
    assert w.tobytes() == match_numpy(bo.quantize(F, 0, 1), bo.quantize(W, 0, 1), first, 1, count, b, r).tobytes()
    assert (w[..., 3] == 0).all() and (shifts(w) == np.array((0, 0, -1), np.int32)).all() and (w[..., 4] == 0).all() and (w[..., 5] == top).all()
    for axis in (0, 1, 2):
        F, W = stripes(shape, axis)
        w = bo.match(F, W, first, 1, count, b, r)
        want = np.zeros(3, np.int32)
        want[2 - axis] = -1                              # the words hold (x, y, z)
        assert (w[..., 3] == 0).all() and (shifts(w) == want).all() and (w[..., 4] == 0).all() and (w[..., 5] == top).all()


# ---- the quantiser ---------------------------------------------------------------------------------------------------------------
def test_quantiser_at_half_way_values_the_ends_and_the_widest_range(bo):
    v = half_way_values()
    vol, first, count = quantiser_probe(v, 0.0, 1023.0)
    assert bo.range(vol) == (np.float32(0.0), np.float32(1023.0))
    q = bo.quantize(v, 0.0, 1023.0)
    assert np.array_equal(q, quantize_numpy(v, 0.0, 1023.0))
    assert np.array_equal(q[:1023], 2 * ((np.arange(1023) + 1) // 2)) and q[-6:].tolist() == [0, 1023, 0, 0, 0, 1023]   # ties to even
    w = bo.match(vol, vol, first, 3, count, 1, 1)
    assert (w[..., 3] == 0).all() and np.array_equal(probe_read(w, len(v), 12), q) and np.array_equal(probe_read(w, len(v), 13), q)
    # a range wider than a float holds: hi - lo overflows in float and not in double
    lo, hi = np.float32(-3.0e38), np.float32(3.0e38)
    v = np.array([3.4028235e38, -3.4028235e38, 1e38, -1e38, 0.0, 3.0e38, -3.0e38], np.float32)
    q = bo.quantize(v, lo, hi)
    assert np.array_equal(q, quantize_numpy(v, lo, hi)) and q.tolist() == [1023, 0, 682, 341, 512, 1023, 0]
    Fv, first, count = quantiser_probe(np.full(len(v), lo, np.float32), lo, hi)
    Wv, _, _ = quantiser_probe(v, lo, hi)
    w = bo.match(Fv, Wv, first, 3, count, 1, 1)
    assert (w[..., 3] == 0).all() and np.array_equal(probe_read(w, len(v), 5), q)
    # a range one float ulp wide
    lo, hi = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))
    v = np.array([lo, hi, np.nextafter(lo, np.float32(0.0)), np.nextafter(hi, np.float32(2.0)), 0.5, 2.0, -3.4e38, 3.4e38], np.float32)
    q = bo.quantize(v, lo, hi)
    assert np.array_equal(q, quantize_numpy(v, lo, hi)) and q.tolist() == [0, 1023, 0, 1023, 0, 1023, 0, 1023]
    # outside a given range it clamps; what is not finite is -1
    v = np.array([-1.0, 0.0, 0.25, 0.75, 1.0, 2.0, np.nan, np.inf, -np.inf], np.float32)
    q = bo.quantize(v, 0.25, 0.75)
    assert np.array_equal(q, quantize_numpy(v, 0.25, 0.75)) and q.tolist() == [0, 0, 0, 1023, 1023, 1023, -1, -1, -1]


@pytest.mark.parametrize("s", [(0, 0, 0), (1, -2, 3), (-3, 3, -3), (2, 0, -1)])
def test_planted_translation_is_found(bo, s):
    """W(x + s) = F(x) on a textured volume: cost(s) = 0 at every node, and nowhere else"""
    F = volume("random", (30, 26, 28), 5)
    W = np.roll(F, s[::-1], (0, 1, 2))
    first, count = lattice_numpy(F.shape, 4, 4, 3)
    w = bo.match(F, W, first, 4, count, 4, 3)
    assert (w[..., 3] == 0).all() and (shifts(w) == np.array(s, np.int32)).all() and (w[..., 4] == 0).all()
    nb = w[..., 6:12]
    for k in range(3):   # a neighbour outside the search cube has no cost
        assert ((nb[..., 2 * k] == NONE) == (s[k] == -3)).all() and ((nb[..., 2 * k + 1] == NONE) == (s[k] == 3)).all()
    assert (nb[nb != NONE] > 0).all()


def test_ties_resolve_by_length_then_z_y_x(bo):
    F = volume("constant", (20, 20, 20), 0)
    first, count = lattice_numpy(F.shape, 1, 4, 3)
    w = bo.match(F, F, first, 1, count, 4, 3)
    assert (w[..., 3] == 0).all() and (shifts(w) == 0).all() and (w[..., 4:12] == 0).all()
    # two equal minima at s = (+1, 0, 0) and (0, 0, -1) (x, y, z): |s|^2 ties, the lower z wins; then (0, -1, 0) against (1, 0, 0): y
    qf = np.zeros((9, 9, 9), np.int16)
    qf[4, 4, 4] = 100
    for spots, want in ((((4, 4, 5), (3, 4, 4)), (0, 0, -1)), (((4, 3, 4), (4, 4, 5)), (0, -1, 0)), (((4, 4, 5), (4, 4, 3)), (-1, 0, 0)),
                        (((4, 4, 5), (4, 4, 2)), (1, 0, 0))):
        qw = np.zeros_like(qf)
        for z, y, x in spots:
            qw[z, y, x] = 100
        w = bo.match_q(qf, qw, (4, 4, 4), 1, (1, 1, 1), 1, 3)
        assert tuple(shifts(w)[0, 0, 0]) == want and w[0, 0, 0, 4] < w[0, 0, 0, 5]


def test_flags_border_and_non_finite_and_only_they(bo):
    rng = np.random.default_rng(8)
    shape = (24, 22, 26)
    F = volume("smooth", shape, 3)
    W = np.roll(F, 1, 2)
    for vol, bad in ((F, np.nan), (F, np.inf), (W, -np.inf), (W, np.nan)):
        vol[tuple(rng.integers(0, n) for n in shape)] = bad
    b, r, stride = 1, 3, 1
    first, count = (0, 0, 0), shape[::-1]
    w = bo.match(F, W, first, stride, count, b, r)
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    m = b + r
    want = (x < m) | (y < m) | (z < m) | (x > nx - 1 - m) | (y > ny - 1 - m) | (z > nz - 1 - m)
    for vol, reach in ((F, b), (W, m)):
        for bz, by, bx in np.argwhere(~np.isfinite(vol)):
            want |= (abs(x - bx) <= reach) & (abs(y - by) <= reach) & (abs(z - bz) <= reach)
    assert ((w[..., 3] != 0) == want).all() and 0 < (~want).sum()
    # a W outside F's range clamps, it does not flag
    w2 = bo.match(F, np.where(np.isfinite(W), W * 3.0, W), first, stride, count, b, r)
    assert ((w2[..., 3] != 0) == want).all()


def _words(n, **kw):
    w = np.zeros((n, WORDS), np.uint32)
    w[:, 4], w[:, 5] = 10, 100
    w[:, 6:12] = 50
    w[:, 12], w[:, 13] = 1000, 2000 + np.arange(n) * 1000   # variances ascending with the node index
    for k, v in kw.items():
        w[:, int(k[1:])] = v
    return w


def test_gates_subvoxel_and_samples(built):
    shape = (23, 23, 23)   # lattice 3 x 3 x 3 at the defaults
    first, count = built.blockmatch_lattice(shape)
    assert count == (3, 3, 3) and first == (7, 7, 7)
    n = 27
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = 2.0 * np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32)   # L = R^T / 2
    L = np.linalg.inv(T[:3, :3].astype(np.float64))
    fv = built.key_vox2key((1.0, 1.0, 1.0))
    # every gate in turn
    w = _words(n)
    w[0, 3] = 1                                      # flagged
    w[5, 0] = np.uint32(3)                           # |s| = r: border
    w[6, 2] = np.array(-3, np.int32).view(np.uint32)
    w[9, 0], w[9, 4], w[9, 5] = 1, 81, 100           # 81 < (double)0.8f * 100 fails
    w[10, 0], w[10, 4], w[10, 5] = 1, 80, 100        # passes: (double)0.8f = 0.800000011920929
    w[11, 4], w[11, 5] = 100, 100                    # zero shift passes whatever the costs
    y, v, counts = built.blockmatch_samples(w, shape, T, None, fv)
    # the variance threshold: 26 unflagged nodes, index floor(0.25 * 26) = 6 of the ascending variances -> nodes 1 .. 7 drop
    assert counts == (1, 7, 0, 1) and len(y) == 27 - 9
    # variance_quantile 0: only the least variance drops; then the border gate sees nodes 5 and 6
    y, v, counts = built.blockmatch_samples(w, shape, T, None, fv, variance_quantile=0.0)
    assert counts == (1, 1, 2, 1) and len(y) == 22
    kept = [i for i in range(2, 27) if i not in (5, 6, 9)]
    P = np.array([[7 + 4 * (i % 3), 7 + 4 * ((i // 3) % 3), 7 + 4 * (i // 9)] for i in kept], np.float64)
    assert np.array_equal(y, (P + 0.5).astype(np.float32))
    want = np.zeros((len(kept), 3))
    want[kept.index(10)] = L @ np.array([1.0, 0, 0])
    assert np.array_equal(v, want.astype(np.float32))
    # the sub-voxel step: d = 0.5 (c- - c+) / (c- - 2 c0 + c+), 0 where the denominator is not positive
    w = _words(n)
    w[:, 0], w[:, 4], w[:, 5] = 1, 10, 100
    w[:, 6], w[:, 7] = 30, 50          # x: 0.5 * (30 - 50) / (30 - 20 + 50) = -1/6
    w[:, 8], w[:, 9] = 10, 10          # y: denominator 0
    w[:, 10], w[:, 11] = 12, 10        # z: 0.5 * 2 / 2 = 0.5
    y, v, counts = built.blockmatch_samples(w, shape, T, None, fv, variance_quantile=0.0)
    D = np.array([1.0 - 1.0 / 6.0, 0.0, 0.5])
    assert np.array_equal(v, np.broadcast_to((L @ D).astype(np.float32), v.shape))
    # through an input field: v = v_in(key(p + D)) + L C D, and a zero shift returns the field's values at the nodes
    rng = np.random.default_rng(4)
    g = built.blockmatch_grid(shape, fv)
    field = dict(g, disp=rng.normal(0, 1.0, (3,) + g["n"][::-1]).astype(np.float32))
    y, v, _ = built.blockmatch_samples(w, shape, T, field, fv, variance_quantile=0.0)
    at = built.field_eval(field, (y.astype(np.float64) + D).astype(np.float32)).astype(np.float64)
    assert np.array_equal(v, (at + L @ D).astype(np.float32))
    y, v, _ = built.blockmatch_samples(_words(n), shape, T, field, fv, variance_quantile=0.0)
    assert np.array_equal(v, built.field_eval(field, y)) and np.abs(v).max() > 0
    # an anisotropic vox2key scales the shift: C D in key units
    fw = built.key_vox2key((1.0, 2.0, 4.0), np.diag([1.0, 2.0, 4.0, 1.0]).astype(np.float32))
    y, v, _ = built.blockmatch_samples(w, shape, np.eye(4, dtype=np.float32), None, fw, variance_quantile=0.0)
    assert np.allclose(v, fw[:3, :3].astype(np.float64) @ D, atol=1e-6)


def test_host_helpers_and_refusals(built):
    assert built.blockmatch_range(np.full((4, 4, 4), 2.0, np.float32)) is None
    assert built.blockmatch_range(np.full((4, 4, 4), np.nan, np.float32)) is None
    v = np.array([np.nan, 3.0, -np.inf, -2.0, np.inf], np.float32)
    assert built.blockmatch_range(v) == (np.float32(-2.0), np.float32(3.0))
    p = built.blockmatch_params()
    assert (p.stride, p.block, p.search, p.rounds, p.radius, p.spacing) == (4, 4, 3, 2, 20.0, 4.0)
    assert abs(p.variance_quantile - 0.25) < 1e-7 and abs(p.cost_fraction - 0.8) < 1e-7 and abs(p.lambda_ - 0.1) < 1e-7
    assert built.blockmatch_lattice((15, 15, 15)) == ((7, 7, 7), (1, 1, 1))
    for shape, kw in (((14, 15, 15), {}), ((15, 15, 15), dict(block=7)), ((15, 15, 15), dict(search=0)), ((15, 15, 15), dict(stride=0))):
        with pytest.raises(built.Sift3DError):
            built.blockmatch_lattice(shape, **kw)
    # the output grid covers the box: R past the corner voxels' keys
    g = built.blockmatch_grid((128, 100, 64))
    assert g["n"] == tuple(int(np.floor((n - 1 + 40.0) / 4.0)) + 2 for n in (64, 100, 128)) and (g["origin"] == -20.0).all()
    fv = built.key_vox2key((1.0, 1.0, 1.0))
    assert (built.blockmatch_grid((128, 100, 64), fv)["origin"] == -19.5).all()
    with pytest.raises(built.Sift3DError):
        built.blockmatch_grid((128, 128, 128), max_nodes=1000)
    # folds under a 4 x 4 equal sift3d_field_folds under the similarity it came from
    rng = np.random.default_rng(2)
    t = {"scale": 1.25, "rot": np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32), "trans": np.zeros(3, np.float32),
         "center0": np.zeros(3, np.float32), "center1": np.array([1, 2, 3], np.float32)}
    field = dict(built.blockmatch_grid((20, 20, 20)), disp=None)
    field["disp"] = rng.normal(0, 3.0, (3,) + field["n"][::-1]).astype(np.float32)
    try:
        a = built.field_folds(t, field)
    except Exception:   # a similarity dict of another shape: the 4 x 4 alone is checked
        a = None
    T4 = np.eye(4, dtype=np.float32)
    T4[:3, :3] = 1.25 * t["rot"]
    b = built.blockmatch_folds(T4, field)
    assert b[0] > 0 and (a is None or (a[0] == b[0] and a[1] == b[1]))


@pytest.mark.parametrize("world", [False, True])
def test_intensity_scenario_cpu(built, bo, fo, tmp_path, world):
    """The nonrigid scenario of section 7e refined on the CPU at the defaults (the keypoint field in, two rounds).  Asserted:
    RMS map error below 0.6 x the keypoint field's (-u, computed in this run), a smaller largest error, a higher correlation
    and no folded node.  Reached when this was written: voxel keys RMS 0.795 (0.43 x), largest 2.44, correlation 0.9945;
    -w keys 0.976 (0.34 x), 3.72, 0.9965.  Section 7e's own targets (RMS <= 0.75 voxel, <= 1.0 under -w; largest <= 2;
    correlation >= 0.98) are met for the correlation and for the RMS under -w, and missed for the RMS with voxel keys and for
    the largest error."""
    s = scenario_setup(built, tmp_path, world)
    field, rep = cpu_refine_intensity(built, bo, fo, s["V"], s["M"], s["T4"], s["parent"]["field_dict"], s["fv"], s["mv"])
    (c0, rms0, max0), (c1, rms1, max1) = s["parent"]["field"], scenario_score(built, fo, s, field)
    print("intensity%s: -u corr %.4f rms %.3f max %.3f; -i corr %.4f rms %.3f max %.3f; %s" % (" -w" if world else "", c0, rms0, max0, c1, rms1, max1,
                                                                                               rep["round"]))
    assert rep["rounds"] == 2 and rep["round"][1]["kept"] > 10000 and rep["round"][1]["folds"] == 0
    assert rms1 < 0.6 * rms0 and max1 < max0 and c1 > c0, (s["parent"]["field"], (c1, rms1, max1))
