"""CPU suite: the correlation cost of the block search without a GPU -- the oracle
tests/blockmatch_ncc_oracle.c against a numpy restatement and against hand-made sums, its exact invariance under a gain and an
offset of W, the planted translation that the SSD cost loses under an intensity remap and this cost does not, the degenerate
blocks, the flags, and the nonrigid scenario of section 7e refined on the CPU from a remapped moving volume."""
import numpy as np
import pytest

from blockmatch_cases import WORDS, binary as _binary, cpu_refine_intensity, ends_pair, lattice_numpy, scenario_score, scenario_setup, shifts, volume
from blockmatch_ncc_cases import FLAT, NccOracle, cost_python, cpu_refine_intensity_metric, match_numpy_ncc, remap
from field_cases import FieldOracle


@pytest.fixture(scope="module")
def no(tmp_path_factory):
    return NccOracle(tmp_path_factory.mktemp("blockmatch_ncc_oracle"))


@pytest.fixture(scope="module")
def fo(tmp_path_factory):
    return FieldOracle(tmp_path_factory.mktemp("field_oracle"))


ENDS = ["speckled", "solid", "bright"]   # blockmatch_cases.ends_pair: volumes of two values alone, W on a scale of its own


@pytest.mark.parametrize("kind", ["random", "smooth", "constant", "binary"] + ENDS)
@pytest.mark.parametrize("b,r,stride", [(1, 1, 1), (1, 3, 4), (4, 1, 5), (4, 3, 1), (4, 3, 4), (6, 1, 1), (6, 2, 3), (6, 4, 3)])
def test_oracle_equals_numpy(no, kind, b, r, stride):
    """The restatement's sums are int64 and its products Python integers: it settles the words where Sff, Sww and Sfw pass 2^31,
    which they do at b = 6 on the bright pair (the 21^3 window of (6, 4) takes the larger volume)."""
    shape = (19, 17, 24) if b + r < 10 else (26, 27, 29)   # (nz, ny, nx)
    if kind == "binary":
        qf, qw = _binary(shape, 7)
    elif kind in ENDS:
        F, W = ends_pair(kind, shape, 11, own_scale=True)
        qf, qw = no.quantize(F, *no.range(F)), no.quantize(W, *no.range(W))
        assert set(np.unique(qf)) == {0, 1023} and set(np.unique(qw)) == {0, 1023} and W.max() < -54.0
    else:
        F = volume(kind, shape, 11)
        W = 0.7 * np.roll(F, (1, 0, -1), (0, 1, 2)) + 40.0
        if kind != "constant":
            W = W + np.random.default_rng(2).normal(0, 1.0, shape)
        W = W.astype(np.float32)
        qf, qw = no.quantize(F, *no.range(F)), no.quantize(W, *no.range(W))
        assert qf.min() == 0 and qf.max() == 1023 and qw.min() == 0 and qw.max() == 1023
    first, count = lattice_numpy(shape, stride, b, r)
    # one node more on every side: those leave the volume and are flagged
    first, count = tuple(f - stride for f in first), tuple(c + 2 for c in count)
    got, want = no.match_q(qf, qw, first, stride, count, b, r), match_numpy_ncc(qf, qw, first, stride, count, b, r)
    assert got.tobytes() == want.tobytes()
    inner = got[1:-1, 1:-1, 1:-1]
    assert (inner[..., 3] == 0).all() and (got[..., 3] != 0).sum() == got[..., 3].size - inner[..., 3].size
    assert (got[got[..., 3] != 0] == np.eye(WORDS, dtype=np.uint32)[3]).all()
    assert (inner[..., 4:6] <= FLAT).all() and ((inner[..., 12] == 0).sum() == 0 or kind in ("speckled", "solid"))   # those two have blocks of 0 alone
    if kind == "solid":      # F's blocks are flat
        assert (shifts(inner) == 0).all() and (inner[..., 4:12] == FLAT).all() and (inner[..., 12:14] == 0).all()
    if kind == "bright":     # Sff beyond 2^31 (and with it Sww and Sfw of the matching shift), blocks that are not flat
        cost = inner[..., 4]
        print("bright b %d r %d: Sff %d .. %d, cost %d .. %d, at 2^31 %.3f, at 0 %.3f" % (b, r, inner[..., 13].min(), inner[..., 13].max(), cost.min(),
                                                                                      cost.max(), (cost == FLAT).mean(), (cost == 0).mean()))
        if b == 6:
            assert inner[..., 13].min() >= 2 ** 31
            assert ((cost > 0) & (cost < FLAT)).mean() > 0.5 and (cost == FLAT).mean() < 0.1
    if kind == "constant":   # every block is flat: every cost is 2^31 and the zero shift wins every tie
        assert (shifts(inner) == 0).all() and (inner[..., 4:6] == FLAT).all()


def test_cost_from_hand_made_sums(no):
    N = 13 ** 3
    q, h = 1023, 13 ** 3 // 2
    # identical blocks, half 0 and half 1023: A = Vf = Vw, the largest they get ((13^3 1023 / 2)^2, above 2^40); rho^2 = 1
    A = N * q * q * h - (q * h) ** 2
    assert 2 ** 40 < A < 2 ** 43
    assert no.cost(N, q * h, q * q * h, q * h, q * q * h, q * q * h) == 0
    # complementary blocks: A = -Vf; a flat F; a flat W; A = 0
    assert no.cost(N, q * h, q * q * h, q * (N - h), q * q * (N - h), 0) == FLAT
    assert no.cost(N, q * N, q * q * N, q * h, q * q * h, q * q * h) == FLAT
    assert no.cost(N, q * h, q * q * h, 5 * N, 25 * N, 5 * q * h) == FLAT
    assert no.cost(4, 2, 2, 2, 2, 1) == FLAT
    # rho^2 = 1/3; then random blocks and nearly equal ones
    assert no.cost(4, 2, 2, 3, 3, 2) == cost_python(4, 2, 2, 3, 3, 2) == round((1 - 1 / 3) * 2 ** 31)
    assert no.cost(4, 6, 14, 10, 30, 20) == cost_python(4, 6, 14, 10, 30, 20)
    rng = np.random.default_rng(3)
    for _ in range(20000):
        n = int(rng.integers(2, 14)) ** 3
        f, w = rng.integers(0, 1024, n).astype(np.int64), rng.integers(0, 1024, n).astype(np.int64)
        if rng.random() < 0.5:
            w = np.clip(f + rng.integers(-2, 3, n), 0, 1023)         # nearly equal blocks: costs near 0
        a = (n, int(f.sum()), int((f * f).sum()), int(w.sum()), int((w * w).sum()), int((f * w).sum()))
        assert no.cost(*a) == cost_python(*a), a


@pytest.mark.parametrize("g,o", [(0.5, 0.0), (4.0, -1024.0), (0.25, 4096.0), (2.0, 512.0)])
def test_gain_and_offset_change_nothing(no, g, o):
    """W integer-valued with its extremes kept, g and o powers of two: g W + o is exact in float32 and quantises to the same
    integers, so every word is the same"""
    rng = np.random.default_rng(12)
    shape = (24, 22, 26)
    F = volume("smooth", shape, 3)
    W = np.rint(np.roll(F, (1, -1, 2), (0, 1, 2)) + rng.normal(0, 20.0, shape)).astype(np.float32)
    W2 = (np.float32(g) * W + np.float32(o)).astype(np.float32)
    assert np.array_equal(W2.astype(np.float64), g * W.astype(np.float64) + o)
    assert (no.quantize(W, *no.range(W)) == no.quantize(W2, *no.range(W2))).all()
    first, count = lattice_numpy(shape, 3, 4, 3)
    a, b = no.match(F, W, first, 3, count, 4, 3), no.match(F, W2, first, 3, count, 4, 3)
    assert a.tobytes() == b.tobytes() and (a[..., 3] == 0).all() and len(np.unique(a[..., 4])) > 10
    # the SSD cost is not: its words change
    assert no.ssd.match(F, W, first, 3, count, 4, 3).tobytes() != no.ssd.match(F, W2, first, 3, count, 4, 3).tobytes()


@pytest.mark.parametrize("kind,exact", [("half", True), ("half_offset", True), ("bias", False)])
def test_planted_translation_survives_a_remap(no, kind, exact):
    """The gap section 7g closes: the 40^3 smooth volume, W = F translated by (2, -1, 1) with its intensities remapped.  The
    correlation cost finds the translation at all 125 nodes (with cost 0 under a gain and an offset); the SSD cost, which
    quantises W with F's range, at fewer than a quarter of them (5, 2 and 9 when this was written; under the bias the largest
    argmin cost of the correlation was 7 476 115 = 0.0035 x 2^31)."""
    F = volume("smooth", (40, 40, 40), 1)
    s = (2, -1, 1)
    W = remap(np.roll(F, s[::-1], (0, 1, 2)), kind)
    first, count = lattice_numpy(F.shape, 6, 4, 3)
    assert count == (5, 5, 5)
    wn, ws = no.match(F, W, first, 6, count, 4, 3), no.ssd.match(F, W, first, 6, count, 4, 3)
    right_n = int((shifts(wn) == np.array(s, np.int32)).all(-1).sum())
    right_s = int((shifts(ws) == np.array(s, np.int32)).all(-1).sum())
    print("%s: correlation right at %d / 125, largest argmin cost %d; SSD right at %d / 125" % (kind, right_n, wn[..., 4].max(), right_s))
    assert (wn[..., 3] == 0).all() and (ws[..., 3] == 0).all()
    assert right_n == 125
    assert right_s < 125 / 4
    if exact:
        assert (wn[..., 4] == 0).all()
    else:
        assert wn[..., 4].max() < 0.01 * FLAT
    # and with W's intensities as they were both costs find it everywhere
    W = np.roll(F, s[::-1], (0, 1, 2))
    for w in (no.match(F, W, first, 6, count, 4, 3), no.ssd.match(F, W, first, 6, count, 4, 3)):
        assert (shifts(w) == np.array(s, np.int32)).all() and (w[..., 4] == 0).all()


def test_degenerate_blocks_cost_2_31_and_the_zero_shift_wins(built, no):
    shape = (23, 23, 23)   # lattice 3 x 3 x 3 at the defaults
    first, count = built.blockmatch_lattice(shape)
    assert count == (3, 3, 3) and first == (7, 7, 7)
    # anticorrelated: F a ramp, W = -F translated (a translated ramp is the ramp plus a constant): A < 0 at every shift
    z, y, x = np.meshgrid(*(np.arange(23.0),) * 3, indexing="ij")
    F = (3.0 * x + 5.0 * y + 7.0 * z).astype(np.float32)
    W = (-(3.0 * (x + 2) + 5.0 * (y - 1) + 7.0 * (z + 1))).astype(np.float32)
    w = no.match(F, W, first, 4, count, 4, 3)
    assert (w[..., 3] == 0).all() and (shifts(w) == 0).all() and (w[..., 4:12] == FLAT).all() and (w[..., 12:14] > 0).all()
    # the sign is what does it: against +F translated every shift correlates, to within the quantisation
    w = no.match(F, -W, first, 4, count, 4, 3)
    assert (w[..., 3] == 0).all() and (w[..., 4:12] < FLAT // 1000).all()
    # a flat F block (node 13, the middle one) and a flat W window (node 0)
    rng = np.random.default_rng(6)
    qf, qw = (rng.integers(0, 1024, shape).astype(np.int16) for _ in range(2))
    qf[11 - 4:11 + 5, 11 - 4:11 + 5, 11 - 4:11 + 5] = 400
    qw[:15, :15, :15] = 77
    w = no.match_q(qf, qw, first, 4, count, 4, 3).reshape(27, WORDS)
    for node in (13, 0):
        assert (w[node, :4] == 0).all() and (w[node, 4:12] == FLAT).all()
    assert w[13, 12] == 400 * 729 and w[13, 13] == 400 * 400 * 729 and 729 * int(w[0, 13]) > int(w[0, 12]) ** 2
    others = np.delete(w, (0, 13), 0)
    assert (others[:, 4] < FLAT).all()
    # the variance gate drops the flat F node (its variance, 0, is the least) and nothing else at quantile 0
    y_, v_, counts = built.blockmatch_samples(w, shape, np.eye(4, dtype=np.float32), None, None, variance_quantile=0.0)
    assert counts[0] == 0 and counts[1] == 1
    # the flat W node has a zero shift, which passes the cost gate, and a zero parabola step: a sample with v = 0
    assert np.array_equal(y_[0], np.array([7, 7, 7], np.float32)) and np.array_equal(v_[0], np.zeros(3, np.float32))


def test_flags_are_those_of_the_ssd_search(no):
    rng = np.random.default_rng(8)
    shape = (24, 22, 26)
    F = volume("smooth", shape, 3)
    W = remap(np.roll(F, 1, 2), "half_offset")
    for vol, bad in ((F, np.nan), (F, np.inf), (W, -np.inf), (W, np.nan)):
        vol[tuple(rng.integers(0, n) for n in shape)] = bad
    b, r = 1, 3
    first, count = (0, 0, 0), shape[::-1]
    wn, ws = no.match(F, W, first, 1, count, b, r), no.ssd.match(F, W, first, 1, count, b, r)
    assert (wn[..., 3] == ws[..., 3]).all() and 0 < (wn[..., 3] != 0).sum() < wn[..., 3].size
    assert (wn[wn[..., 3] != 0] == np.eye(WORDS, dtype=np.uint32)[3]).all()
    ok = wn[..., 3] == 0
    assert (wn[ok][:, 12:14] == ws[ok][:, 12:14]).all()          # sum qF and sum qF^2 are the record's, whatever the cost


@pytest.mark.parametrize("world", [False, True])
def test_remapped_scenario_cpu(built, no, fo, tmp_path, world):
    """The nonrigid scenario of section 7e refined on the CPU at the defaults (the keypoint field in, two rounds) from a moving
    volume whose intensities are remapped: 0.45 M + 310, and M (0.6 + 0.5 x/nx + 0.3 sin 2 pi y/ny) + 120.  Map errors as
    scenario_score gives them; the correlation is scored against the unremapped moving volume.  Asserted for the correlation
    cost on both volumes: section 7f's bar (RMS map error below 0.6 x the keypoint field's, a smaller largest error, a higher
    correlation, no folded node, two rounds, more than 10 000 samples kept), and an RMS of at most 1.05 x that of the SSD cost
    on the unremapped volume, computed in this run.  Asserted for the SSD cost on the remapped volumes: it misses the 0.6 bar.
    Reached when this was written (correlation, RMS, largest):
      voxel keys: -u 0.9627 1.865 7.97; SSD on M 0.9945 0.795 2.44; the correlation cost 0.9947 0.782 2.38 (0.42 x, 0.98 x SSD)
      on 0.45 M + 310 and 0.9946 0.787 2.43 (0.42 x, 0.99 x) under the bias; SSD there 0.9611 1.781 4.90 and 0.8353 3.624 6.33.
      -w keys: -u 0.9505 2.853 10.26; SSD on M 0.9965 0.976 3.72; the correlation cost 0.9965 0.948 3.50 (0.33 x, 0.97 x) and
      0.9964 0.963 3.48 (0.34 x, 0.99 x); SSD there 0.9517 2.633 7.04 and 0.8303 4.649 8.28."""
    s = scenario_setup(built, tmp_path, world)
    start = s["parent"]["field_dict"]
    c0, rms0, max0 = s["parent"]["field"]
    tag = " -w" if world else ""
    field, _ = cpu_refine_intensity(built, no.ssd, fo, s["V"], s["M"], s["T4"], start, s["fv"], s["mv"])
    cs, rms_ssd, maxs = scenario_score(built, fo, s, field)
    print("ncc scenario%s: -u corr %.4f rms %.3f max %.3f; ssd on M corr %.4f rms %.3f max %.3f" % (tag, c0, rms0, max0, cs, rms_ssd, maxs))
    for kind in ("affine", "smooth_bias"):
        M2 = remap(s["M"], kind)
        field, rep = cpu_refine_intensity_metric(built, no, fo, s["V"], M2, s["T4"], start, s["fv"], s["mv"], metric="ncc")
        c1, rms1, max1 = scenario_score(built, fo, s, field)
        field_s, rep_s = cpu_refine_intensity_metric(built, no, fo, s["V"], M2, s["T4"], start, s["fv"], s["mv"], metric="ssd")
        c2, rms2, max2 = scenario_score(built, fo, s, field_s)
        print("ncc scenario%s %s: ncc corr %.4f rms %.3f max %.3f (%.3f x -u, %.3f x ssd on M) kept %d; ssd corr %.4f rms %.3f max %.3f (%.3f x -u) "
              "samples %s" % (tag, kind, c1, rms1, max1, rms1 / rms0, rms1 / rms_ssd, rep["round"][-1].get("kept", 0), c2, rms2, max2, rms2 / rms0,
                              [r["samples"] for r in rep_s["round"]]))
        assert rep["rounds"] == 2 and rep["round"][1]["kept"] > 10000 and rep["round"][1]["folds"] == 0
        assert rms1 < 0.6 * rms0 and max1 < max0 and c1 > c0, ((c0, rms0, max0), (c1, rms1, max1))
        assert rms1 <= 1.05 * rms_ssd, (rms1, rms_ssd)
        assert not rms2 < 0.6 * rms0, (rms2, rms0)
