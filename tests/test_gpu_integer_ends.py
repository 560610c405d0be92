"""GPU suite: the kernels that work on 10-bit quantised volumes, at the ends of their integer sums -- block_match_kernel and
block_match_ncc_kernel (DESIGN.md sections 7f, 7g), fuse_weight_kernel (7j), fuse_search_kernel (7k) and bm_quantize_kernel, which
feeds them all -- against their CPU oracles, bit for bit, always through the C-ABI.

A block of 13^3 voxels (b = 6) of quantised values 0 and 1023 reaches 13^3 1023^2 = 2 299 224 213, between 2^31 and 2^32: the
kernels' 32-bit sums are right there only while every accumulator, compare, widening and division is unsigned.  The volumes are
blockmatch_cases.py's of the two values 0.0 and 1.0 (speckled, solid, bright; the checkerboard and the stripes, on which shifts of
equal length tie), and every case asserts on the oracle's words that it is where it claims to be; the CPU suites hold the oracles to
int64 numpy restatements on the same volumes (the "oracle equals numpy" tests of test_blockmatch_cpu.py, test_blockmatch_ncc_cpu.py,
test_fuse_cpu.py and test_fuse_search_cpu.py).  The quantiser is probed at exact half-way values, at the ends of its range, outside
it, and over the widest and the narrowest range a float admits.  Each test takes a second or two, most of it the serial oracle."""
import numpy as np
import pytest

from blockmatch_cases import (NONE as NO_COST, SUM_MAX_B6, ends_lattice, ends_pair, half_way_values, lattice3, lattice_numpy, probe_read, quantiser_probe, quantize_numpy, shifts,
                              stripes)
from blockmatch_ncc_cases import FLAT, NccOracle
from field_cases import FieldOracle
from fuse_cases import ENDS, ENDS_SHAPE, FALLBACK, NONE, U_ONE, cpu_fuse, ends_volumes, same_report, speckled_pair
from fuse_search_cases import (NO_SHIFT, SEARCH_ENDS, SEARCH_ENDS_BR, FuseSearchOracle, block_labels, ends_search_volumes, shift_vectors, tie_pick)
from resample_cases import ResampleOracle
from test_gpu_fuse_search import same_search

pytestmark = pytest.mark.gpu

SHAPE = (26, 27, 29)   # (nz, ny, nx): the smallest that holds the 25^3 window of (b, r) = (6, 6), as test_kernel_widest_search has it
# (b, r, stride): the two with specialised forms, and b = 6, where the sums are widest, at the least, a middle and the widest search
BLOCK_CASES = [(4, 3, 4), (4, 4, 4), (6, 1, 1), (6, 4, 3), (6, 6, 1)]
KINDS = ["speckled", "solid", "bright"]


@pytest.fixture(scope="module")
def no(tmp_path_factory):
    return NccOracle(tmp_path_factory.mktemp("blockmatch_ncc_oracle"))


@pytest.fixture(scope="module")
def fs(tmp_path_factory):
    return FuseSearchOracle(tmp_path_factory.mktemp("fuse_search_oracle"))


@pytest.fixture(scope="module")
def ro(tmp_path_factory):
    return ResampleOracle(tmp_path_factory.mktemp("resample_oracle"))


@pytest.fixture(scope="module")
def fo(tmp_path_factory):
    return FieldOracle(tmp_path_factory.mktemp("field_oracle"))


def same_words(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype
    assert got.tobytes() == want.tobytes(), (what, np.argwhere((got != want).any(-1))[:5], got[(got != want).any(-1)][:2], want[(got != want).any(-1)][:2])


# ---- the block search ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS + ["straddling"])
@pytest.mark.parametrize("b,r,stride", BLOCK_CASES)
def test_block_search_ssd_where_the_costs_pass_2_31(built, no, kind, b, r, stride):
    """every form (generic 0, 1, 2; the register forms exist at b = 4 only, and at b = 6 the three must still agree) against the oracle:
    speckled -- every cost near the largest there is, and different from shift to shift; straddling -- within one node costs below and
    beyond 2^31, which a signed compare of two costs or of two keys would order wrongly; solid -- every cost the largest there is;
    bright -- sum qF^2 beyond 2^31, small costs"""
    F, W = ends_pair(kind, SHAPE, 21)
    first, count = ends_lattice(kind, SHAPE, stride, b, r)
    want = no.ssd.match(F, W, first, stride, count, b, r)
    top = (2 * b + 1) ** 3 * 1023 ** 2
    print("%s (%d, %d): least cost %d .. %d of at most %d, sum qF^2 up to %d" % (kind, b, r, want[..., 4].min(), want[..., 4].max(), top, want[..., 13].max()))
    assert (want[..., 3] == 0).all()
    if kind == "speckled":
        assert len(np.unique(want[..., 4:6])) > 6 and (b < 6 or want[..., 4].min() >= 2 ** 31) and want[..., 4:6].max() <= top
    if kind == "straddling" and b == 6:
        assert ((want[..., 4] < 2 ** 31) & (np.where(want[..., 5:12] == NO_COST, 0, want[..., 5:12]).max(-1) >= 2 ** 31)).mean() > 0.25
    if kind == "solid":
        assert (want[..., 4:12] == top).all() and (shifts(want) == 0).all() and (b < 6 or top == SUM_MAX_B6 > 2 ** 31)
    if kind == "bright":
        assert (b < 6 or want[..., 13].min() >= 2 ** 31) and want[..., 4].max() < top // 4
    for generic in (0, 1, 2):
        same_words(built.block_match(F, W, first, stride, count, b, r, generic=generic), want, generic)


def test_block_search_flagged_and_saturated_nodes_in_one_brick(built, no):
    """a lattice that starts outside the volume: flagged nodes (every word but the flag 0) beside nodes whose costs pass 2^31"""
    F, W = ends_pair("speckled", SHAPE, 22)
    for metric, (b, r, stride) in (("ssd", (6, 1, 1)), ("ssd", (6, 4, 3)), ("ncc", (6, 1, 1))):
        f0, count = lattice_numpy(SHAPE, stride, b, r)
        first = (f0[0] - 2 * stride, f0[1] - 2 * stride, f0[2] - (2 if stride == 1 else 0))      # at stride 3 the lattice has two planes of nodes along z
        if metric == "ssd":
            want = no.ssd.match(F, W, first, stride, count, b, r)
            assert want[want[..., 3] == 0][:, 4].min() >= 2 ** 31
        else:
            F, W = ends_pair("bright", SHAPE, 22, own_scale=True)
            want = no.match(F, W, first, stride, count, b, r)
            assert want[want[..., 3] == 0][:, 13].min() >= 2 ** 31
        flagged = want[..., 3] != 0
        assert flagged[:, :2].all() and flagged[:, :, :2].all() and 0 < (~flagged).sum() and not want[flagged][:, [0, 1, 2] + list(range(4, 16))].any()
        entry = built.block_match if metric == "ssd" else built.block_match_ncc
        for generic in (0, 1):
            same_words(entry(F, W, first, stride, count, b, r, generic=generic), want, (metric, generic))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("b,r,stride", BLOCK_CASES)
def test_block_search_correlation_where_the_sums_pass_2_31(built, no, kind, b, r, stride):
    """both forms against the oracle, W on a scale of its own (0.37 W - 55) so that W's own range is what quantises it: bright -- Sff,
    Sww and Sfw beyond 2^31 at b = 6, blocks that are not flat, variances that are small differences of large products; speckled -- Sww
    beyond 2^31 and blocks of F with few voxels that are not 0; solid -- flat blocks, every cost 2^31"""
    F, W = ends_pair(kind, SHAPE, 21, own_scale=True)
    first, count = ends_lattice(kind, SHAPE, stride, b, r)
    want = no.match(F, W, first, stride, count, b, r)
    cost = want[..., 4]
    print("%s (%d, %d): cost %d .. %d, at 2^31 %.3f, sum qF^2 up to %d" % (kind, b, r, cost.min(), cost.max(), (cost == FLAT).mean(), want[..., 13].max()))
    assert (want[..., 3] == 0).all() and want[..., 4:6].max() <= FLAT and set(np.unique(no.quantize(W, *no.range(W)))) == {0, 1023}
    if kind == "solid":
        assert (want[..., 4:12] == FLAT).all() and (shifts(want) == 0).all()
    if kind == "bright" and b == 6:
        assert want[..., 13].min() >= 2 ** 31 and ((cost > 0) & (cost < FLAT)).mean() > 0.5 and (cost == FLAT).mean() < 0.1
    if kind == "speckled" and b == 6:
        qw = no.quantize(W, *no.range(W)).astype(np.int64)
        assert (qw[:13, :13, :13] ** 2).sum() >= 2 ** 31 and len(np.unique(cost)) > 1
    for generic in (0, 1):
        same_words(built.block_match_ncc(F, W, first, stride, count, b, r, generic=generic), want, generic)


# ---- ties between shifts of equal length -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,r", [(1, 1), (4, 3), (4, 4), (6, 1)])
def test_block_search_ties_between_unit_shifts(built, no, b, r):
    """the checkerboard against its complement: six unit shifts of cost 0, decided in bm_key by z, then y, then x: s_z = -1; stripes
    along one axis: -1 along it.  Every form of both kernels (the zero shift costs the most: the sum of squares' largest value, 2^31
    under the correlation)."""
    shape = (17, 18, 19)
    first, count = lattice_numpy(shape, 1, b, r)
    for axis in (None, 0, 1, 2):
        F, W = lattice3(shape) if axis is None else stripes(shape, axis)
        pick = np.zeros(3, np.int32)
        pick[0 if axis is None else axis] = -1
        pick = pick[::-1]                                # the words hold (x, y, z)
        for entry, oracle, forms, zero in ((built.block_match, no.ssd, (0, 1, 2), (2 * b + 1) ** 3 * 1023 ** 2), (built.block_match_ncc, no, (0, 1), FLAT)):
            want = oracle.match(F, W, first, 1, count, b, r)
            assert (want[..., 3] == 0).all() and (shifts(want) == pick).all() and (want[..., 4] == 0).all() and (want[..., 5] == zero).all()
            for generic in forms:
                got = entry(F, W, first, 1, count, b, r, generic=generic)
                same_words(got, want, (axis, generic))
                assert (shifts(got) == pick).all()


@pytest.mark.parametrize("metric", ["ssd", "ncc"])
@pytest.mark.parametrize("b,r", [(1, 1), (2, 1), (2, 3), (3, 3), (5, 1)])
def test_fuse_search_ties_between_unit_shifts(built, fs, metric, b, r):
    """the same volumes through fuse_search_kernel in both forms: six candidates of u = 32768, decided in u << 14 | (0x3fff - rank) by
    the least tz, then ty, then tx: t = (tz, ty, tx) = (-1, 0, 0) at the interior, and at the low faces, where that shift leaves the
    volume, the next of the order (fuse_search_cases.tie_pick); stripes along x: tx = -1, and +1 at x = 0"""
    shape = (7, 9, 37)
    for axis in (None, 0, 1, 2):
        T, W = lattice3(shape) if axis is None else stripes(shape, axis)
        want = fs.search(T, W, None, b, r, metric)
        pick = tie_pick(shape, axis)
        assert (want[0] == U_ONE).all() and np.array_equal(shift_vectors(want[1], r), pick)
        for generic in (0, 1):
            got = built.fuse_search(T, W, None, block=b, radius=r, metric=metric, generic=generic)
            same_search(got, want)
            assert np.array_equal(shift_vectors(got[1], r), pick)
    assert (pick[:, :, 1:] == np.array((-1, 0, 0))).all() and (pick[:, :, 0] == np.array((1, 0, 0))).all()      # stripes along x, (tx, ty, tz)
    assert (tie_pick(shape)[1:, :, :] == np.array((0, 0, -1))).all() and (tie_pick(shape)[0, 1:, :] == np.array((0, -1, 0))).all()


# ---- the fusion weights ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ssd", "ncc"])
@pytest.mark.parametrize("b", [1, 2, 6])
@pytest.mark.parametrize("kind", ENDS)
def test_fuse_weights_where_the_sums_pass_2_31(built, fs, kind, b, metric):
    """both forms against the oracle on 15 x 17 x 37, where some patches are unclipped at b = 6: speckled -- D near n 1023^2 (with
    holes: a pair that leaked in would move D by 1023^2); bright -- Sff, Sww, Sfw beyond 2^31 and patches that are not flat;
    bright_same -- D = Sff - 2 Sfw + Sww = 0 from three sums beyond 2^31"""
    T, W = ends_volumes(kind, ENDS_SHAPE, 31)
    qt, qw = fs.quantised(T, W, metric)
    want, sums = fs.weights_q(qt, qw, b, metric, sums=True)
    D = sums[..., 2] - 2 * sums[..., 5] + sums[..., 4]
    print("%s %s b %d: largest sum %d, D up to %d, u %d .. %d" % (kind, metric, b, sums.max(), D.max(), want.min(), want.max()))
    assert (qt.min() == -1) == (kind == "speckled_holes") and np.array_equal(want, fs.weights(T, W, b, metric))
    if b == 6:
        assert 2 ** 31 <= sums.max() <= SUM_MAX_B6 < 2 ** 32 and (sums[..., 0].max() == 13 ** 3 or kind == "speckled_holes")
        assert D.max() >= 2 ** 31 if kind.startswith("speckled") else min(sums[..., i].max() for i in (2, 4, 5)) >= 2 ** 31
    if kind.startswith("speckled") and metric == "ssd":
        assert not want.any()
    if kind == "bright_same":
        assert (D == 0).all() and (want == U_ONE).any() and (((want == 0) & (metric == "ncc")) | (want == U_ONE)).all()    # a patch of 1 alone is flat
    if kind == "bright" and metric == "ncc" and b == 6:
        assert ((want > 0) & (want < U_ONE)).mean() > 0.9
    for generic in (0, 1):
        got = built.fuse_weights(T, W, block=b, metric=metric, generic=generic)
        assert got.dtype == np.uint16 and np.array_equal(got, want), (generic, int((got != want).sum()))


@pytest.mark.parametrize("metric", ["ssd", "ncc"])
def test_fuse_weights_a_range_narrower_than_w_clamps_at_both_ends(built, fs, metric):
    """W of 0 and 1 with a few voxels at 0.25, 0.5 and 0.75, quantised over 0.25 .. 0.75: what lies below goes to 0, what lies above to
    1023, the ends themselves to 0 and 1023 and the middle to the even neighbour of 511.5; NaN and infinite voxels to -1, which
    a W of these alone shows as u = 0 everywhere"""
    T, W = ends_volumes("bright", ENDS_SHAPE, 33)
    rng = np.random.default_rng(34)
    at = rng.random(ENDS_SHAPE) < 0.05
    W[at] = rng.choice(np.array([0.25, 0.5, 0.75], np.float32), int(at.sum()))
    w_range = (np.float32(0.25), np.float32(0.75))
    qw = fs.quantize(W, *w_range)
    assert np.array_equal(qw, quantize_numpy(W, *w_range)) and sorted(np.unique(qw)) == [0, 512, 1023]
    assert (qw[W < 0.25] == 0).all() and (qw[W > 0.75] == 1023).all() and (W < 0.25).any() and (W > 0.75).sum() > W.size // 2
    none = np.full(ENDS_SHAPE, np.nan, np.float32)
    none[rng.random(ENDS_SHAPE) < 0.3], none[rng.random(ENDS_SHAPE) < 0.3] = np.inf, -np.inf
    for b in (2, 6):
        want = fs.weights(T, W, b, metric, w_range=w_range)
        assert want.max() > 0
        for generic in (0, 1):
            assert np.array_equal(built.fuse_weights(T, W, block=b, metric=metric, w_range=w_range, generic=generic), want)
            assert not built.fuse_weights(T, none, block=b, metric=metric, w_range=w_range, generic=generic).any()
    assert (fs.quantize(none, *w_range) == -1).all() and not fs.weights(T, none, 2, metric, w_range=w_range).any()


# ---- the fusion search -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ssd", "ncc"])
@pytest.mark.parametrize("b,r", SEARCH_ENDS_BR)
@pytest.mark.parametrize("kind", SEARCH_ENDS)
def test_fuse_search_where_the_sums_pass_2_31(built, fs, kind, b, r, metric):
    """both forms against the oracle, with labels that say which voxels may be picked: speckled -- u = 0 at every candidate (with
    holes: which pairs count changes with the shift, and a pair that leaked in would move D by 1023^2); bright -- a planted shift to
    find among sums beyond 2^31.  At (6, 0) u is also sift3d_fuse_weights' at b = 6.  The oracle's summed-area form (int64 tables),
    which test_fuse_search_cpu.py holds to its brute force on these volumes at every (b, r) here, keeps a case at a second; the
    sums come from the brute force where they are widest, at (6, 0)."""
    T, W = ends_search_volumes(kind, ENDS_SHAPE, 31)
    labels = block_labels(ENDS_SHAPE, 3, nan_block=kind == "speckled_holes")
    qt, qw = fs.quantised(T, W, metric)
    u, shift, picked = fs.search_q(qt, qw, labels, b, r, metric, sat=True)
    votes = shift != NO_SHIFT
    print("%s %s (%d, %d): u %d .. %d" % (kind, metric, b, r, u[votes].min(), u[votes].max()))
    assert votes.any() and votes.all() == (kind != "speckled_holes")
    if b == 6:
        bu, bshift, bpicked, sums = fs.search_q(qt, qw, labels, b, r, metric, sums=True)
        same_search((bu, bshift, bpicked), (u, shift, picked))
        D = sums[..., 2] - 2 * sums[..., 5] + sums[..., 4]
        print("  largest sum %d, D up to %d" % (sums.max(), D.max()))
        assert 2 ** 31 <= sums.max() <= SUM_MAX_B6 < 2 ** 32 and (kind == "bright" or D.max() >= 2 ** 31)
    if kind.startswith("speckled") and metric == "ssd":
        assert not u[votes].any()
    if kind == "bright" and r >= 1:
        assert (shift == fs.code(r, (-1, 1, 0))).mean() > 0.3 and u.max() > 0
    for generic in (0, 1):
        got = built.fuse_search(T, W, labels, block=b, radius=r, metric=metric, generic=generic)
        same_search(got, (u, shift, picked))
    if r == 0:
        w = built.fuse_weights(T, W, block=b, metric=metric)
        assert np.array_equal(got[0][votes], w[votes]) and (got[0][~votes] == 0xffff).all()


# ---- the quantiser ---------------------------------------------------------------------------------------------------------------------
def test_quantiser_read_back_through_the_block_search(built, no):
    """bm_quantize_kernel has no entry point of its own; quantiser_probe's cells bring its values out through the records of the block
    search (words 12 and 13 of F's cells, word 5 of W's cells against an F of lo alone).  Over 0 .. 1023: every exact half-way value
    and the floats beside a few of them, both ends, -0.0, a denormal, 1e-30 and the last float below 1023.  Over -3e38 .. 3e38: hi - lo
    overflows in float, so the difference must be formed in double; values beyond the range clamp.  Over a range one float ulp
    wide: the quotient's denominator is 2^-23."""
    bo = no.ssd
    v = half_way_values()
    vol, first, count = quantiser_probe(v, 0.0, 1023.0)
    q = bo.quantize(v, 0.0, 1023.0)
    want = bo.match(vol, vol, first, 3, count, 1, 1)
    assert np.array_equal(probe_read(want, len(v), 12), q) and np.array_equal(q, quantize_numpy(v, 0.0, 1023.0)) and (want[..., 3] == 0).all()
    got = built.block_match(vol, vol, first, 3, count, 1, 1)
    same_words(got, want, "half-way values")
    assert np.array_equal(probe_read(got, len(v), 12), q) and np.array_equal(probe_read(got, len(v), 13), q)
    same_words(built.block_match_ncc(vol, vol, first, 3, count, 1, 1), no.match(vol, vol, first, 3, count, 1, 1), "half-way values, W by its own range")
    ulp_lo, ulp_hi = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))
    for lo, hi, v in ((np.float32(-3.0e38), np.float32(3.0e38), np.array([3.4028235e38, -3.4028235e38, 1e38, -1e38, 0.0, 3.0e38, -3.0e38], np.float32)),
                      (ulp_lo, ulp_hi, np.array([ulp_lo, ulp_hi, np.nextafter(ulp_lo, np.float32(0.0)), np.nextafter(ulp_hi, np.float32(2.0)), 0.5, 2.0, -3.4e38,
                                                 3.4e38], np.float32))):
        q = bo.quantize(v, lo, hi)
        assert np.array_equal(q, quantize_numpy(v, lo, hi)) and q.min() == 0 and q.max() == 1023
        Fv, first, count = quantiser_probe(np.full(len(v), lo, np.float32), lo, hi)
        Wv, _, _ = quantiser_probe(v, lo, hi)
        assert bo.range(Fv) == (lo, hi)
        want = bo.match(Fv, Wv, first, 3, count, 1, 1)
        assert (want[..., 3] == 0).all() and np.array_equal(probe_read(want, len(v), 5), q)
        got = built.block_match(Fv, Wv, first, 3, count, 1, 1)
        same_words(got, want, (lo, hi))
        assert np.array_equal(probe_read(got, len(v), 5), q)
        inside = v[(v >= lo) & (v <= hi)]                 # as F, a volume holds nothing beyond its own range
        Fi, first, count = quantiser_probe(inside, lo, hi)
        got = built.block_match(Fi, Fi, first, 3, count, 1, 1)
        same_words(got, bo.match(Fi, Fi, first, 3, count, 1, 1), (lo, hi, "F"))
        assert np.array_equal(probe_read(got, len(inside), 12), bo.quantize(inside, lo, hi))


# ---- the stage -------------------------------------------------------------------------------------------------------------------------
def test_stage_every_voter_weighs_nothing(built, fs, ro, fo):
    """sift3d_fuse_labels, power 2, block 2, identity transforms, no fields: two atlases whose images are the complement of a speckled
    target.  Every patch's D is n 1023^2, every u is 0, and the vote takes the fall-back wherever somebody votes."""
    target, _ = speckled_pair(ENDS_SHAPE, 41)
    image = (1.0 - target).astype(np.float32)
    labels = [block_labels(ENDS_SHAPE, 5), block_labels(ENDS_SHAPE, 6, nan_block=False)]
    labels[1][:, :, 20:] = np.nan                        # beyond x = 20 the second atlas does not vote, and inside the first one's NaN box nobody does
    atlases = [{"image": image, "labels": lab, "t": np.eye(4, dtype=np.float32)} for lab in labels]
    want, want_rep = cpu_fuse(built, fs, ro, fo, target, atlases, block=2, metric="ssd", power=2)
    somebody = (want[..., 0] & NONE) == 0
    assert 0 < somebody.sum() < somebody.size and ((want[..., 0] & FALLBACK) != 0)[somebody].all() and want_rep["fallback"] == int(somebody.sum())
    assert all(r["mean_u"] == 0 for r in want_rep["atlas"]) and (((want[..., 0] >> 16) & 63).max() == 2)
    words, rep = built.fuse_labels(target, atlases, block=2, metric="ssd", power=2)
    assert np.array_equal(words, want)
    same_report(rep, want_rep)
