"""CPU suite: the local search of the label fusion without a GPU -- the oracle tests/fuse_search_oracle.c
against a numpy restatement and against its own contract (r = 0 is section 7j, flat volumes keep the shift 0, a moved volume is
found, unlabelled regions, the order of ties), its summed-area form against its brute force, the product's shift-code helpers at
their bounds and under the sanitizers as a stand-alone program, and the five-atlas scenario at every radius."""
import os
import subprocess

import numpy as np
import pytest

from field_cases import FieldOracle
from fuse_cases import NONE, U_ONE, fused_labels, leg, mean_dice, pair, scenario
from fuse_search_cases import (ENDS_SHAPE, NO_SHIFT, SEARCH_ENDS, SEARCH_ENDS_BR, SUM_MAX_B6, FuseSearchOracle, block_labels, ends_search_volumes, fuse_planes, lattice3,
                               shift_stats, shift_vectors, shifted_pair, stripes, tie_pick, warped_planes)
from resample_cases import ResampleOracle
from test_fuse_cpu import SCENARIO_DICE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fs(tmp_path_factory):
    return FuseSearchOracle(tmp_path_factory.mktemp("fuse_search_oracle"))


@pytest.fixture(scope="module")
def ro(tmp_path_factory):
    return ResampleOracle(tmp_path_factory.mktemp("resample_oracle"))


@pytest.fixture(scope="module")
def fo(tmp_path_factory):
    return FieldOracle(tmp_path_factory.mktemp("field_oracle"))


@pytest.fixture(scope="module")
def scen(built, ro, tmp_path_factory):
    return scenario(built, ro, tmp_path_factory.mktemp("fuse_scenario"))


def box(a, b):
    """the sums of a (nz, ny, nx, ...) over every voxel's clipped box of half-width b, by differences of cumulative sums"""
    for ax in range(3):
        n = a.shape[ax]
        c = np.concatenate([np.zeros_like(np.take(a, [0], ax)), np.cumsum(a, ax)], ax)
        i = np.arange(n)
        a = np.take(c, np.minimum(i + b + 1, n), ax) - np.take(c, np.maximum(i - b, 0), ax)
    return a


def u_numpy(metric, s):
    """the similarity of the sums s[..., 6] in numpy integers and doubles, one operation at a time (np.rint is ties-to-even)"""
    n, sf, sff, sw, sww, sfw = (s[..., i] for i in range(6))
    if metric == "ssd":
        u = (n << 15) // np.maximum(sff - 2 * sfw + sww + n, 1)
    else:
        A, Vf, Vw = n * sfw - sf * sw, n * sff - sf * sf, n * sww - sw * sw
        ok = (A > 0) & (Vf > 0) & (Vw > 0)
        Af, Vff, Vwf = A.astype(np.float64), np.where(ok, Vf, 1).astype(np.float64), np.where(ok, Vw, 1).astype(np.float64)
        rho2 = np.where(ok, (Af * Af) / (Vff * Vwf), 0.0)
        u = ((1 << 31) - np.rint((1.0 - np.minimum(rho2, 1.0)) * 2147483648.0).astype(np.int64)) >> 16
    return np.where(n > 0, u, 0)


def search_numpy(qt, qw, labels, b, r, metric):
    """the contract in numpy: per shift the six sums of every voxel, its u, and the choice as the maximum of a key that orders
    (u, -|t|^2, -tz, -ty, -tx).  Returns (u, shift, picked or None, the chosen candidate's sums)."""
    qt, qw = np.asarray(qt, np.int64), np.asarray(qw, np.int64)
    nz, ny, nx = qt.shape
    can = np.ones(qt.shape, bool) if labels is None else np.isfinite(labels)
    pw, pc = np.pad(qw, r, constant_values=-1), np.pad(can, r, constant_values=False)
    pl = None if labels is None else np.pad(np.asarray(labels, np.float32), r, constant_values=np.nan)
    best = np.full(qt.shape, -1, np.int64)
    code = np.full(qt.shape, NO_SHIFT, np.int64)
    picked = np.full(qt.shape, np.nan, np.float32)
    sums = np.zeros(qt.shape + (6,), np.int64)
    for tz in range(-r, r + 1):
        for ty in range(-r, r + 1):
            for tx in range(-r, r + 1):
                cut = (slice(r + tz, r + tz + nz), slice(r + ty, r + ty + ny), slice(r + tx, r + tx + nx))
                w = pw[cut]
                ok = (qt >= 0) & (w >= 0)
                f, w = np.where(ok, qt, 0), np.where(ok, w, 0)
                s = box(np.stack([ok.astype(np.int64), f, f * f, w, w * w, f * w], -1), b)
                u = u_numpy(metric, s)
                key = (((u * 32 + (27 - (tx * tx + ty * ty + tz * tz))) * 8 + (r - tz)) * 8 + (r - ty)) * 8 + (r - tx)
                take = pc[cut] & (key > best)
                best = np.where(take, key, best)
                code = np.where(take, ((tz + r) * (2 * r + 1) + (ty + r)) * (2 * r + 1) + (tx + r), code)
                sums = np.where(take[..., None], s, sums)
                if pl is not None:
                    picked = np.where(take, pl[cut], picked)
    u = np.where(best >= 0, best >> 14, 0xffff)
    return u.astype(np.uint16), code.astype(np.uint16), (None if labels is None else picked), sums


def same_picked(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32) & 0x7fffffff > 0x7f800000, np.asarray(b, np.float32).view(np.uint32) & 0x7fffffff > 0x7f800000) \
        and np.array_equal(np.nan_to_num(a, nan=-1.0), np.nan_to_num(b, nan=-1.0))


BR = [(1, 1), (1, 2), (1, 3), (2, 1), (2, 2), (2, 3), (3, 3), (5, 1), (6, 0)]


@pytest.mark.parametrize("metric", ["ssd", "ncc"])
@pytest.mark.parametrize("shape,holes,kind", [pytest.param(*c, "shifted", id="shape%d-%s" % (i, c[1])) for i, c in enumerate(
    [((2, 3, 4), False), ((5, 9, 33), False), ((7, 11, 21), True)])] +                                       # the ids these cases have always had
    [pytest.param(ENDS_SHAPE, k == "speckled_holes", k, id=k) for k in SEARCH_ENDS])
def test_oracle_equals_numpy_and_its_summed_area_form(fs, metric, shape, holes, kind):
    """kind "shifted": shifted_pair.  The others are fuse_search_cases.ends_search_volumes on a shape with unclipped patches at b = 6: the
    restatement's sums are int64 and cannot wrap, so it settles the chosen candidate's sums and u where they pass 2^31."""
    ends = kind != "shifted"
    T, W = ends_search_volumes(kind, shape, 5) if ends else shifted_pair(shape, 5, (1, -1, 1), holes)
    qt, qw = fs.quantised(T, W, metric)
    assert qt.max() == 1023 and qt.min() == (-1 if holes else 0)
    labels = block_labels(shape, 3, nan_block=holes)
    for b, r in (SEARCH_ENDS_BR if ends else BR):
        u, shift, picked, sums = fs.search_q(qt, qw, labels, b, r, metric, sums=True)
        nu, nshift, npicked, nsums = search_numpy(qt, qw, labels, b, r, metric)
        assert np.array_equal(u, nu) and np.array_equal(shift, nshift) and same_picked(picked, npicked) and np.array_equal(sums, nsums), (b, r)
        assert sums[..., 0].max() <= (2 * b + 1) ** 3 and sums.max() < 2 ** 32
        su, sshift, spicked = fs.search_q(qt, qw, labels, b, r, metric, sat=True)
        assert np.array_equal(su, u) and np.array_equal(sshift, shift) and same_picked(spicked, picked), (b, r)
        votes = shift != NO_SHIFT
        assert np.array_equal(votes, u != 0xffff) and np.array_equal(votes, np.isfinite(picked)) and u[votes].max() <= U_ONE
        assert shift[votes].max() < (2 * r + 1) ** 3
        if ends:      # what test_gpu_integer_ends.py relies on, asserted on the oracle's sums
            D = sums[..., 2] - 2 * sums[..., 5] + sums[..., 4]
            print("%s %s b %d r %d: largest sum %d, D %d .. %d, u %d .. %d" % (kind, metric, b, r, sums.max(), D.min(), D.max(), u[votes].min(), u[votes].max()))
            assert set(np.unique(qt)) - {-1} == {0, 1023} and set(np.unique(qw)) - {-1} == {0, 1023}
            if b == 6:
                assert 2 ** 31 <= sums.max() <= SUM_MAX_B6 < 2 ** 32 and (kind == "bright" or D.max() >= 2 ** 31)
            if kind.startswith("speckled") and metric == "ssd":
                assert (u[votes] == 0).all() and (holes or (shift == fs.code(r, (0, 0, 0))).all())    # u = 0 at every candidate: the nearest that may be picked
            if kind == "bright" and r >= 1:     # the planted shift is found (many patches of 5^3 voxels are all 1 and tell nothing)
                found = (shift == fs.code(r, (-1, 1, 0)))[1:-1, 1:-1, 1:-1].mean()
                print("  planted shift found at %.3f of the inner voxels" % found)
                assert found > 0.4 and u[votes].max() > 0
    if ends:
        return
    # without labels every shift inside the volume is a candidate
    u, shift, picked = fs.search_q(qt, qw, None, 2, 2, metric)
    nu, nshift, _, _ = search_numpy(qt, qw, None, 2, 2, metric)
    assert picked is None and np.array_equal(u, nu) and np.array_equal(shift, nshift) and (shift != NO_SHIFT).all()
    if shape == (5, 9, 33):
        assert shift_stats(shift, 2)[0] > 0.5 * shift.size       # the moved W is found


@pytest.mark.parametrize("metric", ["ssd", "ncc"])
@pytest.mark.parametrize("b,r", [(1, 1), (2, 1), (2, 3), (5, 1)])
def test_ties_between_unit_shifts_at_the_interior_and_at_the_faces(fs, metric, b, r):
    """the checkerboard against its complement: the six unit shifts all give u = 32768 and every even shift 0 (under the correlation
    too: the patches are equal, or anticorrelated); t = (tz, ty, tx) = (-1, 0, 0) is picked, and at the low faces, where it leaves
    the volume, the next of the order.  Stripes along one axis: -1 along it, and +1 at the low face."""
    shape = (7, 9, 37)
    for axis in (None, 0, 1, 2):
        T, W = lattice3(shape) if axis is None else stripes(shape, axis)
        qt, qw = fs.quantised(T, W, metric)
        u, shift, _, sums = fs.search_q(qt, qw, None, b, r, metric, sums=True)
        nu, nshift, _, nsums = search_numpy(qt, qw, None, b, r, metric)
        assert np.array_equal(u, nu) and np.array_equal(shift, nshift) and np.array_equal(sums, nsums)
        assert (u == U_ONE).all() and np.array_equal(shift_vectors(shift, r), tie_pick(shape, axis)), axis
    inner = shift_vectors(shift, r)[1:, 1:, 1:]
    assert (inner == np.array((-1, 0, 0))).all() and (shift_vectors(shift, r)[:, :, 0] == np.array((1, 0, 0))).all()   # stripes along x: (tx, ty, tz)


@pytest.mark.parametrize("metric", ["ssd", "ncc"])
@pytest.mark.parametrize("b", [1, 2, 6])
def test_radius_zero_is_the_weights_of_section_7j(fs, metric, b):
    T, W = pair((7, 11, 21), 9, holes=True)
    qt, qw = fs.quantised(T, W, metric)
    u, shift, picked = fs.search_q(qt, qw, None, b, 0, metric)
    assert np.array_equal(u, fs.weights_q(qt, qw, b, metric)) and (shift == 0).all() and fs.code(0, (0, 0, 0)) == 0
    labels = block_labels(T.shape, 1)
    u2, shift2, picked2 = fs.search_q(qt, qw, labels, b, 0, metric)
    votes = np.isfinite(labels)
    assert np.array_equal(u2[votes], u[votes]) and (u2[~votes] == 0xffff).all() and (shift2[votes] == 0).all() and (shift2[~votes] == NO_SHIFT).all()
    assert same_picked(picked2, np.where(votes, labels, np.nan))


@pytest.mark.parametrize("metric", ["ssd", "ncc"])
def test_flat_w_keeps_the_shift_zero(fs, metric):
    """every candidate of a voxel has the same qW under its patch voxels only where no patch is clipped by the shift; in a flat W
    the clipped ones have fewer voxels, never a larger u under NCC (0 everywhere) and, under SSD, ties or less inside"""
    T, _ = pair((9, 12, 20), 2)
    qt = fs.quantize(T, *fs.range(T))
    qw = np.full(qt.shape, 500, np.int16)
    for r in (1, 2, 3):
        u, shift, _ = fs.search_q(qt, qw, None, 2, r, metric)
        if metric == "ncc":
            assert (shift == fs.code(r, (0, 0, 0))).all() and (u == 0).all()
        else:
            inner = (slice(2 + r, -2 - r),) * 3          # the patch stays inside under every shift: every candidate has the same sums
            assert (shift[inner] == fs.code(r, (0, 0, 0))).all()
    # qT flat as well: every candidate of every voxel is identical, u = 32768 under SSD
    u, shift, _ = fs.search_q(qw, qw, None, 2, 3, "ssd")
    assert (u == U_ONE).all() and (shift == fs.code(3, (0, 0, 0))).all()


@pytest.mark.parametrize("metric", ["ssd", "ncc"])
def test_w_moved_by_a_shift_is_found_with_full_similarity(fs, metric):
    rng = np.random.default_rng(8)
    qt = rng.integers(0, 1024, (13, 12, 15)).astype(np.int16)
    t = (2, -1, 3)
    qw = np.roll(qt, (t[2], t[1], t[0]), (0, 1, 2))        # qW(x + t) = qT(x)
    u, shift, _ = fs.search_q(qt, qw, None, 2, 3, metric)
    # where the patch around x + t stays inside and does not wrap: x + t + v in the volume and not rolled across its border
    inner = (slice(2, 13 - 3 - 2), slice(1 + 2, 12 - 2), slice(2, 15 - 2 - 2))
    assert (shift[inner] == fs.code(3, t)).all() and (u[inner] == U_ONE).all() and fs.code(3, t) == ((3 + 3) * 7 + (-1 + 3)) * 7 + (2 + 3)
    assert (u <= U_ONE).all()


def test_unlabelled_regions_vote_from_within_the_radius_and_not_beyond(fs):
    T, W = shifted_pair((12, 14, 20), 4)
    qt, qw = fs.quantised(T, W, "ssd")
    labels = np.full(T.shape, 3.0, np.float32)
    labels[:, :, :11] = np.nan                               # x <= 10 unlabelled
    labels[6, 7, 2] = 9.0                                    # one labelled voxel deep inside the unlabelled region
    for r in (1, 2, 3):
        u, shift, picked = fs.search_q(qt, qw, labels, 2, r, "ssd")
        x = np.arange(20)[None, None, :]
        z, y = np.arange(12)[:, None, None], np.arange(14)[None, :, None]
        near_island = (abs(z - 6) <= r) & (abs(y - 7) <= r) & (abs(x - 2) <= r)
        votes = (x >= 11 - r) | near_island
        assert np.array_equal(shift != NO_SHIFT, votes) and np.array_equal(u != 0xffff, votes) and np.array_equal(np.isfinite(picked), votes)
        assert (picked[near_island & (x < 11 - r)] == 9.0).all() and (picked[..., 11:] [~near_island[..., 11:]] == 3.0).all()
        # voters of the unlabelled region have moved; the vote over this one atlas gives NONE exactly where it has no candidate
        assert (shift[..., :11 - r][near_island[..., :11 - r]] != fs.code(r, (0, 0, 0))).sum() >= near_island.sum() - 1
        words = fs.vote([np.where(u == 0xffff, 0, u)], [picked], 2)
        assert np.array_equal((words[..., 0] & NONE) != 0, ~votes) and ((words[..., 0] & 0xffff)[near_island & (x < 11 - r)] == 9).all()


def test_ties_go_to_the_smallest_distance_then_z_then_y_then_x(fs):
    """qT is 0 but for one voxel c of 1000; qW is 0 but for voxels of 1000 at chosen offsets from c.  At b = 1 the patch around c sees
    under the shift t the voxel of qW at c + t + v: a W voxel at c + o matches T's peak exactly under t = o, u = 32768, and every
    other shift that brings a W peak into the patch misplaces it.  Two offsets of equal |t|^2 tie."""
    shape, c = (11, 11, 11), (5, 5, 5)

    def run(offsets, r=2, labels=None):
        qt, qw = np.zeros(shape, np.int16), np.zeros(shape, np.int16)
        qt[c] = 1000
        for o in offsets:                                    # o = (tx, ty, tz)
            qw[c[0] + o[2], c[1] + o[1], c[2] + o[0]] = 1000
        u, shift, _ = fs.search_q(qt, qw, labels, 1, r, "ssd")
        return int(u[c]), int(shift[c])

    assert run([(2, 0, 0), (0, 0, 2)]) == (U_ONE, fs.code(2, (2, 0, 0)))        # equal |t|^2 = 4: tz = 0 before tz = 2
    assert run([(-2, 0, 0), (0, 0, -2)]) == (U_ONE, fs.code(2, (0, 0, -2)))     # tz = -2 before tz = 0
    assert run([(2, 0, 0), (0, 2, 0)]) == (U_ONE, fs.code(2, (2, 0, 0)))        # equal tz: ty = 0 before ty = 2
    assert run([(0, -2, 0), (2, 0, 0)]) == (U_ONE, fs.code(2, (0, -2, 0)))      # ty = -2 before ty = 0
    assert run([(2, 0, 0), (-2, 0, 0)]) == (U_ONE, fs.code(2, (-2, 0, 0)))      # equal tz and ty: tx = -2 before tx = 2
    assert run([(1, 0, 0), (0, 0, -2)]) == (U_ONE, fs.code(2, (1, 0, 0)))       # the smaller |t|^2 before the smaller tz
    assert run([(1, 1, 0), (0, 0, -2)]) == (U_ONE, fs.code(2, (1, 1, 0)))
    # the nearer candidate may not be picked (its label is not finite): the farther one of the same u wins
    labels = np.zeros(shape, np.float32)
    labels[5, 5, 6] = np.nan
    assert run([(1, 0, 0), (0, 0, -2)], labels=labels) == (U_ONE, fs.code(2, (0, 0, -2)))
    # a candidate of u = 0 is still a candidate: qW invalid everywhere
    u, shift, _ = fs.search_q(np.zeros(shape, np.int16), np.full(shape, -1, np.int16), None, 1, 2, "ssd")
    assert (u == 0).all() and (shift == fs.code(2, (0, 0, 0))).all()


def test_shift_code_helpers_at_their_bounds(built, fs):
    for r in (0, 1, 2, 3):
        codes = []
        for tz in range(-r, r + 1):
            for ty in range(-r, r + 1):
                for tx in range(-r, r + 1):
                    c = built.fuse_shift_code(r, (tx, ty, tz))
                    assert c == fs.code(r, (tx, ty, tz)) and built.fuse_shift_of(r, c) == (tx, ty, tz)
                    codes.append(c)
        assert codes == list(range((2 * r + 1) ** 3))
        assert built.fuse_shift_of(r, (2 * r + 1) ** 3) is None and built.fuse_shift_of(r, NO_SHIFT) is None
        for bad in ((r + 1, 0, 0), (0, -r - 1, 0), (0, 0, r + 1)):
            assert built.fuse_shift_code(r, bad) == NO_SHIFT
    assert built.fuse_shift_code(4, (0, 0, 0)) == NO_SHIFT and built.fuse_shift_code(-1, (0, 0, 0)) == NO_SHIFT and built.fuse_shift_of(4, 0) is None
    assert built.FUSE_MAX_SEARCH == 3 and built.FUSE_NO_SHIFT == NO_SHIFT
    rng = np.random.default_rng(6)
    plane = rng.integers(0, 343, 5000).astype(np.uint16)
    plane[::9] = NO_SHIFT
    voters, moved, d2 = built.fuse_shift_stats(3, plane)
    assert voters == int((plane != NO_SHIFT).sum()) and (moved, d2) == shift_stats(plane, 3) and 0 < moved < voters
    with pytest.raises(built.Sift3DError):
        built.fuse_shift_stats(2, plane)


def test_host_helpers_under_sanitizers(tmp_path):
    """fuse_host.c and tests/fuse_search_host_san.c as one program, with and without -fsanitize=address,undefined: both exit clean
    and print the same lines"""
    src = [os.path.join(ROOT, "tests", "fuse_search_host_san.c"), os.path.join(ROOT, "3d_sift_cuda_amd", "csrc", "fuse_host.c")]
    base = ["cc", "-std=c11", "-ffp-contract=off", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include")]
    out = {}
    for name, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])):
        exe = str(tmp_path / ("fuse_search_host_" + name))
        subprocess.run(base + flags + ["-o", exe] + src + ["-lm"], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
        out[name] = r.stdout
    assert out["san"] == out["plain"]
    assert "radius 3 codes sum %d refused %d back 343\n" % (sum(range(343)), 11 ** 3 - 343) in out["san"]
    assert "stats 686 684 8232\n" in out["san"] and "stats under 2 -1 0 0\n" in out["san"] and "of 3 343 -1 " in out["san"]


# The scenario's Dice (mean over the labels 0 .. 4) on the oracle when this was written, per metric and radius (power 1, power 2);
# DESIGN.md section 7k has the table.  Radius 0 is section 7j's SCENARIO_DICE.
SEARCH_DICE = {"ssd": {0: (0.9041, 0.9029), 1: (0.9190, 0.9114), 2: (0.9456, 0.9361), 3: (0.9680, 0.9647)},
               "ncc": {0: (0.8989, 0.9020), 1: (0.9256, 0.9284), 2: (0.9502, 0.9517), 3: (0.9687, 0.9698)}}


@pytest.mark.parametrize("metric", ["ssd", "ncc"])
def test_scenario_the_search_recovers_misregistered_atlases(built, fs, ro, fo, scen, metric):
    """fuse_cases.scenario: in every z slab three of five atlases are wrong by three voxels, which weighted voting can only
    down-weigh.  With a search radius the atlases vote from where their patches fit.  Asserted: the values at r = 0 are section
    7j's recorded ones; power 2 at r = 3 exceeds power 2 at r = 0 by at least half the gap measured on the oracle when this was
    written (SEARCH_DICE); the GPU equals the oracle to the bit (test_gpu_fuse_search.py), so the same holds there."""
    rec = SEARCH_DICE[metric]
    rt, qt, planes = warped_planes(built, fs, ro, fo, scen["target"], leg(scen, metric), scen["vox2key"], metric)
    dice = {}
    for r in (0, 1, 2, 3):
        for power in (1, 2):
            words, rep = fuse_planes(fs, rt, qt, planes, 2, metric, power, r)
            dice[r, power] = mean_dice(fs, fused_labels(words), scen["truth"])[0]
            assert rep["none"] == 0
        print("fuse search scenario %s r %d: power 1 %.4f power 2 %.4f moved %s mean |t|^2 %s" % (
            metric, r, dice[r, 1], dice[r, 2], " ".join(str(a["moved"]) for a in rep["search"]["atlas"]),
            " ".join("%.3f" % (a["dist2_sum"] / v["voters"]) for a, v in zip(rep["search"]["atlas"], rep["atlas"]))))
    assert round(dice[0, 1], 4) == rec[0][0] == SCENARIO_DICE[metric][1] and round(dice[0, 2], 4) == rec[0][1] == SCENARIO_DICE[metric][2]
    gap = rec[3][1] - rec[0][1]
    assert gap >= 0.03
    assert dice[3, 2] >= dice[0, 2] + 0.5 * gap, (dice, rec)
    for r in (1, 2, 3):       # every voxel more of radius helps, under either power
        assert dice[r, 1] > dice[r - 1, 1] and dice[r, 2] > dice[r - 1, 2], (r, dice)
