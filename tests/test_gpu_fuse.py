"""GPU suite: multi-atlas label fusion against the CPU oracle tests/fuse_oracle.c, bit for bit, always through
the C-ABI: fuse_weight_kernel in both forms and under both similarities, fuse_label_kernel and fuse_vote_kernel on constructed
votes, the stage on the five-atlas scenario against its restatement (fuse_cases.cpu_fuse), and featFuse end to end."""
import os
import subprocess

import numpy as np
import pytest

from _helpers import run
from field_cases import FieldOracle
from blockmatch_cases import lattice_numpy
from fuse_cases import FALLBACK, NONE, U_ONE, ZERO_SHIFT_SHAPE, FuseOracle, assert_zero_shift_identity, cpu_fuse, fused_labels, leg, pair, same_report, scenario
from resample_cases import ResampleOracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fz(tmp_path_factory):
    return FuseOracle(tmp_path_factory.mktemp("fuse_oracle"))


@pytest.fixture(scope="module")
def ro(tmp_path_factory):
    return ResampleOracle(tmp_path_factory.mktemp("resample_oracle"))


@pytest.fixture(scope="module")
def fo(tmp_path_factory):
    return FieldOracle(tmp_path_factory.mktemp("field_oracle"))


@pytest.fixture(scope="module")
def scen(built, ro, tmp_path_factory):
    return scenario(built, ro, tmp_path_factory.mktemp("fuse_scenario"))


@pytest.fixture(scope="module")
def wanted(built, fz, ro, fo, scen):
    """the scenario through the restatement, once per (metric, power)"""
    memo = {}

    def get(metric, power):
        if (metric, power) not in memo:
            memo[metric, power] = cpu_fuse(built, fz, ro, fo, scen["target"], leg(scen, metric), scen["vox2key"], metric=metric, power=power)
        return memo[metric, power]
    return get


# ---- sift3d_fuse_weights ---------------------------------------------------------------------------------------------------------------
# (nz, ny, nx), b: every patch clipped on every axis; one brick plus one voxel per axis; several bricks at the three half-widths
WEIGHT_CASES = [((2, 3, 4), 2), ((5, 9, 33), 2), ((11, 19, 70), 1), ((11, 19, 70), 2), ((11, 19, 70), 6)]


@pytest.mark.parametrize("generic", [0, 1])
@pytest.mark.parametrize("metric", ["ssd", "ncc"])
@pytest.mark.parametrize("shape,b", WEIGHT_CASES)
def test_weights_equal_the_oracle(built, fz, shape, b, metric, generic):
    T, W = pair(shape, 7)
    got = built.fuse_weights(T, W, block=b, metric=metric, generic=generic)
    want = fz.weights(T, W, b, metric)
    assert got.dtype == np.uint16 and np.array_equal(got, want)
    assert 0 < want.max() <= U_ONE and len(np.unique(want)) > 1


@pytest.mark.parametrize("generic", [0, 1])
@pytest.mark.parametrize("metric", ["ssd", "ncc"])
def test_weights_with_holes_a_given_range_and_a_volume_of_nan(built, fz, metric, generic):
    T, W = pair((11, 19, 70), 9, holes=True)
    assert (~np.isfinite(T)).sum() > 100 and (~np.isfinite(W)).sum() > 100
    want = fz.weights(T, W, 2, metric)
    assert np.array_equal(built.fuse_weights(T, W, block=2, metric=metric, generic=generic), want) and want.max() > 0
    # the range the stage passes under the correlation: another volume's
    rng = (np.float32(-900.0), np.float32(1300.0))
    assert np.array_equal(built.fuse_weights(T, W, block=2, metric=metric, w_range=rng, generic=generic), fz.weights(T, W, 2, metric, w_range=rng))
    # identical volumes; a W of NaN alone: no patch has a voxel, u = 0 everywhere
    assert (built.fuse_weights(T, T, block=2, metric=metric, generic=generic)[np.isfinite(T)] > 0).any()
    nan = np.full(T.shape, np.nan, np.float32)
    got = built.fuse_weights(T, nan, block=2, metric=metric, generic=generic)
    assert np.array_equal(got, fz.weights(T, nan, 2, metric)) and not got.any()
    got = built.fuse_weights(T, nan, block=2, metric=metric, w_range=rng, generic=generic)   # the kernel itself on a volume of -1
    assert not got.any()


def test_weights_equal_the_block_matchers_cost_at_the_zero_shift(built):
    """The weight kernel, the block matcher and the search take a patch's worth from one source (patch_cost.h), so they are held to
    each other: fuse_cases.assert_zero_shift_identity between fuse_weights and the block matchers' words (both quantise T with T's
    range, and W with W's own under "ncc" and with T's under "ssd"), and the search at radius 0 gives the weight kernel's u.
    test_fuse_cpu.py has the same identity between the oracles."""
    T, W = pair(ZERO_SHIFT_SHAPE, 5)
    first, count = lattice_numpy(ZERO_SHIFT_SHAPE, 1, 2, 1)
    for metric, match in (("ssd", built.block_match), ("ncc", built.block_match_ncc)):
        u = built.fuse_weights(T, W, block=2, metric=metric)
        assert_zero_shift_identity(metric, u, match(T, W, first, 1, count, 2, 1), first)
        assert np.array_equal(built.fuse_search(T, W, block=2, radius=0, metric=metric)[0], u)


def test_weights_of_identical_volumes_and_refusals(built):
    T, _ = pair((5, 9, 33), 1)
    for metric in ("ssd", "ncc"):
        for generic in (0, 1):
            assert (built.fuse_weights(T, T, block=2, metric=metric, generic=generic) == U_ONE).all()
    for kw, text in ((dict(block=0), "half-width"), (dict(block=7), "half-width"), (dict(metric=2), "metric")):
        with pytest.raises(built.Sift3DError, match=text):
            built.fuse_weights(T, T, **kw)
    with pytest.raises(built.Sift3DError, match="no two distinct finite values"):
        built.fuse_weights(np.full(T.shape, 3.0, np.float32), T)


# ---- sift3d_fuse_vote ------------------------------------------------------------------------------------------------------------------
def votes(K, n, seed):
    """K planes of u and labels over n voxels: few labels (ties are common), label 65535 among them, unlabelled voxels, voxels where
    every u is 0, voxels where nobody votes"""
    rng = np.random.default_rng(seed)
    u = rng.choice(np.array([0, 1, 2, 3, 100, 32767, U_ONE], np.uint16), (K, n))
    labels = rng.choice(np.array([0, 1, 2, 7, 65535, np.nan, np.inf], np.float32), (K, n), p=[0.15, 0.2, 0.2, 0.15, 0.15, 0.1, 0.05])
    u[:, ::7] = 0
    labels[:, 5::11] = np.nan
    u[:, 3::13] = U_ONE
    return list(u), list(labels)


@pytest.mark.parametrize("power", [0, 1, 2])
@pytest.mark.parametrize("K", [1, 2, 32])
def test_vote_equals_the_oracle(built, fz, K, power):
    u, labels = votes(K, 3001, K)
    got, want = built.fuse_vote(u, labels, power=power), fz.vote(u, labels, power)
    assert np.array_equal(got, want)
    w0 = want[:, 0]
    assert ((w0 & NONE) != 0).sum() >= 3001 // 11 and (w0 & 0xffff == 65535).any()
    assert ((w0 >> 16) & 63).max() == K and (((w0 & FALLBACK) != 0).any() == (power > 0))


def test_vote_constructed_ties_and_refusals(built, fz):
    nan = np.float32(np.nan)
    labels = [np.array([9, 5, 1, 4, nan], np.float32), np.array([3, 65535, 1, nan, nan], np.float32), np.array([3, 7, 2, 4, np.inf], np.float32)]
    u = [np.array([20, 10, 10, 0, 5], np.uint16), np.array([10, 10, 10, 7, 5], np.uint16), np.array([10, 10, 30, 0, 5], np.uint16)]
    for power, winners in ((0, [3, 5, 1, 4, 0]), (1, [3, 5, 2, 4, 0]), (2, [9, 5, 2, 4, 0])):
        got = built.fuse_vote(u, labels, power=power)
        assert np.array_equal(got, fz.vote(u, labels, power)) and [int(x) & 0xffff for x in got[:, 0]] == winners
    one = np.array([U_ONE], np.uint16)
    words = built.fuse_vote([one] * 32, [np.array([65535], np.float32)] * 32, power=2)
    assert int(words[0, 0]) == 65535 | (32 << 16) and int(words[0, 1]) == 65535
    # refused on the host, before any launch
    with pytest.raises(built.Sift3DError, match="33 atlases"):
        built.fuse_vote([one] * 33, [np.array([1], np.float32)] * 33)
    with pytest.raises(built.Sift3DError, match=r"atlas 1: the label 0\.5 at voxel 2 "):
        built.fuse_vote([u[0], u[1]], [labels[0], np.array([3, 1, 0.5, 2, 0.5], np.float32)])
    with pytest.raises(built.Sift3DError, match="power"):
        built.fuse_vote(u, labels, power=3)
    with pytest.raises(built.Sift3DError, match="exceeds 32768"):
        built.fuse_vote([np.array([U_ONE + 1], np.uint16)], [np.array([1], np.float32)])


# ---- sift3d_fuse_labels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,power", [("ssd", 2), ("ncc", 2), ("ncc", 1), ("ssd", 0)])
def test_stage_equals_its_restatement_on_the_scenario(built, scen, wanted, metric, power):
    words, rep = built.fuse_labels(scen["target"], leg(scen, metric), scen["vox2key"], metric=metric, power=power)
    want, want_rep = wanted(metric, power)
    assert np.array_equal(words, want)
    same_report(rep, want_rep)
    assert all((r["weight_ms"] > 0) == (power > 0) and r["warp_ms"] > 0 for r in rep["atlas"]) and rep["vote_ms"] > 0


def test_stage_zero_field_no_field_nan_atlas_and_refusals(built, fz, ro, fo, scen):
    a = dict(leg(scen, "ncc")[1])
    zero = dict(a["field"], disp=np.zeros_like(a["field"]["disp"]))
    flat = dict(a, image=np.full(a["image"].shape, 5.0, np.float32), field=None)             # an empty range under the correlation
    holes = a["labels"].copy()
    holes[10:20] = np.nan
    atlases = [dict(a, field=zero), dict(a, field=None), flat, dict(a, labels=holes, field=None)]
    words, rep = built.fuse_labels(scen["target"], atlases, scen["vox2key"], metric="ncc", block=1)
    want, want_rep = cpu_fuse(built, fz, ro, fo, scen["target"], atlases, scen["vox2key"], block=1, metric="ncc")
    assert np.array_equal(words, want)
    same_report(rep, want_rep)
    assert [r["empty_range"] for r in rep["atlas"]] == [0, 0, 1, 0] and rep["atlas"][2]["mean_u"] == 0 and rep["atlas"][3]["voters"] < rep["atlas"][1]["voters"]
    # an atlas with a zero field gives the words of the same atlas with no field
    w_zero, r_zero = built.fuse_labels(scen["target"], [dict(a, field=zero)], scen["vox2key"], metric="ncc")
    w_none, r_none = built.fuse_labels(scen["target"], [dict(a, field=None)], scen["vox2key"], metric="ncc")
    assert np.array_equal(w_zero, w_none) and r_zero["atlas"][0]["mean_u"] == r_none["atlas"][0]["mean_u"] > 0
    # refusals: all on the host
    bad = a["labels"].copy()
    bad[3, 2, 1] = 0.5
    with pytest.raises(built.Sift3DError, match=r"atlas 1: the label 0\.5 at voxel %d " % ((3 * 48 + 2) * 48 + 1)):
        built.fuse_labels(scen["target"], [a, dict(a, labels=bad)], scen["vox2key"])
    with pytest.raises(built.Sift3DError, match="33 atlases"):
        built.fuse_labels(scen["target"], [a] * 33, scen["vox2key"])
    with pytest.raises(built.Sift3DError, match="max_voxels"):
        built.fuse_labels(scen["target"], [a] * 3, scen["vox2key"], max_voxels=2 * scen["target"].size)
    with pytest.raises(built.Sift3DError, match="no two distinct finite values"):
        built.fuse_labels(np.zeros((4, 4, 4), np.float32), [a], scen["vox2key"])


# ---- featFuse --------------------------------------------------------------------------------------------------------------------------
def report_text(K, block, metric, power, fill, rep, fused, truth, built):
    """<output labels>.fuse.txt as featFuse.c writes it"""
    t = "# atlases %d block %d metric %s power %d fill %g\n" % (K, block, metric, power, fill)
    t += "# target quantised over %g .. %g\n" % (float(rep["lo"]), float(rep["hi"]))
    t += "# voxels %d none %d fallback %d\n" % (fused.size, rep["none"], rep["fallback"])
    t += "# atlas voters support mean_u empty_range\n"
    for k, r in enumerate(rep["atlas"]):
        t += "%d\t%d\t%d\t%.6f\t%d\n" % (k + 1, r["voters"], r["support"], r["mean_u"], r["empty_range"])
    labels, ca, cb, cc = built.label_overlap(fused, fused if truth is None else truth)
    t += "# label voxels\n" + "".join("%d\t%d\n" % (l, a) for l, a in zip(labels, ca) if a > 0)
    if truth is not None:
        dice = [2 * int(c) / (int(a) + int(b)) for a, b, c in zip(ca, cb, cc)]
        t += "# label fused truth both dice\n" + "".join("%d\t%d\t%d\t%d\t%.6f\n" % (l, a, b, c, d) for l, a, b, c, d in zip(labels, ca, cb, cc, dice))
        t += "# mean dice %.6f over %d labels\n" % (sum(dice) / len(dice), len(dice))
    return t


@pytest.mark.parametrize("options,metric,power,fill,fields", [(["-t", "truth.nii"], "ssd", 2, 0.0, True), (["-c", "-p0", "-f-1"], "ncc", 0, -1.0, True),
                                                              (["-c", "-b1", "-t", "truth.nii"], "ncc", 2, 0.0, False)])
def test_featfuse_end_to_end(built, fz, ro, fo, scen, wanted, tmp_path, options, metric, power, fill, fields):
    assert os.path.exists(built.FEATFUSE)
    built.write_nifti(str(tmp_path / "target.nii"), scen["target"])
    built.write_nifti(str(tmp_path / "truth.nii"), scen["truth"])
    atlases = leg(scen, metric) if fields else [dict(a, field=None) for a in leg(scen, metric)[:2]]
    groups = []
    for k, a in enumerate(atlases):
        built.write_nifti(str(tmp_path / ("atlas%d.nii" % k)), a["image"])
        built.write_nifti(str(tmp_path / ("labels%d.nii" % k)), a["labels"])
        built.write_matrix(str(tmp_path / ("atlas%d.trans.txt" % k)), a["t"])
        if fields:
            built.write_field(str(tmp_path / ("atlas%d.field.nii" % k)), a["field"])
        groups += ["atlas%d.nii" % k, "labels%d.nii" % k, "atlas%d.trans.txt" % k, "atlas%d.field.nii" % k if fields else "-"]
        assert np.array_equal(built.read_similarity(str(tmp_path / ("atlas%d.trans.txt" % k))), a["t"])
    run(["timeout", "-k", "10", "120", built.FEATFUSE, "-d0"] + options + ["target.nii", "out.nii"] + groups, tmp_path)
    block = 1 if "-b1" in options else 2
    want, rep = wanted(metric, power) if fields else cpu_fuse(built, fz, ro, fo, scen["target"], atlases, scen["vox2key"], block=block, metric=metric,
                                                              power=power)
    none = (want[..., 0] & NONE) != 0
    if fill != 0.0:
        assert none.sum() == 0   # the scenario's atlases cover the target: -f is exercised by the argument parser and the report's first line
    labels = fused_labels(want, fill)
    conf = (want[..., 1].astype(np.float32) / np.float32(65535.0)).astype(np.float32)
    for name, vol in (("out.nii", labels), ("out.nii.conf.nii", conf)):
        got, hdr = built.read_nifti(str(tmp_path / name))
        assert hdr["dims"] == (40, 40, 40, 1) and hdr["datatype"] == 16 and got.tobytes() == vol.tobytes()
        assert open(str(tmp_path / name), "rb").read()[-vol.nbytes:] == vol.tobytes()
    truth = scen["truth"] if "-t" in options else None
    text = open(str(tmp_path / "out.nii.fuse.txt")).read()
    assert text == report_text(len(atlases), block, metric, power, fill, rep, fused_labels(want), truth, built)
    if truth is not None:
        assert "# mean dice " in text and "\n4\t" in text


def test_featfuse_usage_errors(built, tmp_path):
    """argument errors end the program before it opens a file or a device"""
    for argv in (["target.nii", "out.nii", "atlas.nii", "labels.nii", "atlas.trans.txt"],            # the fourth argument of the group is missing
                 ["target.nii", "out.nii"], ["-p3", "t.nii", "o.nii", "a", "b", "c", "-"], ["-b7", "t.nii", "o.nii", "a", "b", "c", "-"],
                 ["-x", "t.nii", "o.nii", "a", "b", "c", "-"]):
        r = subprocess.run(["timeout", "-k", "10", "60", built.FEATFUSE] + argv, cwd=tmp_path, capture_output=True, text=True)
        assert r.returncode == 255 and "Usage: featFuse" in r.stdout, (argv, r.returncode, r.stdout[-500:])
    r = subprocess.run(["timeout", "-k", "10", "60", built.FEATFUSE, "target.nii", "out.nii", "atlas.nii", "labels.nii", "atlas.trans.txt"], cwd=tmp_path,
                       capture_output=True, text=True)
    assert "every atlas takes four arguments" in r.stdout
    r = subprocess.run(["timeout", "-k", "10", "60", built.FEATFUSE, "missing.nii", "out.nii", "a.nii", "b.nii", "c.txt", "-"], cwd=tmp_path,
                       capture_output=True, text=True)
    assert r.returncode == 255 and "could not read input file: missing.nii" in r.stdout
