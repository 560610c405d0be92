"""GPU suite: the local search of the label fusion against the CPU oracle tests/fuse_search_oracle.c, bit for
bit, always through the C-ABI: fuse_search_kernel in both forms and under both similarities, its output through the vote, the stage
sift3d_fuse_labels_search on the five-atlas scenario against its restatement (fuse_search_cases.cpu_fuse_search), featFuse -s end to
end, and the refusals with their text."""
import os
import subprocess

import numpy as np
import pytest

from _helpers import run
from field_cases import FieldOracle
from fuse_cases import NONE, U_ONE, cpu_fuse, fused_labels, leg, pair, same_report, scenario
from fuse_search_cases import NO_SHIFT, FuseSearchOracle, block_labels, cpu_fuse_search, same_search_report, shift_stats, shifted_pair
from resample_cases import ResampleOracle
from test_gpu_fuse import report_text

pytestmark = pytest.mark.gpu


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


@pytest.fixture(scope="module")
def wanted(built, fs, ro, fo, scen):
    """the scenario through the restatement at r = 2, once per (metric, power)"""
    memo = {}

    def get(metric, power):
        if (metric, power) not in memo:
            memo[metric, power] = cpu_fuse_search(built, fs, ro, fo, scen["target"], leg(scen, metric), scen["vox2key"], metric=metric, power=power,
                                                  search=2)
        return memo[metric, power]
    return get


@pytest.fixture(scope="module")
def oracle_of(fs):
    """the oracle's brute force, once per case: both kernel forms are held to the same words"""
    memo = {}

    def get(key, T, W, labels, b, r, metric, w_range=None):
        if key not in memo:
            memo[key] = fs.search(T, W, labels, b, r, metric, w_range=w_range)
        return memo[key]
    return get


def same_nan(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.nan_to_num(a, nan=-1.0), np.nan_to_num(b, nan=-1.0))


def same_search(got, want):
    assert got[0].dtype == np.uint16 and got[1].dtype == np.uint16
    assert np.array_equal(got[0], want[0]), "u: %d voxels differ" % int((got[0] != want[0]).sum())
    assert np.array_equal(got[1], want[1]), "shift: %d voxels differ" % int((got[1] != want[1]).sum())
    assert (got[2] is None) == (want[2] is None) and (got[2] is None or same_nan(got[2], want[2]))


# ---- sift3d_fuse_search ----------------------------------------------------------------------------------------------------------------
# (nz, ny, nx), b, r: every patch and every shift clipped; one brick plus one voxel per axis; several bricks at every (b, r) that
# has a form of its own, the largest tiles (3, 3) and (5, 1), and the smallest
SEARCH_CASES = [((2, 3, 4), 2, 3), ((5, 9, 33), 2, 2), ((11, 19, 70), 1, 1), ((11, 19, 70), 2, 1), ((11, 19, 70), 2, 2), ((11, 19, 70), 2, 3),
                ((11, 19, 70), 3, 3), ((11, 19, 70), 5, 1)]


@pytest.mark.parametrize("generic", [0, 1])
@pytest.mark.parametrize("metric", ["ssd", "ncc"])
@pytest.mark.parametrize("shape,b,r", SEARCH_CASES)
def test_search_equals_the_oracle(built, oracle_of, shape, b, r, metric, generic):
    T, W = shifted_pair(shape, 7, (1, -1, 1))
    labels = block_labels(shape, 2, nan_block=False)
    got = built.fuse_search(T, W, labels, block=b, radius=r, metric=metric, generic=generic)
    want = oracle_of((shape, b, r, metric), T, W, labels, b, r, metric)
    same_search(got, want)
    assert 0 < want[0].max() <= U_ONE and len(np.unique(want[0])) > 1 and (want[1] != NO_SHIFT).all()
    if min(shape) > 2 * r:
        assert shift_stats(want[1], r)[0] > 0          # some voxels moved


@pytest.mark.parametrize("generic", [0, 1])
@pytest.mark.parametrize("metric", ["ssd", "ncc"])
def test_search_with_holes_nan_labels_no_labels_a_given_range_and_a_w_of_nan(built, fs, oracle_of, metric, generic):
    shape = (11, 19, 70)
    T, W = shifted_pair(shape, 9, (-1, 1, 2), holes=True)
    assert (~np.isfinite(T)).sum() > 100 and (~np.isfinite(W)).sum() > 100
    labels = block_labels(shape, 4)                       # a NaN block wider than the radius, and scattered NaN and infinite voxels
    want = oracle_of(("holes", metric), T, W, labels, 2, 2, metric)
    same_search(built.fuse_search(T, W, labels, block=2, radius=2, metric=metric, generic=generic), want)
    none = want[1] == NO_SHIFT
    assert 0 < none.sum() < none.size / 4 and np.array_equal(none, want[0] == 0xffff) and (want[0][~none] > 0).any()
    # without labels: every shift inside the volume is a candidate, nothing is picked
    got = built.fuse_search(T, W, None, block=2, radius=3, metric=metric, generic=generic)
    same_search(got, oracle_of(("holes, no labels", metric), T, W, None, 2, 3, metric))
    assert got[2] is None and (got[1] != NO_SHIFT).all()
    # the range the stage passes under the correlation: another volume's
    rng = (np.float32(-900.0), np.float32(1300.0))
    same_search(built.fuse_search(T, W, labels, block=2, radius=1, metric=metric, w_range=rng, generic=generic),
                oracle_of(("holes, range", metric), T, W, labels, 2, 1, metric, w_range=rng))
    # a W of NaN alone: no patch has a voxel, u = 0 and every tie goes to the smallest shift that may be picked
    nan = np.full(shape, np.nan, np.float32)
    for kw in ({}, {"w_range": rng}):
        got = built.fuse_search(T, nan, labels, block=2, radius=2, metric=metric, generic=generic, **kw)
        same_search(got, oracle_of(("holes, nan", metric), T, nan, labels, 2, 2, metric))
        assert not got[0][~none].any() and (got[1][np.isfinite(labels)] == fs.code(2, (0, 0, 0))).all()


@pytest.mark.parametrize("metric", ["ssd", "ncc"])
@pytest.mark.parametrize("b", [1, 2, 6])
def test_radius_zero_is_fuse_weights(built, metric, b):
    T, W = pair((11, 19, 70), 9, holes=True)
    u, shift, picked = built.fuse_search(T, W, None, block=b, radius=0, metric=metric)
    assert np.array_equal(u, built.fuse_weights(T, W, block=b, metric=metric)) and not shift.any() and picked is None and u.max() > 0


@pytest.mark.parametrize("power", [1, 2])
def test_search_output_through_the_vote_equals_the_oracle(built, fs, power):
    """three atlases (one moved, one with unlabelled regions, one of NaN alone) searched and voted on the GPU, and on the oracle"""
    shape = (11, 19, 70)
    T, W1 = shifted_pair(shape, 3, (2, 0, -1))
    _, W2 = shifted_pair(shape, 4, (0, 0, 0), holes=True)
    Ws = [W1, W2, np.full(shape, np.nan, np.float32)]
    Ms = [block_labels(shape, 1, nan_block=False), block_labels(shape, 5), np.where(block_labels(shape, 6) > 1, np.nan, 7).astype(np.float32)]
    got = [built.fuse_search(T, W, M, block=2, radius=2, metric="ssd") for W, M in zip(Ws, Ms)]
    want = [fs.search(T, W, M, 2, 2, "ssd", sat=True) for W, M in zip(Ws, Ms)]
    for g, w in zip(got, want):
        same_search(g, w)
    # u = 0xffff comes with a picked label of NaN: sift3d_fuse_vote takes u <= 32768, so those voxels' u is sent as 0
    words = built.fuse_vote([np.where(g[0] == 0xffff, 0, g[0]) for g in got], [g[2] for g in got], power=power)
    want_words = fs.vote([np.where(w[0] == 0xffff, 0, w[0]) for w in want], [w[2] for w in want], power)
    assert np.array_equal(words, want_words)
    w0 = want_words[..., 0]
    assert ((w0 >> 16) & 63).max() == 3 and ((w0 >> 16) & 63).min() < 3 and len(np.unique(w0 & 0xffff)) >= 4


# ---- sift3d_fuse_labels_search ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,power", [("ssd", 2), ("ncc", 1)])
def test_stage_with_a_search_equals_its_restatement_on_the_scenario(built, fs, scen, wanted, metric, power):
    words, rep = built.fuse_labels(scen["target"], leg(scen, metric), scen["vox2key"], metric=metric, power=power, search=2)
    want, want_rep = wanted(metric, power)
    assert np.array_equal(words, want)
    same_report(rep, want_rep)
    same_search_report(rep, want_rep)
    assert all(a["search_ms"] > 0 and a["moved"] > 0 for a in rep["search"]["atlas"]) and all(r["weight_ms"] > 0 for r in rep["atlas"])
    # the search pays on the scenario: the fused labels are nearer the truth than section 7j's
    from fuse_cases import mean_dice
    plain = built.fuse_labels(scen["target"], leg(scen, metric), scen["vox2key"], metric=metric, power=power)[0]
    assert mean_dice(fs, fused_labels(words), scen["truth"])[0] > mean_dice(fs, fused_labels(plain), scen["truth"])[0] + 0.02


def test_stage_search_zero_empty_range_and_refusals(built, fs, ro, fo, scen):
    atlases = leg(scen, "ncc")[:2]
    plain, plain_rep = built.fuse_labels(scen["target"], atlases, scen["vox2key"], metric="ncc")
    words, rep = built._fuse_stage("sift3d_fuse_labels_search", scen["target"], atlases, scen["vox2key"], 0, 0, {"metric": "ncc"})
    assert np.array_equal(words, plain) and rep["search"]["radius"] == 0 and all(a["moved"] == 0 and a["dist2_sum"] == 0 for a in rep["search"]["atlas"])
    same_report(rep, plain_rep)
    # an atlas without a range under the correlation has nothing to search by: it votes as in section 7j; block 1, no field
    a = dict(atlases[1], field=None)
    holes = a["labels"].copy()
    holes[10:22] = np.nan
    mixed = [a, dict(a, image=np.full(a["image"].shape, 5.0, np.float32)), dict(a, labels=holes)]
    words, rep = built.fuse_labels(scen["target"], mixed, scen["vox2key"], metric="ncc", block=1, search=3)
    want, want_rep = cpu_fuse_search(built, fs, ro, fo, scen["target"], mixed, scen["vox2key"], block=1, metric="ncc", search=3)
    assert np.array_equal(words, want)
    same_report(rep, want_rep)
    same_search_report(rep, want_rep)
    assert [r["empty_range"] for r in rep["atlas"]] == [0, 1, 0] and rep["search"]["atlas"][1]["moved"] == 0 and rep["search"]["atlas"][0]["moved"] > 0
    # refusals: all on the host, before any launch
    T = scen["target"]
    for kw, text in ((dict(search=4), "search radius must be 0 .. 3"), (dict(search=-1), "search radius must be 0 .. 3"),
                     (dict(search=3, block=4), "half-width plus the search radius must not exceed 6"),
                     (dict(search=1, power=0), "a search needs weights to search by"), (dict(search=1, block=7), "half-width")):
        with pytest.raises(built.Sift3DError, match=text):
            built.fuse_labels(T, atlases, scen["vox2key"], **kw)
    small, _ = pair((5, 9, 33), 1)
    for kw, text in ((dict(radius=4), "search radius must be 0 .. 3"), (dict(radius=3, block=4), "must not exceed 6"), (dict(radius=1, block=0), "half-width"),
                     (dict(radius=1, metric=2), "metric")):
        with pytest.raises(built.Sift3DError, match=text):
            built.fuse_search(small, small, None, **kw)
    with pytest.raises(built.Sift3DError, match=r"the label 0\.5 at voxel 3 "):
        built.fuse_search(small, small, np.where(np.arange(small.size).reshape(small.shape) == 3, 0.5, 1).astype(np.float32))


# ---- featFuse -s -----------------------------------------------------------------------------------------------------------------------
def search_text(rep):
    """the lines <output labels>.fuse.txt gains with -s, as featFuse.c writes them after the atlas table"""
    t = "# search radius %d\n# atlas moved mean_dist2\n" % rep["search"]["radius"]
    for k, (a, s) in enumerate(zip(rep["atlas"], rep["search"]["atlas"])):
        t += "%d\t%d\t%.6f\n" % (k + 1, s["moved"], s["dist2_sum"] / a["voters"] if a["voters"] else 0.0)
    return t


def featfuse(built, scen, tmp_path, metric, options):
    built.write_nifti(str(tmp_path / "target.nii"), scen["target"])
    built.write_nifti(str(tmp_path / "truth.nii"), scen["truth"])
    groups = []
    for k, a in enumerate(leg(scen, metric)):
        built.write_nifti(str(tmp_path / ("atlas%d.nii" % k)), a["image"])
        built.write_nifti(str(tmp_path / ("labels%d.nii" % k)), a["labels"])
        built.write_matrix(str(tmp_path / ("atlas%d.trans.txt" % k)), a["t"])
        built.write_field(str(tmp_path / ("atlas%d.field.nii" % k)), a["field"])
        groups += ["atlas%d.nii" % k, "labels%d.nii" % k, "atlas%d.trans.txt" % k, "atlas%d.field.nii" % k]
    run(["timeout", "-k", "10", "120", built.FEATFUSE, "-d0"] + options + ["target.nii", "out.nii"] + groups, tmp_path)
    return [open(str(tmp_path / name), "rb").read() for name in ("out.nii", "out.nii.conf.nii", "out.nii.fuse.txt")]


def test_featfuse_with_a_search_end_to_end(built, fs, ro, fo, scen, wanted, tmp_path):
    assert os.path.exists(built.FEATFUSE)
    got = featfuse(built, scen, tmp_path, "ssd", ["-s2", "-t", "truth.nii"])
    want, rep = wanted("ssd", 2)
    labels = fused_labels(want, 0.0)
    conf = (want[..., 1].astype(np.float32) / np.float32(65535.0)).astype(np.float32)
    for name, vol, raw in (("out.nii", labels, got[0]), ("out.nii.conf.nii", conf, got[1])):
        vol_got, hdr = built.read_nifti(str(tmp_path / name))
        assert hdr["dims"] == (40, 40, 40, 1) and hdr["datatype"] == 16 and vol_got.tobytes() == vol.tobytes() and raw[-vol.nbytes:] == vol.tobytes()
    # the report of section 7j with the search's lines after the atlas table
    base = report_text(5, 2, "ssd", 2, 0.0, rep, fused_labels(want), scen["truth"], built)
    cut = base.index("# label voxels\n")
    assert got[2].decode() == base[:cut] + search_text(rep) + base[cut:]
    assert "# search radius 2\n" in got[2].decode() and "# mean dice " in got[2].decode()


def test_featfuse_without_a_search_is_unchanged_and_usage_errors(built, fs, ro, fo, scen, tmp_path):
    got = featfuse(built, scen, tmp_path, "ssd", ["-t", "truth.nii"])
    want, rep = cpu_fuse(built, fs, ro, fo, scen["target"], leg(scen, "ssd"), scen["vox2key"], metric="ssd", power=2)
    labels = fused_labels(want, 0.0)
    conf = (want[..., 1].astype(np.float32) / np.float32(65535.0)).astype(np.float32)
    assert got[0][-labels.nbytes:] == labels.tobytes() and got[1][-conf.nbytes:] == conf.tobytes()
    assert got[2].decode() == report_text(5, 2, "ssd", 2, 0.0, rep, fused_labels(want), scen["truth"], built) and b"search" not in got[2]
    # argument errors end the program before it opens a file or a device
    for argv, text in ((["-s4"], "bad search radius"), (["-s0"], "bad search radius"), (["-s"], "bad search radius"), (["-s1x"], "bad search radius"),
                       (["-p0", "-s1"], "a search needs weights to search by"), (["-s1", "-p0"], "a search needs weights to search by"),
                       (["-b4", "-s3"], "must not exceed 6")):
        r = subprocess.run(["timeout", "-k", "10", "60", built.FEATFUSE] + argv + ["t.nii", "o.nii", "a", "b", "c", "-"], cwd=tmp_path, capture_output=True,
                           text=True)
        assert r.returncode == 255 and "Usage: featFuse" in r.stdout and text in r.stdout, (argv, r.returncode, r.stdout[-500:])
    assert "-s<radius>" in r.stdout
