"""GPU suite: the image similarity against the CPU oracle tests/similarity_oracle.c, always through the C-ABI:
sift3d_joint_histogram and sift3d_image_similarity on every voxel count, pair, bins and same_scale setting, past the launch cap,
with labels, under poisoned allocations, call after call, their refusals, and featCompare end to end.  Every comparison is integer
equality with the oracle; the derived values are host arithmetic on those integers and are held to the oracle's bits."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from _helpers import run
from blockmatch_cases import volume
from similarity_cases import BIG, BINS, COUNT_SHAPES, LABEL_SHAPE, PAIR_SHAPES, PAIRS, SimilarityOracle, labels_of, pair, same_result

pytestmark = pytest.mark.gpu

FLUSHES = ("slices", "atomics")


@pytest.fixture(scope="module")
def so(tmp_path_factory):
    return SimilarityOracle(tmp_path_factory.mktemp("similarity_oracle"))


# ---- voxel counts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", COUNT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_voxel_count_equals_the_oracle(built, so, shape):
    """1, 24, counts of every remainder mod the voxels per thread, around one workgroup's stretch, several workgroups: the kernel alone
    with given ranges (a single voxel has none of its own), and the stage with both flush forms"""
    A, B = pair("smooth_holes", shape) if min(shape) > 1 else pair("iid", shape)
    ra, rb = (np.float32(-900.0), np.float32(1100.0)), (np.float32(-500.0), np.float32(400.0))
    if min(shape) == 1:
        ra, rb = (np.float32(0.0), np.float32(200.0)), (np.float32(50.0), np.float32(150.0))
    for bins in BINS:
        hist, sums, excluded = built.joint_histogram(A, B, ra, rb, bins)
        want = so.count(A, B, ra, rb, bins)
        assert hist.dtype == np.int64 and np.array_equal(hist, want[0]) and sums == want[1] and excluded == want[2], (bins, sums, want[1])
        assert sums[0] + excluded == A.size
    for flush in FLUSHES:
        same_result(built.image_similarity(A, B, flush=flush), so.similarity(A, B))


# ---- pairs ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", PAIR_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", PAIRS)
def test_pairs_equal_the_oracle(built, so, kind, shape):
    A, B = pair(kind, shape)
    for same_scale in (False, True):
        for bins in BINS:
            got, want = built.image_similarity(A, B, bins=bins, same_scale=same_scale), so.similarity(A, B, bins=bins, same_scale=same_scale)
            same_result(got, want)
            assert got["kernel_ms"] >= 0 and np.isfinite(got["kernel_ms"])      # reported, never judged
    s = 10 - int(np.log2(bins))
    if kind == "binary":          # q is 0 or 1023: all mass in the four corner cells, Saa at its end
        corners = got["hist"][[0, 0, -1, -1], [0, -1, 0, -1]]
        assert corners.sum() == got["n"] == A.size and got["sums"][3] == int((A == 1).sum()) * 1023 * 1023 and got["sums"][1] == int((A == 1).sum()) * 1023
    if kind == "equal":
        assert np.array_equal(got["hist"], np.diag(np.diag(got["hist"]))) and got["nmi"] == 2.0
    if kind == "constant":        # one cell holds all but the two corner voxels
        assert got["hist"].max() == A.size - 2 and got["hist"][int(round(3.25 / 10 * 1023)) >> s].max() == A.size - 2
    if kind == "smooth_holes":
        assert 0 < got["excluded"] < A.size


def test_flush_forms_agree_on_a_full_histogram(built, so):
    """iid values fill most of the 4096 cells in every workgroup; the one-cell pair sends every add to one LDS word and one result word"""
    for kind in ("iid", "constant"):
        A, B = pair(kind, (11, 19, 70))
        want = so.similarity(A, B)
        for flush in FLUSHES:
            same_result(built.image_similarity(A, B, flush=flush), want)
    assert (so.similarity(*pair("iid", (11, 19, 70)))["hist"] > 0).sum() > 1500


# ---- past the launch cap ----------------------------------------------------------------------------------------------------------------
def test_past_the_launch_cap(built, so):
    """BIG has more voxels than one grid of workgroups takes in a trip (test_similarity_cpu.py holds it to the kernel's #defines): the
    last 32 stretches and more are reached only by the grid loop's second trip, and the last thread loads a part of its voxels"""
    A = volume("smooth", BIG, 5)
    B = (np.float32(-0.5) * np.roll(A, 2, 1) + np.float32(7.0)).astype(np.float32)
    B[-1, -1, -40:] = np.nan          # holes in the second trip
    rng = np.random.default_rng(1)
    L = labels_of("blobby", BIG)
    for flush in FLUSHES:
        same_result(built.image_similarity(A, B, flush=flush), so.similarity(A, B))
    same_result(built.image_similarity(A, B, L, bins=32, same_scale=True), so.similarity(A, B, L, bins=32, same_scale=True))
    # what only the second trip sees decides: a change in the last stretch changes the result
    B2 = B.copy()
    B2[-1, -1, -100:-50] = rng.normal(0, 300, 50).astype(np.float32)
    got = built.image_similarity(A, B2)
    same_result(got, so.similarity(A, B2))
    assert not np.array_equal(got["hist"], so.similarity(A, B)["hist"])


# ---- labels -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["blobby", "iid", "one", "top", "n64"])
def test_label_sums_equal_the_oracle(built, so, kind):
    A, B = pair("smooth_holes", LABEL_SHAPE)
    L = labels_of(kind, LABEL_SHAPE)
    for same_scale in (False, True):
        for bins, flush in ((64, "slices"), (16, "atomics")):
            got, want = built.image_similarity(A, B, L, bins=bins, same_scale=same_scale, flush=flush), so.similarity(A, B, L, bins=bins, same_scale=same_scale)
            same_result(got, want)
    rows = got["labels"]
    assert [r["label"] for r in rows] == sorted(r["label"] for r in rows) and all(r["n"] > 0 for r in rows)
    labelled = sum(r["n"] for r in rows)
    if kind == "blobby":          # NaN, +-inf and -0 among the labels: unlabelled voxels are in no row and stay in the whole-image numbers
        assert [r["label"] for r in rows] == [0, 1, 2, 3, 4] and labelled < got["n"] and not np.isfinite(L).all() and np.signbit(L[L == 0]).any()
    else:
        assert labelled == got["n"]
    assert {"one": [3], "top": [0, 65535]}.get(kind, [r["label"] for r in rows]) == [r["label"] for r in rows]
    assert kind != "n64" or len(rows) == 64
    # the whole-image numbers do not depend on the labels
    same_result({k: v for k, v in got.items() if k != "labels"}, so.similarity(A, B, bins=16, same_scale=True))


def test_labels_on_excluded_voxels_take_no_row(built, so):
    """a label that stands only on voxels that do not count is in no row, and does not count towards max_labels"""
    A, B = pair("smooth", LABEL_SHAPE)
    L = labels_of("n64", LABEL_SHAPE)
    L[0, 0, :5] = 7
    A[0, 0, :5] = np.nan
    got = built.image_similarity(A, B, L)
    same_result(got, so.similarity(A, B, L))
    assert len(got["labels"]) == 64 and 7 not in [r["label"] for r in got["labels"]]


def test_refusals(built):
    """all on the host, before anything is allocated: the extents below are never backed by memory"""
    L = built.hip_lib()
    tiny = np.arange(8, dtype=np.float32)

    def stage(nx, ny, nz, labels=None, a=tiny, **kw):
        err, p, rec, n = C.create_string_buffer(512), built.similarity_params(**kw), built.SimilarityRecord(), C.c_int32(-1)
        lrec = (built.SimilarityLabelRecord * 64)()
        rc = L.sift3d_image_similarity(a.ctypes.data, tiny.ctypes.data, None if labels is None else labels.ctypes.data, nx, ny, nz, C.byref(p), C.byref(rec), lrec,
                                       C.byref(n), err, len(err))
        return rc, err.value.decode()

    def kernel(nx, ny, nz, bins, ra=(0.0, 7.0), rb=(0.0, 7.0)):
        err, hist, sums, ex = C.create_string_buffer(512), np.zeros(64 * 64, np.int64), np.zeros(6, np.int64), C.c_int64(0)
        rc = L.sift3d_joint_histogram(0, tiny.ctypes.data, tiny.ctypes.data, nx, ny, nz, (C.c_float * 2)(*ra), (C.c_float * 2)(*rb), bins, hist.ctypes.data,
                                      sums.ctypes.data, C.byref(ex), None, err, len(err))
        return rc, err.value.decode()

    for args, kw, text in (((4097, 2, 2), {}, "nx = 4097: an extent must be 1 .. 4096"), ((2, 0, 2), {}, "ny = 0"), ((2, 2, 4097), {}, "nz = 4097"),
                           ((4096, 4096, 65), {}, "more than 2^30 voxels"), ((2, 2, 2), {"bins": 128}, "bins = 128: 8, 16, 32 or 64"),
                           ((2, 2, 2), {"bins": 12}, "bins = 12"), ((2, 2, 2), {"same_scale": 2}, "same_scale = 2: 0 or 1"),
                           ((2, 2, 2), {"max_labels": 65}, "max_labels = 65: 1 .. 64"), ((2, 2, 2), {"max_labels": 0}, "max_labels = 0"), ((2, 2, 2), {"flush": 2}, "flush = 2: 0 or 1")):
        rc, err = stage(*args, **kw)
        assert rc == -1 and text in err, (args, kw, rc, err)
    for args, kw, text in (((4097, 2, 2, 64), {}, "nx = 4097"), ((2, 2, 2, 48), {}, "bins = 48: 8, 16, 32 or 64"), ((2, 2, 2, 64), {"ra": (1.0, 1.0)}, "a_range = 1 .. 1"),
                           ((2, 2, 2, 64), {"rb": (0.0, float("inf"))}, "b_range = 0 .. inf"), ((2, 2, 2, 64), {"ra": (float("nan"), 1.0)}, "a_range = nan .. 1")):
        rc, err = kernel(*args, **kw)
        assert rc == -1 and text in err, (args, kw, rc, err)
    bad = tiny.copy()
    bad[5] = 0.5
    rc, err = stage(2, 2, 2, labels=bad)
    assert rc == -1 and "the label 0.5 at voxel 5 is neither non-finite nor an integer 0 .. 65535" in err
    # 65 labels: refused with the count, nothing dropped; 64 of them: accepted (test_label_sums_equal_the_oracle[n64])
    A, B = pair("smooth", LABEL_SHAPE)
    with pytest.raises(built.Sift3DError, match="65 labels on counted voxels: more than max_labels = 64") as e:
        built.image_similarity(A, B, labels_of("n65", LABEL_SHAPE))
    assert e.value.code == -1
    with pytest.raises(built.Sift3DError, match="7 labels on counted voxels: more than max_labels = 6"):
        built.image_similarity(A, B, labels_of("iid", LABEL_SHAPE), max_labels=6)
    assert len(built.image_similarity(A, B, labels_of("iid", LABEL_SHAPE), max_labels=7)["labels"]) == 7


def test_empty_ranges_launch_nothing(built, so):
    flat, nans, ok = np.full((2, 3, 4), 2.5, np.float32), np.full((2, 3, 4), np.nan, np.float32), volume("random", (2, 3, 4), 1)
    for a, b, same_scale, want in ((flat, ok, False, 1), (ok, nans, False, 2), (nans, flat, False, 3), (flat, ok, True, 1), (ok, flat, True, 0)):
        with built.alloc_fill(0x5A) as stats:
            got = built.image_similarity(a, b, ok.round() if want else None, same_scale=same_scale)
            blocks, _ = stats()
        same_result(got, so.similarity(a, b, ok.round() if want else None, same_scale=same_scale))
        assert got["empty_range"] == want and (blocks == 0) == (want != 0)      # nothing allocated, so nothing launched
        if want:
            assert got["n"] == 0 and got["excluded"] == 24 and got["labels"] == [] and np.isnan(got["mi"])


# ---- poisoned allocations -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", [0xA7, 0x00])
def test_stage_under_poisoned_allocations(built, so, byte):
    """every device block of the call holds the byte before the call uses it: a result word, a slice word or a table byte that the call
    does not write itself would show"""
    A, B = pair("smooth_holes", LABEL_SHAPE)
    L = labels_of("blobby", LABEL_SHAPE)
    with built.alloc_fill(byte) as stats:
        for flush in FLUSHES:
            for bins in (64, 8):
                got = built.image_similarity(A, B, L, bins=bins, flush=flush)
                blocks, nbytes = stats()
                assert blocks >= 5 and nbytes >= 12 * A.size, (blocks, nbytes)
                same_result(got, so.similarity(A, B, L, bins=bins))
        hist, sums, excluded = built.joint_histogram(A, B, (-900.0, 1100.0), (-500.0, 400.0), 32)
        assert stats()[0] >= 3
        want = so.count(A, B, (-900.0, 1100.0), (-500.0, 400.0), 32)
        assert np.array_equal(hist, want[0]) and sums == want[1] and excluded == want[2]


# ---- state between calls --------------------------------------------------------------------------------------------------------------
def test_second_call_equals_its_oracle(built, so):
    """two calls in one process with different bins, sizes and label sets: nothing of the first is left in the second"""
    A, B = pair("iid", (11, 19, 70))
    same_result(built.image_similarity(A, B, labels_of("n64", (11, 19, 70)), bins=64), so.similarity(A, B, labels_of("n64", (11, 19, 70)), bins=64))
    A, B = pair("smooth_holes", (5, 9, 33))
    same_result(built.image_similarity(A, B, labels_of("one", (5, 9, 33)), bins=8, same_scale=True), so.similarity(A, B, labels_of("one", (5, 9, 33)), bins=8, same_scale=True))
    same_result(built.image_similarity(A, B, bins=16), so.similarity(A, B, bins=16))


# ---- featCompare ----------------------------------------------------------------------------------------------------------------------
def test_featcompare_end_to_end(built, so, tmp_path):
    """on NIfTI files the test writes: the text is the Python mirror's, whose numbers are the oracle's; the two error paths"""
    assert os.path.exists(built.FEATCOMPARE)
    shape = (11, 19, 70)
    A, B = pair("smooth_holes", shape)
    L = labels_of("blobby", shape)
    for name, vol in (("a.nii", A), ("b.nii", B), ("l.nii", L), ("short.nii", A[:, :, :-1])):
        built.write_nifti(str(tmp_path / name), vol)
    for options, kw, labels in (([], {}, None), (["-b16", "-s"], {"bins": 16, "same_scale": True}, None), (["-l", "l.nii", "-b32"], {"bins": 32}, L),
                                (["-s", "-l", "l.nii"], {"same_scale": True}, L)):
        got = built.image_similarity(A, B, labels, **kw)
        same_result(got, so.similarity(A, B, labels, **kw))
        want = "# featCompare v1.0 bins %d\n" % got["bins"] + built.similarity_report_text(got)
        run(["timeout", "-k", "10", "120", built.FEATCOMPARE, "-d0"] + options + ["a.nii", "b.nii", "out.txt"], tmp_path)
        assert open(str(tmp_path / "out.txt")).read() == want
        lines = want.split("\n")
        assert lines[1].startswith("# range_a ") and lines[2].startswith("# range_b ") and lines[3] == "# same_scale %d" % got["same_scale"]
        assert lines[4] == "# voxels %d %d" % (got["n"], got["excluded"]) and len(lines[5].split()) == 7 and (lines[5].split()[3] == "nan") == (not got["same_scale"])
        if labels is not None:
            assert lines[6] == "# label n rho rms" and [l.split()[0] for l in lines[7:-1]] == ["0", "1", "2", "3", "4"]
    r = run(["timeout", "-k", "10", "120", built.FEATCOMPARE, "a.nii", "b.nii"], tmp_path)     # without <out.txt>: the standard output
    assert r.stdout == "# featCompare v1.0 bins 64\n" + built.similarity_report_text(built.image_similarity(A, B))
    for argv, text in ((["a.nii", "short.nii"], "not on one grid: 70 x 19 x 11 voxels against 69 x 19 x 11"),
                       (["-l", "short.nii", "a.nii", "b.nii"], "not on the images' grid: 70 x 19 x 11 voxels against 69 x 19 x 11"),
                       (["-x", "a.nii", "b.nii"], "Usage: featCompare"), (["-b12", "a.nii", "b.nii"], "bad number of bins: -b12"), (["a.nii"], "Usage: featCompare"),
                       (["a.nii", "missing.nii"], "could not read input file: missing.nii")):
        r = subprocess.run(["timeout", "-k", "10", "60", built.FEATCOMPARE] + argv + ["o.txt"] * (len(argv) > 1), cwd=tmp_path, capture_output=True, text=True)
        assert r.returncode == 255 and text in r.stdout, (argv, r.returncode, r.stdout[-500:])
        assert not os.path.exists(str(tmp_path / "o.txt"))
