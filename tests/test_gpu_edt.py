"""GPU suite: the exact distance map and the surface distances against the CPU oracle tests/edt_oracle.c, word
for word, always through the C-ABI: sift3d_distance_map on every site pattern, spacing and line length, its refusals,
sift3d_surface_distances against the oracle's lists pushed through sift3d_surface_stats, and featFuse -t -m and featOverlap end to
end.  No comparison has a tolerance."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from _helpers import run
from edt_cases import NONE, PATTERNS, SPACINGS, EdtOracle, blocky_pair, cube_pair, distance_block, oracle_records, same_record, sites
from fuse_cases import leg, scenario
from resample_cases import ResampleOracle

pytestmark = pytest.mark.gpu

# kernels_edt.hip: edt_x_kernel turns a row into words of 64 voxels (one ballot each); edt_line_kernel stages EDT_CHUNK = 64
# candidates of a y or z line at a time and sweeps the line's outputs 64 at a time
CHUNK_X, CHUNK_Y, CHUNK_Z = 64, 64, 64
# (nz, ny, nx): every line shorter than a wave; odd extents; more than one tile along x; a line longer than a wave's row and a
# workgroup on each axis in turn; one voxel more than the chunk on each axis in turn; more rows (4 x 2048) and more line tiles (2048)
# than the launches have waves and workgroups for, so that both kernels go round their grid loops
SHAPES = [(2, 3, 4), (5, 9, 33), (11, 19, 70), (3, 5, 300), (5, 300, 3), (300, 3, 5), (3, 5, CHUNK_X + 1), (5, CHUNK_Y + 1, 3), (CHUNK_Z + 1, 3, 5),
          (2060, 4, 1)]


@pytest.fixture(scope="module")
def ed(tmp_path_factory):
    return EdtOracle(tmp_path_factory.mktemp("edt_oracle"))


# ---- sift3d_distance_map ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES)
def test_distance_map_equals_the_oracle(built, ed, shape, pattern):
    s = sites(shape, pattern)
    for spacing in SPACINGS:
        got, want = built.distance_map(s, spacing), ed.map(s, spacing)
        assert got.dtype == np.uint64 and got.shape == s.shape and np.array_equal(got, want), (spacing, int((got != want).sum()))
        if pattern == "none":
            assert (got == NONE).all()
        else:
            assert ((got == 0) == (s != 0)).all() and (got < 2 ** 58).all()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_distance_map_at_the_edge_of_its_range(built, ed, axis):
    """4096 voxels along one axis (x, y and z in turn) at 65535 um, the only site at one end: the far end reads (4095 * 65535)^2"""
    shape = [2, 2, 2]
    shape[2 - axis] = 4096
    spacing = [1, 1, 1]
    spacing[axis] = 65535
    s = np.zeros(shape, np.uint8)
    s[0, 0, 0] = 1
    got, ms = built.distance_map(s, spacing, return_ms=True)
    assert np.array_equal(got, ed.map(s, spacing))
    far = [0, 0, 0]
    far[2 - axis] = 4095
    assert int(got[tuple(far)]) == (4095 * 65535) ** 2 and int(got[-1, -1, -1]) == (4095 * 65535) ** 2 + 2
    assert len(ms) == 4 and all(np.isfinite(t) and t >= 0 for t in ms)   # total, x, y, z: reported, never judged


def test_distance_map_refusals(built):
    """all on the host, before anything is allocated: the extents below are never backed by memory"""
    L = built.hip_lib()
    tiny, out = np.zeros(8, np.uint8), np.zeros(8, np.uint64)

    def call(nx, ny, nz, sp):
        err = C.create_string_buffer(512)
        rc = L.sift3d_distance_map(0, tiny.ctypes.data, nx, ny, nz, (C.c_uint32 * 3)(*sp), out.ctypes.data, None, err, len(err))
        return rc, err.value.decode()

    one = (1000, 1000, 1000)
    for args, text in (((0, 2, 2, one), "nx = 0"), ((2, 4097, 2, one), "ny = 4097"), ((2, 2, 0, one), "nz = 0"), ((2, 2, 4097, one), "nz = 4097"),
                       ((2, 2, 2, (0, 1, 1)), r"spacing_um[0] = 0"), ((2, 2, 2, (1, 65536, 1)), r"spacing_um[1] = 65536"),
                       ((2, 2, 2, (1, 1, 65536)), r"spacing_um[2] = 65536"), ((4096, 4096, 65, one), "more than 2^30 voxels")):
        rc, err = call(*args)
        assert rc != 0 and text in err, (args, rc, err)
    assert call(4096, 4096, 65, one)[1].startswith("nx ny nz = %d" % (4096 * 4096 * 65))
    with pytest.raises(built.Sift3DError, match="spacing_um"):
        built.distance_map(np.ones((2, 2, 2), np.uint8), (1000, 0, 1000))


# ---- sift3d_surface_distances ----------------------------------------------------------------------------------------------------------
def same_records(got, want):
    assert [r["label"] for r in got] == [r["label"] for r in want]
    for g, w in zip(got, want):
        same_record(g, w)


def test_surface_distances_of_the_cube_pair(built, ed):
    a, b = cube_pair()
    spacing = (3000, 700, 1300)
    got, ms = built.surface_distances(a, b, spacing, return_ms=True)
    same_records(got, oracle_records(built, ed, a, b, spacing))
    assert len(got) == 1 and got[0]["max_ab"] == got[0]["max_ba"] == 4 * 3000 ** 2 and got[0]["hausdorff_mm"] == 6.0 and np.isfinite(ms) and ms >= 0
    zero = built.surface_distances(a, a, spacing)
    same_records(zero, oracle_records(built, ed, a, a, spacing))
    assert zero[0]["max_ab"] == 0 and zero[0]["assd_mm"] == 0.0
    # first_label 0 includes the background, 1 skips it
    with_zero = built.surface_distances(a, b, spacing, first_label=0)
    same_records(with_zero, oracle_records(built, ed, a, b, spacing, first_label=0))
    assert [r["label"] for r in with_zero] == [0, 1]
    same_record(with_zero[1], got[0])


@pytest.mark.parametrize("spacing", [(1000, 1000, 1000), (700, 1300, 3000)])
def test_surface_distances_of_blocky_volumes_with_unlabelled_voxels(built, ed, spacing):
    a, b = blocky_pair()
    assert (~np.isfinite(a)).sum() > 100 and (~np.isfinite(b)).sum() > 100 and (a == 65535).any()
    got = built.surface_distances(a, b, spacing, first_label=0)
    want = oracle_records(built, ed, a, b, spacing, first_label=0)
    same_records(got, want)
    assert [r["label"] for r in got] == [0, 1, 2, 7, 65535] and all(r["n_a"] > 100 and r["n_b"] > 100 and r["max_ab"] > 0 for r in got)
    same_records(built.surface_distances(a, b, spacing), want[1:])


def test_surface_distances_of_a_label_in_one_volume_only(built, ed):
    a, b = blocky_pair(seed=6)
    a[a == 7] = 9                  # 9 only in a, 7 only in b
    b[2:5, 3:9, 10:30] = 12        # 12 only in b
    got = built.surface_distances(a, b, (1000, 2000, 500))
    same_records(got, oracle_records(built, ed, a, b, (1000, 2000, 500)))
    by = {r["label"]: r for r in got}
    assert sorted(by) == [1, 2, 7, 9, 12, 65535]
    for l, in_a in ((9, True), (7, False), (12, False)):
        r = by[l]
        assert (r["n_a"] > 0) == in_a and (r["n_b"] > 0) == (not in_a) and (r["voxels_a"] > 0) == in_a
        assert r["max_ab"] == r["p95_ba"] == NONE and np.isnan(r["hausdorff_mm"]) and np.isnan(r["hd95_mm"]) and np.isnan(r["assd_mm"])
    assert by[1]["n_a"] > 0 and by[1]["n_b"] > 0 and by[1]["hausdorff_mm"] > 0


def test_surface_distances_past_one_grid_of_the_label_kernel(built, ed):
    """kernels_label.hip: label_plane_kernel has at most 2048 workgroups of 256 threads and goes round a grid loop beyond them.  578000
    voxels are more than one round and no multiple of 64, so the last validity word holds 16 voxels.  Label 1 is a box around voxel
    524288, where the second round starts; label 2 lies wholly in the first round; NaN voxels are scattered in both volumes, in both
    boxes and among the last 16 voxels."""
    shape = (5, 340, 340)
    n, grid = shape[0] * shape[1] * shape[2], 2048 * 256
    assert n > grid and n % 64 == 16
    a, b = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    a[3:5, 176:192, 0:40] = 1
    b[3:5, 178:194, 3:43] = 1
    a[0:3, 10:20, 10:30] = 2
    b[0:3, 12:22, 9:29] = 2
    fa, fb = a.reshape(-1), b.reshape(-1)
    assert fa[grid - 1] == 1 and fa[grid] == 1 and fb[grid + 3] == 1 and fa[:grid].max() == 2 and (fa[grid:] != 2).all() and (fb[grid:] != 2).all()
    rng = np.random.default_rng(11)
    for flat, last in ((fa, (n - 16, n - 7, n - 1)), (fb, (n - 16, n - 2))):
        flat[rng.random(n) < 0.001] = np.nan
        flat[list(last)] = np.nan
    a[3, 176, 5] = a[0, 10, 15] = b[3, 178, 8] = b[0, 12, 14] = np.nan     # one inside every box
    spacing = (700, 1300, 3000)
    got = built.surface_distances(a, b, spacing, first_label=1)
    want = oracle_records(built, ed, a, b, spacing, first_label=1)
    same_records(got, want)
    assert [r["label"] for r in got] == [1, 2] and all(0 < r["n_a"] < 2000 and 0 < r["n_b"] < 2000 and r["max_ab"] > 0 for r in got)


def test_surface_distances_refusals(built):
    a, b = blocky_pair()
    with pytest.raises(built.Sift3DError, match=r"5 labels from 0 on .* max_labels = 4"):
        built.surface_distances(a, b, first_label=0, max_labels=4)
    with pytest.raises(built.Sift3DError, match=r"4 labels from 1 on .* max_labels = 3"):
        built.surface_distances(a, b, max_labels=3)
    assert len(built.surface_distances(a, b, max_labels=4)) == 4
    bad = b.copy()
    bad[3, 2, 1] = 0.5
    with pytest.raises(built.Sift3DError, match=r"volume b: the label 0\.5 at voxel %d " % ((3 * 19 + 2) * 70 + 1)):
        built.surface_distances(a, bad)
    with pytest.raises(built.Sift3DError, match=r"volume a: the label 0\.5 at voxel %d " % ((3 * 19 + 2) * 70 + 1)):
        built.surface_distances(bad, b)
    with pytest.raises(built.Sift3DError, match=r"spacing_um\[2\] = 70000"):
        built.surface_distances(a, b, (1000, 1000, 70000))


# ---- featFuse -t -m and featOverlap ----------------------------------------------------------------------------------------------------
def dice_block(built, a, b):
    """the Dice table as featFuse -t and featOverlap write it"""
    labels, ca, cb, cc = built.label_overlap(a, b)
    dice = [2 * int(c) / (int(x) + int(y)) for x, y, c in zip(ca, cb, cc)]
    t = "# label fused truth both dice\n" + "".join("%d\t%d\t%d\t%d\t%.6f\n" % (l, x, y, c, d) for l, x, y, c, d in zip(labels, ca, cb, cc, dice))
    return t + "# mean dice %.6f over %d labels\n" % (sum(dice) / len(dice), len(dice))


def test_featfuse_with_surface_distances(built, ed, tmp_path_factory, tmp_path):
    """the scenario through featFuse -t with and without -m: the report with -m is the report without it plus the block that the
    oracle's lists of (fused, truth) imply; the fused labels themselves are test_gpu_fuse.py's business"""
    scen = scenario(built, ResampleOracle(tmp_path_factory.mktemp("resample_oracle")), tmp_path_factory.mktemp("fuse_scenario"))
    built.write_nifti(str(tmp_path / "target.nii"), scen["target"])
    built.write_nifti(str(tmp_path / "truth.nii"), scen["truth"])
    groups = []
    for k, a in enumerate(leg(scen, "ssd")):
        built.write_nifti(str(tmp_path / ("atlas%d.nii" % k)), a["image"])
        built.write_nifti(str(tmp_path / ("labels%d.nii" % k)), a["labels"])
        built.write_matrix(str(tmp_path / ("atlas%d.trans.txt" % k)), a["t"])
        built.write_field(str(tmp_path / ("atlas%d.field.nii" % k)), a["field"])
        groups += ["atlas%d.nii" % k, "labels%d.nii" % k, "atlas%d.trans.txt" % k, "atlas%d.field.nii" % k]
    run(["timeout", "-k", "10", "120", built.FEATFUSE, "-d0", "-t", "truth.nii", "target.nii", "plain.nii"] + groups, tmp_path)
    run(["timeout", "-k", "10", "120", built.FEATFUSE, "-d0", "-t", "truth.nii", "-m", "target.nii", "out.nii"] + groups, tmp_path)
    plain, text = open(str(tmp_path / "plain.nii.fuse.txt")).read(), open(str(tmp_path / "out.nii.fuse.txt")).read()
    for name in ("", ".conf.nii"):
        assert open(str(tmp_path / ("plain.nii" + name)), "rb").read() == open(str(tmp_path / ("out.nii" + name)), "rb").read()
    fused, _ = built.read_nifti(str(tmp_path / "out.nii"))
    assert " none 0 " in plain and "spacing_um" not in plain       # every voxel has a voter: the written labels are the scored ones
    want = oracle_records(built, ed, fused, scen["truth"], (1000, 1000, 1000))
    assert [r["label"] for r in want] == [1, 2, 3, 4]
    assert text == plain + distance_block(want, (1000, 1000, 1000))
    assert "# spacing_um 1000 1000 1000\n" in text and "# mean hausdorff_mm " in text
    # usage: -m needs -t; a voxel size that has no micrometres
    r = subprocess.run(["timeout", "-k", "10", "60", built.FEATFUSE, "-m", "target.nii", "o.nii"] + groups, cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 255 and "-m without -t" in r.stdout and "Usage: featFuse" in r.stdout
    built.write_nifti(str(tmp_path / "wide.nii"), scen["target"], voxel=(1.0, 70.0, 1.0))
    r = subprocess.run(["timeout", "-k", "10", "60", built.FEATFUSE, "-t", "truth.nii", "-m", "wide.nii", "o.nii"] + groups, cwd=tmp_path, capture_output=True,
                       text=True)
    assert r.returncode == 255 and "the voxel size 70 mm along y" in r.stdout and not os.path.exists(str(tmp_path / "o.nii"))


def test_featoverlap(built, ed, tmp_path):
    assert os.path.exists(built.FEATOVERLAP)
    a, b = blocky_pair()
    voxel, spacing = (0.7, 1.3, 3.0), (700, 1300, 3000)
    built.write_nifti(str(tmp_path / "a.nii"), a, voxel=voxel)
    built.write_nifti(str(tmp_path / "b.nii"), b, voxel=voxel)
    dice = dice_block(built, a, b)
    blocks = {z: distance_block(oracle_records(built, ed, a, b, spacing, first_label=0 if z else 1), spacing) for z in (False, True)}
    assert blocks[True].count("\n") == blocks[False].count("\n") + 1 and "\n65535\t" in blocks[False]
    for options, want in (([], dice), (["-z"], dice), (["-m"], dice + blocks[False]), (["-m", "-z"], dice + blocks[True])):
        run(["timeout", "-k", "10", "60", built.FEATOVERLAP, "-d0"] + options + ["a.nii", "b.nii", "out.txt"], tmp_path)
        assert open(str(tmp_path / "out.txt")).read() == want, options
    r = run(["timeout", "-k", "10", "60", built.FEATOVERLAP, "-m", "a.nii", "b.nii"], tmp_path)     # without <out.txt>: the standard output
    assert r.stdout == dice + blocks[False]
    # errors with text: another grid, another voxel size, a label that is none, a missing file, usage
    built.write_nifti(str(tmp_path / "short.nii"), b[:, :, :-1], voxel=voxel)
    built.write_nifti(str(tmp_path / "wide.nii"), b, voxel=(0.7, 1.3, 3.5))
    bad = b.copy()
    bad[0, 0, 0] = 0.5
    built.write_nifti(str(tmp_path / "bad.nii"), bad, voxel=voxel)
    for argv, text in ((["a.nii", "short.nii"], "not on one grid: 70 x 19 x 11 voxels against 69 x 19 x 11"),
                       (["-m", "a.nii", "wide.nii"], "not on one grid: voxels of 700 x 1300 x 3000 um against 700 x 1300 x 3500 um"),
                       (["a.nii", "bad.nii"], "neither non-finite nor an integer 0 .. 65535: bad.nii"), (["a.nii", "missing.nii"], "could not read input file: missing.nii"),
                       (["a.nii"], "Usage: featOverlap"), (["-x", "a.nii", "b.nii"], "Usage: featOverlap")):
        r = subprocess.run(["timeout", "-k", "10", "60", built.FEATOVERLAP] + argv, cwd=tmp_path, capture_output=True, text=True)
        assert r.returncode == 255 and text in r.stdout, (argv, r.returncode, r.stdout[-500:])
