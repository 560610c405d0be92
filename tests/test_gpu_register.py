"""GPU suite: the affine registration by mutual information against the CPU oracle tests/register_oracle.c,
always through the C-ABI: sift3d_warp_histogram on every map kind, shape, stride, bins, K and form, past the workgroup cap, with
non-finite voxels, under poisoned allocations, call after call, its refusals; sift3d_register_affine on the scenario pair; and
featRegister end to end.  Every comparison of the kernel is integer equality with the oracle; the stage is compared to equal bits
of theta*, M1, every level's iteration count and every score."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from _helpers import run
from register_cases import (BIG, BINS, MAP_KINDS, ODD_PAIR, SCENARIO_SHAPE, SCENARIO_THETA, SMALL_PAIRS, STRIDES, RegisterOracle, all_maps, bits32, corner_error, holes,
                            image_pair, map_of, same_histograms, same_registration, scenario)
from blockmatch_cases import volume

pytestmark = pytest.mark.gpu

FORMS = ("by_brick", "by_map", "by_brick_plane", "by_map_plane")
FV = np.array([[0.0, -0.9, 0.0, 12.5], [1.1, 0.0, 0.0, -3.0], [0.0, 0.0, 1.0, 7.25], [0, 0, 0, 1]], np.float32)
MV = np.array([[0.0, -0.9, 0.0, 12.0], [1.1, 0.0, 0.0, -2.5], [0.0, 0.0, 1.0, 7.0], [0, 0, 0, 1]], np.float32)
M0 = np.array([[1.0, 0.0, 0.0, 0.5], [0.0, 1.0, 0.0, -0.25], [0.0, 0.0, 1.0, 0.0], [0, 0, 0, 1]], np.float32)


@pytest.fixture(scope="module")
def ro(tmp_path_factory):
    return RegisterOracle(tmp_path_factory.mktemp("register_oracle"))


@pytest.fixture(scope="module")
def scene(ro):
    true = ro.map(SCENARIO_THETA, SCENARIO_SHAPE)
    F, M = scenario(tuple(float(v) for v in true.reshape(-1)))
    return true, F, M


def many_maps(K, fshape, mshape, seed=1):
    """K maps: the kinds in turn, each after the first round moved by a small random matrix"""
    rng = np.random.default_rng(seed)
    base = all_maps(fshape, mshape)
    out = []
    for k in range(K):
        A = base[k % len(base)].copy()
        if k >= len(base):
            A += rng.normal(0, 0.02, (3, 4)).astype(np.float32)
        out.append(A)
    return np.stack(out)


# ---- maps, shapes, strides ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shapes", SMALL_PAIRS + [ODD_PAIR], ids=lambda p: "x".join(map(str, p[0])))
def test_every_map_kind_equals_the_oracle(built, ro, shapes):
    """1 voxel, 24 voxels, a brick plus one in x, and 31 x 17 x 13 into 29 x 19 x 11: the seven map kinds in one launch at every
    stride and bins, holes in F and in M"""
    fshape, mshape = shapes
    F, M, fr, mr = image_pair(fshape, mshape)
    maps = all_maps(fshape, mshape)
    for stride in STRIDES:
        for bins in BINS:
            got, want = built.warp_histogram(F, M, maps, fr, mr, stride, bins), ro.warp_hist(F, M, maps, fr, mr, stride, bins)
            same_histograms(got, want)
            assert all(s[0] + e == ro.N and o <= e for s, e, o in zip(got[1], got[2], got[3]))
    if F.size > 24:
        kinds = dict(zip(MAP_KINDS, range(len(MAP_KINDS))))
        assert got[1][kinds["outside"]][0] == 0 and got[3][kinds["outside"]] == ro.N and got[2][kinds["nan"]] == ro.N
        stride1 = built.warp_histogram(F, M, maps, fr, mr, 1, 8)
        assert stride1[1][kinds["identity"]][0] > 0 and 0 < stride1[3][kinds["rotation"]] < F.size and stride1[1][kinds["half"]][0] > 0


@pytest.mark.parametrize("form", FORMS)
def test_every_form_gives_the_same_integers(built, ro, form):
    """the block order and the int16 plane are placement and storage only"""
    F, M, fr, mr = image_pair(*ODD_PAIR)
    maps = many_maps(9, *ODD_PAIR)
    for stride in STRIDES:
        same_histograms(built.warp_histogram(F, M, maps, fr, mr, stride, 32, form=form), ro.warp_hist(F, M, maps, fr, mr, stride, 32))


@pytest.mark.parametrize("K", [1, 2, 24, 32])
def test_map_counts(built, ro, K):
    F, M, fr, mr = image_pair(*ODD_PAIR)
    maps = many_maps(K, *ODD_PAIR)
    for form in ("by_brick", "by_map_plane"):
        got = built.warp_histogram(F, M, maps, fr, mr, 2, 16, form=form)
        assert got[0].shape == (K, 16, 16)
        same_histograms(got, ro.warp_hist(F, M, maps, fr, mr, 2, 16))


def test_past_the_workgroup_cap(built, ro):
    """BIG has more bricks than four trips of the workgroups of a map (test_register_cpu.py holds it to the kernel's #defines): the last
    plane is reached by the fifth trip only, and a change there changes the result"""
    F = volume("smooth", BIG, 5)
    M = (np.float32(-0.5) * np.roll(F, 2, 1) + np.float32(7.0)).astype(np.float32)
    M[-1, -1, -40:] = np.nan
    fr, mr = ro.range(F), ro.range(M)
    maps = np.stack([map_of("identity", BIG, BIG), map_of("rotation", BIG, BIG)])
    want = ro.warp_hist(F, M, maps, fr, mr, 1, 64)
    for form in FORMS:
        same_histograms(built.warp_histogram(F, M, maps, fr, mr, 1, 64, form=form), want)
    F2 = F.copy()
    F2[-1, -1, -100:-50] = np.random.default_rng(1).normal(0, 300, 50).astype(np.float32)
    got, want2 = built.warp_histogram(F2, M, maps, fr, mr, 1, 64), ro.warp_hist(F2, M, maps, fr, mr, 1, 64)
    same_histograms(got, want2)
    assert not np.array_equal(got[0], want[0])
    same_histograms(built.warp_histogram(F, M, maps, fr, mr, 2, 32), ro.warp_hist(F, M, maps, fr, mr, 2, 32))


# ---- non-finite voxels ----------------------------------------------------------------------------------------------------------------------
def test_weight_zero_corner_reaches_the_sample(built, ro):
    """a NaN or infinite moving voxel makes the samples that read it with weight 0 NaN too, as in the oracle"""
    F = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    fr = mr = (np.float32(0), np.float32(23))
    ident = map_of("identity", F.shape, F.shape)
    for bad in (np.nan, np.inf, -np.inf):
        M = F.copy()
        M[0, 0, 1] = bad
        got = built.warp_histogram(F, M, ident, fr, mr, 1, 8)
        same_histograms(got, ro.warp_hist(F, M, ident, fr, mr, 1, 8))
        assert got[2] == [2] and got[3] == [0]
    Fh = F.copy()
    Fh[1, 2, 3], Fh[0, 1, 1] = np.nan, -np.inf
    got = built.warp_histogram(Fh, F, ident, fr, mr, 1, 8)
    same_histograms(got, ro.warp_hist(Fh, F, ident, fr, mr, 1, 8))
    assert got[2] == [2]


def test_identity_map_is_the_joint_histogram_entry(built):
    """on one grid, with finite moving voxels, the identity map gives sift3d_joint_histogram's integers"""
    F, M, fr, mr = image_pair((11, 19, 70), (11, 19, 70), with_holes=False)
    F = holes(F, 3)
    for bins in BINS:
        hist, sums, excluded, outside = built.warp_histogram(F, M, map_of("identity", F.shape, M.shape), fr, mr, 1, bins)
        want = built.joint_histogram(F, M, fr, mr, bins)
        assert np.array_equal(hist[0], want[0]) and sums[0] == want[1] and excluded[0] == want[2] > 0 and outside == [0]


# ---- poisoned allocations, state between calls ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", [0xA7, 0x00])
def test_under_poisoned_allocations(built, ro, byte):
    """every device block of the call holds the byte before the call uses it: a result word or a plane entry that the call does not
    write itself would show"""
    F, M, fr, mr = image_pair(*ODD_PAIR)
    maps = many_maps(9, *ODD_PAIR)
    with built.alloc_fill(byte) as stats:
        for form, blocks in (("by_brick", 4), ("by_map_plane", 5)):
            for stride, bins in ((1, 64), (4, 8)):
                got = built.warp_histogram(F, M, maps, fr, mr, stride, bins, form=form)
                n_blocks, nbytes = stats()
                assert n_blocks == blocks and nbytes >= 4 * (F.size + M.size), (n_blocks, nbytes)
                same_histograms(got, ro.warp_hist(F, M, maps, fr, mr, stride, bins))


def test_second_call_equals_its_oracle(built, ro):
    """two calls in one process with other shapes, bins and K: nothing of the first is left in the second"""
    F, M, fr, mr = image_pair(*ODD_PAIR)
    same_histograms(built.warp_histogram(F, M, many_maps(24, *ODD_PAIR), fr, mr, 1, 64), ro.warp_hist(F, M, many_maps(24, *ODD_PAIR), fr, mr, 1, 64))
    F, M, fr, mr = image_pair(*SMALL_PAIRS[2])
    maps = many_maps(3, *SMALL_PAIRS[2])
    same_histograms(built.warp_histogram(F, M, maps, fr, mr, 2, 8), ro.warp_hist(F, M, maps, fr, mr, 2, 8))
    same_histograms(built.warp_histogram(F, M, maps[:1], fr, mr, 1, 16, form="by_map_plane"), ro.warp_hist(F, M, maps[:1], fr, mr, 1, 16))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals(built, ro):
    """all on the host, before anything is allocated: the extents below are never backed by memory"""
    L = built.hip_lib()
    tiny = np.arange(8, dtype=np.float32)
    ident = map_of("identity", (2, 2, 2), (2, 2, 2))

    def kernel(f=(2, 2, 2), m=(2, 2, 2), n_maps=1, stride=1, fr=(0.0, 7.0), mr=(0.0, 7.0), bins=64, form=-1, maps=ident):
        err, hist, sums = C.create_string_buffer(512), np.zeros(33 * 64 * 64, np.int64), np.zeros(33 * 6, np.int64)
        ex, out = np.zeros(33, np.int64), np.zeros(33, np.int64)
        a = np.ascontiguousarray(np.resize(ident if maps is None else maps, (max(n_maps, 1), 12)), np.float32)
        rc = L.sift3d_warp_histogram(0, tiny.ctypes.data, *f, tiny.ctypes.data, *m, None if maps is None else a.ctypes.data, n_maps, stride, (C.c_float * 2)(*fr),
                                     (C.c_float * 2)(*mr), bins, form, hist.ctypes.data, sums.ctypes.data, ex.ctypes.data, out.ctypes.data, None, err, len(err))
        return rc, err.value.decode()

    with built.alloc_fill(0x5A) as stats:
        for kw, text in (({"f": (4097, 2, 2)}, "fixed: nx = 4097: an extent must be 1 .. 4096"), ({"f": (2, 0, 2)}, "fixed: ny = 0"), ({"m": (2, 2, 4097)}, "moving: nz = 4097"),
                         ({"m": (4096, 4096, 65)}, "moving: nx ny nz = 1090519040: more than 2^30 voxels"), ({"f": (4096, 4096, 65)}, "fixed: nx ny nz = 1090519040: more than 2^30 voxels"),
                         ({"bins": 128}, "bins = 128: 8, 16, 32 or 64"), ({"bins": 12}, "bins = 12"), ({"stride": 3}, "stride = 3: 1, 2, 4 or 8"), ({"stride": 0}, "stride = 0"),
                         ({"stride": 16}, "stride = 16"), ({"n_maps": 0}, "n_maps = 0: 1 .. 32"), ({"n_maps": 33}, "n_maps = 33: 1 .. 32"),
                         ({"fr": (1.0, 1.0)}, "fixed_range = 1 .. 1"), ({"mr": (0.0, float("inf"))}, "moving_range = 0 .. inf"), ({"fr": (float("nan"), 1.0)}, "fixed_range = nan .. 1"),
                         ({"form": 4}, "form = 4: -1 or 0 .. 3"), ({"form": -2}, "form = -2"), ({"maps": None}, "null pointer")):
            rc, err = kernel(**kw)
            assert rc == -1 and text in err, (kw, rc, err)
        with pytest.raises(built.Sift3DError, match="n_maps = 33: 1 .. 32"):
            built.warp_histogram(tiny.reshape(2, 2, 2), tiny.reshape(2, 2, 2), np.zeros((33, 12)), (0, 7), (0, 7))
        # the stage
        F, M, _, _ = image_pair((5, 9, 33), (5, 9, 33), with_holes=False)
        flat, nans = np.full((2, 3, 4), 2.5, np.float32), np.full((2, 3, 4), np.nan, np.float32)
        singular = np.zeros((4, 4), np.float32)
        singular[3, 3] = 1
        for args, kw, text in (((flat, M), {}, "the fixed image has no two distinct finite values"), ((F, nans), {}, "the moving image has no two distinct finite values"),
                               ((F, M), {"dof": 5}, "dof = 5: 3, 6, 7, 9 or 12"), ((F, M), {"bins": 48}, "bins = 48"), ((F, M), {"levels": [(3, 1, 1)]}, "stride[0] = 3"),
                               ((F, M), {"min_overlap": 2.0}, "min_overlap = 2"), ((F, M), {"max_iterations": 0}, "max_iterations = 0"), ((F, M), {"form": 7}, "form = 7"),
                               ((F, M), {"initial": singular}, "a matrix is singular"), ((F, M), {"fixed_vox2key": singular}, "a matrix is singular"),
                               ((F, M), {"moving_vox2key": singular}, "a matrix is singular")):
            with pytest.raises(built.Sift3DError, match=re.escape(text)) as e:
                built.register_affine(*args, **kw)
            assert e.value.code == -1
        assert stats()[0] == 0          # nothing was allocated by any of them
        # the start that is inadmissible: the session's four blocks, and nothing after the check
        far = np.eye(4, dtype=np.float32)
        far[0, 3] = 1000.0
        N = ro.lattice(F.shape, 4)[0]
        with pytest.raises(built.Sift3DError, match="the start is inadmissible: n = 0 of N = %d lattice voxels count, min_overlap = 0.25" % N) as e:
            built.register_affine(F, M, initial=far)
        assert e.value.code == -1 and stats()[0] == 4 and ro.register(F, M, m0=far) == -2


# ---- the stage ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dof, metric", [(12, "nmi"), (12, "mi"), (6, "nmi"), (6, "mi")])
def test_register_affine_equals_the_oracle(built, ro, scene, dof, metric):
    true, F, M = scene
    got, want = built.register_affine(F, M, dof=dof, metric=metric), ro.register(F, M, dof=dof, metric=metric)
    same_registration(got, want)
    assert np.array_equal(bits32(got["map"]), bits32(ro.map(want["theta"], SCENARIO_SHAPE))) and got["stop"] == 0
    before, after = (corner_error(true, m, SCENARIO_SHAPE) for m in (ro.map(np.zeros(12), SCENARIO_SHAPE), got["map"]))
    assert after < before / (4 if dof == 12 else 1)
    # the two records: one K = 2 launch on the whole lattice, held to the oracle's integers
    fr, mr = ro.range(F), ro.range(M)
    hist, sums, excluded, outside = ro.warp_hist(F, M, [ro.map(np.zeros(12), SCENARIO_SHAPE), got["map"]], fr, mr, 1, 32)
    for k, name in enumerate(("before", "after")):
        rec = got[name]
        assert np.array_equal(rec["hist"], hist[k]) and rec["sums"] == sums[k] and rec["excluded"] == excluded[k] and got["outside_" + name] == outside[k]
        assert rec["range_a"] == fr and rec["range_b"] == mr and rec[metric] == ro.measures(hist[k], sums[k])[metric]
    assert got["after"][metric] > got["before"][metric]
    assert all(l["device_ms"] > 0 and l["n_lattice"] == ro.lattice(SCENARIO_SHAPE, l["stride"])[0] for l in got["levels"])


def test_register_affine_in_key_space_and_forms(built, ro, scene):
    """vox2key matrices with a permutation and anisotropic voxels, a start matrix, other levels and bins: the oracle's bits under every form"""
    _, F, M = scene
    kw = dict(dof=9, metric="mi", bins=16, levels=[(8, 2.0, 1.0), (4, 1.0, 0.5)], min_overlap=0.1)
    want = ro.register(F, M, FV, MV, M0, **kw)
    assert sum(l["iterations"] for l in want["levels"]) > 4
    for form in ("default",) + FORMS:
        same_registration(built.register_affine(F, M, FV, MV, M0, form=form, **kw), want)
    got = built.register_affine(F, M, dof=3, levels=[(1, 1.0, 0.001)], max_iterations=3)
    same_registration(got, ro.register(F, M, dof=3, levels=[(1, 1.0, 0.001)], max_iterations=3))
    assert got["stop"] == 1 and got["levels"][0]["stop"] == 1 and got["levels"][0]["iterations"] == 3


# ---- featRegister ---------------------------------------------------------------------------------------------------------------------------
def mi_of(built, tmp_path, a, b):
    r = run(["timeout", "-k", "10", "120", built.FEATCOMPARE, "-d0", a, b], tmp_path)
    return float(r.stdout.split("\n")[5].split()[0])


def test_featregister_end_to_end(built, ro, scene, tmp_path):
    """on NIfTI files the test writes: the .trans.txt is sift3d_write_matrix's of the Python mirror's M1, sift3d_read_similarity reads it
    back, featResample with it raises featCompare's mi over featResample with the start; the report; the error paths"""
    assert os.path.exists(built.FEATREGISTER)
    _, F, M = scene
    built.write_nifti(str(tmp_path / "f.nii"), F)
    built.write_nifti(str(tmp_path / "m.nii"), M)
    start = np.eye(4, dtype=np.float32)
    start[0, 3] = 0.5
    assert built.host_lib().sift3d_write_matrix(os.fsencode(str(tmp_path / "start.trans.txt")), start.ctypes.data) == 0
    key = built.key_vox2key()
    for trans, options, kw in (("-", [], {}), ("start.trans.txt", ["-f6", "-mmi", "-b16", "-o0.5"], {"dof": 6, "metric": "mi", "bins": 16, "min_overlap": 0.5, "initial": start})):
        run(["timeout", "-k", "10", "300", built.FEATREGISTER, "-d0"] + options + ["f.nii", "m.nii", trans, "out"], tmp_path)
        want = built.register_affine(F, M, key, key, **kw)
        same_registration(want, ro.register(F, M, key, key, kw.get("initial"), **{k: v for k, v in kw.items() if k != "initial"}))
        assert built.host_lib().sift3d_write_matrix(os.fsencode(str(tmp_path / "want.trans.txt")), np.ascontiguousarray(want["result"]).ctypes.data) == 0
        assert open(str(tmp_path / "out.trans.txt")).read() == open(str(tmp_path / "want.trans.txt")).read()
        got = built.read_similarity(str(tmp_path / "out.trans.txt"))
        assert np.abs(got - want["result"]).max() < 1e-6 * max(1.0, np.abs(want["result"]).max()) and np.array_equal(got[3], [0, 0, 0, 1])
        # the report: the mirror's text but for the device times
        strip = lambda text: [" ".join(l.split()[:-1]) if l[:1].isdigit() and len(l.split()) == 10 else l for l in text.split("\n")]
        report = open(str(tmp_path / "out.register.txt")).read()
        assert report.startswith("# featRegister v1.0\n# dof %d metric %s bins %d stop 0\n" % (want["dof"], kw.get("metric", "nmi"), want["bins"]))
        assert strip(report)[1:] == strip(built.register_report_text(want))
    # the default run's matrix goes through featResample unchanged and improves the match
    run(["timeout", "-k", "10", "300", built.FEATREGISTER, "f.nii", "m.nii", "-", "out"], tmp_path)
    assert built.host_lib().sift3d_write_matrix(os.fsencode(str(tmp_path / "unit.trans.txt")), np.eye(4, dtype=np.float32).ctypes.data) == 0
    run(["timeout", "-k", "10", "120", built.FEATRESAMPLE, "-d0", "f.nii", "m.nii", "unit.trans.txt", "w0.nii"], tmp_path)
    run(["timeout", "-k", "10", "120", built.FEATRESAMPLE, "-d0", "f.nii", "m.nii", "out.trans.txt", "w1.nii"], tmp_path)
    mi0, mi1 = mi_of(built, tmp_path, "f.nii", "w0.nii"), mi_of(built, tmp_path, "f.nii", "w1.nii")
    assert mi1 > mi0 > 0, (mi0, mi1)
    for argv, text in ((["-x", "f.nii", "m.nii", "-", "o"], "Usage: featRegister"), (["-f5", "f.nii", "m.nii", "-", "o"], "bad degrees of freedom: -f5"),
                       (["-mssd", "f.nii", "m.nii", "-", "o"], "bad metric: -mssd"), (["-b12", "f.nii", "m.nii", "-", "o"], "bad number of bins: -b12"),
                       (["-o2", "f.nii", "m.nii", "-", "o"], "bad overlap fraction: -o2"), (["f.nii", "m.nii", "o"], "Usage: featRegister"),
                       (["f.nii", "missing.nii", "-", "o"], "could not read input file: missing.nii"), (["f.nii", "m.nii", "missing.trans.txt", "o"], "could not read transform file: missing.trans.txt")):
        r = subprocess.run(["timeout", "-k", "10", "60", built.FEATREGISTER] + argv, cwd=tmp_path, capture_output=True, text=True)
        assert r.returncode == 255 and text in r.stdout, (argv, r.returncode, r.stdout[-500:])
        assert not os.path.exists(str(tmp_path / "o.trans.txt")) and not os.path.exists(str(tmp_path / "o.register.txt"))
