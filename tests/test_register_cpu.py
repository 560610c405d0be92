"""CPU suite: the affine registration by mutual information without a GPU -- the oracle
tests/register_oracle.c against a float32 numpy restatement that shares no code with it, the hand cases, the product's host code
(register_host.c) against the oracle bit for bit, the shapes that take the GPU kernel past its launch cap, the host file under the
sanitizers as a stand-alone program, and the scenario the feature is there for, on the oracle.

The scenario's figures (oracle, 48 x 44 x 40 voxels, 60 blobs, folded intensities, corners moved by 4.71 voxels): 12 dof nmi 32 bins
ends at 0.087 voxels, 6 dof at 1.92; DESIGN.md section 7q has the table."""
import os
import subprocess

import numpy as np
import pytest

from register_cases import (BIG, BINS, BRICK, CAP, DEFAULT_LEVELS, DOFS, MAP_KINDS, ODD_PAIR, SCENARIO_SHAPE, SCENARIO_THETA, SMALL_PAIRS, STRIDES, RegisterOracle,
                            all_maps, bits32, bits64, bricks, corner_error, holes, image_pair, kernel_constants, map_of, scenario, warp_hist_numpy)
from similarity_cases import SimilarityOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FV = np.array([[0.0, -0.9, 0.0, 12.5], [1.1, 0.0, 0.0, -3.0], [0.0, 0.0, 2.5, 7.25], [0, 0, 0, 1]], np.float32)
MV = np.array([[1.2, 0.1, 0.0, 1.0], [0.0, 0.8, 0.05, -2.0], [0.0, 0.0, 1.5, 0.5], [0, 0, 0, 1]], np.float32)
M0 = np.array([[0.98, -0.1, 0.02, 3.0], [0.12, 1.03, 0.0, -1.5], [-0.03, 0.01, 0.95, 0.25], [0, 0, 0, 1]], np.float32)
THETAS = np.array([[0.0] * 12, [1.5, -2.0, 0.25] + [0.0] * 9, [0, 0, 0, 0.3, -0.2, 0.1, 0, 0, 0, 0, 0, 0],
                   [0.5, 0.25, -1.0, 0.03, 0.02, -0.05, 0.1, -0.05, 0.02, 0.04, -0.02, 0.03], [0, 0, 0, 0, 0, 3.0, 2.0, -2.0, 0, 0, 5.0, 0]])


@pytest.fixture(scope="module", autouse=True)
def entry_points(built):
    """the feature under test: the C-ABI's registration functions in both libraries, the mirror's functions and the command line's path"""
    for name in ("sift3d_warp_histogram", "sift3d_register_affine", "sift3d_register_map", "sift3d_register_result", "sift3d_register_candidates",
                 "sift3d_register_lattice", "sift3d_register_defaults", "sift3d_register_check", "sift3d_register_report_text"):
        assert hasattr(built.hip_lib(), name), name
        assert name in ("sift3d_warp_histogram", "sift3d_register_affine") or hasattr(built.host_lib(), name), name
    for name in ("register_params", "register_map", "register_result", "warp_histogram", "register_affine", "FEATREGISTER"):
        assert hasattr(built, name), name


@pytest.fixture(scope="module")
def ro(tmp_path_factory):
    return RegisterOracle(tmp_path_factory.mktemp("register_oracle"))


@pytest.fixture(scope="module")
def so(tmp_path_factory):
    return SimilarityOracle(tmp_path_factory.mktemp("similarity_oracle"))


# ---- the kernel's contract: the oracle against numpy ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shapes", [((1, 1, 1), (1, 1, 1)), ((2, 3, 4), (2, 3, 4)), ((11, 9, 7), (9, 8, 10))], ids=["1", "24", "7x9x11_into_10x8x9"])
def test_oracle_histograms_equal_numpy(ro, shapes):
    """1 voxel, 24 voxels and 7 x 9 x 11 into 10 x 8 x 9: every map kind, stride and bins, NaN and +-inf voxels in F and in M"""
    fshape, mshape = shapes
    F, M, fr, mr = image_pair(fshape, mshape)
    if F.size > 1:
        assert not np.isfinite(F).all() and not np.isfinite(M).all()
    maps = all_maps(fshape, mshape)
    counted = 0
    for stride in STRIDES:
        for bins in BINS:
            want = ro.warp_hist(F, M, maps, fr, mr, stride, bins)
            assert ro.N == np.prod([(d - 1) // stride + 1 for d in fshape])
            for k in range(len(maps)):
                hist, sums, excluded, outside = warp_hist_numpy(F, M, maps[k], fr, mr, stride, bins)
                assert np.array_equal(hist, want[0][k]) and sums == want[1][k] and (excluded, outside) == (want[2][k], want[3][k]), (stride, bins, MAP_KINDS[k])
                assert sums[0] + excluded == ro.N and outside <= excluded and int(hist.sum()) == sums[0]
                counted += sums[0]
    assert counted > 0


def test_identity_map_is_the_joint_histogram(ro, so):
    """the identity map on equal finite grids: similarity_oracle's histogram and sums of (F, M), nothing outside"""
    F, M, fr, mr = image_pair((5, 9, 33), (5, 9, 33), with_holes=False)
    F = holes(F, 3)        # F's holes stay where they are; a hole in M would reach its neighbours' samples with weight 0
    for bins in BINS:
        hist, sums, excluded, outside = ro.warp_hist(F, M, map_of("identity", F.shape, M.shape), fr, mr, 1, bins)
        want = so.count(F, M, fr, mr, bins)
        assert np.array_equal(hist[0], want[0]) and sums[0] == want[1] and excluded[0] == want[2] and outside == [0]


def test_integer_shift_is_the_histogram_of_the_crops(ro, so):
    """q = p + (2, -1, 1): the fixed voxels whose image is inside pair with the moving voxels there; the others are outside"""
    F, M, fr, mr = image_pair((7, 9, 12), (7, 9, 12), with_holes=False)
    hist, sums, excluded, outside = ro.warp_hist(F, M, map_of("shift", F.shape, M.shape), fr, mr, 1, 32)
    Fc, Mc = F[:-1, 1:, :-2], M[1:, :-1, 2:]
    want = so.count(Fc, Mc, fr, mr, 32)
    assert np.array_equal(hist[0], want[0]) and sums[0] == want[1]
    assert outside[0] == excluded[0] == F.size - Fc.size and want[2] == 0


def test_everything_outside_and_nan_maps_count_nothing(ro):
    F, M, fr, mr = image_pair((5, 9, 33), (4, 7, 20))
    for stride in STRIDES:
        hist, sums, excluded, outside = ro.warp_hist(F, M, [map_of("outside", F.shape, M.shape), map_of("nan", F.shape, M.shape)], fr, mr, stride, 16)
        assert not hist.any() and sums == [[0] * 6] * 2 and excluded == [ro.N] * 2
        assert outside[0] == ro.N and 0 < outside[1] <= ro.N      # the NaN entry meets j = 0 rows as 0 * NaN too: NaN everywhere but where it is never used


def test_weight_zero_corner_reaches_the_sample(ro):
    """q on a lattice point reads its neighbours with weight 0: a NaN or infinite neighbour makes the sample NaN (0 * inf, 0 * NaN), so
    the voxel is excluded though it is inside"""
    F = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    M = F.copy()
    fr = mr = (np.float32(0), np.float32(23))
    ident = map_of("identity", F.shape, M.shape)
    assert ro.warp_hist(F, M, ident, fr, mr, 1, 8)[2] == [0]
    for bad in (np.nan, np.inf, -np.inf):
        M2 = M.copy()
        M2[0, 0, 1] = bad
        hist, sums, excluded, outside = ro.warp_hist(F, M2, ident, fr, mr, 1, 8)
        # the voxel itself and (0, 0, 0), whose x neighbour it is
        assert excluded == [2] and outside == [0] and sums[0][0] == 22


# ---- the host code ------------------------------------------------------------------------------------------------------------------------
def test_theta_zero_is_resample_map(built):
    for fv, mv, m0 in ((None, None, None), (FV, MV, M0), (FV, None, M0), (None, MV, None)):
        got = built.register_map(np.zeros(12), (13, 17, 31), fv, mv, m0)
        want = built.resample_map(np.eye(4, dtype=np.float32) if m0 is None else m0, fv, mv)
        assert np.array_equal(bits32(got), bits32(want))
        assert np.array_equal(built.register_result(np.zeros(12), (13, 17, 31), fv, m0), np.eye(4, dtype=np.float32) if m0 is None else m0)


def test_host_matrices_equal_the_oracle(built, ro):
    rng = np.random.default_rng(5)
    thetas = list(THETAS) + [rng.normal(0, 1, 12) * np.repeat([3.0, 0.2, 0.1, 0.1], 3) for _ in range(20)]
    for shape, fv, mv, m0 in (((48, 44, 40), None, None, None), ((13, 17, 31), FV, MV, M0), ((1, 1, 1), FV, None, None)):
        for th in thetas:
            assert np.array_equal(bits32(built.register_map(th, shape, fv, mv, m0)), bits32(ro.map(th, shape, fv, mv, m0)))
            assert np.array_equal(bits32(built.register_result(th, shape, fv, m0)), bits32(ro.result(th, shape, fv, m0)))


def test_result_inverts_the_map(built):
    """M1 = inv(D) M0 and A = inv(mv) inv(M0) D fv: mv A inv(fv) M1 is the identity within 1e-6 (of entries of size 1), and featResample's
    map of M1 is A"""
    for th in THETAS[:4]:
        for shape, fv, mv, m0 in (((48, 44, 40), None, None, None), ((13, 17, 31), FV, MV, M0)):
            A = np.vstack([built.register_map(th, shape, fv, mv, m0).astype(np.float64), [0, 0, 0, 1]])
            M1 = built.register_result(th, shape, fv, m0).astype(np.float64)
            f = np.eye(4) if fv is None else fv.astype(np.float64)
            m = np.eye(4) if mv is None else mv.astype(np.float64)
            prod = m @ A @ np.linalg.inv(f) @ M1
            assert np.abs(prod[:3, :3] - np.eye(3)).max() < 1e-6 and np.abs(prod[:3, 3]).max() < 1e-6 * max(1.0, np.abs(M1[:3, 3]).max(), np.abs(f[:3, 3]).max())
            again = built.resample_map(M1.astype(np.float32), fv, mv)
            assert np.abs(again - A[:3]).max() < 1e-5 * max(1.0, np.abs(A).max())


def test_transform_family_by_hand(built):
    """a translation moves the map's last column; a rotation about z by 90 degrees, a scale and a shear act about the volume's centre"""
    shape = (9, 7, 5)      # centre (2, 3, 4)
    c = np.array([2.0, 3.0, 4.0])
    A = built.register_map([1, 2, 3] + [0] * 9, shape)
    assert np.array_equal(A, np.concatenate([np.eye(3), [[1], [2], [3]]], 1).astype(np.float32))
    A = built.register_map([0, 0, 0, 0, 0, np.pi / 2] + [0] * 6, shape).astype(np.float64)
    R = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])
    assert np.abs(A[:, :3] - R).max() < 1e-7 and np.abs(A[:, 3] - (c - R @ c)).max() < 1e-6
    A = built.register_map([0] * 6 + [np.log(2.0), 0, np.log(0.5)] + [0] * 3, shape).astype(np.float64)
    assert np.abs(A[:, :3] - np.diag([2, 1, 0.5])).max() < 1e-7 and np.abs(A[:, 3] - (c - np.diag([2, 1, 0.5]) @ c)).max() < 1e-6
    A = built.register_map([0] * 9 + [0.1, 0.2, 0.3], shape).astype(np.float64)
    G = np.array([[1, 0.1, 0.2], [0, 1, 0.3], [0, 0, 1.0]])
    assert np.abs(A[:, :3] - G).max() < 1e-7 and np.abs(A[:, 3] - (c - G @ c)).max() < 1e-6


def test_candidates_follow_the_dof(built, ro):
    """+ before -, the parameters in the order t, r, s, g; a step is u for t and u / rho for the others; 7 moves the three scales
    together; the inactive parameters keep their values"""
    th = THETAS[3]
    u, rho = 0.5, 20.0
    for dof in DOFS:
        got, want = built.register_candidates(th, dof, u, rho), ro.candidates(th, dof, u, rho)
        assert got.shape == (2 * dof, 12) and np.array_equal(bits64(got), bits64(want))
        for c, row in enumerate(got):
            k, sign = c // 2, 1.0 if c % 2 == 0 else -1.0
            moved = [6, 7, 8] if (dof == 7 and k == 6) else [k]
            step = u if k < 3 else u / rho
            for e in range(12):
                want_e = th[k if (dof == 7 and e in moved) else e] + sign * step if e in moved else th[e]
                assert row[e] == want_e, (dof, c, e)
    for dof in (0, 5, 8, 13):
        with pytest.raises(built.Sift3DError):
            built.register_candidates(th, dof, u, rho)
        assert ro.candidates(th, dof, u, rho) is None


def test_lattice_and_units(built, ro):
    for shape in ((1, 1, 1), (2, 3, 4), (5, 9, 33), (13, 17, 31), (64, 4096, 4096)):
        for stride in STRIDES:
            for fv in (None, FV):
                got, want = built.register_lattice(shape, stride, fv), ro.lattice(shape, stride, fv)
                assert got[:2] == want[:2] and bits64(got[2]) == bits64(want[2]) and bits64(got[3]) == bits64(want[3])
                assert got[0] == np.prod([(d - 1) // stride + 1 for d in shape], dtype=np.int64) and got[0] >= 1
    N, n, h, rho = built.register_lattice((13, 17, 31), 2, FV)
    assert n == (16, 9, 7) and h == pytest.approx(0.9) and rho == pytest.approx(max(30 * 1.1, 16 * 0.9, 12 * 2.5) / 2)
    assert built.register_lattice((1, 1, 1), 1)[2:] == (1.0, 0.5)
    for bad in (3, 0, 16):
        with pytest.raises(built.Sift3DError):
            built.register_lattice((4, 4, 4), bad)


def test_parameters_and_their_check(built):
    p = built.register_params()
    assert (p.dof, p.metric, p.bins, p.n_levels, p.max_iterations, p.device, p.form, p.min_overlap) == (12, 1, 32, 3, 200, 0, -1, 0.25)
    assert [(p.stride[l], p.first_step[l], p.last_step[l]) for l in range(3)] == [tuple(l) for l in DEFAULT_LEVELS]
    assert built.register_check(p) is None
    for kw, text in (({"dof": 5}, "dof = 5: 3, 6, 7, 9 or 12"), ({"metric": 2}, "metric = 2"), ({"bins": 128}, "bins = 128: 8, 16, 32 or 64"),
                     ({"levels": []}, "n_levels = 0: 1 .. 4"), ({"n_levels": 5}, "n_levels = 5"), ({"levels": [(3, 1, 1)]}, "stride[0] = 3: 1, 2, 4 or 8"),
                     ({"levels": [(1, 1, 1), (2, 0.0, 0.0)]}, "first_step[1] = 0"), ({"levels": [(1, 1.0, 2.0)]}, "last_step[0] = 2"),
                     ({"levels": [(1, float("inf"), 1.0)]}, "first_step[0] = inf"), ({"max_iterations": 0}, "max_iterations = 0: at least 1"),
                     ({"min_overlap": 1.5}, "min_overlap = 1.5: 0 .. 1"), ({"min_overlap": float("nan")}, "min_overlap = nan"), ({"form": 4}, "form = 4")):
        assert text in built.register_check(built.register_params(**kw)), kw
    for kw in ({"dof": 7, "metric": "mi", "bins": 8, "form": "by_map_plane"}, {"levels": [(8, 8, 8)] * 4, "min_overlap": 0.0}, {"min_overlap": 1.0}):
        assert built.register_check(built.register_params(**kw)) is None
    with pytest.raises(ValueError):
        built.register_params(smoothing=1)


# ---- the shapes of the GPU suite --------------------------------------------------------------------------------------------------------
def test_shapes_follow_the_kernel_file(built):
    K = kernel_constants()
    assert K["REG_THREADS"] == 256 and 4 * K["REG_THREADS"] == BRICK[0] * BRICK[1] * BRICK[2] and K["REG_MAX_BLOCKS"] == CAP and CAP % 8 == 0
    assert K["REG_MAX_MAPS"] == built.REGISTER_MAX_MAPS == 32 and K["REG_MAX_BINS"] == 64 and K["REG_WORDS"] == 7
    assert 4 * K["REG_MAX_BINS"] ** 2 + 8 * K["REG_WORDS"] <= 65536      # the workgroup's LDS
    warp = open(os.path.join(ROOT, "3d_sift_cuda_amd", "csrc", "warp_device.h")).read()
    for name, value in (("BRICK_TX", 8), ("BRICK_VX", 4), ("BRICK_BY", BRICK[1]), ("BRICK_BZ", BRICK[0])):
        assert "#define %s %d" % (name, value) in warp
    assert all(max(s) <= 4096 for pair in SMALL_PAIRS + [ODD_PAIR] for s in pair) and max(BIG) <= 4096
    assert [int(np.prod(f)) for f, _ in SMALL_PAIRS[:2]] == [1, 24] and SMALL_PAIRS[2][0][2] == BRICK[2] + 1
    # every stride changes the lattice of the odd pair, none of its extents is a multiple of the brick's, and it has several bricks
    assert len({built.register_lattice(ODD_PAIR[0], s)[1] for s in STRIDES}) == 4 and bricks(ODD_PAIR[0]) > 1
    assert all(d % b for d, b in zip(ODD_PAIR[0], BRICK))
    # past the cap by more than one trip: the last bricks are reached by the fifth trip only
    assert bricks(BIG) > 4 * CAP and bricks(BIG) % CAP != 0 and BIG[2] % 4 != 0


# ---- register_host.c under the sanitizers -------------------------------------------------------------------------------------------------
def test_host_file_under_sanitizers(built, ro, tmp_path):
    """register_host.c and tests/register_host_san.c as one program (with align_host.c for sift3d_resample_map), with and without
    -fsanitize=address,undefined: both exit clean and print the same lines, and the lines are the oracle's"""
    csrc = os.path.join(ROOT, "3d_sift_cuda_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "register_host_san.c"), os.path.join(csrc, "register_host.c"), os.path.join(csrc, "align_host.c")]
    base = ["cc", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-ffp-contract=off", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-I" + csrc]
    out = {}
    for name, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])):
        exe = str(tmp_path / ("register_host_" + name))
        subprocess.run(base + flags + ["-o", exe] + src + ["-lm"], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
        out[name] = r.stdout
    text = out["san"]
    assert text == out["plain"]
    lines = text.split("\n")
    assert "defaults 12 1 32 3 200 0 -1 0.25 4 4 1 2 1 0.25 1 0.25 0.0625 1 0.0625 0.0625" in lines
    for line in ("check null -1 null pointer", "check defaults 0 ", "check dof 0 -1 dof = 0: 3, 6, 7, 9 or 12", "check dof 3 0 ", "check dof 5 -1 dof = 5: 3, 6, 7, 9 or 12",
                 "check dof 7 0 ", "check dof 12 0 ", "check dof 13 -1 dof = 13: 3, 6, 7, 9 or 12", "check metric 2 -1 metric = 2: 0 (mi) or 1 (nmi)", "check metric 0 0 ",
                 "check bins 48 -1 bins = 48: 8, 16, 32 or 64", "check bins 8 0 ", "check n_levels 0 -1 n_levels = 0: 1 .. 4", "check n_levels 4 0 ",
                 "check n_levels 5 -1 n_levels = 5: 1 .. 4", "check stride 3 -1 stride[1] = 3: 1, 2, 4 or 8", "check stride 8 0 ", "check stride unused 0 ",
                 "check first nan -1 first_step[0] = nan: finite and above 0", "check first 0 -1 first_step[2] = 0: finite and above 0",
                 "check last above -1 last_step[1] = 2: above 0 and at most first_step = 1", "check last 0 -1 last_step[1] = 0: above 0 and at most first_step = 1",
                 "check max_iterations 0 -1 max_iterations = 0: at least 1", "check min_overlap -1 -1 min_overlap = -1: 0 .. 1", "check min_overlap nan -1 min_overlap = nan: 0 .. 1",
                 "check min_overlap 1 0 ", "check form 4 -1 form = 4: -1 or 0 .. 3", "check form 3 0 ", "check form -2 -1 form = -2: -1 or 0 .. 3", "check short_err -1 dof = 5",
                 "check no_err -1 ", "map singular -1 -1 -1", "result refused -1 -1", "map overflow -1", "lattice refused -1 8 8", "lattice zero column -1",
                 "report refused -1 -1"):
        assert line in lines, line
    hexes = lambda v: " ".join(float(x).hex() for x in np.asarray(v, np.float32).reshape(-1))
    canon = lambda s: " ".join(float.fromhex(x).hex() for x in s.split())
    by_name = {" ".join(l.split()[:3]): l.split()[3:] for l in lines if l.startswith(("map plain", "map keys", "result plain", "result keys"))}
    for k, th in enumerate(THETAS):
        for name, want in (("map plain %d" % k, ro.map(th, (48, 44, 40))), ("map keys %d" % k, ro.map(th, (13, 17, 31), FV, MV, M0)),
                           ("result plain %d" % k, ro.result(th, (48, 44, 40))), ("result keys %d" % k, ro.result(th, (13, 17, 31), FV, M0))):
            got = by_name[name]
            assert got[0] == "0" and canon(" ".join(got[1:])) == hexes(want), name
    unit = [l for l in lines if l.startswith("resample_map 0 ")][0].split()[2:]
    assert unit == by_name["map keys 0"][1:]
    for dof in (0, 5, 8, 13):
        assert "candidates %d -1" % dof in lines
    for dof in DOFS:
        row = [l for l in lines if l.startswith("candidates %d %d" % (dof, 2 * dof))][0].split()[3:]
        want = ro.candidates(THETAS[3], dof, 0.5, 20.0)
        changed = ["%d:%d:%s" % (c, e, float(want[c, e]).hex()) for c in range(2 * dof) for e in range(12) if want[c, e] != THETAS[3][e]]
        assert ["%s:%s:%s" % (a.split(":")[0], a.split(":")[1], float.fromhex(a.split(":", 2)[2]).hex()) for a in row] == changed
    for shape in ((1, 1, 1), (2, 3, 4), (5, 9, 33), (64, 4096, 4096)):
        for stride in STRIDES + (3,):
            line = [l for l in lines if l.startswith("lattice %d %d %d stride %d:" % (shape[2], shape[1], shape[0], stride))][0].split(": ")[1].split()
            if stride == 3:
                assert line[0] == "-1"
                continue
            N, n, h, rho = ro.lattice(shape, stride, FV if shape in ((2, 3, 4), (64, 4096, 4096)) else None)
            assert [int(v) for v in line[:4]] == [N] + list(n) and float.fromhex(line[4]) == h and float.fromhex(line[5]) == rho
    # the report: the whole text at the length asked for, and every shorter buffer a prefix of it
    head = [l for l in lines if l.startswith("report ") and not l.startswith(("report part", "report refused"))][0].split()
    assert head[1] == head[2] == head[3]
    at = lines.index(" ".join(head))
    body = lines[at + 1:at + 16]
    assert body[0] == "# dof 12 metric nmi bins 32 stop 0" and body[1] == "# h 0.9 rho 58.75" and body[2].startswith("# level stride lattice iterations")
    assert body[3] == "0 4 100 10 241 0 1.25 1.3 0.45 1.500" and body[5] == "2 1 6400 12 289 0 1.45 nan 0.028125 4.500"
    assert body[6] == "# theta t r s g" and body[7] == "0.5 0.25 -1" and body[10] == "0.04 -0.02 0.03" and body[11] == "# result"
    parts = [l.split() for l in lines if l.startswith("report part")]
    assert len(parts) >= 5 and all(p[3] == head[1] and int(p[4]) == int(p[2]) - 1 and p[5] == "0" for p in parts)
    assert "before 6851 12 0 0.5 1.125 nan" in lines and "after 6851 12 7 0.5 1.5 nan" in lines


def test_python_report_text(built):
    rep = built.RegisterReport()
    rep.dof, rep.metric, rep.bins, rep.n_levels = 6, 0, 16, 1
    text = built.register_report_text(rep)
    assert text.startswith("# dof 6 metric mi bins 16 stop 0\n") and text.count("\n") == 17


# ---- the scenario, on the oracle --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(ro):
    true = ro.map(SCENARIO_THETA, SCENARIO_SHAPE)
    F, M = scenario(tuple(float(v) for v in true.reshape(-1)))
    return true, F, M


def test_scenario_true_transform_is_admissible(ro, scene):
    """min_overlap is never what refuses a step at the true transform: there, and one first step away from it in every parameter, far
    more than a quarter of every level's lattice counts"""
    true, F, M = scene
    fr, mr = ro.range(F), ro.range(M)
    N1, _, h, rho = ro.lattice(SCENARIO_SHAPE, 1)
    for stride, first, _ in DEFAULT_LEVELS:
        maps = [true] + [ro.map(c, SCENARIO_SHAPE) for c in ro.candidates(SCENARIO_THETA, 12, first * h, rho)]
        _, sums, excluded, _ = ro.warp_hist(F, M, maps, fr, mr, stride, 32)
        assert min(s[0] for s in sums) >= 0.6 * ro.N, (stride, min(s[0] for s in sums), ro.N)


def test_scenario_twelve_parameters_recover_the_map(ro, scene):
    """the 12-dof search ends below a quarter of the corner error it began with and below the 6-dof search on the same pair; the score
    rises from entry to exit at every level.  Oracle figures: 4.71 voxels before; 0.087 after at 12 dof nmi
    32 bins (15, 17, 15 iterations); 1.92 at 6 dof"""
    true, F, M = scene
    before = corner_error(true, ro.map(np.zeros(12), SCENARIO_SHAPE), SCENARIO_SHAPE)
    assert 4.0 < before < 5.5
    errors = {}
    for dof, metric, bins in ((12, "nmi", 32), (12, "mi", 32), (12, "mi", 64), (12, "mi", 16), (6, "nmi", 32)):
        r = ro.register(F, M, dof=dof, metric=metric, bins=bins)
        errors[dof, metric, bins] = err = corner_error(true, ro.map(r["theta"], SCENARIO_SHAPE), SCENARIO_SHAPE)
        print(dof, metric, bins, "corner error %.3f -> %.3f" % (before, err), [(l["iterations"], l["evaluations"], l["score_in"], l["score_out"]) for l in r["levels"]])
        for l in r["levels"]:
            assert l["score_out"] > l["score_in"] and l["stop"] == 0 and l["evaluations"] == 1 + 2 * dof * l["iterations"], l
        if dof == 6:
            assert not r["theta"][6:].any()
        # M1 is the matrix a reader of the .trans.txt turns into the same map
        assert np.array_equal(bits32(r["result"]), bits32(ro.result(r["theta"], SCENARIO_SHAPE)))
    for key, err in errors.items():
        if key[0] == 12:
            assert err < before / 4, (key, err, before)
            assert err < errors[6, "nmi", 32], (key, err, errors[6, "nmi", 32])


def test_oracle_stage_edges(ro):
    """an image without a range and a singular matrix are refused; a start with nothing inside is inadmissible; max_iterations stops a level"""
    F, M, _, _ = image_pair((5, 9, 33), (5, 9, 33), with_holes=False)
    assert ro.register(np.full((2, 2, 2), 3.0, np.float32), M) == -1 and ro.register(F, np.full((2, 2, 2), np.nan, np.float32)) == -1
    assert ro.register(F, M, m0=np.zeros((4, 4), np.float32)) == -1
    far = np.eye(4, dtype=np.float32)
    far[0, 3] = 1000.0
    assert ro.register(F, M, m0=far) == -2
    r = ro.register(F, np.roll(M, 1, 2), dof=3, levels=[(1, 1.0, 0.001)], max_iterations=3)
    assert r["levels"][0]["iterations"] == 3 and r["levels"][0]["stop"] == 1 and r["levels"][0]["evaluations"] == 19
