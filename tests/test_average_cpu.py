"""CPU suite: the template from warped images without a GPU -- the oracle tests/average_oracle.c against a
float64 numpy restatement that shares no code with it, the hand cases, the product's host code (average_host.c) against the oracle
bit for bit, the shapes that take the GPU kernel past its launch cap, the host file under the sanitizers as a stand-alone program,
featAverage's refusals, and the scenario the feature is there for, on the oracle.

The scenario's figures (oracle, 40^3 target, five images of which one is misregistered by three voxels in every z slab; RMS against
the target over the 62 312 of 64 000 voxels that all five reach): single images 138.0 - 153.1, mean 103.0, trim 1 82.3, median 81.8;
DESIGN.md section 7r has the table."""
import os
import re
import subprocess

import numpy as np
import pytest

from average_cases import (BIG, BRICK, CAP, COUNTS, GROUP_EDGES, SHAPES, TRIMS, AverageOracle, average_numpy, bits32, bricks, cpu_average, group, kernel_constants, rms,
                           same_planes, scenario, warped_planes)
from resample_cases import ResampleOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def entry_points(built):
    """the feature under test: the C-ABI's functions in both libraries, the mirror's functions and the command line's path"""
    for name in ("sift3d_average_warped", "sift3d_average_defaults", "sift3d_average_check", "sift3d_average_counts", "sift3d_average_report_text", "sift3d_mean_field"):
        assert hasattr(built.hip_lib(), name), name
        assert name == "sift3d_average_warped" or hasattr(built.host_lib(), name), name
    for name in ("average_params", "average_check", "average_counts", "average_report_text", "mean_field", "average_warped", "FEATAVERAGE"):
        assert hasattr(built, name), name


@pytest.fixture(scope="module")
def ao(tmp_path_factory):
    return AverageOracle(tmp_path_factory.mktemp("average_oracle"))


@pytest.fixture(scope="module")
def ro(tmp_path_factory):
    return ResampleOracle(tmp_path_factory.mktemp("resample_oracle"))


def f32(*values):
    """K planes of one voxel each"""
    return [np.array([[[v]]], np.float32) for v in values]


# ---- the contract: the oracle against numpy --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, K", [((1, 1, 1), 1), ((2, 3, 4), 2), ((5, 9, 33), 5), ((5, 9, 33), 32), ((11, 19, 70), 5)], ids=lambda v: str(v).replace(" ", ""))
def test_oracle_equals_numpy(built, ao, shape, K):
    """1 voxel with K = 1, 4 x 3 x 2 with K = 2, 33 x 9 x 5 with K = 5 and K = 32, 70 x 19 x 11: sources of differing shapes with NaN and
    +-inf voxels, with and without fields, every trim and two minimum counts"""
    seen = 0
    for fields in ("none", "mixed"):
        images = group(built, shape, K, fields, seed=3)
        assert K == 1 or len({a["image"].shape for a in images}) > 1
        assert np.prod(shape) < 1000 or not any(np.isfinite(a["image"]).all() for a in images)
        planes = warped_planes(built, ao, shape, images)
        for trim in TRIMS:
            for min_count, fill in ((1, np.nan), (min(K, 3), -7.0)):
                want = ao.average(planes, trim, min_count, fill)
                same_planes(want, average_numpy(planes, trim, min_count, fill))
                seen += int((want[2] != 0).sum())
    assert seen > 0


def test_oracle_equals_numpy_on_planted_values(ao):
    """planes of values that meet the rule's corners: duplicates, +-0, NaN and +-inf, values whose sum depends on the order"""
    rng = np.random.default_rng(11)
    pool = np.array([0.0, -0.0, 1.0, 1.0, -1.0, 1e30, -1e30, 1e-30, 3.5, np.nan, np.inf, -np.inf, 16777216.0, 1.0000001], np.float32)
    for K in (1, 2, 3, 4, 5, 8, 31, 32):
        planes = [rng.choice(pool, (3, 5, 7)) for _ in range(K)]
        for trim in (0, 1, 2, 7, 15):
            for min_count in (1, K):
                same_planes(ao.average(planes, trim, min_count, 0.5), average_numpy(planes, trim, min_count, 0.5))


# ---- hand cases -------------------------------------------------------------------------------------------------------------------------
def test_identical_images_give_the_image(built, ao):
    """K copies of one image under the identity: the image's bits, var 0 and a full mask, under every trim"""
    v = group(built, (5, 9, 33), 1, with_holes=False)[0]["image"][:5, :9, :33]
    v = np.ascontiguousarray(v)
    for K in (1, 2, 5, 32):
        images = [{"image": v} for _ in range(K)]
        for trim in TRIMS:
            avg, var, mask = cpu_average(built, ao, v.shape, images, trim=trim)
            assert np.array_equal(bits32(avg), bits32(v)) and not var.any() and (mask == (1 << K) - 1).all()


def test_image_outside_clears_its_bit(built, ao):
    v = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    far = np.eye(4, dtype=np.float32)
    far[0, 3] = 100.0
    avg, var, mask = cpu_average(built, ao, v.shape, [{"image": v}, {"image": v + 2, "t": far}, {"image": v + 4}])
    assert (mask == 0b101).all() and np.array_equal(avg, v + 2) and np.array_equal(var, np.full(v.shape, 8.0, np.float32))


def test_median_of_odd_and_even_counts(ao):
    """t = 15: the middle value for odd n, the mean of the middle two for even n; a non-finite value is no contributor"""
    for values, want in (((5.0, 1.0, 9.0), 5.0), ((5.0, 1.0, 9.0, 2.0), 3.5), ((4.0,), 4.0), ((4.0, 8.0), 6.0), ((5.0, np.nan, 1.0, np.inf, 9.0), 5.0),
                         (tuple(float(x) for x in range(32, 0, -1)), 16.5), (tuple(float(x) for x in range(31)), 15.0)):
        avg, var, mask = ao.average(f32(*values), trim=15)
        assert avg.item() == want, (values, avg.item())


def test_trim_larger_than_half_is_capped(ao):
    """t_eff = min(t, (n - 1) / 2): with n = 5, t = 1 drops one at either end, t = 2 .. 15 leave the median; with n = 2 nothing is dropped"""
    five = f32(10.0, 0.0, 100.0, 1.0, 4.0)
    assert ao.average(five, trim=1)[0].item() == 5.0
    for t in (2, 3, 15):
        assert ao.average(five, trim=t)[0].item() == 4.0
    assert ao.average(f32(1.0, 2.0), trim=7)[0].item() == 1.5 and ao.average(f32(3.0), trim=7)[0].item() == 3.0


def test_zero_signs_and_duplicates_are_ranked_by_index(ao):
    """-0 == 0: the earlier image ranks lower; a sum that starts from +0 gives +0 whichever zero the trim keeps.  Duplicates rank by index"""
    pz, nz = np.float32(0.0), np.float32(-0.0)
    a = ao.average(f32(nz, pz, 5.0), trim=1)[0]       # ranks: -0, +0, 5: the middle is +0
    b = ao.average(f32(pz, nz, 5.0), trim=1)[0]       # ranks: +0, -0, 5: the middle is -0, and +0 + -0 = +0
    assert bits32(a).item() == 0 and bits32(b).item() == 0
    c = ao.average(f32(nz, nz, nz), trim=0)[0]        # the sum starts from +0
    assert bits32(c).item() == 0
    d = ao.average(f32(2.0, 2.0, 2.0, 7.0, -3.0), trim=1)
    assert d[0].item() == 2.0 and d[2].item() == 31


def test_min_count_and_no_contributor(ao):
    planes = [np.array([[[1.0, np.nan, np.nan, 4.0]]], np.float32), np.array([[[3.0, 5.0, np.inf, np.nan]]], np.float32)]
    avg, var, mask = ao.average(planes, trim=0, min_count=2, fill=-1.0)
    assert avg.reshape(-1).tolist() == [2.0, -1.0, -1.0, -1.0] and var.reshape(-1).tolist() == [2.0, -1.0, -1.0, -1.0] and mask.reshape(-1).tolist() == [3, 2, 0, 1]
    avg, var, mask = ao.average(planes, trim=0, min_count=1)
    assert avg.reshape(-1).tolist()[:2] == [2.0, 5.0] and np.isnan(avg.reshape(-1)[2]) and var.reshape(-1).tolist()[1] == 0.0 and np.isnan(var.reshape(-1)[2])
    assert mask.reshape(-1).tolist() == [3, 2, 0, 1]


def test_variance_by_hand(ao):
    avg, var, mask = ao.average(f32(1.0, 2.0, 3.0, 6.0))
    assert avg.item() == 3.0 and var.item() == np.float32(14.0 / 3.0)


def test_permuting_the_images_permutes_the_mask(built, ao):
    """for trim > 0 the ranks depend on the values and, among equal values, on the order of their images alone: the same sum in the same order,
    so avg keeps its bits.  (For trim 0 the order of the additions changes.)  Duplicates are planted so that the index rule is used."""
    shape = (5, 9, 33)
    planes = warped_planes(built, ao, shape, group(built, shape, 5, "mixed", seed=9))
    planes[3] = np.where(np.arange(33) % 2 == 0, planes[1], planes[3]).astype(np.float32)
    perm = [3, 0, 4, 2, 1]
    for trim in (1, 15):
        a, b = ao.average(planes, trim), ao.average([planes[k] for k in perm], trim)
        finite = ~np.isnan(a[0])
        assert finite.sum() > 500 and np.array_equal(bits32(a[0])[finite], bits32(b[0])[finite]) and np.array_equal(np.isnan(a[0]), np.isnan(b[0]))
        moved = np.zeros_like(a[2])
        for new, old in enumerate(perm):
            moved |= ((a[2] >> np.uint32(old)) & np.uint32(1)) << np.uint32(new)
        assert np.array_equal(moved, b[2])


# ---- the host code ----------------------------------------------------------------------------------------------------------------------
def test_parameters_and_their_check(built):
    p = built.average_params()
    assert (p.trim, p.min_count, p.device, p.max_voxels, p.form) == (0, 1, 0, 1 << 32, -1) and np.isnan(p.fill)
    assert built.average_check(p, 1) is None and built.average_check(built.average_params(trim="median", min_count=32, form="column"), 32) is None
    for kw, K, text in (({"trim": 16}, 3, "trim = 16: 0 .. 15"), ({"trim": -1}, 3, "trim = -1"), ({"min_count": 0}, 3, "min_count = 0: 1 .. K = 3"),
                        ({"min_count": 4}, 3, "min_count = 4: 1 .. K = 3"), ({}, 0, "K = 0 images: 1 .. 32"), ({}, 33, "K = 33 images"), ({"max_voxels": 0}, 1, "max_voxels = 0"),
                        ({"form": 1}, 1, "form = 1: -1 or 0")):
        assert text in built.average_check(built.average_params(**kw), K), kw
    with pytest.raises(ValueError):
        built.average_params(weights=1)


def test_counts_and_report_equal_the_oracle(built, ao):
    shape = (5, 9, 33)
    for K in (1, 5, 32):
        mask = ao.average(warped_planes(built, ao, shape, group(built, shape, K, "mixed", seed=K)))[2]
        for min_count in (1, K):
            got, want = built.average_counts(mask, K, 1, min_count), ao.counts(mask, K, min_count)
            assert (got["none"], got["below"], got["count"]) == (want["none"], want["below"], want["count"])
            assert [i["contributing"] for i in got["image"]] == want["contributing"] and got["voxels"] == mask.size and sum(got["count"]) == mask.size
            text = built.average_report_text(got).split("\n")
            assert text[0] == "# images %d trim 1 min_count %d" % (K, min_count) and text[1] == "# voxels %d none %d below %d" % (mask.size, want["none"], want["below"])
            assert text[3:3 + K] == ["%d %d 0.000" % (k + 1, c) for k, c in enumerate(want["contributing"])]
            assert text[4 + K:5 + 2 * K] == ["%d %d" % (c, v) for c, v in enumerate(want["count"])]
    with pytest.raises(built.Sift3DError):
        built.average_counts(np.array([4], np.uint32), 2)


def test_mean_field_equals_the_oracle(built, ao):
    """the node-wise mean in double, in image order, on a grid of 40^3's size; the grids must agree to the bit"""
    from invert_cases import forward_field
    grid = built.blockmatch_grid((40, 40, 40), built.key_vox2key(), spacing=4.0)
    for K in (1, 2, 5, 32):
        fields = [forward_field("random", grid, seed=k, amp=3.0 + k) for k in range(K)]
        got = built.mean_field(fields)
        assert got["n"] == tuple(grid["n"]) and np.array_equal(got["origin"], grid["origin"]) and got["spacing"] == grid["spacing"]
        assert np.array_equal(bits32(got["disp"]), bits32(ao.mean_field(fields)))
    f = forward_field("random", grid, seed=1)
    other = built.blockmatch_grid((40, 40, 44), built.key_vox2key(), spacing=4.0)
    for bad, text in ((forward_field("random", other, seed=2), "field 1: n[0] = 22 differs from field 0's 21"), (dict(f, origin=f["origin"] + np.float32(0.5)), "field 1: origin[0] = "),
                      (dict(f, spacing=np.float32(4.5)), "field 1: spacing = 4.5 differs from field 0's 4")):
        with pytest.raises(built.Sift3DError, match=re.escape(text)) as e:
            built.mean_field([f, bad])
        assert e.value.code == -1
    with pytest.raises(built.Sift3DError, match="K = 0 fields"):
        built.mean_field([])
    with pytest.raises(built.Sift3DError, match="K = 33 fields"):
        built.mean_field([f] * 33)


# ---- the shapes of the GPU suite ----------------------------------------------------------------------------------------------------------
def test_shapes_follow_the_kernel_file(built):
    K = kernel_constants()
    assert K["AVG_THREADS"] == 256 and 4 * K["AVG_THREADS"] == BRICK[0] * BRICK[1] * BRICK[2] and K["AVG_MAX_BLOCKS"] == CAP and CAP % 8 == 0
    assert K["AVG_MAX_IMAGES"] == built.AVERAGE_MAX_IMAGES == 32
    # four, two or one voxel of a thread per walk over the images: the workgroup's LDS columns stay within 32 KB, and the GPU suite runs either side of both thresholds
    assert GROUP_EDGES == (K["AVG_GROUP4_MAX"], K["AVG_GROUP4_MAX"] + 1, K["AVG_GROUP2_MAX"], K["AVG_GROUP2_MAX"] + 1)
    assert 4 * K["AVG_THREADS"] * max(4 * K["AVG_GROUP4_MAX"], 2 * K["AVG_GROUP2_MAX"], K["AVG_MAX_IMAGES"]) <= 32768
    assert all(k <= K["AVG_GROUP4_MAX"] for k in COUNTS[:3]) and COUNTS[3] > K["AVG_GROUP2_MAX"]
    warp = open(os.path.join(ROOT, "3d_sift_cuda_amd", "csrc", "warp_device.h")).read()
    for name, value in (("BRICK_TX", 8), ("BRICK_VX", 4), ("BRICK_BY", BRICK[1]), ("BRICK_BZ", BRICK[0])):
        assert "#define %s %d" % (name, value) in warp
    assert [int(np.prod(s)) for s in SHAPES[:2]] == [1, 24] and SHAPES[2] == tuple(b + 1 for b in BRICK)
    assert all(d % b for d, b in zip(SHAPES[3], BRICK)) and bricks(SHAPES[3]) > 1 and SHAPES[3][2] % 4 != 0 and SHAPES[2][2] % 4 != 0
    # past the cap by more than one trip: the last bricks are reached by the third trip only
    assert bricks(BIG) > 2 * CAP and bricks(BIG) % CAP != 0 and BIG[2] % 4 != 0
    assert COUNTS == (1, 2, 5, 32) and TRIMS == (0, 1, 15)


# ---- average_host.c under the sanitizers --------------------------------------------------------------------------------------------------
def test_host_file_under_sanitizers(built, ao, tmp_path):
    """average_host.c and tests/average_host_san.c as one program, with and without -fsanitize=address,undefined: both exit clean and print
    the same lines, and the mean field's lines are the oracle's"""
    csrc = os.path.join(ROOT, "3d_sift_cuda_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "average_host_san.c"), os.path.join(csrc, "average_host.c")]
    base = ["cc", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-ffp-contract=off", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-I" + csrc]
    out = {}
    for name, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])):
        exe = str(tmp_path / ("average_host_" + name))
        subprocess.run(base + flags + ["-o", exe] + src + ["-lm"], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
        out[name] = r.stdout
    text = out["san"]
    assert text == out["plain"]
    lines = text.split("\n")
    for line in ("defaults 0 1 nan 0 4294967296 -1", "check null -1 null pointer", "check defaults 0 ", "check K 0 -1 K = 0 images: 1 .. 32", "check K 33 -1 K = 33 images: 1 .. 32",
                 "check K 32 0 ", "check trim -1 -1 trim = -1: 0 .. 15", "check trim 15 0 ", "check trim 16 -1 trim = 16: 0 .. 15", "check min_count 0 -1 min_count = 0: 1 .. K = 5",
                 "check min_count 5 0 ", "check min_count 6 -1 min_count = 6: 1 .. K = 5", "check max_voxels 0 -1 max_voxels = 0: at least 1", "check form 0 0 ",
                 "check form 1 -1 form = 1: -1 or 0", "check form -2 -1 form = -2: -1 or 0", "check short_err 9 -1 trim = 1", "check no_err -1 ",
                 "counts 0 3 1 2 9 2 5 : 2 3 2 2 : 5 4 4", "counts stray_bit -1", "counts refused -1 -1 -1 -1", "counts K32 0 1", "report refused -1 -1",
                 "mean capacity -4 out holds fewer than 3 n0 n1 n2 = 36 floats", "mean grid 2 3 2 -0x1.8p+0 0x1p+1 0x1p-2 0x1p+2", "mean K 0 -1 K = 0 fields: 1 .. 32",
                 "mean K 33 -1 K = 33 fields: 1 .. 32", "mean null -1 null pointer", "mean null out -1 null pointer", "mean n differs -1 field 1: n[1] = 4 differs from field 0's 3",
                 "mean origin differs -1 field 1: origin[2] = 0.5 differs from field 0's 0.25", "mean origin sign differs -1 field 1: origin[0] = -0 differs from field 0's 0",
                 "mean spacing differs -1 field 1: spacing = 4.5 differs from field 0's 4", "mean short disp -1 field 1: disp holds fewer than 3 n0 n1 n2 floats",
                 "mean null disp -1 field 1: disp holds fewer than 3 n0 n1 n2 floats", "mean one node -1 field 0: n[0] = 1: 2 .. 2^24 nodes per axis"):
        assert line in lines, line
    # the mean of the program's three fields (value = scale * index / 7 + shift, in float) is the oracle's
    idx = np.arange(36, dtype=np.float32)
    fields = [{"disp": (np.float32(s) * idx / np.float32(7.0) + np.float32(o)).astype(np.float32)} for s, o in ((1.0, 0.0), (-2.5, 1.0), (0.3, -4.0))]
    hexes = lambda v: [float(x).hex() for x in np.asarray(v, np.float32).reshape(-1)]
    canon = lambda words: [float.fromhex(x).hex() for x in words]
    three = [l for l in lines if l.startswith("mean three 0 ")][0].split()[3:]
    one = [l for l in lines if l.startswith("mean one 0 ")][0].split()[3:]
    assert canon(three) == hexes(ao.mean_field(fields)) and canon(one) == hexes(fields[1]["disp"])
    # the report: the whole text at the length asked for, and every shorter buffer a prefix of it
    head = [l for l in lines if l.startswith("report ") and not l.startswith(("report part", "report refused"))][0].split()
    assert head[1] == head[2] == head[3]
    at = lines.index(" ".join(head))
    assert lines[at + 1:at + 14] == ["# images 3 trim 1 min_count 2", "# voxels 9 none 2 below 5", "# image contributing upload_ms", "1 5 0.000", "2 4 0.125", "3 4 0.000",
                                    "# n voxels", "0 2", "1 3", "2 2", "3 2", "# kernel_ms wall_ms", "1.500 20.250"]
    parts = [l.split() for l in lines if l.startswith("report part")]
    assert len(parts) >= 5 and all(p[3] == head[1] and int(p[4]) == int(p[2]) - 1 and p[5] == "0" for p in parts)


# ---- featAverage's refusals -----------------------------------------------------------------------------------------------------------------
G5 = ["g.nii", "o.nii", "a.nii", "-", "-"]
UNKNOWN = "unknown command line argument: "
THREE = "every image takes three arguments: <image> <image.trans.txt|-> <image.field.nii|->"


@pytest.mark.parametrize("argv, text", [
    ([], None), (["g.nii"], None), (["g.nii", "o.nii"], None), (["-w", "-ws", "-mmean", "-mmedian", "-mtrim", "-k3", "-fnan", "-f0", "-u", "g.nii", "o.nii"], None),
    (G5[:4], THREE), (G5 + ["b.nii"], THREE), (G5[:2] + G5[2:] * 33, "more than 32 images"), (["-x"] + G5, UNKNOWN + "-x"), (["-ux"] + G5, UNKNOWN + "-ux"),
    (["-m"] + G5, "bad average: -m"), (["-mmode"] + G5, "bad average: -mmode"), (["-t"] + G5, "bad trim: -t"), (["-t0"] + G5, "bad trim: -t0"),
    (["-t16"] + G5, "bad trim: -t16"), (["-t1x"] + G5, "bad trim: -t1x"), (["-k"] + G5, "bad minimum count: -k"), (["-k0"] + G5, "bad minimum count: -k0"),
    (["-k33"] + G5, "bad minimum count: -k33"), (["-f"] + G5, "bad fill value: -f"), (["-f1x"] + G5, "bad fill value: -f1x"), (["-d"] + G5, "unknown device: "),
    (["-dx"] + G5, "unknown device: x"), (["-d0x"] + G5, "unknown device: 0x"), (["-mmedian", "-t2"] + G5, "the median drops all but the middle: -t with -mmedian"),
    (["-t2", "-mmedian"] + G5, "the median drops all but the middle: -t with -mmedian"), (["-k2"] + G5, "the minimum count exceeds the 1 images: -k2"),
    (["-k3"] + G5 + G5[2:], "the minimum count exceeds the 2 images: -k3"),
], ids=lambda v: "_".join(v[:3]) if isinstance(v, list) else None)
def test_feataverage_refuses(built, tmp_path, argv, text):
    """usage, status 255, no file left behind: none of these command lines reaches a file or asks for a device"""
    r = subprocess.run([built.FEATAVERAGE] + argv, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 255 and "Usage: featAverage [options] <grid image> <out> <image> <image.trans.txt|-> <image.field.nii|-> [...]" in r.stdout, (r.returncode, r.stdout[-400:])
    first = r.stdout.split("\n")[0]
    assert first == ("Error: " + text if text is not None else "Volumetric template from a group of registered images v1.0"), first
    assert os.listdir(tmp_path) == []


def test_feataverage_missing_files(built, tmp_path):
    """a grid image, an image, a transform or a field that cannot be read: its name, status 255, nothing written"""
    v = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    built.write_nifti(str(tmp_path / "g.nii"), v)
    before = sorted(os.listdir(tmp_path))
    for argv, text in ((["missing.nii", "o.nii", "g.nii", "-", "-"], "could not read input file: missing.nii"), (["g.nii", "o.nii", "missing.nii", "-", "-"], "could not read input file: missing.nii"),
                       (["g.nii", "o.nii", "g.nii", "missing.trans.txt", "-"], "could not read transform file: missing.trans.txt"),
                       (["g.nii", "o.nii", "g.nii", "-", "missing.field.nii"], "could not read displacement field file: missing.field.nii"),
                       (["-u", "g.nii", "o.nii", "g.nii", "-", "-"], "-u takes the mean of the displacement fields: 1 of 1 images have none")):
        r = subprocess.run([built.FEATAVERAGE] + argv, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert r.returncode == 255 and text in r.stdout, (argv, r.returncode, r.stdout[-400:])
        assert sorted(os.listdir(tmp_path)) == before


# ---- the scenario, on the oracle -----------------------------------------------------------------------------------------------------------
def test_scenario_median_beats_mean_beats_every_image(built, ao, ro, tmp_path):
    """five registered images, one of them three voxels off in every z slab: the mean is below the best single image by at least half the gap
    measured on the oracle when this was written (138.0 - 103.0), and the median below the mean by at least half that gap (103.0 - 81.8)"""
    target, gv, images = scenario(built, ro, tmp_path)
    planes = warped_planes(built, ao, target.shape, images, gv)
    mean, _, mask = ao.average(planes, 0)
    trim1, median = ao.average(planes, 1)[0], ao.average(planes, 15)[0]
    full = mask == 31
    single = [rms(p, target, full) for p in planes]
    r_mean, r_trim, r_median = rms(mean, target, full), rms(trim1, target, full), rms(median, target, full)
    print("voxels %d of %d; single %s; mean %.1f; trim 1 %.1f; median %.1f" % (full.sum(), full.size, " ".join("%.1f" % s for s in single), r_mean, r_trim, r_median))
    assert full.sum() > 0.9 * full.size
    assert r_mean < min(single) - 0.5 * (138.0 - 103.0)
    assert r_median < r_mean - 0.5 * (103.0 - 81.8)
    assert r_trim < r_mean
