"""CPU suite: the intensity matching without a GPU -- the oracle tests/normalize_oracle.c against a float64 numpy
restatement that shares no code with it, the product's host code (normalize_host.c) against the oracle bit for bit, the hand cases, the
shapes that take the GPU kernels past their launch caps, the host file under the sanitizers as a stand-alone program, featNormalize's
refusals, and the scenario the feature is there for, on the oracle.

The scenario's figures (oracle, section 7r's scenario with every atlas on a scale of its own; RMS of the mean of five images against
the target over the voxels all five reach) are printed by the scenario tests and recorded in DESIGN.md section 7s."""
import os
import re
import subprocess

import numpy as np
import pytest

from average_cases import AverageOracle, warped_planes
from normalize_cases import (APPLY_CAP, APPLY_STRETCH, BIG_IMAGE, BIG_REF, BRICK, HIST_CAP, KNOTS, MAP_KINDS, MODES, SHAPES, NormalizeOracle, Refused, apply_numpy, bits32, bits64,
                             bricks, inside_numpy, kernel_constants, one_bin_pair, pair, rms, same_tables, scenario, transfer_numpy, words_numpy)
from resample_cases import ResampleOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = ("sift3d_normalize_defaults", "sift3d_normalize_check", "sift3d_normalize_transfer", "sift3d_transfer_check", "sift3d_normalize_report_text")


@pytest.fixture(scope="module", autouse=True)
def entry_points(built):
    """the feature under test: the C-ABI's functions in both libraries, the mirror's functions and the command line's path"""
    for name in ("sift3d_overlap_histograms", "sift3d_apply_transfer", "sift3d_normalize_intensity") + HOST:
        assert hasattr(built.hip_lib(), name), name
    for name in HOST:
        assert hasattr(built.host_lib(), name), name
    for name in ("normalize_params", "normalize_check", "normalize_transfer", "transfer_check", "overlap_histograms", "apply_transfer", "normalize_intensity",
                 "normalize_report_text", "FEATNORMALIZE"):
        assert hasattr(built, name), name
    assert built.ABI_VERSION == 7           # only declarations were added


@pytest.fixture(scope="module")
def no(tmp_path_factory):
    return NormalizeOracle(tmp_path_factory.mktemp("normalize_oracle"))


@pytest.fixture(scope="module")
def ao(tmp_path_factory):
    return AverageOracle(tmp_path_factory.mktemp("average_oracle"))


@pytest.fixture(scope="module")
def ro(tmp_path_factory):
    return ResampleOracle(tmp_path_factory.mktemp("resample_oracle"))


def random_words(rng, n, kind):
    """(hist_a, hist_b, sums) of n voxel pairs: spread, one dominant bin, or many empty bins"""
    a, b = rng.integers(0, 1024, n), rng.integers(0, 1024, n)
    if kind == "dominant":
        keep = rng.random(n) < 0.1
        a, b = np.where(keep, a, 500), np.where(keep, b, 17)
    elif kind == "empty":
        a, b = a // 64 * 64, b // 128 * 128 + 3
    elif kind == "ends":
        a, b = np.where(a < 512, 0, 1023), np.where(b < 300, 0, 1023)
    la, lb = [int(x) for x in a], [int(x) for x in b]
    sums = [n, sum(la), sum(lb), sum(x * x for x in la), sum(x * x for x in lb), sum(x * y for x, y in zip(la, lb))]
    return np.bincount(a, minlength=1024).astype(np.int64), np.bincount(b, minlength=1024).astype(np.int64), sums


AR, BR = (np.float32(-100.0), np.float32(923.5)), (np.float32(0.5), np.float32(2.25))


# ---- the contract: the oracle against numpy --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES[1:], ids=lambda s: "x".join(map(str, s[::-1])))
def test_oracle_words_equal_numpy(built, no, ao, shape):
    """the histograms by np.bincount, the sums as Python integers and the classes, for every map kind, with and without a mask and a field"""
    seen = 0
    for n, kind in enumerate(MAP_KINDS):
        for field in (False, True):
            R, a, M = pair(built, shape, kind, field=field, seed=n, masked=bool(n % 2) or field)
            ar, br = no.range(R), no.range(a["image"])
            got = no.overlap(built, R, a, ar, br, None, M)
            W = warped_planes(built, ao, shape, [a])[0]
            A = built.resample_map(np.eye(4, dtype=np.float32) if a["t"] is None else a["t"], None, a.get("vox2key"))
            want = words_numpy(R, W, ar, br, M, None if field else inside_numpy(A, shape, a["image"].shape))
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
            assert got[3]["masked"] == want[3]["masked"] and sum(got[3].values()) + got[2][0] == R.size
            if field:
                assert got[3]["outside"] + got[3]["excluded"] == want[3]["excluded"]
            else:
                assert got[3] == want[3]
            assert kind != "outside" or got[3]["outside"] + got[3]["masked"] == R.size
            seen += got[2][0]
    assert seen > 0


@pytest.mark.parametrize("kind", ["spread", "dominant", "empty", "ends"])
def test_oracle_and_host_tables_equal_numpy(built, no, kind):
    """normalize_host.c against the oracle, and the oracle against numpy, bit for bit over random histograms: n = 2, 3 and more, Q = 2, 64, 256
    and the others of KNOTS, empty bins, one dominant bin, the two end bins alone"""
    rng = np.random.default_rng(len(kind))
    tables = 0
    for n in (2, 3, 7, 1000, 50000):
        ha, hb, sums = random_words(rng, n, kind)
        for mode in MODES:
            for Q in (KNOTS if mode == "hist" else (64,)):
                try:
                    want = no.transfer(mode, ha, hb, sums, AR, BR, Q)
                except Refused as e:
                    with pytest.raises(Refused) as e2:
                        transfer_numpy(mode, ha, hb, sums, AR, BR, Q)
                    assert e2.value.code == e.code
                    with pytest.raises(built.Sift3DError, match=e.text):
                        built.normalize_transfer(mode, ha, hb, sums, AR, BR, Q)
                    continue
                same_tables(want, transfer_numpy(mode, ha, hb, sums, AR, BR, Q))
                got = built.normalize_transfer(mode, ha, hb, sums, AR, BR, Q)
                same_tables(got, want)
                assert built.transfer_check(got) is None
                assert (np.diff(got["xb"]) > 0).all() and (np.diff(got["xa"]) >= 0).all() and 2 <= got["m"] <= Q + 1
                tables += 1
    assert tables > 10


def test_oracle_apply_equals_numpy(no):
    """the apply rule array by array: values below, at, between and above the knots, outside the image's range, non-finite ones"""
    rng = np.random.default_rng(5)
    for kind, mode, Q in (("spread", "hist", 64), ("dominant", "hist", 256), ("empty", "hist", 3), ("spread", "linear", 64), ("ends", "hist", 2)):
        ha, hb, sums = random_words(rng, 20000, kind)
        t = no.transfer(mode, ha, hb, sums, AR, BR, Q)
        lo, hi = float(BR[0]), float(BR[1])
        at_knots = (lo + (hi - lo) * t["xb"] / 1023.0).astype(np.float32)
        v = np.concatenate([rng.uniform(lo, hi, 4000), rng.uniform(lo - 3, hi + 3, 500), at_knots, np.nextafter(at_knots, np.float32(-np.inf)), np.nextafter(at_knots, np.float32(np.inf)),
                            [lo, hi, np.nan, np.inf, -np.inf, 0.0, -0.0, 1e30, -1e30]]).astype(np.float32)
        got, want = no.apply(v, t), apply_numpy(v, t)
        assert np.array_equal(bits32(got), bits32(want)), (kind, mode, Q, int((bits32(got) != bits32(want)).sum()))


# ---- hand cases -------------------------------------------------------------------------------------------------------------------------
def test_an_image_matched_to_itself(built, no):
    """R = B under the identity in hist mode: xa and xb have equal bits, and the output is the image to within one float ulp of the
    larger end of its range"""
    R, a, _ = pair(built, SHAPES[3], "identity", seed=2, k=0)
    a = {"image": R}
    out, info = no.stage(built, R, a, mode="hist", knots=64)
    t = info["table"]
    assert np.array_equal(bits64(t["xa"]), bits64(t["xb"])) and np.array_equal(info["hist_a"], info["hist_b"]) and info["counts"]["outside"] == 0
    lo, hi = no.range(R)
    ulp = float(np.spacing(np.float32(max(abs(lo), abs(hi)))))
    fin = np.isfinite(R)
    assert fin.sum() > 0.9 * R.size and np.abs(out[fin].astype(np.float64) - R[fin].astype(np.float64)).max() <= ulp


@pytest.mark.parametrize("mode", MODES)
def test_output_is_monotone_and_keeps_the_non_finite_bits(built, no, mode):
    """out is non-decreasing over the sorted finite voxels, exactly; a non-finite voxel keeps its bits, NaN payloads and signs included"""
    for seed, kind, field in ((3, "half", False), (4, "rotation", True)):
        R, a, M = pair(built, SHAPES[3], kind, field=field, seed=seed, masked=field)
        B = a["image"]
        raw = bits32(B).copy().reshape(B.shape)
        raw[1, 2, 3:7] = [0x7FC12345, 0xFFC00001, 0x7F800001, 0xFF800000]
        a["image"] = raw.view(np.float32)
        out, info = no.stage(built, R, a, None, M, mode=mode, knots=17)
        fin = np.isfinite(a["image"])
        assert 0 < (~fin).sum() < 0.1 * fin.size and np.array_equal(bits32(out)[~fin], bits32(a["image"])[~fin])
        order = np.argsort(a["image"][fin], kind="stable")
        assert (np.diff(out[fin][order].astype(np.float64)) >= 0).all()
        assert np.isfinite(out[fin]).all() and out[fin].max() > out[fin].min()


def test_refusals_come_with_their_text(built, no):
    rng = np.random.default_rng(9)
    ha, hb, sums = random_words(rng, 1000, "spread")
    flat_b, flat_a = np.zeros(1024, np.int64), np.zeros(1024, np.int64)
    flat_b[1023], flat_a[0] = 1000, 1000
    sb = [sums[0], sums[1], 1000 * 1023, sums[3], 1000 * 1023 * 1023, 0]
    sa = [sums[0], 0, sums[2], 0, sums[4], 0]
    zero = np.zeros(1024, np.int64)
    one = np.zeros(1024, np.int64)
    one[7] = 1
    for args, code, text in (((("linear", ha, flat_b, sb, AR, BR)), -4, "the counted voxels of the image all fall in one bin: no variance to match"),
                             ((("linear", flat_a, hb, sa, AR, BR)), -3, "the counted voxels of the reference all fall in one bin: no variance to match"),
                             ((("linear", zero, zero, [0] * 6, AR, BR)), -2, "0 voxels are counted: at least 2 are needed"),
                             ((("hist", one, one, [1, 7, 7, 49, 49, 49], AR, BR)), -2, "1 voxels are counted: at least 2 are needed")):
        with pytest.raises(built.Sift3DError, match=re.escape(text)) as e:
            built.normalize_transfer(*args)
        assert e.value.code == -1
        for f in (no.transfer, transfer_numpy):
            with pytest.raises(Refused) as r:
                f(*args)
            assert r.value.code == code and r.value.text in text
    for args, text in ((("linear", ha, hb, sums, (1.0, 1.0), BR), "a_range = 1 1: finite, hi > lo"), (("linear", ha, hb, sums, AR, (0.0, np.inf)), "b_range = 0 inf: finite, hi > lo"),
                       (("hist", ha, hb, sums, AR, BR, 1), "knots = 1: 2 .. 256"), (("hist", ha, hb, sums, AR, BR, 257), "knots = 257: 2 .. 256"),
                       ((2, ha, hb, sums, AR, BR), "mode = 2: 0 (linear) or 1 (hist)"), (("linear", ha, hb, [sums[0] + 1] + sums[1:], AR, BR), "they must agree"),
                       (("linear", ha - 5, hb, sums, AR, BR), "holds a negative count")):
        with pytest.raises(built.Sift3DError, match=re.escape(text)):
            built.normalize_transfer(*args)
    assert built.normalize_transfer("linear", ha, hb, sums, AR, BR, knots=64)["m"] == 2
    p = built.normalize_params()
    assert (p.mode, p.knots, p.device) == (0, 64, 0) and built.normalize_check(p) is None and built.normalize_check(built.normalize_params(mode="linear", knots=0)) is None
    assert "knots = 0: 2 .. 256" in built.normalize_check(built.normalize_params(mode="hist", knots=0))
    with pytest.raises(ValueError):
        built.normalize_params(bins=64)


def test_a_mask_of_zeros_leaves_nothing_to_count(built, no):
    R, a, _ = pair(built, SHAPES[2], "identity", seed=1)
    for mode in MODES:
        with pytest.raises(Refused) as r:
            no.stage(built, R, a, None, np.zeros(R.shape, np.float32), mode=mode)
        assert r.value.code == -2
    ha, hb, sums, counts = no.overlap(built, R, a, no.range(R), no.range(a["image"]), None, np.zeros(R.shape, np.float32))
    assert counts == {"masked": R.size, "outside": 0, "excluded": 0} and sums == [0] * 6 and not ha.any() and not hb.any()


def test_one_bin_volumes_on_the_oracle(built, no):
    """every counted voxel in bin 0, or in bin 1023: the sums reach their ends; linear refuses (no variance), hist places its knots inside the
    one bin by rank, so that it has a table, with every knot within half a quantiser unit of the bin"""
    for top in (False, True):
        R, a, M = one_bin_pair(SHAPES[3], top)
        ha, hb, sums, counts = no.overlap(built, R, a, no.range(R), no.range(a["image"]), None, M)
        n, q = R.size - 1, 1023 if top else 0
        assert counts == {"masked": 1, "outside": 0, "excluded": 0} and sums == [n, n * q, n * q, n * q * q, n * q * q, n * q * q] and ha[q] == hb[q] == n
        with pytest.raises(Refused) as r:
            no.stage(built, R, a, None, M, mode="linear")
        assert r.value.code == -3
        t = no.stage(built, R, a, None, M, mode="hist")[1]["table"]
        assert t["m"] == 65 and np.abs(t["xb"] - q).max() <= 0.5 and np.abs(t["xa"] - q).max() <= 0.5


def test_report_text(built, no):
    R, a, M = pair(built, SHAPES[2], "half", seed=6, masked=True)
    out, info = no.stage(built, R, a, None, M, mode="hist", knots=8)
    rep = built.NormalizeReport()
    rep.mode, rep.knots, rep.reference_voxels, rep.image_voxels = 1, 8, R.size, a["image"].size
    rep.counts[:] = [info["counts"][k] for k in built.NORMALIZE_COUNTS]
    rep.sums[:] = info["sums"]
    rep.table = built.transfer_struct(dict(info["table"], struct=None))
    rep.hist_ms, rep.apply_ms, rep.wall_ms = 1.5, 0.25, 20.125
    lines = built.normalize_report_text(rep).split("\n")
    m = info["table"]["m"]
    assert lines[0] == "# mode hist knots 8 kept %d" % m and lines[1].startswith("# range_reference ") and lines[2].startswith("# range_image ")
    assert lines[3] == "# reference_voxels %d counted %d masked %d outside %d excluded %d" % (R.size, info["sums"][0], info["counts"]["masked"], info["counts"]["outside"], info["counts"]["excluded"])
    assert lines[4] == "# image_voxels %d" % a["image"].size and lines[5] == "# knot xb xa slope"
    rows = [l.split() for l in lines[6:6 + m]]
    assert [int(r[0]) for r in rows] == list(range(m)) and np.array_equal(bits64([float(r[1]) for r in rows]), bits64(info["table"]["xb"]))
    assert np.array_equal(bits64([float(r[2]) for r in rows]), bits64(info["table"]["xa"]))
    assert lines[6 + m] == "# tail wa" and lines[8 + m:10 + m] == ["# hist_ms apply_ms wall_ms", "1.500 0.250 20.125"]
    rep.table.m = 1
    with pytest.raises(built.Sift3DError):
        built.normalize_report_text(rep)


# ---- the shapes of the GPU suite ----------------------------------------------------------------------------------------------------------
def test_shapes_follow_the_kernel_file(built):
    K = kernel_constants()
    assert K["NORM_THREADS"] == 256 and 4 * K["NORM_THREADS"] == BRICK[0] * BRICK[1] * BRICK[2] and K["NORM_MAX_BLOCKS"] == HIST_CAP and HIST_CAP % 8 == 0
    assert K["NORM_BINS"] == built.NORMALIZE_BINS == 1024 and K["NORM_WORDS"] == 9 and K["APPLY_MAX_KNOTS"] == built.NORMALIZE_MAX_KNOTS == 257
    assert K["APPLY_MAX_BLOCKS"] == APPLY_CAP and K["APPLY_THREADS"] * K["APPLY_VPT"] == APPLY_STRETCH
    # each capped loop goes round more than twice, the last trip a partial one
    assert bricks(BIG_REF) > 2 * HIST_CAP and bricks(BIG_REF) % HIST_CAP != 0 and BIG_REF[2] % 4 != 0
    n = int(np.prod(BIG_IMAGE))
    assert n > 2 * APPLY_CAP * APPLY_STRETCH and n % APPLY_STRETCH != 0 and n % 4 != 0 and -(-n // APPLY_STRETCH) % APPLY_CAP != 0
    # the bisection's steps change where m passes a power of two: m = Q + 1 kept knots at most
    assert KNOTS == (2, 3, 64, 65, 255, 256) and max(KNOTS) + 1 == K["APPLY_MAX_KNOTS"]
    assert SHAPES[2] == tuple(b + 1 for b in BRICK) and all(d % b for d, b in zip(SHAPES[3], BRICK))


# ---- normalize_host.c under the sanitizers ------------------------------------------------------------------------------------------------
def test_host_file_under_sanitizers(tmp_path):
    """normalize_host.c and tests/normalize_host_san.c as one program, with and without -fsanitize=address,undefined: both exit clean and
    print the same lines"""
    csrc = os.path.join(ROOT, "3d_sift_cuda_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "normalize_host_san.c"), os.path.join(csrc, "normalize_host.c")]
    base = ["cc", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-ffp-contract=off", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-I" + csrc]
    out = {}
    for name, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])):
        exe = str(tmp_path / ("normalize_host_" + name))
        subprocess.run(base + flags + ["-o", exe] + src + ["-lm"], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
        out[name] = r.stdout
    text = out["san"]
    assert text == out["plain"]
    lines = text.split("\n")
    for line in ("defaults 0 64 0", "check null -1 null pointer", "check defaults 0 ", "check mode -1 -1 mode = -1: 0 (linear) or 1 (hist)", "check mode 0 0 ", "check mode 1 0 ",
                 "check mode 2 -1 mode = 2: 0 (linear) or 1 (hist)", "check knots 1 mode 0 0 ", "check knots 1 mode 1 -1 knots = 1: 2 .. 256", "check knots 2 mode 1 0 ",
                 "check knots 256 mode 1 0 ", "check knots 257 mode 1 -1 knots = 257: 2 .. 256", "check knots -5 mode 1 -1 knots = -5: 2 .. 256", "check short_err -1 mode = 7",
                 "check no_err -1", "transfer null -1 null pointer", "transfer mode -1 mode = 2: 0 (linear) or 1 (hist)", "transfer knots -1 knots = 1: 2 .. 256",
                 "transfer a_range -1 a_range = 1 1: finite, hi > lo", "transfer b_range -1 b_range = 0 nan: finite, hi > lo",
                 "transfer total -1 sums[0] = 1001, hist_a holds 1000 and hist_b 1000 voxels: they must agree", "transfer negative -1 bin 5 holds a negative count",
                 "transfer one -1 1 voxels are counted: at least 2 are needed", "transfer none -1 0 voxels are counted: at least 2 are needed",
                 "transfer flat image linear -1 the counted voxels of the image all fall in one bin: no variance to match",
                 "transfer flat image hist 0 ",
                 "transfer flat reference linear -1 the counted voxels of the reference all fall in one bin: no variance to match",
                 "transfer flat reference hist 0 ", "transfer short_err -1 mode = 5",
                 "tcheck null -1 null pointer", "tcheck m -1 table: m = 1 knots: 2 .. 257", "tcheck m -1 table: m = 258 knots: 2 .. 257", "tcheck xb -1 table: xb[3] is not above xb[2]",
                 "tcheck xa -1 table: xa[4] is below xa[3]", "tcheck nan -1 table: knot 1 is not finite", "tcheck range -1 table: a range is not finite or has hi <= lo",
                 "tcheck tail -1 table: wa or tail is not finite", "report refused -1 -1"):
        assert line in lines, line
    tables = [l for l in lines if l.startswith("table ") and not l.startswith("table check")]
    assert len(tables) == 48 and sum(" 0 m " in l for l in tables) > 30 and all(l == "table check 0 " for l in lines if l.startswith("table check"))
    head = [l for l in lines if l.startswith("report ") and not l.startswith(("report part", "report refused"))][0].split()
    assert head[1] == head[2] == head[3]
    at = lines.index(" ".join(head))
    assert lines[at + 1] == "# mode hist knots 8 kept 9" and lines[at + 4] == "# reference_voxels 1200 counted 1000 masked 100 outside 60 excluded 40"
    parts = [l.split() for l in lines if l.startswith("report part")]
    assert len(parts) == 5 and all(p[3] == head[1] and int(p[4]) == int(p[2]) - 1 and p[5] == "0" for p in parts)


# ---- featNormalize's refusals ---------------------------------------------------------------------------------------------------------------
A5 = ["r.nii", "i.nii", "-", "-", "o.nii"]
UNKNOWN = "unknown command line argument: "
USAGE = "Usage: featNormalize [options] <reference image> <image> <image.trans.txt|-> <image.field.nii|-> <out>"


@pytest.mark.parametrize("argv, text", [
    ([], None), (["r.nii"], None), (A5[:4], None), (A5 + ["x"], None), (["-w", "-ws", "-mlinear", "-mhist", "-q2", "-q256"] + A5[:4], None), (["-x"] + A5, UNKNOWN + "-x"),
    (["-m"] + A5, "bad mode: -m"), (["-mmedian"] + A5, "bad mode: -mmedian"), (["-mhistx"] + A5, "bad mode: -mhistx"), (["-q64"] + A5, "the knots are the quantile matching's: -q without -mhist"),
    (["-q64", "-mlinear"] + A5, "the knots are the quantile matching's: -q without -mhist"), (["-mhist", "-q1"] + A5, "bad knots: -q1"), (["-mhist", "-q257"] + A5, "bad knots: -q257"),
    (["-mhist", "-q"] + A5, "bad knots: -q"), (["-mhist", "-q8x"] + A5, "bad knots: -q8x"), (["-kmask.nii"] + A5, "-k takes the mask image as the next argument: -kmask.nii"),
    (["-k"], "-k takes the mask image as the next argument: -k"), (["-d"] + A5, "unknown device: "), (["-dx"] + A5, "unknown device: x"), (["-d0x"] + A5, "unknown device: 0x"),
], ids=lambda v: "_".join(v[:3]) if isinstance(v, list) else None)
def test_featnormalize_refuses(built, tmp_path, argv, text):
    """usage, status 255, no file left behind: none of these command lines reaches a file or asks for a device"""
    r = subprocess.run([built.FEATNORMALIZE] + argv, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 255 and USAGE in r.stdout, (r.returncode, r.stdout[-400:])
    first = r.stdout.split("\n")[0]
    assert first == ("Error: " + text if text is not None else "Volumetric intensity matching of a registered image v1.0"), first
    assert os.listdir(tmp_path) == []


def test_featnormalize_missing_files_and_mask_extents(built, tmp_path):
    """an image, a transform, a field or a mask that cannot be read, and a mask on another grid: the text, status 255, nothing written"""
    v = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    built.write_nifti(str(tmp_path / "g.nii"), v)
    built.write_nifti(str(tmp_path / "m.nii"), np.ones((2, 3, 5), np.float32))
    before = sorted(os.listdir(tmp_path))
    for argv, text in ((["missing.nii", "g.nii", "-", "-", "o.nii"], "could not read input file: missing.nii"), (["g.nii", "missing.nii", "-", "-", "o.nii"], "could not read input file: missing.nii"),
                       (["g.nii", "g.nii", "missing.trans.txt", "-", "o.nii"], "could not read transform file: missing.trans.txt"),
                       (["g.nii", "g.nii", "-", "missing.field.nii", "o.nii"], "could not read displacement field file: missing.field.nii"),
                       (["-k", "missing.nii", "g.nii", "g.nii", "-", "-", "o.nii"], "could not read input file: missing.nii"),
                       (["-k", "m.nii", "g.nii", "g.nii", "-", "-", "o.nii"], "Error: the mask's extents 5 3 2 differ from the reference's 4 3 2")):
        r = subprocess.run([built.FEATNORMALIZE] + argv, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert r.returncode == 255 and text in r.stdout, (argv, r.returncode, r.stdout[-400:])
        assert sorted(os.listdir(tmp_path)) == before
    r = subprocess.run([built.FEATNORMALIZE, "-k", "m.nii", "g.nii", "g.nii", "-", "-", "o.nii"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert USAGE in r.stdout


# ---- the scenario, on the oracle -----------------------------------------------------------------------------------------------------------
def scenario_figures(built, no, ao, ro, tmp, gamma):
    """RMS of the mean of the five images against the target over the voxels all five reach: clean, remapped, after linear, after hist; and
    "image ...": the RMS of an atlas image against its own clean version, over all its voxels, averaged over the five"""
    target, gv, clean, remapped = scenario(built, ro, tmp, gamma)
    planes = warped_planes(built, ao, target.shape, clean, gv)
    mean, _, mask = ao.average(planes, 0)
    full = mask == 31
    assert full.sum() > 0.9 * full.size
    out = {"clean": rms(mean, target, full), "raw": rms(ao.average(warped_planes(built, ao, target.shape, remapped, gv), 0)[0], target, full)}
    for mode in MODES:
        fixed = [dict(a, image=no.stage(built, target, a, gv, None, mode=mode, knots=64)[0]) for a in remapped]
        avg, _, m2 = ao.average(warped_planes(built, ao, target.shape, fixed, gv), 0)
        assert np.array_equal(m2, mask)
        out[mode] = rms(avg, target, full)
        out["image " + mode] = float(np.mean([rms(f["image"], c["image"], np.isfinite(c["image"])) for f, c in zip(fixed, clean)]))
    out["image raw"] = float(np.mean([rms(r["image"], c["image"], np.isfinite(c["image"])) for r, c in zip(remapped, clean)]))
    return out


def test_scenario_normalised_atlases_average_like_clean_ones(built, no, ao, ro, tmp_path):
    """section 7r's five atlases, each on a scale of its own (gain 0.6 .. 1.5, offset -400 .. 250): after either mode the mean is below the
    unnormalised one by at least half the gap between unnormalised and clean (section 7j's half-the-gap convention)"""
    f = scenario_figures(built, no, ao, ro, tmp_path, False)
    print("gain and offset: clean %.1f; remapped %.1f; linear %.1f; hist %.1f; per image: remapped %.1f; linear %.1f; hist %.1f"
          % (f["clean"], f["raw"], f["linear"], f["hist"], f["image raw"], f["image linear"], f["image hist"]))
    assert abs(f["clean"] - 103.0) < 0.05           # DESIGN.md section 7r's figure
    assert f["raw"] > f["clean"]
    for mode in MODES:
        assert f[mode] < f["raw"] - 0.5 * (f["raw"] - f["clean"]), (mode, f)


def test_scenario_quantile_matching_undoes_a_gamma_curve(built, no, ao, ro, tmp_path):
    """second leg: well registered atlases, each through a gamma curve of its own (1.4 .. 1.8) on its own range, which no gain and offset
    undo: linear stays above clean, and hist is below linear by at least half of (linear - clean)"""
    f = scenario_figures(built, no, ao, ro, tmp_path, True)
    print("gamma, gain and offset: clean %.1f; remapped %.1f; linear %.1f; hist %.1f; per image: remapped %.1f; linear %.1f; hist %.1f"
          % (f["clean"], f["raw"], f["linear"], f["hist"], f["image raw"], f["image linear"], f["image hist"]))
    assert f["raw"] > f["linear"] > f["clean"], f         # the leg's premise: there is a gap for the rule to halve
    assert f["hist"] < f["linear"] - 0.5 * (f["linear"] - f["clean"]), f
