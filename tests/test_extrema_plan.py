"""CPU suite: the launch plan of the extrema passes (3d_sift_cuda_amd/csrc/extrema_plan.h).

Every form of the first phase gives the same lists, so the exact-list suites cannot tell which form ran, on which grid, or how
the own-level list was cut into segments: a wrong branch costs only time.  tests/extrema_plan_check.cpp prints the plan with the
host C++ compiler; here it is held, field by field, against a restatement of the rules sift3d_launch_extrema applied inline
before the plan existed, against the rows the kernels' comments state literally, and against invariants the kernels rely on.
The same program is built once more under AddressSanitizer + UndefinedBehaviorSanitizer (a host program of its own, nothing
preloaded) and must print the same answers.

The third phase's workgroup count is asserted to lie in [min(64, list2_cap), 4096] and to be a multiple of 8 from 8 up; the grid
keeps list2_cap a multiple of 8, as every caller does (it is the own-level list's capacity, 64 * 1024 at the least): for a
capacity below 64 that is no multiple of 8 the rule rounds down below the capacity, which is the rule as it was, moved unchanged.
"""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3d_sift_cuda_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "extrema_plan_check.cpp")
SEGS = 64


def cdiv(a, b):
    return -(-a // b)


# ---- the rules, restated ------------------------------------------------------------------------------------------------------
def want_plan(X, Xl, Y, Z, z_lo, z_hi, own, surv_cap, strict, pair, defer, ntaps, list2_cap):
    """(status, form, z0, z1, zchunk, z_blocks, segments, seg_cap, tiles_x, tiles_y, gx, gy, gz, vx, vy, pair, defer, lazy_wgs,
    list2_seg_cap) as the launcher decided them inline."""
    nothing = ("nothing", "none") + (0,) * 17
    if Xl < 3 or Y < 3 or Z < 3:
        return nothing
    z0, z1 = max(z_lo, 1), min(z_hi, Z - 1)
    if z1 <= z0:
        return nothing
    planes = z1 - z0
    if not (X % 4 == 0 and X >= 8 and own and surv_cap > 0):      # one launch, every voxel takes all three tests
        bx, by = cdiv(X, 64), cdiv(Y, 4)
        return ("unsupported" if pair or defer else "ok", "generic", z0, z1, 1, planes, 0, 0, bx, by, bx, by, planes, 0, 0, pair, defer, 0, 0)
    xt_m, yt_m = cdiv(X, 256), cdiv(Y - 2, 4)
    waves, zchunk = xt_m * yt_m, 1
    if not strict:
        for need in (2048, 512):
            fits = [zc for zc in (64, 32, 16, 8) if waves * cdiv(planes, zc) >= need and (zc + 2) * X * Y * 4 < 2 ** 32]
            if fits:
                zchunk = fits[0]
                break
    nz = cdiv(planes, zchunk)
    nseg = min(nz, SEGS)
    segcap = surv_cap // nseg
    if strict:
        form, tx, ty = "strict", cdiv(X, 64), cdiv(Y, 4)
        gx = tx * ty
    elif zchunk >= 2:
        form, tx, ty = "march", xt_m, cdiv(yt_m, 4)
        gx = tx * ty
    else:
        form, tx, ty = "plane", cdiv(X - 2, 248), cdiv(Y - 2, 2)
        gx = cdiv(tx * ty, 4)
    head = (form, z0, z1, zchunk, nz, nseg, segcap, tx, ty, gx, nz, 1, cdiv(segcap, 256), nseg, pair, defer)
    if not defer:
        return ("ok",) + head + (0, 0)
    R = ntaps // 2 if ntaps >= 0 else -((-ntaps) // 2)
    if ntaps != 2 * R + 1 or R < 1 or R > 8 or list2_cap <= 0 or X * Y >= 2 ** 29:
        return ("invalid",) + head + (0, 0)
    if R != 8:
        return ("unsupported",) + head + (0, 0)
    wgs = min(max(X * Y * Z // 2048, 64), 4096, list2_cap)
    if wgs >= 8:
        wgs -= wgs % 8
    return ("ok",) + head + (wgs, list2_cap // nseg)


def want_segment(b, n):
    return b * SEGS // n if n >= SEGS else b


# ---- the grid -----------------------------------------------------------------------------------------------------------------
CUBES = [(n, n, n, n) for n in (16, 24, 32, 48, 64, 96, 128, 192, 256, 384, 512, 768, 1024)]
# (X, Xl, Y, Z): the shapes of the GPU suites (tests/test_gpu_parity.py, test_gpu_image_like.py, test_gpu_extrema_forms.py) dense
# and with pitched rows, rows of 7 and 9, two x tiles of either form, more than 64 z blocks, planes near the 4 GiB bound of the
# march's buffer descriptor and beyond 2^29 voxels, and shapes with nothing to search
ODD = [(17, 17, 13, 11), (20, 17, 13, 11), (32, 32, 32, 32), (64, 64, 48, 40), (36, 33, 21, 19), (33, 33, 21, 19), (132, 130, 6, 9),
       (8, 5, 70, 7), (256, 256, 8, 8), (300, 300, 20, 12), (44, 44, 36, 40), (43, 43, 36, 40), (256, 256, 40, 24), (64, 64, 48, 40),
       (16, 16, 11, 12), (13, 13, 11, 12), (112, 112, 104, 96), (8, 8, 514, 34), (260, 260, 258, 34), (8, 8, 3, 3), (252, 252, 6, 5),
       (12, 12, 10, 70), (7, 7, 5, 3), (9, 9, 9, 9), (4, 4, 9, 9), (8, 3, 9, 9), (8, 2, 9, 9), (8, 8, 2, 9), (8, 8, 9, 2),
       (4096, 4096, 4096, 70), (8192, 8192, 8192, 80), (16384, 16384, 16384, 40), (32768, 32768, 16384, 12), (32768, 32768, 16383, 12),
       (2048, 2048, 2048, 300), (512, 512, 512, 130), (512, 510, 512, 66)]


def windows(Z):
    """the whole volume, and slab windows strictly inside it (one of them empty)"""
    w = [(0, Z)]
    if Z >= 8:
        w += [(Z // 4, Z - Z // 4), (2, Z // 2), (Z // 2, Z // 2)]
    return w


def plan_grid():
    for (X, Xl, Y, Z) in CUBES + ODD:
        for (z_lo, z_hi), strict, (pair, defer), surv_cap in itertools.product(windows(Z), (0, 1), ((0, 0), (0, 1), (1, 0), (1, 1)),
                                                                               (4096, 64 * 1024 - 8, 64 * 1024 + X * Y * Z // 64)):
            cap8 = surv_cap - surv_cap % 8
            yield (X, Xl, Y, Z, z_lo, z_hi, 1, surv_cap, strict, pair, defer, 17, cap8)
    for (X, Xl, Y, Z) in ((64, 64, 64, 64), (256, 256, 256, 256), (63, 63, 64, 64)):
        yield (X, Xl, Y, Z, 0, Z, 0, 1 << 20, 0, 0, 0, 0, 0)                  # no own-level list offered
        yield (X, Xl, Y, Z, 0, Z, 1, 0, 0, 0, 0, 0, 0)                        # ... or one that holds nothing
        for ntaps, cap in ((17, 0), (17, -1), (15, 4096), (16, 4096), (18, 4096), (19, 4096), (1, 4096), (0, 4096), (-3, 4096), (3, 4096),
                           (17, 40), (17, 8), (17, 4096)):
            yield (X, Xl, Y, Z, 0, Z, 1, 1 << 20, 0, 0, 1, ntaps, cap)             # what the third phase refuses, small second lists


def build(tmp, name, extra):
    exe = str(tmp / name)
    r = subprocess.run([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", CSRC] + extra + ["-o", exe, SRC],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        assert r.stderr == "", r.stderr[-3000:]
        return r.stdout.split("\n")[:-1]
    run.exe = exe
    return run


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return build(tmp_path_factory.mktemp("extrema_plan"), "extrema_plan_check", [])


def ask(g):
    return "plan " + " ".join(str(int(v)) for v in g)


def parse(line):
    f = line.split(" ")
    assert f[0] == "plan" and len(f) == 20, line
    return (f[1], f[2]) + tuple(int(v) for v in f[3:])


FIELDS = ("status", "form", "z0", "z1", "zchunk", "z_blocks", "segments", "seg_cap", "tiles_x", "tiles_y", "gx", "gy", "gz", "vx", "vy",
          "pair", "defer", "lazy_wgs", "list2_seg_cap")


@pytest.fixture(scope="module")
def planned(check):
    """The plan over the grid, asked once: [(request, answer as a dict)]."""
    grid = list(plan_grid())
    got = check([ask(g) for g in grid])
    assert len(got) == len(grid)
    return [(g, dict(zip(FIELDS, parse(a)))) for g, a in zip(grid, got)]


def test_plan_equals_the_restated_rules(planned):
    bad = []
    for g, p in planned:
        want = dict(zip(FIELDS, want_plan(*g)))
        diff = [f for f in FIELDS if p[f] != want[f]]
        if diff:
            bad.append((g, diff, [p[f] for f in diff], [want[f] for f in diff]))
    assert not bad, (len(bad), bad[:5])
    # the grid reaches what it is meant to reach
    seen = {(p["status"], p["form"]) for _, p in planned}
    assert seen >= {("ok", f) for f in ("generic", "plane", "march", "strict")} | {("nothing", "none"), ("unsupported", "generic"),
                                                                                  ("invalid", "march"), ("unsupported", "march")}
    assert {p["zchunk"] for _, p in planned} >= {1, 8, 16, 32, 64}
    assert any(p["z_blocks"] > SEGS for _, p in planned) and any(1 < p["z_blocks"] < SEGS for _, p in planned)
    assert {(p["pair"], p["defer"]) for _, p in planned if p["status"] == "ok" and p["form"] == "march"} == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_rows_the_kernels_comments_state(check):
    def one(X, Xl, Y, Z, z_lo=0, z_hi=None, strict=0, own=1):
        return dict(zip(FIELDS, parse(check([ask((X, Xl, Y, Z, z_lo, Z if z_hi is None else z_hi, own, 1 << 22, strict, 0, 0, 0, 0))])[0])))
    p = one(512, 512, 512, 512)
    assert (p["form"], p["zchunk"], p["z_blocks"], p["segments"], p["gx"], p["gy"]) == ("march", 64, 8, 8, 2 * 32, 8)
    p = one(256, 256, 256, 256)
    assert (p["form"], p["zchunk"]) == ("march", 8)
    p = one(128, 128, 128, 128)
    assert (p["form"], p["zchunk"]) == ("march", 8)
    p = one(64, 64, 64, 64)
    assert (p["form"], p["zchunk"], p["z_blocks"], p["tiles_x"], p["tiles_y"]) == ("plane", 1, 62, 1, 31)
    for X in (5, 7, 9, 13, 4, 6, 63, 130, 513):       # X % 4 != 0 or X < 8
        assert one(X, X, 64, 64)["form"] == "generic", X
    for X, Xl, Y, Z, z_lo, z_hi in ((8, 2, 9, 9, 0, 9), (8, 8, 2, 9, 0, 9), (8, 8, 9, 2, 0, 2), (64, 64, 64, 64, 30, 30), (64, 64, 64, 64, 40, 30),
                                     (64, 64, 64, 64, 63, 64), (64, 64, 64, 64, 0, 1)):
        assert one(X, Xl, Y, Z, z_lo, z_hi)["status"] == "nothing", (X, Xl, Y, Z, z_lo, z_hi)
    for n in (16, 64, 128, 512, 1024):                # strict: one plane per block, whatever the size
        p = one(n, n, n, n, strict=1)
        assert (p["form"], p["zchunk"], p["z_blocks"], p["gx"]) == ("strict", 1, n - 2, cdiv(n, 64) * cdiv(n, 4)), n


def test_invariants_over_the_grid(planned, check):
    for g, p in planned:
        X, Xl, Y, Z, z_lo, z_hi, own, surv_cap, strict, pair, defer, ntaps, list2_cap = g
        if p["status"] == "nothing":
            continue
        # the z blocks cover [z0, z1) exactly once
        assert (p["z0"], p["z1"]) == (max(z_lo, 1), min(z_hi, Z - 1))
        assert (p["z_blocks"] - 1) * p["zchunk"] < p["z1"] - p["z0"] <= p["z_blocks"] * p["zchunk"], g
        if p["form"] == "generic":
            assert (p["gz"], p["zchunk"]) == (p["z_blocks"], 1)
            continue
        assert p["gy"] == p["z_blocks"] and p["gz"] == 1
        assert 1 <= p["segments"] <= SEGS and p["segments"] * p["seg_cap"] <= surv_cap, g
        assert p["vy"] == p["segments"] and p["vx"] * 256 >= p["seg_cap"], g
        if p["form"] == "march":
            assert (p["zchunk"] + 2) * X * Y * 4 < 2 ** 32 and p["zchunk"] in (8, 16, 32, 64), g
            assert p["tiles_x"] * 256 >= X and p["tiles_y"] * 16 >= Y - 2 and p["gx"] == p["tiles_x"] * p["tiles_y"], g
        elif p["form"] == "plane":
            assert p["tiles_x"] * 248 >= X - 2 and p["tiles_y"] * 2 >= Y - 2 and p["gx"] * 4 >= p["tiles_x"] * p["tiles_y"], g
        else:
            assert p["form"] == "strict" and p["zchunk"] == 1 and p["gx"] == p["tiles_x"] * p["tiles_y"], g
            assert p["tiles_x"] * 64 >= X and p["tiles_y"] * 4 >= Y
        if p["status"] == "ok" and defer:
            assert list2_cap % 8 == 0 and min(64, list2_cap) <= p["lazy_wgs"] <= 4096, g
            assert p["lazy_wgs"] < 8 or p["lazy_wgs"] % 8 == 0, g
            assert p["lazy_wgs"] <= list2_cap and p["list2_seg_cap"] * p["segments"] <= list2_cap, g
        else:
            assert p["lazy_wgs"] == 0
    # the segment function: monotone in the z block and onto [0, segments)
    counts = list(range(1, 200)) + [255, 256, 257, 1022, 4096]
    got = check(["seg %d" % n for n in counts])
    for n, line in zip(counts, got):
        f = [int(v) for v in line.split(" ")[1:]]
        segs, of = f[0], f[1:]
        assert segs == min(n, SEGS) and of == [want_segment(b, n) for b in range(n)]
        assert of == sorted(of) and set(of) == set(range(segs)), n


def test_lazy_shapes(check):
    grid = [(8, 3, 3), (4, 3, 3), (8, 2, 3), (8, 3, 2), (10, 8, 8), (12, 8, 8), (32768, 16384, 8), (32768, 16383, 8), (512, 512, 512)]
    got = check(["lazy %d %d %d" % g for g in grid])
    want = ["lazy %d" % (nx % 4 == 0 and nx >= 8 and ny >= 3 and nz >= 3 and nx * ny < 2 ** 29) for nx, ny, nz in grid]
    assert got == want and "lazy 1" in got and "lazy 0" in got


def test_same_answers_under_the_sanitizers(tmp_path_factory, check):
    """The plan program under AddressSanitizer + UndefinedBehaviorSanitizer, stand-alone, over the same cases: it exits clean
    (any report fails the run: -fno-sanitize-recover) with the same output; one case goes through its command line."""
    san = build(tmp_path_factory.mktemp("extrema_plan_san"), "extrema_plan_check_san",
                ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    lines = [ask(g) for g in plan_grid()] + ["seg %d" % n for n in (1, 63, 64, 65, 4096)] + ["lazy 8 3 3"]
    assert san(lines) == check(lines)
    one = ask((512, 512, 512, 512, 0, 512, 1, 1 << 20, 0, 1, 1, 17, 1 << 20))
    r = subprocess.run([san.exe] + one.split(" "), capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    assert r.stdout.split("\n")[:-1] == check([one])
