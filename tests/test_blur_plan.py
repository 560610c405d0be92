"""CPU suite: the launch plan of the fused blur (3d_sift_cuda_amd/csrc/blur_plan.h).

Every form of blur_fused_ring_kernel gives the same bits, so the bit-exact suites cannot tell which form ran: a wrong branch in
the choice costs only time.  tests/blur_plan_check.cpp prints the plan (form, z chunks, tile order, fused or three passes, shape
inside or not) with the host C++ compiler; here it is held against a restatement of the rules, against the production forms at
512^3 spelled out literally, and against the kernels the object file really holds.
"""
import itertools
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3d_sift_cuda_amd", "csrc")
PAIRS = ((1, 0), (0, 1), (1, 1))                     # level only, DoG only, both


def fmt(R, rows, out, dog, pf, tx, ty, sub, stg):
    b = lambda v: "true" if v else "false"
    return "<%d,%d,%s,%s,%d,%d,%d,%s,%s>" % (R, rows, b(out), b(dog), pf, tx, ty, b(sub), b(stg))


# ---- the rules, restated ------------------------------------------------------------------------------------------------------
def want_form(R, out, dog, X, Y, Z, zo0, zo1, sub, rows_knob, tile, stagger):
    rows = rows_knob if rows_knob in (1, 2) else (1 if R >= 7 or X * Y * (zo1 - zo0) < 2 ** 22 else 2)
    stg = 3 <= R <= 6 and (stagger == 2 or (stagger == 0 and R >= 5))
    both = out and dog
    if R == 5 and sub and rows == 2 and both and zo0 == 0 and zo1 == Z and X % 8 == 0 and Y >= 2 and Z >= 2:
        wide = (tile == 2 or (tile == 0 and stg)) and X >= 128
        return (5, 2, 1, 1, 2) + ((128, 16) if wide else (64, 32)) + (1, stg)
    if rows == 1:
        return (R, 1, out, dog, 1, 64, 32, 0, 0)
    wide = tile == 2 or (tile == 0 and (R == 3 or (R == 4 and both)))
    return (R, 2, out, dog, 3 if R <= 4 and not both else 2) + ((128, 16) if R <= 6 and wide and X >= 128 else (64, 32)) + (0, stg)


def want_chunks(form, X, Y, zo0, zo1, resident, forced, order):
    """None where the 32-bit offsets cannot address a chunk, else (zlen, chunks, tiles_x, tiles_y, workgroups, order)."""
    R, tx, ty, sub = form[0], form[5], form[6], form[7]
    max_planes = 0xFFFFFFF0 // (X * Y * 4) - 2 * R - 2
    if max_planes < 1:
        return None
    tiles_x, tiles_y, Zo = -(-X // tx), -(-Y // ty), zo1 - zo0
    n = forced
    if forced < 1:        # the fewest rounds of resident workgroups (256 CUs) times planes marched, lead-in included
        n, best = 1, None
        for k in range(1, 257):
            zlen = -(-Zo // k)
            if k > 1 and zlen < 4 * R:
                break
            wgs = float(tiles_x * tiles_y) * float(-(-Zo // zlen))
            cost = (1.0 if wgs <= 256.0 * resident else wgs / (256.0 * resident)) * float(zlen + 2 * R)
            if best is None or cost < best:
                n, best = k, cost
    if -(-Zo // n) > max_planes:
        n = -(-Zo // max_planes)
    zlen = -(-Zo // n)
    if sub and zlen % 2:
        zlen += 1
    nch = -(-Zo // zlen)
    if order == 0:
        order = 1
    if order == 3:
        M = tiles_y * nch
        if not (tiles_x % 8 == 0 if tiles_x >= 8 else (8 % tiles_x == 0 and M % (8 // tiles_x) == 0)):
            order = 1
    return (zlen, nch, tiles_x, tiles_y, tiles_x * tiles_y * nch, order)


def want_fused(mode, ntaps, N):
    return mode == 2 or (mode == 1 and (N >= 2 ** 22 or (N >= 2 ** 18 and ntaps <= 9)))


def want_inside(ntaps, X, Y):
    return 3 <= ntaps <= 17 and ntaps % 2 == 1 and X % 4 == 0 and X * Y < 2 ** 29


# ---- the grid -----------------------------------------------------------------------------------------------------------------
# (X, Y, Z, zo0, zo1, resident): both sides of 2^22 voxels, of X = 128 and of X % 8, windows shorter than the volume, tile counts
# that do and do not divide for order 3, one plane / one row, an odd chunk length under the carry, planes large enough for the
# 4 GiB clamp and beyond it
SHAPES = ((128, 128, 256, 0, 256, 1), (128, 128, 255, 0, 255, 2), (120, 160, 256, 0, 256, 1), (124, 160, 256, 0, 256, 1),
          (128, 128, 256, 0, 128, 2), (256, 128, 256, 0, 128, 1), (256, 128, 256, 64, 256, 2), (512, 512, 512, 0, 512, 1),
          (192, 96, 301, 0, 301, 1), (576, 64, 130, 0, 130, 2), (256, 96, 129, 0, 129, 1), (4096, 1, 2048, 0, 2048, 1),
          (2048, 2048, 1, 0, 1, 1), (64, 64, 64, 0, 64, 2), (8192, 4096, 64, 0, 64, 1), (16384, 8192, 8, 0, 8, 1))


def plan_grid():
    for R, (out, dog), rows, tile, stagger, shape, sub, order in itertools.product(
            range(1, 9), PAIRS, (0, 1, 2), (0, 1, 2), (0, 1, 2), SHAPES, (0, 1), (1, 2, 3)):
        yield (R, out, dog) + shape[:5] + (sub, 0, rows, tile, order, stagger, shape[5])
    for R, shape, chunks, order in itertools.product(range(1, 9), SHAPES, (1, 3, 7), (0, 3)):   # forced chunks, order 0
        yield (R, 1, 1) + shape[:5] + (1, chunks, 0, 0, order, 0, shape[5])


FUSE_GRID = [(mode, ntaps, X, Y, Z) for mode in (0, 1, 2) for ntaps in (9, 11)
             for X, Y, Z in ((64, 64, 64), (64, 64, 63), (128, 128, 256), (128, 128, 255), (512, 512, 512), (32, 32, 32))]
INSIDE_GRID = [(ntaps, X, Y) for ntaps in (1, 3, 4, 15, 17, 19) for X, Y in ((64, 64), (66, 64), (65, 64), (32768, 16384), (32768, 16383), (4, 1))]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("blur_plan") / "blur_plan_check")
    r = subprocess.run([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", CSRC, "-o", exe,
                        os.path.join(ROOT, "tests", "blur_plan_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.split("\n")[:-1]
    return run


@pytest.fixture(scope="module")
def planned(check):
    """The plan over the grid, asked once: [(request, form, rest of the answer)]."""
    grid = list(plan_grid())
    got = check(["plan " + " ".join(str(v) for v in g) for g in grid])
    assert len(got) == len(grid)
    return [(g,) + tuple(a.split(" ", 2)[1:]) for g, a in zip(grid, got)]


def test_plan_equals_the_restated_rules(planned):
    bad = []
    for g, form, rest in planned:
        R, out, dog, X, Y, Z, zo0, zo1, sub, chunks, rows, tile, order, stagger, resident = g
        f = want_form(R, out, dog, X, Y, Z, zo0, zo1, sub, rows, tile, stagger)
        c = want_chunks(f, X, Y, zo0, zo1, resident, chunks, order)
        if form != fmt(*f) or rest != ("outside" if c is None else " ".join(str(v) for v in c)):
            bad.append((g, form, rest, fmt(*f), c))
    assert not bad, (len(bad), bad[:5])
    # the grid reaches what it is meant to reach
    rests = [rest for _, _, rest in planned]
    assert "outside" in rests and any(r.endswith(" 3") for r in rests) and any(r.endswith(" 2") for r in rests)
    assert any(g[12] == 3 and rest.endswith(" 1") for g, _, rest in planned)      # order 3 asked, counts do not divide


def test_fused_or_three_passes_and_shape_limits(check):
    got = check(["fuse %d %d %d %d %d" % g for g in FUSE_GRID] + ["inside %d %d %d" % g for g in INSIDE_GRID])
    want = ["fuse %d" % want_fused(m, n, X * Y * Z) for m, n, X, Y, Z in FUSE_GRID] + ["inside %d" % want_inside(*g) for g in INSIDE_GRID]
    assert got == want
    assert "fuse 1" in got and "fuse 0" in got and "inside 1" in got and "inside 0" in got


def test_production_forms_at_512(check):
    """The forms the pyramid's launches take at 512^3 with every knob at 0, literally: the restatement above cannot drift with the
    code unnoticed."""
    def ask(ntaps, out, dog, sub):
        return check(["plan %d %d %d 512 512 512 0 512 %d 0 0 0 0 0 1" % (ntaps // 2, out, dog, sub)])[0].split(" ")[1]
    assert ask(7, 1, 0, 0) == "<3,2,true,false,3,128,16,false,false>"
    assert ask(9, 1, 0, 0) == "<4,2,true,false,3,64,32,false,false>"
    assert ask(9, 1, 1, 0) == "<4,2,true,true,2,128,16,false,false>"
    assert ask(11, 1, 1, 1) == "<5,2,true,true,2,128,16,true,true>"
    assert ask(13, 1, 1, 0) == "<6,2,true,true,2,64,32,false,true>"
    for out, dog in PAIRS:
        assert ask(17, out, dog, 0) == fmt(8, 1, out, dog, 1, 64, 32, 0, 0)


def test_no_dead_kernels(built, check, planned):
    """The forms the plan returns over the grid, the forms the table holds and the kernels in the object file are one set: none
    unreachable, none missing.  Its size is 94: 24 forms of one row per thread (8 filters x 3 output pairs), 66 of two rows (3
    output pairs x [2 tiles for 3 and 5 taps, 2 tiles x 2 staggers for 7 - 13 taps, 1 for 15 and 17 taps]) and 4 that carry the
    half-size volume (11 taps: 2 tiles x 2 staggers).  The launcher before the plan built 130: besides these, three planes of
    prefetch with both arrays stored (12) and two planes with one array stored up to 9 taps (24), which no input reaches."""
    reached = {form for _, form, _ in planned}
    table = [line.split(" ")[1] for line in check(["forms"])]
    assert len(table) == len(set(table))
    assert reached == set(table), (sorted(reached - set(table)), sorted(set(table) - reached))
    nm = subprocess.run(["nm", "-C", os.path.join(CSRC, "_build", "kernels_blur_fused.o")], capture_output=True, text=True)
    assert nm.returncode == 0, nm.stderr
    built_forms = re.findall(r"__device_stub__blur_fused_ring_kernel(<[^>]*>)", nm.stdout)
    assert len(built_forms) == len(set(built_forms))
    assert {f.replace(" ", "") for f in built_forms} == set(table)
    assert len(table) == 94
