"""CPU suite: the ledger of built blur kernels against the cases of tests/blur_cases.py ("Blur ledger").

tests/test_blur_plan.py proves every form of blur_fused_ring_kernel reachable; nothing there says a test runs it.  Here every case
of the table is put through the launch plan (tests/blur_plan_check.cpp) and through a restatement of the three-pass dispatch, and
the kernels reached are held against the kernels built: the 94 forms of the plan's table, and the blur_x_kernel / blur_col_kernel
instantiations `nm -C` finds in kernels_volume.o.  Each kernel is listed with the cases that reach it, so an orphaned one is named.
tests/test_gpu_blur_ledger.py then runs every case against the oracle.  The floors of that file's pipeline cases are held here too.
"""
import collections
import os
import re
import subprocess

import pytest

import blur_cases as bc
import pyramid_cases as pc
from test_blur_plan import CSRC, check  # noqa: F401  (check: the fixture that builds and runs blur_plan_check)

FAST_MAX_R = 8   # SIFT3D_FAST_MAX_R: the templated kernels take 3 .. 17 taps

PIPELINE_FLOOR = 20   # candidates each pipeline case of the GPU file must have, by the oracle alone


def ntaps_of(oracle, case):
    return len(oracle.taps(case.sigma))


# ---- fused ----------------------------------------------------------------------------------------------------------------------
def plan_line(case, ntaps):
    """the request blur_dev's fused launch makes of the plan: `sub` only where the half entry offers the half-size volume"""
    out, dog = bc.OUTPUTS[case.entry]
    nx, ny, nz = case.dims
    k = case.knobs
    sub = 1 if case.entry == bc.HALF and k.get("FUSED_SUB", 1) == 1 and nx % 8 == 0 else 0
    return "plan %d %d %d %d %d %d 0 %d %d %d %d %d 0 %d 1" % (ntaps // 2, out, dog, nx, ny, nz, nz, sub, k.get("FUSED_CHUNKS", 0),
                                                              k.get("FUSED_ROWS", 0), k.get("FUSED_TILE", 0), k.get("FUSED_STAGGER", 0))


@pytest.fixture(scope="module")
def fused_ledger(check, oracle):  # noqa: F811
    """{form: [cases that run it]} over the cases whose fused expectation holds, and the plan's own table of forms"""
    taps = [ntaps_of(oracle, c) for c in bc.CASES]
    takes = check(["fuse %d %d %d %d %d" % ((c.knobs.get("BLUR_FUSED", 1), n) + c.dims) for c, n in zip(bc.CASES, taps)])
    inside = check(["inside %d %d %d" % (n, c.dims[0], c.dims[1]) for c, n in zip(bc.CASES, taps)])
    wrong = [bc.describe(c) for c, t, i in zip(bc.CASES, takes, inside) if c.fused != (t == "fuse 1" and i == "inside 1")]
    assert not wrong, "cases whose fused / three-pass expectation the plan does not share: %s" % wrong
    fused = [(c, n) for c, n in zip(bc.CASES, taps) if c.fused]
    ledger = collections.defaultdict(list)
    for (c, n), answer in zip(fused, check([plan_line(c, n) for c, n in fused])):
        _, form, rest = answer.split(" ", 2)
        assert rest != "outside", bc.describe(c)
        if "FUSED_CHUNKS" in c.knobs:
            assert int(rest.split(" ")[1]) == c.knobs["FUSED_CHUNKS"], (bc.describe(c), rest)
        ledger[form].append(c)
    table = [line.split(" ")[1] for line in check(["forms"])]
    return ledger, table


def orphans(ledger, built_kernels):
    return sorted(k for k in built_kernels if not ledger.get(k))


def test_every_fused_form_has_a_case(fused_ledger):
    ledger, table = fused_ledger
    assert len(table) == len(set(table)) == 94
    assert not orphans(ledger, table), "fused forms no case of tests/blur_cases.py runs: %s" % orphans(ledger, table)
    assert set(ledger) == set(table), "forms outside the table: %s" % sorted(set(ledger) - set(table))
    # the block the table is built around reaches all of them by itself; the rest (thin volume, forced chunks, the default
    # knobs, non-finite input) adds cases, not forms
    forced = set(bc.CASES[:bc.N_FORCED_FUSED])
    assert len(forced) == bc.N_FORCED_FUSED == 196 and all(c.knobs.get("BLUR_FUSED") == 2 for c in forced)
    assert {f for f, cs in ledger.items() if forced & set(cs)} == set(table)
    # the nine 3-tap forms that no case ran before this table: each also on the thin volume and with three z chunks
    three_tap = [f for f in table if f.startswith("<1,")]
    assert len(three_tap) == 9
    for f in three_tap:
        assert any(c.dims in bc.THIN_OF_TILE.values() for c in ledger[f]) and any(c.knobs.get("FUSED_CHUNKS") == 3 for c in ledger[f]), f
    # and what a caller gets with every knob untouched at 2^18 voxels
    assert [c.dims for c in ledger["<1,1,true,false,1,64,32,false,false>"] if not c.knobs] == [bc.DEFAULT_FUSED]
    assert bc.DEFAULT_FUSED[0] * bc.DEFAULT_FUSED[1] * bc.DEFAULT_FUSED[2] == 2 ** 18


def test_the_carry_cases_are_the_four_forms_with_the_half_size_volume(fused_ledger):
    ledger, table = fused_ledger
    carry = [f for f in table if f.endswith(",true,true>") or f.endswith(",true,false>")]
    assert len(carry) == 4
    for f in carry:
        assert [c.entry for c in ledger[f]] == [bc.HALF], f


# ---- three passes ---------------------------------------------------------------------------------------------------------------
def three_pass_kernels(case, ntaps):
    """The dispatch of kernels_volume.hip restated, for a blur that takes three passes with a filter of 3 .. 17 taps:
    R = ntaps / 2 (sift3d_launch_blur_x / _y / _z: lines 395, 452, 470); the x pass is blur_x_kernel<R, VEC> with VEC = 4 iff
    X % 4 == 0 (dispatch_x, line 367); the y pass blur_col_kernel<R, VEC, false, FULL> with the same VEC (line 455) along Y; the z
    pass blur_col_kernel<R, VEC, DOG, FULL> with VEC = 4 iff X * Y % 4 == 0 (line 474) and DOG iff a DoG is asked for (lines 476,
    482) along Z; FULL iff the axis holds the smallest full chunk, 2 * U - 2 * R = 2 * R + 2 rows (chunk_len, lines 408 - 427, and
    launch_col, lines 435 - 446)."""
    R = ntaps // 2
    nx, ny, nz = case.dims
    b = lambda v: "true" if v else "false"
    vx, vz = (4 if nx % 4 == 0 else 1), (4 if nx * ny % 4 == 0 else 1)
    return ("blur_x_kernel<%d, %d>" % (R, vx),
            "blur_col_kernel<%d, %d, false, %s>" % (R, vx, b(ny >= 2 * R + 2)),
            "blur_col_kernel<%d, %d, %s, %s>" % (R, vz, b(bc.OUTPUTS[case.entry][1]), b(nz >= 2 * R + 2)))


@pytest.fixture(scope="module")
def three_pass_ledger(oracle):
    ledger = collections.defaultdict(list)
    for c in bc.CASES:
        n = ntaps_of(oracle, c)
        if not c.fused and 1 <= n // 2 <= FAST_MAX_R:
            for k in three_pass_kernels(c, n):
                ledger[k].append(c)
    return ledger


def test_every_three_pass_kernel_has_a_case(built, three_pass_ledger):
    nm = subprocess.run(["nm", "-C", os.path.join(CSRC, "_build", "kernels_volume.o")], capture_output=True, text=True)
    assert nm.returncode == 0, nm.stderr
    stubs = re.findall(r"__device_stub__(blur_(?:x|col)_kernel<[^>]*>)", nm.stdout)
    assert len(stubs) == len(set(stubs))
    assert sum(s.startswith("blur_x_kernel") for s in stubs) == 16 and sum(s.startswith("blur_col_kernel") for s in stubs) == 64
    assert not orphans(three_pass_ledger, stubs), "three-pass kernels no case of tests/blur_cases.py runs: %s" % orphans(three_pass_ledger, stubs)
    assert set(three_pass_ledger) == set(stubs), "kernels the object file does not hold: %s" % sorted(set(three_pass_ledger) - set(stubs))


def test_wider_filters_take_the_generic_kernel_with_and_without_a_level(oracle):
    """more than 17 taps are outside the templates: the table asks them of the generic kernel, through its DoG branch; no case
    has one tap (tests/blur_cases.py says why)"""
    seen = collections.defaultdict(set)
    for c in bc.CASES:
        n = ntaps_of(oracle, c)
        assert n >= 3 and (c.family == "generic") == (n > 2 * FAST_MAX_R + 1), bc.describe(c)
        if c.family == "generic":
            assert not c.fused and not c.knobs
            seen[c.sigma].add(bc.OUTPUTS[c.entry])
    assert set(seen) == set(bc.GENERIC_SIGMAS)
    assert all((True, True) in v and (False, True) in v for v in seen.values())


# ---- the table itself -----------------------------------------------------------------------------------------------------------
def test_the_table_is_what_it_says(oracle):
    assert len(set(bc.CASES)) == len(bc.CASES)
    for R, sigma in bc.SIGMA_OF_R.items():
        assert len(oracle.taps(sigma)) == 2 * R + 1, (R, sigma)
    for c in bc.CASES:
        nx, ny, nz = c.dims
        assert c.family in bc.FAMILIES and c.entry in bc.OUTPUTS and nz >= 2
        assert c.fused or not c.knobs                             # three passes: default knobs ...
        assert c.fused or nx * ny * nz < 2 ** 18                  # ... and below the size where a narrow filter takes the fused launch
        assert c.family.startswith("fused") == c.fused
    # every family has exactly one case that runs again on non-finite input
    again = [c for c in bc.CASES if c.nonfinite]
    assert sorted(c.family for c in again) == sorted(bc.FAMILIES)
    assert all(c._replace(nonfinite=False) in bc.CASES for c in again)
    # the input: the planted row, and nothing non-finite unless asked for
    import numpy as np
    for dims in {c.dims for c in bc.CASES}:
        v = bc.volume(dims)
        assert v.shape == dims[::-1] and v.dtype == np.float32 and np.isfinite(v).all() and not v.flags.writeable
        assert v[0, 0, :8].tobytes() == np.array(bc.EXTREMES, np.float32).tobytes() and np.signbit(v[0, 0, 1])
    v = bc.volume((20, 20, 20), nonfinite=True)
    assert np.isnan(v).sum() == 2 and np.isposinf(v).sum() == 1 and np.isneginf(v).sum() == 1


def test_one_tap_is_a_filter_in_the_oracle(oracle):
    """What the one-tap filter is in the oracle, as in the reference: out = 0 + 1 * v turns -0.0 into +0.0, and in - out is -0.0
    there and NaN at NaN and +-inf voxels -- neither a copy nor a zero volume.  The library still copies and clears (blur_dev);
    tests/blur_cases.py says why no GPU case holds it to this yet."""
    import numpy as np
    vol = bc.volume((20, 20, 20), nonfinite=True)
    for sigma in bc.ONE_TAP_SIGMAS:
        assert len(oracle.taps(sigma)) == 1
        out = oracle.blur(vol, sigma)
        dog = oracle.dog(vol, out)
        assert np.signbit(vol[0, 0, 1]) and out[0, 0, 1] == 0 and not np.signbit(out[0, 0, 1])
        assert dog[0, 0, 1] == 0 and np.signbit(dog[0, 0, 1])
        for zyx, _ in bc.nonfinite_voxels((20, 20, 20)):
            assert np.isnan(dog[zyx])
        fin = np.isfinite(vol) & (vol != 0)
        assert (pc.bits(out)[fin] == pc.bits(vol)[fin]).all() and np.isnan(dog).sum() == 4 and (dog[fin] == 0).all()


# ---- the pipeline cases of the GPU file ------------------------------------------------------------------------------------------
def test_pipeline_cases_start_with_three_taps_and_have_candidates(built, oracle):
    assert len(oracle.taps(pc.initial_sigma(bc.PIPELINE_SCALE))) == 3
    for dims, seed in bc.PIPELINE_CASES:
        n = len(oracle.candidates(built.synth_blobs(*dims, seed=seed), init_scale=bc.PIPELINE_SCALE))
        assert n >= PIPELINE_FLOOR, (dims, seed, n)
    (d0, _), (d1, _) = bc.PIPELINE_CASES
    assert d0[0] * d0[1] * d0[2] == 2 ** 18 and d0[0] % 4 == 0       # the first blur takes the fused launch ...
    assert d1[0] * d1[1] * d1[2] < 2 ** 18 and d1[0] % 4 != 0        # ... or three passes, on rows padded to whole vectors
