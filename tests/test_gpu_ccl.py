"""GPU suite: the connected components and the island removal against the CPU oracle tests/ccl_oracle.c, word
for word and field for field, always through the C-ABI: sift3d_label_components on every shape and pattern under both
connectivities, sift3d_clean_labels on the planted cases and the random patterns, their refusals, and featClean end to end.  No
comparison has a tolerance."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from _helpers import run
from ccl_cases import BX, BY, BZ, PATTERNS, RECORD, CclOracle, corner_pair, pattern, planted, same_bits, same_records
from edt_cases import EdtOracle, distance_block, oracle_records
from fuse_cases import fused_labels, leg, scenario
from resample_cases import ResampleOracle

pytestmark = pytest.mark.gpu

# kernels_ccl.hip: every launch has at most CCL_MAX_BLOCKS = 2048 workgroups of 256 threads; the brick pass takes a brick of
# 32 x 8 x 4 voxels per workgroup, the other kernels a voxel or a component per thread.  BIG has more voxels (780000) than
# 2048 x 256 = 524288, so every kernel over voxels goes round its grid loop; its checkerboard has as many components as voxels, so the
# kernels over components do too.  BRICKS has 2 x 76 x 15 = 2280 bricks, so the brick pass does.
BIG = (13, 300, 200)
BRICKS = (60, 602, 40)
# (nz, ny, nx): one voxel; smaller than a brick; odd extents; several bricks each way; one voxel past the brick on each axis in turn;
# lines and sheets along each axis
SHAPES = [(1, 1, 1), (2, 3, 4), (5, 9, 33), (11, 19, 70), (3, 5, BX + 1), (3, BY + 1, 5), (BZ + 1, 3, 5), (1, 1, 300), (1, 300, 1), (300, 1, 1), BIG]


@pytest.fixture(scope="module")
def oc(tmp_path_factory):
    return CclOracle(tmp_path_factory.mktemp("ccl_oracle"))


def same_report(got, want):
    assert {k: got[k] for k in ("rounds_run", "rounds", "total")} == want, (got, want)


# ---- sift3d_label_components -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES)
def test_components_equal_the_oracle(built, oc, shape, name):
    v = pattern(shape, name)
    for conn in (6, 26):
        comp, rec = built.label_components(v, conn)
        want_comp, want_rec = oc.label(v, conn)
        assert comp.dtype == np.uint32 and comp.shape == v.shape and rec.dtype == RECORD
        assert np.array_equal(comp, want_comp), (conn, int((comp != want_comp).sum()))
        same_records(rec, want_rec)
        if name == "nan":
            assert len(rec) == 0 and not comp.any()
        if name == "one":
            assert len(rec) == 1 and rec["voxels"][0] == v.size and (comp == 1).all()
        if name == "checker" and min(shape) > 1:
            assert len(rec) == (v.size if conn == 6 else 2)


def test_brick_pass_goes_round_its_grid_loop(built, oc):
    """more bricks than the brick pass has workgroups: all one label (one component across every brick) and the serpentine"""
    for name in ("one", "serpentine", "random5"):
        v = pattern(BRICKS, name)
        for conn in (6, 26):
            comp, rec = built.label_components(v, conn)
            want_comp, want_rec = oc.label(v, conn)
            assert np.array_equal(comp, want_comp), (name, conn)
            same_records(rec, want_rec)


def test_corner_pair_across_a_brick_corner(built, oc):
    """label 5 at (31, 7, 3) and (32, 8, 4), eight bricks meeting there: one component under 26, two under 6"""
    v = corner_pair((11, 19, 70))
    assert v[BZ - 1, BY - 1, BX - 1] == 5 and v[BZ, BY, BX] == 5 and (v == 5).sum() == 2
    for conn, n in ((6, 3), (26, 2)):
        comp, rec = built.label_components(v, conn)
        assert len(rec) == n and (comp[BZ - 1, BY - 1, BX - 1] == comp[BZ, BY, BX]) == (conn == 26)
        same_records(rec, oc.label(v, conn)[1])


def test_components_report_their_times(built):
    comp, rec, ms = built.label_components(pattern((11, 19, 70), "blocky"), 6, return_ms=True)
    assert len(ms) == built.CCL_STAGES and all(np.isfinite(t) and t >= 0 for t in ms)   # reported, never judged


# ---- sift3d_clean_labels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(planted()))
def test_planted_cases_equal_the_oracle(built, oc, name):
    v, kw = planted()[name]
    out, rep = built.clean_labels(v, **kw)
    want, want_rep = oc.clean(v, **kw)
    same_bits(out, want)
    same_report(rep, want_rep)


@pytest.mark.parametrize("min_voxels", [1, 2, 8, 1000])
@pytest.mark.parametrize("name", ["random2", "random5", "blocky"])
def test_random_patterns_equal_the_oracle(built, oc, name, min_voxels):
    v = pattern((11, 19, 70), name)
    for conn in (6, 26):
        for rounds in (1, 4):
            out, rep = built.clean_labels(v, min_voxels=min_voxels, connectivity=conn, rounds=rounds)
            want, want_rep = oc.clean(v, min_voxels, conn, rounds)
            same_bits(out, want)
            same_report(rep, want_rep)
            if min_voxels == 1:
                same_bits(out, v)
                assert rep["rounds_run"] == 1 and rep["total"]["small"] == 0


def test_cleaning_goes_round_its_grid_loops(built, oc):
    """BIG: its checkerboard at 2 has 780000 small components (nobody votes); its five random labels at 8 resolve thousands"""
    for name, min_voxels in (("checker", 2), ("random5", 8)):
        v = pattern(BIG, name)
        out, rep, ms = built.clean_labels(v, min_voxels=min_voxels, return_ms=True)
        want, want_rep = oc.clean(v, min_voxels)
        same_bits(out, want)
        same_report(rep, want_rep)
        assert np.isfinite(ms) and ms >= 0
    assert want_rep["total"]["resolved"] > 1000


def test_nothing_is_kept_at_the_largest_minimum(built, oc):
    v = pattern((11, 19, 70), "one")
    out, rep = built.clean_labels(v, min_voxels=1 << 24)
    same_bits(out, v)
    same_report(rep, oc.clean(v, 1 << 24)[1])
    assert rep["rounds_run"] == 1 and rep["rounds"][0] == {"components": 1, "small": 1, "resolved": 0, "resolved_voxels": 0, "unresolved": 1,
                                                           "unresolved_voxels": v.size}


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(built):
    """all but the label and the room for records on the host, before anything is allocated: those extents are never backed by memory"""
    L = built.hip_lib()
    tiny, out, comp = np.ones(8, np.float32), np.zeros(8, np.float32), np.zeros(8, np.uint32)

    def label(nx, ny, nz, conn, vol=tiny, rec=None, room=0):
        err, n = C.create_string_buffer(512), C.c_int64(-1)
        rc = L.sift3d_label_components(0, vol.ctypes.data, nx, ny, nz, conn, comp.ctypes.data, None if rec is None else rec.ctypes.data, room, C.byref(n), None, err,
                                       len(err))
        return rc, err.value.decode(), n.value

    def clean(nx, ny, nz, vol=tiny, **kw):
        err, p = C.create_string_buffer(512), built.clean_params(**kw)
        rc = L.sift3d_clean_labels(vol.ctypes.data, nx, ny, nz, C.byref(p), out.ctypes.data, None, None, err, len(err))
        return rc, err.value.decode()

    for args, text in (((2, 2, 2, 18), "connectivity = 18: 6 or 26"), ((4097, 2, 2, 6), "nx = 4097: an extent must be 1 .. 4096"), ((2, 0, 2, 6), "ny = 0"),
                       ((2, 2, 4097, 26), "nz = 4097"), ((4096, 4096, 65, 6), "nx ny nz = %d: more than 2^30 voxels" % (4096 * 4096 * 65))):
        rc, err, n = label(*args)
        assert rc != 0 and text in err and n == 0, (args, rc, err)
    for args, kw, text in (((2, 2, 2), {"connectivity": 18}, "connectivity = 18: 6 or 26"), ((2, 2, 2), {"min_voxels": 0}, "min_voxels = 0: 1 .. 16777216"),
                           ((2, 2, 2), {"min_voxels": (1 << 24) + 1}, "min_voxels = 16777217: 1 .. 16777216"), ((2, 2, 2), {"rounds": 0}, "rounds = 0: 1 .. 16"),
                           ((2, 2, 2), {"rounds": 17}, "rounds = 17: 1 .. 16"), ((2, 4097, 2), {}, "ny = 4097"),
                           ((4096, 4096, 65), {}, "more than 2^30 voxels")):
        rc, err = clean(*args, **kw)
        assert rc != 0 and text in err, (args, kw, rc, err)
    bad = tiny.copy()
    bad[5] = 0.5
    assert "the label 0.5 at voxel 5 is neither non-finite nor an integer 0 .. 65535" in label(2, 2, 2, 6, vol=bad)[1]
    assert "the label 0.5 at voxel 5 is neither non-finite nor an integer 0 .. 65535" in clean(2, 2, 2, vol=bad)[1]
    with pytest.raises(built.Sift3DError, match=r"the label 0\.5 at voxel 5 "):
        built.clean_labels(bad.reshape(2, 2, 2))
    # too little room for the records: the count and the map all the same, and no record
    v = pattern((5, 9, 33), "blocky")
    want = built.label_components(v, 6)
    rec = np.full(len(want[1]) - 1, 77, RECORD)
    comp = np.zeros(v.shape, np.uint32)
    rc, err, n = label(33, 9, 5, 6, vol=np.ascontiguousarray(v), rec=rec, room=len(rec))
    assert rc != 0 and n == len(want[1]) and ("%d components: more than max_records = %d" % (n, n - 1)) in err
    assert np.array_equal(comp, want[0]) and (rec["voxels"] == 77).all() and (rec["label"] == 77).all()
    with pytest.raises(built.Sift3DError, match="more than max_records = 3") as e:
        built.label_components(v, 6, max_records=3)
    assert e.value.n_components == n and np.array_equal(e.value.comp, want[0])
    rc, err, n2 = label(33, 9, 5, 6, vol=np.ascontiguousarray(v), rec=np.zeros(n, RECORD), room=n)
    assert rc == 0 and n2 == n and err == ""


# ---- featClean -------------------------------------------------------------------------------------------------------------------------
def dice_block(built, a, b):
    """the Dice table as featFuse -t and featOverlap write it"""
    labels, ca, cb, cc = built.label_overlap(a, b)
    dice = [2 * int(c) / (int(x) + int(y)) for x, y, c in zip(ca, cb, cc)]
    t = "# label fused truth both dice\n" + "".join("%d\t%d\t%d\t%d\t%.6f\n" % (l, x, y, c, d) for l, x, y, c, d in zip(labels, ca, cb, cc, dice))
    return t + "# mean dice %.6f over %d labels\n" % (sum(dice) / len(dice), len(dice))


def report_text(rep):
    """sift3d_clean_report_text restated on a report dict"""
    row = lambda head, r: head + "".join("\t%d" % r[k] for k in ("components", "small", "resolved", "resolved_voxels", "unresolved", "unresolved_voxels")) + "\n"
    t = "# round components small resolved resolved_voxels unresolved unresolved_voxels\n"
    t += "".join(row(str(c + 1), r) for c, r in enumerate(rep["rounds"]))
    return t + row("# total", rep["total"]) + "# rounds run %d\n" % rep["rounds_run"]


def components_block(oc, before, after, conn):
    rb, ra = oc.label(before, conn)[1], oc.label(after, conn)[1]
    t = "# label components_before components_after\n"
    for l in sorted(set(rb["label"]) | set(ra["label"])):
        t += "%d\t%d\t%d\n" % (l, (rb["label"] == l).sum(), (ra["label"] == l).sum())
    return t + "# components %d before %d after\n" % (len(rb), len(ra))


def test_featclean_on_the_scenario(built, oc, tmp_path_factory, tmp_path):
    """the scenario's fused labels (power 2) through featClean: the oracle's output, the report it implies, and with -t -m the two
    blocks that featOverlap -m writes for the same pairs"""
    assert os.path.exists(built.FEATCLEAN)
    ed = EdtOracle(tmp_path_factory.mktemp("edt_oracle"))
    scen = scenario(built, ResampleOracle(tmp_path_factory.mktemp("resample_oracle")), tmp_path_factory.mktemp("fuse_scenario"))
    words, _ = built.fuse_labels(scen["target"], leg(scen, "ssd"), scen["vox2key"], metric="ssd", power=2)
    fused, truth = fused_labels(words), scen["truth"]
    built.write_nifti(str(tmp_path / "fused.nii"), fused)
    built.write_nifti(str(tmp_path / "truth.nii"), truth)
    spacing = (1000, 1000, 1000)
    for options, kw in (([], {}), (["-v4", "-c26", "-r2"], {"min_voxels": 4, "connectivity": 26, "rounds": 2})):
        want, want_rep = oc.clean(fused, **kw)
        p = built.clean_params(**kw)
        head = "# featClean min_voxels %d connectivity %d rounds %d\n" % (p.min_voxels, p.connectivity, p.rounds)
        head += report_text(want_rep) + components_block(oc, fused, want, p.connectivity)
        run(["timeout", "-k", "10", "120", built.FEATCLEAN, "-d0"] + options + ["fused.nii", "out.nii"], tmp_path)
        out, _ = built.read_nifti(str(tmp_path / "out.nii"))
        same_bits(np.ascontiguousarray(out, np.float32), want)
        assert open(str(tmp_path / "out.nii.clean.txt")).read() == head
        assert want_rep["total"]["resolved"] > 0      # the case is not an empty one
        if options:                                   # the truth's blocks do not depend on the options: once, with the defaults
            continue
        blocks = ["# %s against the truth\n" % name + dice_block(built, vol, truth) for name, vol in (("input", fused), ("output", want))]
        run(["timeout", "-k", "10", "120", built.FEATCLEAN, "-d0", "-t", "truth.nii"] + options + ["fused.nii", "out_t.nii"], tmp_path)
        assert open(str(tmp_path / "out_t.nii.clean.txt")).read() == head + blocks[0] + blocks[1]
        dist = [distance_block(oracle_records(built, ed, vol, truth, spacing), spacing) for vol in (fused, want)]
        run(["timeout", "-k", "10", "120", built.FEATCLEAN, "-d0", "-t", "truth.nii", "-m"] + options + ["fused.nii", "out_m.nii"], tmp_path)
        assert open(str(tmp_path / "out_m.nii.clean.txt")).read() == head + blocks[0] + dist[0] + blocks[1] + dist[1]
        for name in ("out_t.nii", "out_m.nii"):
            assert open(str(tmp_path / name), "rb").read() == open(str(tmp_path / "out.nii"), "rb").read()
    # errors with text: usage, another grid, another voxel size, a voxel that is no label, a missing file
    built.write_nifti(str(tmp_path / "short.nii"), truth[:, :, :-1])
    built.write_nifti(str(tmp_path / "wide.nii"), truth, voxel=(1.0, 1.5, 1.0))
    bad = fused.copy()
    bad[0, 0, 0] = 0.5
    built.write_nifti(str(tmp_path / "bad.nii"), bad)
    for argv, text in ((["fused.nii"], "Usage: featClean"), (["-x", "fused.nii", "o.nii"], "Usage: featClean"), (["-v0", "fused.nii", "o.nii"], "bad minimum of voxels: -v0"),
                       (["-v16777217", "fused.nii", "o.nii"], "bad minimum of voxels"), (["-c18", "fused.nii", "o.nii"], "bad connectivity: -c18"),
                       (["-r0", "fused.nii", "o.nii"], "bad number of rounds: -r0"), (["-r17", "fused.nii", "o.nii"], "bad number of rounds"),
                       (["-m", "fused.nii", "o.nii"], "-m without -t"), (["-t", "short.nii", "fused.nii", "o.nii"], "not on one grid: 40 x 40 x 40 voxels against 39 x 40 x 40"),
                       (["-t", "wide.nii", "-m", "fused.nii", "o.nii"], "not on one grid: voxels of 1000 x 1000 x 1000 um against 1000 x 1500 x 1000 um"),
                       (["bad.nii", "o.nii"], "the label 0.5 at voxel 0 is neither non-finite nor an integer 0 .. 65535: bad.nii"),
                       (["missing.nii", "o.nii"], "could not read input file: missing.nii")):
        r = subprocess.run(["timeout", "-k", "10", "60", built.FEATCLEAN] + argv, cwd=tmp_path, capture_output=True, text=True)
        assert r.returncode == 255 and text in r.stdout, (argv, r.returncode, r.stdout[-500:])
        assert not os.path.exists(str(tmp_path / "o.nii"))
