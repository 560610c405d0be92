"""CPU suite: the exact distance map and the surface distances between label volumes without a GPU -- the
oracle tests/edt_oracle.c against a numpy restatement, the product's host helpers (edt_host.c) against Python and at their bounds,
the surface rule, a cube pair whose Hausdorff distance is known, the host file under the sanitizers as a stand-alone program, and
the fusion scenario's boundary distances."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from edt_cases import NONE, PATTERNS, SPACINGS, EdtOracle, bits, cube_pair, map_numpy, means, oracle_records, same_record, sites, stats_python
from field_cases import FieldOracle
from fuse_cases import cpu_fuse, fused_labels, leg, scenario
from fuse_search_cases import FuseSearchOracle, fuse_planes, warped_planes
from resample_cases import ResampleOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ed(tmp_path_factory):
    return EdtOracle(tmp_path_factory.mktemp("edt_oracle"))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", [(2, 3, 4), (5, 9, 33)])
def test_oracle_map_equals_numpy(ed, shape, pattern):
    s = sites(shape, pattern)
    for spacing in SPACINGS:
        got, want = ed.map(s, spacing), map_numpy(s, spacing)
        assert got.dtype == np.uint64 and np.array_equal(got, want)
        if pattern == "none":
            assert (got == NONE).all()
        else:
            assert (got[s != 0] == 0).all() and (got < 2 ** 58).all() and ((got == 0) == (s != 0)).all()
    if pattern == "corner":   # the far corner, in Python integers
        nz, ny, nx = shape
        assert int(ed.map(s, (700, 1300, 3000))[0, 0, 0]) == (700 * (nx - 1)) ** 2 + (1300 * (ny - 1)) ** 2 + (3000 * (nz - 1)) ** 2


@pytest.mark.parametrize("n", [1, 2, 19, 20, 21, 100, 101])
def test_surface_stats_equal_python(built, n):
    """the percentile's index (95 n + 99) / 100 - 1 on both sides of its steps (n = 20 -> 18, 21 -> 19, 100 -> 94, 101 -> 95), equal
    elements, the largest distance, an empty direction"""
    rng = np.random.default_rng(n)
    ab = [int(v) for v in rng.integers(0, 10 ** 9, n)]
    ba = [int(v) for v in rng.choice([0, 49000000, 3 * (4095 * 65535) ** 2], n // 2 + 1)]
    for x, y in ((ab, ba), (ba, ab), (ab, ab), ([7] * n, [7])):
        same_record(built.surface_stats(x, y), stats_python(x, y))
    r = built.surface_stats(list(range(1, n + 1)), [4])
    assert r["p95_ab"] == {1: 1, 2: 2, 19: 19, 20: 19, 21: 20, 100: 95, 101: 96}[n] == (95 * n + 99) // 100 and r["max_ab"] == n and r["n_a"] == n and r["n_b"] == 1
    assert r["hausdorff_mm"] == math.sqrt(n) / 1000.0 if n >= 4 else r["hausdorff_mm"] == 0.002
    # a label that one volume lacks: the counts, UINT64_MAX and NaN
    for x, y in ((ab, []), ([], ba), ([], [])):
        r = built.surface_stats(x, y)
        same_record(r, stats_python(x, y))
        assert (r["n_a"], r["n_b"]) == (len(x), len(y)) and all(r[k] == NONE for k in ("max_ab", "max_ba", "p95_ab", "p95_ba"))
        assert all(math.isnan(r[k]) for k in ("sum_ab", "sum_ba", "hausdorff_mm", "hd95_mm", "assd_mm"))


def spacing_python(mm):
    v = float(np.float32(mm) * np.float32(1000.0))
    if not math.isfinite(v) or v < 0:
        return None
    r = math.floor(v + 0.5)   # lroundf: halves away from zero; v + 0.5 is exact in double for a float32 v below 2^17
    return r if 1 <= r <= 65535 else None


def test_spacing_um_at_its_bounds(built):
    assert built.spacing_um(1.0) == 1000 and built.spacing_um(0.001) == 1 and built.spacing_um(65.535) == 65535 and built.spacing_um(0.7) == 700
    for bad in (0.0, 0.0004, -1.0, 65.536, 70.0, 1e30, -1e30, np.nan, np.inf, -np.inf):
        assert built.spacing_um(bad) is None, bad
    rng = np.random.default_rng(1)
    for mm in list(rng.uniform(0.0, 66.0, 2000)) + [0.0005, 0.00049, 0.0015, 65.5354, 65.5356, 2.5005]:
        assert built.spacing_um(mm) == spacing_python(mm), mm
    p = built.surface_params()
    assert (p.first_label, p.max_labels, p.device) == (1, 64, 0)


def test_cube_moved_by_two_voxels_has_a_hausdorff_distance_of_six_millimetres(built, ed):
    a, b = cube_pair()
    spacing = (3000, 700, 1300)
    (r,) = oracle_records(built, ed, a, b, spacing)
    assert r["label"] == 1 and r["voxels_a"] == r["voxels_b"] == 216 and r["n_a"] == r["n_b"] == 216 - 64
    assert r["max_ab"] == r["max_ba"] == 4 * 3000 ** 2 and r["hausdorff_mm"] == 6.0
    assert 0 < r["assd_mm"] < r["hd95_mm"] <= 6.0
    r0, r1 = oracle_records(built, ed, a, b, spacing, first_label=0)
    same_record(r1, r)
    assert r0["label"] == 0 and r0["n_a"] > 0 and r0["hausdorff_mm"] > 0
    # identical volumes: zeros throughout
    (z,) = oracle_records(built, ed, a, a, spacing)
    assert z["max_ab"] == z["max_ba"] == z["p95_ab"] == z["p95_ba"] == 0
    assert all(bits(z[k]) == 0 for k in ("sum_ab", "sum_ba", "hausdorff_mm", "hd95_mm", "assd_mm"))


def test_surface_rule_at_the_border_and_beside_an_unlabelled_voxel(ed):
    lab = np.zeros((7, 7, 7), np.float32)
    lab[0:5, 1:6, 1:6] = 3                         # touches the volume's first z plane
    s = ed.surface(lab, 3)
    assert s[0, 1:6, 1:6].all()                    # the whole plane on the border is surface
    assert s[1:4, 2:5, 2:5].sum() == 0 and s[4, 1:6, 1:6].all() and s[1:4, 1, 1:6].all()
    assert s.sum() == 5 * 25 - 3 * 9 and (s[lab != 3] == 0).all()
    whole = np.full((3, 4, 5), 2, np.float32)      # a label that fills the volume: only the border voxels
    s = ed.surface(whole, 2)
    assert s.sum() == 60 - 1 * 2 * 3 and s[1, 1:3, 1:4].sum() == 0
    for hole in (np.nan, np.inf, -np.inf, 5.0):    # an interior voxel that does not carry the label makes its six neighbours surface
        lab = np.full((7, 7, 7), 4, np.float32)
        lab[3, 3, 3] = hole
        s = ed.surface(lab, 4)
        inner = s[1:6, 1:6, 1:6]
        assert inner.sum() == 6 and s[3, 3, 3] == 0 and s[2, 3, 3] == s[4, 3, 3] == s[3, 2, 3] == s[3, 4, 3] == s[3, 3, 2] == s[3, 3, 4] == 1
    assert ed.surface(lab, 9).sum() == 0


def test_host_file_under_sanitizers(built, tmp_path):
    """edt_host.c and tests/edt_host_san.c as one program, with and without -fsanitize=address,undefined: both exit clean and print
    the same lines, and those are the restatement's"""
    src = [os.path.join(ROOT, "tests", "edt_host_san.c"), os.path.join(ROOT, "3d_sift_cuda_amd", "csrc", "edt_host.c")]
    base = ["cc", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-ffp-contract=off", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include")]
    out = {}
    for name, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])):
        exe = str(tmp_path / ("edt_host_" + name))
        subprocess.run(base + flags + ["-o", exe] + src + ["-lm"], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
        out[name] = r.stdout
    text = out["san"]
    assert text == out["plain"] and "defaults 1 64 0\n" in text and "spacing null -1\n" in text
    mm = [1.0, 0.001, 0.0004, 0.0005, 65.535, 65.536, 70.0, 0.0, -1.0, 0.7, 1e30, -1e30, np.nan, np.inf, -np.inf]
    for c, v in enumerate(mm):
        um = spacing_python(v)
        assert "spacing %d %d %d\n" % (c, -1 if um is None else 0, um or 0) in text, (c, v)
    for n in (1, 2, 19, 20, 21, 100, 101):
        ab = [(n - i) ** 2 * 1000000 for i in range(n)]
        ba = [3 * (4095 * 65535) ** 2 if i % 3 == 0 else 49000000 for i in range(n // 2 + 1)]
        w = stats_python(ab, ba)
        line = "stats %d %d %d %d %d %d %d " % (n, w["n_a"], w["n_b"], w["max_ab"], w["max_ba"], w["p95_ab"], w["p95_ba"])
        line += " ".join("%016x" % bits(w[k]) for k in ("sum_ab", "sum_ba", "hausdorff_mm", "hd95_mm", "assd_mm"))
        assert line + "\n" in text, line
    nan = "%016x" % bits(stats_python([], [1])["assd_mm"])
    assert re.search(r"^stats absent_both 0 0 %d %d %d %d %s %s %s %s %s$" % ((NONE,) * 4 + (nan,) * 5), text, re.M)
    assert len(re.findall(r"^stats absent_b \d+ 0 %d " % NONE, text, re.M)) == 7 and len(re.findall(r"^stats absent_a 0 \d+ %d " % NONE, text, re.M)) == 7


# The scenario's mean HD95 and ASSD in mm over the labels 1 .. 4 (fused against the truth, 1 mm voxels) on the oracle when this was
# written; DESIGN.md section 7l has the table.  Keys: majority voting, power 2, power 2 with a search radius of 2.
SCENARIO_MM = {"p0": (1.1036, 0.3031), "p2": (1.0000, 0.2038), "s2": (1.0000, 0.1319)}


def test_scenario_boundary_distances_follow_the_dice(built, ed, tmp_path_factory):
    """fuse_cases.scenario under SSD: the boundary distances of the fused labels to the truth for majority voting, weighted voting
    (power 2) and weighted voting with -s2.  Asserted, by section 7j's rule: each step lowers the mean HD95 and the mean ASSD by at
    least half the gap measured on the oracle when this was written (SCENARIO_MM), wherever the oracle showed a gap at all."""
    fs = FuseSearchOracle(tmp_path_factory.mktemp("fuse_search_oracle"))
    ro = ResampleOracle(tmp_path_factory.mktemp("resample_oracle"))
    fo = FieldOracle(tmp_path_factory.mktemp("field_oracle"))
    scen = scenario(built, ro, tmp_path_factory.mktemp("fuse_scenario"))
    atlases = leg(scen, "ssd")
    rt, qt, planes = warped_planes(built, fs, ro, fo, scen["target"], atlases, scen["vox2key"], "ssd")
    words = {"p0": cpu_fuse(built, fs, ro, fo, scen["target"], atlases, scen["vox2key"], metric="ssd", power=0)[0],
             "p2": fuse_planes(fs, rt, qt, planes, 2, "ssd", 2, 0)[0], "s2": fuse_planes(fs, rt, qt, planes, 2, "ssd", 2, 2)[0]}
    got = {}
    for key, w in words.items():
        rec = oracle_records(built, ed, fused_labels(w), scen["truth"], (1000, 1000, 1000))
        assert [r["label"] for r in rec] == [1, 2, 3, 4] and all(r["n_a"] > 0 and r["n_b"] > 0 for r in rec)
        hd, hd95, assd, _ = means(rec)
        got[key] = (hd95, assd)
        print("edt scenario %s: mean hausdorff %.4f hd95 %.4f assd %.4f mm" % (key, hd, hd95, assd))
    for c, name in enumerate(("hd95", "assd")):
        assert all(abs(got[k][c] - SCENARIO_MM[k][c]) < 5e-4 for k in got), (name, got, SCENARIO_MM)   # the record is this oracle's
        for worse, better in (("p0", "p2"), ("p2", "s2")):
            gap = SCENARIO_MM[worse][c] - SCENARIO_MM[better][c]
            if gap > 0:
                assert got[better][c] <= got[worse][c] - 0.5 * gap, (name, worse, better, got)
