"""GPU suite: the guided re-matching of DESIGN.md section 7d -- sift3d_guided_search against the brute-force CPU oracle
tests/refine_oracle.c bit for bit, sift3d_refine_similarity against the loop restated in tests/refine_cases.py (oracle search,
the product's host fit), featMatchMultiple -a -e's files, and the 20-degree end-to-end case with the refined transform."""
import subprocess

import numpy as np
import pytest

from _helpers import extract, run as _run
from align_cases import LINE, AlignOracle, random_records, random_rotation
from refine_cases import (RefineOracle, cpu_refine, interval, noisy_case, scenario_cpu, scenario_map, scenario_score,
                          scenario_volumes)
from resample_cases import ResampleOracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def aorc(tmp_path_factory):
    return AlignOracle(tmp_path_factory.mktemp("align_oracle"))


@pytest.fixture(scope="module")
def rorc(tmp_path_factory):
    return RefineOracle(tmp_path_factory.mktemp("refine_oracle"))


def _transform(seed, box=60.0):
    rng = np.random.default_rng(seed + 77)
    c0 = rng.uniform(0, box, 3).astype(np.float32)
    return {"scale": np.float32(rng.uniform(0.9, 1.1)), "rot": random_rotation(rng).astype(np.float32), "trans": np.zeros(3, np.float32),
            "center0": c0, "center1": (c0 + rng.uniform(-3, 3, 3)).astype(np.float32)}


def _sets(kind, seed, n_f=3000, n_m=2000):
    """fixed records and moving records whose predictions under _transform(seed) land among them (x_m = R^T (x_f - c1) / s +
    c0 for a sample of the fixed records, plus noise)"""
    rng = np.random.default_rng(seed)
    t = _transform(seed)
    f = random_records(rng, n_f, box=60.0)
    if kind == "clustered":   # few centres, a tiny descriptor alphabet, duplicated records: many exact ties
        c = rng.uniform(0, 60, (8, 3))
        k = rng.integers(0, 8, n_f)
        for a, ax in enumerate("xyz"):
            f[ax] = c[k, a] + rng.normal(0, 1.5, n_f)
        f["desc"] = rng.integers(0, 2, (n_f, 64))
        f[100:300] = f[400:600]
    elif kind == "lattice":   # integer lattice points, equal scales: many pairs pass
        g = rng.integers(0, 14, (n_f, 3))
        f["x"], f["y"], f["z"] = g[:, 0], g[:, 1], g[:, 2]
        f["scale"] = 3.0
        f["desc"] = rng.integers(0, 4, (n_f, 64))
    pick = rng.integers(0, n_f, n_m)
    m = f[pick].copy()
    p = np.stack([m["x"], m["y"], m["z"]], 1).astype(np.float64)
    if kind != "lattice":
        p += rng.normal(0, 2.0, p.shape)
        m["scale"] = m["scale"] * rng.uniform(0.8, 1.25, n_m)
    R, sc = t["rot"].astype(np.float64), float(t["scale"])
    q = (p - t["center1"]) @ R / sc + t["center0"]
    m["x"], m["y"], m["z"] = q[:, 0], q[:, 1], q[:, 2]
    m["scale"] = m["scale"] / sc
    m["desc"] = f["desc"][rng.integers(0, n_f, n_m)]
    f["info"][::9] |= LINE
    m["info"][::11] |= LINE
    return f, m


def _specials(f, m):
    f, m = f.copy(), m.copy()
    f["x"][5], f["y"][6], f["z"][7], f["x"][8] = np.nan, np.inf, -np.inf, 1e30
    m["x"][5], m["y"][6], m["z"][7] = np.nan, -np.inf, np.inf
    f["scale"][10], f["scale"][11], f["scale"][12] = 0.0, np.inf, np.nan
    m["scale"][10], m["scale"][11], m["scale"][12] = 0.0, np.inf, np.nan
    return f, m


def _check_search(built, rorc, f, m, t, radius):
    lo, hi = interval()
    want = rorc.search(f, m, t, radius, lo, hi)
    got = built.guided_search(f, m, t, radius)
    for k, (g, w) in enumerate(zip(got[:4], want)):
        assert np.array_equal(g, w), ("i1", "d1", "i2", "d2")[k]
    # the sorted-key form visits the same cells
    keyed = built.guided_search(f, m, t, radius, index_cells_max=1)
    for g, w in zip(keyed[:5], got[:5]):
        assert np.array_equal(g, w)
    visited = got[4]
    assert (visited >= 0).all() and (visited[want[2] >= 0] >= 2).all()
    return want


@pytest.mark.parametrize("kind", ["random", "clustered", "lattice"])
@pytest.mark.parametrize("radius", [0.5, 4.0, 16.0])
def test_guided_search_equals_oracle(built, rorc, kind, radius):
    f, m = _sets(kind, 3)
    want = _check_search(built, rorc, f, m, _transform(3), radius)
    if radius >= 4.0:
        assert (want[2] >= 0).sum() > len(m) // 4   # second-best candidates were there to order


@pytest.mark.parametrize("radius", [0.0, 0.5, 4.0, 16.0])
def test_guided_search_non_finite_and_zero_scales(built, rorc, radius):
    f, m = _specials(*_sets("clustered", 5))
    _check_search(built, rorc, f, m, _transform(5), radius)
    # a transform that sends every prediction to NaN finds nothing
    t = dict(_transform(5), scale=np.float32(np.nan))
    got = built.guided_search(f, m, t, 4.0)
    assert (got[0] == -1).all() and (got[4] == 0).all()


@pytest.mark.parametrize("n_f", [0, 1])
def test_guided_search_tiny_fixed_sets(built, rorc, n_f):
    f, m = _sets("random", 9, n_f=max(n_f, 1), n_m=300)
    f = f[:n_f]
    if n_f:
        m["x"][:50], m["y"][:50], m["z"][:50] = f["x"][0], f["y"][0], f["z"][0]
        m["scale"][:50], m["info"][:50] = f["scale"][0], f["info"][0]
    t = {"scale": np.float32(1), "rot": np.eye(3, dtype=np.float32), "trans": np.zeros(3, np.float32), "center0": np.zeros(3, np.float32),
         "center1": np.zeros(3, np.float32)}
    want = _check_search(built, rorc, f, m, t, 2.0)
    assert (want[0] == 0).sum() >= 50 if n_f else (want[0] == -1).all()


@pytest.fixture(scope="module")
def extractions_256(built):
    v = built.synth_blobs(256, 256, 256, seed=12345)
    w = np.ascontiguousarray(np.roll(v, (3, -5, 7), axis=(0, 1, 2)))
    return extract(built, v), extract(built, w)


@pytest.mark.parametrize("radius", [4.0, 16.0])
def test_guided_search_on_256_extractions(built, rorc, extractions_256, radius):
    f, m = extractions_256
    assert len(f) > 15000 and len(m) > 15000, (len(f), len(m))   # about 20 k queries: many workgroups
    t = built.match_keys(f, m)
    want = _check_search(built, rorc, f, m, t, radius)
    assert (want[0] >= 0).mean() > 0.5


def _same_refine(built, got, rep, f, m, init, rorc, search=None, **params):
    """search(t, radius) -> (i1, d1, i2, d2): the loop's search; None: the brute-force oracle's (record sets too large for it
    pass a search whose results were checked against it on a sample)"""
    lo, hi = interval()
    if search is None:
        search = lambda t, r: rorc.search(f, m, t, r, lo, hi)
    cur, kept, want = cpu_refine(f, m, init, search, built.fit_similarity, **params)
    assert rep["rounds"] == want["rounds"] and rep["stop"] == want["stop"], (rep, want)
    for a, b in zip(rep["round"], want["round"]):
        assert a["radius"].tobytes() == np.float32(b["radius"]).tobytes()
        assert (a["accepted"], a["kept"], a["rms"], a["shift"]) == (b["accepted"], b["kept"], b["rms"], b["shift"]), (a, b)
        assert a["visited"] > 0
    for k in ("scale", "rot", "trans", "center0", "center1"):
        assert np.asarray(got[k], np.float32).tobytes() == np.asarray(cur[k], np.float32).tobytes(), k
    if kept is not None:
        assert np.array_equal(got["moving_idx"], kept[0]) and np.array_equal(got["fixed_idx"], kept[1])
        assert np.array_equal(got["dist2"], kept[2]) and (got["inlier"] == 1).all() and got["winner"] == -1
        assert got["inliers"] == got["n_matches"] == len(kept[0])
    return want


@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("cells_max", [None, 1])
def test_refine_similarity_equals_cpu_loop(built, rorc, seed, cells_max):
    f, m, R, s, t = noisy_case(seed, n=1500)
    init = built.match_keys(f, m)
    params = {} if cells_max is None else {"index_cells_max": cells_max}
    got, rep = built.refine_similarity(f, m, init, **params)
    want = _same_refine(built, got, rep, f, m, init, rorc)
    assert want["stop"] == "converged"


def test_refine_similarity_parameters_and_refusal(built, rorc):
    f, m, R, s, t = noisy_case(4, n=600)
    init = built.match_keys(f, m)
    got, rep = built.refine_similarity(f, m, init, max_rounds=5, min_radius=0.5, max_radius=8.0, ratio_num=9, ratio_den=10, stop_shift=0.0)
    _same_refine(built, got, rep, f, m, init, rorc, max_rounds=5, min_radius=0.5, max_radius=8.0, ratio_num=9, ratio_den=10, stop_shift=0.0)
    # no pair has equal line flags: the fit is refused, the Hough transform and its matches come back unchanged
    g = m.copy()
    g["info"] |= LINE
    f = f.copy()
    f["info"] &= ~np.uint32(LINE)
    init = built.match_keys(f, g)
    got, rep = built.refine_similarity(f, g, init)
    assert rep["stop"] == "fit" and rep["rounds"] == 1
    for k in ("scale", "rot", "trans", "moving_idx", "fixed_idx", "inlier", "dist2"):
        assert np.array_equal(got[k], init[k]), k
    # no moving record
    got, rep = built.refine_similarity(f, m[:0], built.match_keys(f, m[:0]))
    assert rep["stop"] == "none" and rep["rounds"] == 0


@pytest.fixture(scope="module")
def scenario_keys(built, tmp_path_factory):
    """the voxel-key 20-degree scenario, extracted on the GPU"""
    tmp = tmp_path_factory.mktemp("scenario")
    rs = ResampleOracle(tmp)
    vols = scenario_volumes(built, rs, tmp, False)
    _run([built.FEATEXTRACT, "-d0", vols[0], "fixed.key"], tmp)
    _run([built.FEATEXTRACT, "-d0", vols[1], "moving.key"], tmp)
    return tmp, vols


def test_featmatchmultiple_expand_files(built, aorc, rorc, scenario_keys, tmp_path):
    src, _ = scenario_keys
    names = ["fixed.key", "moving.key"]
    for n in names:
        (tmp_path / n).write_bytes((src / n).read_bytes())
    run = _run([built.FEATMATCH, "-a", "-e"] + names, tmp_path)
    F, M = (built.match_filter(built.read_key(str(tmp_path / n)), 1, 4) for n in names)
    init = built.match_keys(F, M)
    ref, rep = built.refine_similarity(F, M, init)
    _same_refine(built, ref, rep, F, M, init, rorc)
    base = str(tmp_path / "want")
    built.write_similarity(base + ".trans.txt", ref)
    inv = built.similarity_invert(ref)
    built.write_similarity(base + ".trans-inverse.txt", dict(ref, scale=inv[0], rot=inv[1], trans=inv[2]))
    built.write_alignment_matches(base, names[0], names[1], F, M, ref)
    for suf in (".trans.txt", ".trans-inverse.txt", ".matches.info.txt", ".matches.img1.txt", ".matches.img2.txt"):
        assert (tmp_path / ("moving.key" + suf)).read_bytes() == (tmp_path / ("want" + suf)).read_bytes(), suf
    assert "moving.key: inliers %d\t%d\t0\t%f" % (init["inliers"], ref["inliers"], float(ref["scale"])) in run.stdout.splitlines()
    lines = (tmp_path / "moving.key.refine.txt").read_text().splitlines()
    assert len([l for l in lines if not l.startswith("#")]) == rep["rounds"] and lines[-1].startswith("# stop: ")
    # -e needs -a
    r = subprocess.run([built.FEATMATCH, "-e"] + names, cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    # -s2 -e: three refined passes, the last (valleys) leaves its files
    _run([built.FEATMATCH, "-a", "-s2", "-e"] + names, tmp_path)
    Fv, Mv = (built.match_filter(built.read_key(str(tmp_path / n)), 1, 1) for n in names)
    refv, _ = built.refine_similarity(Fv, Mv, built.match_keys(Fv, Mv))
    built.write_similarity(base + ".trans.txt", refv)
    assert (tmp_path / "moving.key.trans.txt").read_bytes() == (tmp_path / "want.trans.txt").read_bytes()
    # without -e, in the same directory: the bytes of the oracle's writers, as before
    run = _run([built.FEATMATCH, "-a"] + names, tmp_path)
    r = aorc.match_keys(F, M)
    assert "moving.key: inliers %d\t0\t0\t%f" % (r["inliers"], float(r["scale"])) in run.stdout.splitlines()
    aorc.write_matrix(base + ".trans.txt", r)
    aorc.write_matches(base, names[0], names[1], F, M, r)
    for suf in (".trans.txt", ".matches.info.txt", ".matches.img1.txt", ".matches.img2.txt"):
        assert (tmp_path / ("moving.key" + suf)).read_bytes() == (tmp_path / ("want" + suf)).read_bytes(), suf


@pytest.mark.parametrize("world", [False, True])
def test_end_to_end_refined(built, tmp_path, world):
    """_end_to_end of test_gpu_resample.py with -a -e: the refined transform through featResample.  The CPU restatement
    (oracle extraction, MatchKeys, the loop, the resample oracle) predicts the in-memory figures exactly."""
    rs = ResampleOracle(tmp_path)
    fixed, moving, V, M, A_true, vox_v, vox_m, hv, hm = scenario_volumes(built, rs, tmp_path, world)
    opt = ["-w"] if world else []
    _run([built.FEATEXTRACT, "-d0"] + opt + [fixed, "fixed.key"], tmp_path)
    _run([built.FEATEXTRACT, "-d0"] + opt + [moving, "moving.key"], tmp_path)
    res = {}
    for flag in ("-a", "-e"):
        _run([built.FEATMATCH, "-a"] + ([flag] if flag == "-e" else []) + ["fixed.key", "moving.key"], tmp_path)
        trans = str(tmp_path / "moving.key.trans.txt")
        out_name = "out%s.nii" % flag
        _run([built.FEATRESAMPLE, "-d0"] + opt + [fixed, moving, trans, out_name], tmp_path)
        out, _ = built.read_nifti(str(tmp_path / out_name))
        A = scenario_map(built, built.read_similarity(trans), world, vox_v, vox_m, hv, hm)
        res[flag] = scenario_score(built, V, out, A, A_true)
    (c0, e0), (c1, e1) = res["-a"], res["-e"]
    print("end to end%s: -a corr %.5f err %.4f; -a -e corr %.5f err %.4f voxel" % (" -w" if world else "", c0, e0, c1, e1))
    assert (c1 >= 0.95 and e1 <= 1.0) if world else (c1 >= 0.98 and e1 <= 0.5), (c1, e1)
    assert e1 * 4 <= e0, (e0, e1)
    # the in-memory refined transform equals the CPU prediction's
    F, Mk = (built.match_filter(built.read_key(str(tmp_path / n))) for n in ("fixed.key", "moving.key"))
    ref, _ = built.refine_similarity(F, Mk, built.match_keys(F, Mk))
    A = scenario_map(built, built.similarity_matrix(ref), world, vox_v, vox_m, hv, hm)
    got = scenario_score(built, V, built.resample_affine(M, V.shape, A), A, A_true)
    (tmp_path / "cpu").mkdir()
    want = scenario_cpu(built, tmp_path / "cpu", world)["refined"]
    assert got == want, (got, want)
