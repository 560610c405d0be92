"""CPU suite: the guided re-matching of DESIGN.md section 7d without a GPU -- the host fit (sift3d_fit_similarity), the CPU
oracle of the guided search against a numpy restatement, the refinement loop (oracle search + the product's fit) on noisy
record sets, and the 20-degree end-to-end scenario on the oracle's extraction (which the GPU reproduces bit for bit)."""

import numpy as np
import pytest

from align_cases import FEAT, LINE, AlignOracle, random_records, random_rotation
from refine_cases import INT32_MAX, RefineOracle, cpu_refine, interval, map_error, noisy_case


@pytest.fixture(scope="module")
def aorc(tmp_path_factory):
    return AlignOracle(tmp_path_factory.mktemp("align_oracle"))


@pytest.fixture(scope="module")
def rorc(tmp_path_factory):
    return RefineOracle(tmp_path_factory.mktemp("refine_oracle"))


def umeyama(a, b):
    """float64 numpy restatement: x_b = s R x_a + t, det R = +1"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ma, mb = a.mean(0), b.mean(0)
    A, B = a - ma, b - mb
    S = B.T @ A / len(a)
    U, D, Vt = np.linalg.svd(S)
    d = np.sign(np.linalg.det(U) * np.linalg.det(Vt))
    E = np.diag([1.0, 1.0, d])
    R = U @ E @ Vt
    s = np.trace(np.diag(D) @ E) / (A * A).sum(1).mean()
    return s, R, mb - s * R @ ma


# ---- the fit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_fit_recovers_exact_similarity(built, seed):
    rng = np.random.default_rng(seed)
    R, s, t = random_rotation(rng), rng.uniform(0.5, 2.0), rng.uniform(-50, 50, 3)
    a = rng.uniform(0, 100, (int(rng.integers(3, 200)), 3)).astype(np.float32)
    b = (s * a.astype(np.float64) @ R.T + t).astype(np.float32)
    c0 = rng.uniform(0, 100, 3).astype(np.float32)
    d = built.fit_similarity(a, b, center0=c0)
    assert d is not None
    assert abs(float(d["scale"]) - s) <= 1e-5 * s
    assert np.abs(d["rot"] - R).max() <= 1e-5
    assert np.abs(d["trans"] - t).max() <= 1e-5 * 100
    assert abs(np.linalg.det(d["rot"].astype(np.float64)) - 1) < 1e-5
    # center1 is the fit applied to the caller's center0
    assert np.abs(d["center1"] - (s * R @ c0 + t)).max() <= 1e-3


@pytest.mark.parametrize("seed", range(6))
def test_fit_agrees_with_float64_umeyama_under_noise(built, seed):
    rng = np.random.default_rng(100 + seed)
    R, s, t = random_rotation(rng), rng.uniform(0.5, 2.0), rng.uniform(-50, 50, 3)
    a = rng.uniform(0, 100, (300, 3)).astype(np.float32)
    b = (s * a.astype(np.float64) @ R.T + t + rng.normal(0, 2.0, (300, 3))).astype(np.float32)
    d = built.fit_similarity(a, b)
    ws, wR, wt = umeyama(a, b)
    # the product rounds its double result to float once: float rounding is the whole difference
    assert abs(float(d["scale"]) - ws) <= 1e-6 * ws
    assert np.abs(d["rot"] - wR).max() <= 1e-6
    assert np.abs(d["trans"] - wt).max() <= 1e-6 * max(1.0, np.abs(wt).max())


def test_fit_returns_a_proper_rotation_for_a_mirrored_set(built):
    rng = np.random.default_rng(7)
    a = rng.uniform(-50, 50, (100, 3)).astype(np.float32)
    b = a * np.array([-1, 1, 1], np.float32)
    d = built.fit_similarity(a, b)
    assert d is not None
    assert abs(np.linalg.det(d["rot"].astype(np.float64)) - 1) < 1e-5
    ws, wR, wt = umeyama(a, b)
    assert np.abs(d["rot"] - wR).max() <= 1e-5 and abs(float(d["scale"]) - ws) <= 1e-5


def test_fit_refuses_two_points_and_collinear_points(built):
    a = np.array([[0, 0, 0], [1, 2, 3]], np.float32)
    assert built.fit_similarity(a, a) is None
    line = np.outer(np.arange(10), [1.0, 2.0, 3.0]).astype(np.float32)
    assert built.fit_similarity(line, line + 5) is None
    assert built.fit_similarity(np.zeros((5, 3), np.float32), np.ones((5, 3), np.float32)) is None
    bad = np.random.default_rng(1).uniform(0, 10, (5, 3)).astype(np.float32)
    nan = bad.copy()
    nan[2, 1] = np.nan
    assert built.fit_similarity(nan, bad) is None
    # three points in a plane are enough
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    d = built.fit_similarity(tri, tri * 2 + 1)
    assert d is not None and abs(float(d["scale"]) - 2) < 1e-6 and np.abs(d["rot"] - np.eye(3)).max() < 1e-6


# ---- the oracle of the guided search against numpy ----------------------------------------------------------------------
def numpy_search(fixed, moving, t, radius, lo, hi):
    """the predicate of DESIGN.md section 7d in float32 numpy, brute force; ties by the lower fixed index"""
    f32 = np.float32
    c0, c1 = np.asarray(t["center0"], f32), np.asarray(t["center1"], f32)
    rot, s = np.asarray(t["rot"], f32).reshape(3, 3), f32(t["scale"])
    out = [np.full(len(moving), -1, np.int32), np.full(len(moving), INT32_MAX, np.int32), np.full(len(moving), -1, np.int32),
           np.full(len(moving), INT32_MAX, np.int32)]
    fx, fy, fz, fs = (fixed[k].astype(f32) for k in ("x", "y", "z", "scale"))
    rr = f32(radius) * f32(radius)
    fd = fixed["desc"].astype(np.int64)
    with np.errstate(all="ignore"):
        for m in range(len(moving)):
            p = np.array([moving["x"][m], moving["y"][m], moving["z"][m]], f32)
            d = p - c0
            q = [c1[r] + ((rot[r, 0] * d[0] + rot[r, 1] * d[1]) + rot[r, 2] * d[2]) * s for r in range(3)]
            ms = f32(moving["scale"][m]) * s
            r = fs / ms
            dx, dy, dz = fx - q[0], fy - q[1], fz - q[2]
            ok = ((fixed["info"] & LINE) == (moving["info"][m] & LINE)) & (r >= lo) & (r <= hi) & (((dx * dx + dy * dy) + dz * dz) < rr)
            j = np.nonzero(ok)[0]
            if not len(j):
                continue
            dist = ((fd[j] - moving["desc"][m].astype(np.int64)) ** 2).sum(1)
            o = np.lexsort((j, dist))
            out[0][m], out[1][m] = j[o[0]], dist[o[0]]
            if len(o) > 1:
                out[2][m], out[3][m] = j[o[1]], dist[o[1]]
    return out


def small_sets(seed):
    rng = np.random.default_rng(seed)
    fixed = random_records(rng, 120, box=30.0)
    moving = random_records(rng, 60, box=30.0)
    # ties: descriptors from a tiny alphabet, and duplicated fixed records
    fixed["desc"] = rng.integers(0, 2, (120, 64))
    moving["desc"] = rng.integers(0, 2, (60, 64))
    fixed[60:70] = fixed[50:60]
    fixed["info"][::7] |= LINE
    moving["info"][::5] |= LINE
    fixed["x"][3], fixed["y"][8], fixed["z"][13] = np.nan, np.inf, -np.inf
    moving["x"][4], moving["z"][9] = np.nan, np.inf
    fixed["scale"][20], fixed["scale"][21] = 0.0, np.inf
    moving["scale"][11], moving["scale"][12] = 0.0, np.inf
    return fixed, moving


def small_transform(seed):
    rng = np.random.default_rng(seed + 50)
    return {"scale": np.float32(rng.uniform(0.9, 1.1)), "rot": random_rotation(rng).astype(np.float32),
            "center0": rng.uniform(10, 20, 3).astype(np.float32), "center1": rng.uniform(10, 20, 3).astype(np.float32)}


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("radius", [0.0, 0.5, 4.0, 16.0])
def test_oracle_search_matches_numpy(built, rorc, seed, radius):
    fixed, moving = small_sets(seed)
    t = small_transform(seed)
    lo, hi = interval()
    got = rorc.search(fixed, moving, t, radius, lo, hi)
    want = numpy_search(fixed, moving, t, radius, lo, hi)
    for g, w in zip(got, want):
        assert (g == w).all()
    if radius == 0.0:
        assert (got[0] == -1).all()
    if radius == 16.0:
        assert (got[2] >= 0).sum() > 20   # the case has second-best candidates to order


def test_oracle_search_breaks_ties_by_fixed_index(rorc):
    f = np.zeros(4, FEAT)
    f["scale"] = 2.0
    f["x"] = [0.5, 0.2, 0.1, 0.3]
    m = np.zeros(1, FEAT)
    m["scale"] = 2.0
    t = {"scale": 1.0, "rot": np.eye(3), "center0": np.zeros(3), "center1": np.zeros(3)}
    lo, hi = interval()
    i1, d1, i2, d2 = rorc.search(f, m, t, 1.0, lo, hi)
    assert (i1[0], d1[0], i2[0], d2[0]) == (0, 0, 1, 0)


# ---- the loop --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_loop_beats_the_hough_transform_on_noisy_sets(built, aorc, rorc, seed):
    """recovery sets with sigma = 0.3 key units of position noise and 30 % unrelated records on both sides: the refined map
    is within 0.1 key units of the truth at the moving box's corners, and at most a quarter of the Hough map's error"""
    fixed, moving, R, s, t = noisy_case(seed, n=1500)
    init = aorc.match_keys(fixed, moving)
    lo, hi = interval()
    cur, kept, rep = cpu_refine(fixed, moving, init, lambda tt, r: rorc.search(fixed, moving, tt, r, lo, hi), built.fit_similarity)
    e0, e1 = map_error(init, moving, R, s, t), map_error(cur, moving, R, s, t)
    print("seed %d: Hough %.4f, refined %.4f, %s" % (seed, e0, e1, rep))
    assert e1 <= 0.1 and e1 <= e0 / 4, (e0, e1)
    assert rep["stop"] == "converged" and kept is not None and len(kept[0]) >= 1400
    assert 1.0 <= rep["round"][0]["radius"] <= 16.0


def test_loop_stops_when_the_fit_is_refused(built, aorc, rorc):
    fixed, moving, R, s, t = noisy_case(3, n=200)
    init = aorc.match_keys(fixed, moving)
    lo, hi = interval()
    # no candidate passes the ratio test's interval: nothing is accepted, the Hough transform stays
    cur, kept, rep = cpu_refine(fixed, moving, init, lambda tt, r: rorc.search(fixed, moving, tt, r, 2.0, 3.0), built.fit_similarity)
    assert rep["stop"] == "fit" and rep["rounds"] == 1 and kept is None
    assert np.array_equal(cur["rot"], init["rot"]) and cur["scale"] == init["scale"]


# ---- the 20-degree scenario on the CPU ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [False, True])
def test_scenario_predicts_the_end_to_end_figures(built, tmp_path, world):
    """tests/test_gpu_resample.py's oblique case with the oracle's extraction: the Hough transform reproduces the figures
    measured on the GPU for -a (2.54 / 0.972 voxel keys, 5.22 / 0.892 -w keys), and the refined transform reaches the
    bounds test_gpu_refine.py asserts for -a -e (measured here: 0.037 voxel / 0.99981 and 0.046 / 0.99987)."""
    from refine_cases import scenario_cpu
    r = scenario_cpu(built, tmp_path, world)
    (c0, e0), (c1, e1) = r["hough"], r["refined"]
    print("world=%s: Hough corr %.5f err %.4f; refined corr %.5f err %.4f; %s" % (world, c0, e0, c1, e1, r["report"]))
    want0 = (0.8922, 5.220) if world else (0.9724, 2.545)
    assert abs(c0 - want0[0]) < 1e-3 and abs(e0 - want0[1]) < 1e-2
    assert (c1 >= 0.95 and e1 <= 1.0) if world else (c1 >= 0.98 and e1 <= 0.5), (c1, e1)
    assert e1 * 4 <= e0
