"""GPU tests of the alignment path (featMatchMultiple -a): sift3d_match_ratio, sift3d_hough_similarity
and sift3d_match_keys against the CPU oracle tests/align_oracle.c, exactly; the transforms recovered from real extractions;
the command line's files against the oracle writers' bytes."""
import os
import subprocess

import numpy as np
import pytest

import align_cases as ac
from _helpers import extract

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def aorc(tmp_path_factory):
    return ac.AlignOracle(tmp_path_factory.mktemp("align_oracle"))


def _clustered(rng, n, centres=12, spread=2):
    """descriptors near a few centres, many exact duplicates (distance 0: 0 / 0 ratios) and many ties"""
    c = rng.integers(0, 64, (centres, 64))
    d = c[rng.integers(0, centres, n)] + rng.integers(-spread, spread + 1, (n, 64)) * (rng.random((n, 64)) < 0.1)
    return np.clip(d, 0, 127)


def _geometry_that_fires(rng, f):
    """positions, scales and frames on a coarse lattice so that compatible_features holds for many pairs"""
    n = len(f)
    f["x"], f["y"], f["z"] = (rng.integers(0, 4, n).astype(np.float32) for _ in range(3))
    f["scale"] = rng.choice(np.float32([2.0, 2.5, 3.0, 8.0]), n)
    eye = np.eye(3, dtype=np.float32).ravel()
    f["ori"] = np.where(rng.random((n, 1)) < 0.7, eye, -eye)


def _ratio_case(seed, n_db, n_q, kind):
    rng = np.random.default_rng(seed)
    db, q = ac.random_records(rng, n_db, box=30.0), ac.random_records(rng, n_q, box=30.0)
    if kind in ("clustered", "fires", "special"):
        db["desc"], q["desc"] = _clustered(rng, n_db), _clustered(rng, n_q)
        q["desc"][: n_q // 4] = db["desc"][rng.integers(0, n_db, n_q // 4)]   # exact copies: distance 0
    if kind in ("fires", "special"):
        _geometry_that_fires(rng, db)
    if kind == "special":
        k = max(1, n_db // 10)
        idx = rng.choice(n_db, size=min(n_db, 5 * k), replace=False)
        db["scale"][idx[:k]] = np.nan
        db["scale"][idx[k:2 * k]] = np.inf
        db["scale"][idx[2 * k:3 * k]] = 0.0
        db["x"][idx[3 * k:4 * k]] = np.nan
        db["info"][idx[4 * k:]] |= ac.LINE
        db["info"][rng.random(n_db) < 0.2] |= ac.LINE
    return db, q


RATIO_CASES = [(2, 1, "random"), (2, 300, "clustered"), (3, 77, "fires"), (255, 1000, "clustered"), (256, 5000, "fires"),
               (257, 129, "special"), (4097, 1500, "fires"), (4097, 3000, "special"), (20000, 2000, "clustered"),
               (20000, 1000, "fires")]


@pytest.mark.parametrize("n_db,n_q,kind", RATIO_CASES)
def test_match_ratio_equals_oracle(built, aorc, n_db, n_q, kind):
    db, q = _ratio_case(n_db * 7 + n_q, n_db, n_q, kind)
    got = built.match_ratio(db, q)[:4]
    want = aorc.ratio(db, q)
    for g, w, name in zip(got, want[:4], ("i1", "d1", "i2", "d2")):
        assert (g == w).all(), (name, int(np.argmax(g != w)))
    if kind in ("fires", "special") and n_db >= 256:
        # the state machine's four branches all occur (closer / second x compatible / not), often
        assert (want[4] >= n_q // 20).all(), want[4]


def test_match_ratio_refuses_bad_input(built):
    rng = np.random.default_rng(3)
    db, q = ac.random_records(rng, 10), ac.random_records(rng, 4)
    with pytest.raises(built.Sift3DError):
        built.match_ratio(db[:1], q)
    bad = db.copy()
    bad["desc"][3, 5] = 128
    with pytest.raises(built.Sift3DError):
        built.match_ratio(bad, q)
    bad = q.copy()
    bad["desc"][0, 0] = -1
    with pytest.raises(built.Sift3DError):
        built.match_ratio(db, bad)


def _hough_case(seed, m):
    """m correspondences: 60 % from one similarity (with jitter), the rest unrelated; a few degenerate (zero scale)"""
    rng = np.random.default_rng(seed)
    fixed, moving, R, s, t, n, partner = ac.recovery_case(seed, n=max(2, int(0.6 * m)), extra=1.0)
    mv = moving[:m]
    fx = fixed[np.where(partner[:m] >= 0, partner[:m], rng.integers(0, len(fixed), m))]
    p0 = np.stack([mv["x"], mv["y"], mv["z"]], 1)
    p1 = np.stack([fx["x"], fx["y"], fx["z"]], 1) + rng.normal(0, 0.3, (m, 3)).astype(np.float32)
    s0, s1 = mv["scale"].copy(), fx["scale"].copy()
    s0[rng.choice(m, size=max(1, m // 25), replace=False)] = 0.0
    return p0, p1, s0, s1, mv["ori"], fx["ori"]


@pytest.mark.parametrize("m", [4, 100, 3000])
def test_hough_similarity_equals_oracle(built, aorc, m):
    args = _hough_case(m, m)
    got, want = built.hough_similarity(*args), aorc.hough(*args)
    assert (got["counts"] == want["counts"]).all()
    assert (want["counts"] == -1).any()
    assert got["winner"] == want["winner"] >= 0
    assert (got["flags"] == want["flags"]).all()
    assert got["rot"].tobytes() == want["rot"].tobytes() and got["scale"].tobytes() == want["scale"].tobytes()


KEYS = ("scale", "rot", "trans", "center0", "center1")


def _same(got, want):
    for k in KEYS:
        assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), k
    for k in ("n_matches", "inliers", "winner"):
        assert got[k] == want[k], k
    for k in ("moving_idx", "fixed_idx", "inlier", "dist2"):
        assert (got[k] == want[k]).all(), k


def test_match_keys_constructed_and_edges(built, aorc):
    fixed, moving, R, s, t, n, _ = ac.recovery_case(11, n=500)
    _same(built.match_keys(fixed, moving), aorc.match_keys(fixed, moving))
    _same(built.match_keys(fixed, moving, max_matches=200), aorc.match_keys(fixed, moving, max_matches=200))
    for f, m in ((fixed, moving[:0]), (fixed[:1], moving[:5]), (fixed, moving[:3])):
        _same(built.match_keys(f, m), aorc.match_keys(f, m))


def _volumes(built):
    big = built.synth_blobs(144, 144, 144, seed=21)
    fixed = np.ascontiguousarray(big[:128, :128, :128])
    return fixed, {"shift": np.ascontiguousarray(big[5:133, 9:137, 3:131]),          # x_f = x_m + (3, 9, 5)
                   "rot90": np.ascontiguousarray(np.rot90(fixed, 1, axes=(1, 2))),  # a quarter turn in the x-y plane
                   "half": np.ascontiguousarray(fixed[::2, ::2, ::2])}              # every other voxel: x_f ~ 2 x_m


@pytest.fixture(scope="module")
def extractions(built):
    fixed, moving = _volumes(built)
    return extract(built, fixed), {k: extract(built, v) for k, v in moving.items()}


# Tolerances fixed beforehand from the CPU oracle on the oracle's own extractions of the same volumes (which the GPU's
# equal): shift -> rot within 1e-6 of I, scale 0.9999995, trans (3.00015, 8.99995, 4.99992); rot90 -> rot within 1e-6 of
# [[0,-1,0],[1,0,0],[0,0,1]], scale 1, trans (128.0000, 0.00002, -0.00002); half -> scale 1.973, rot within 0.081 of I,
# trans (2.72, 4.24, -2.09) (one-match hypotheses on a quarter as many records).
EXPECT = {"shift": (np.eye(3), 1.0, (3, 9, 5), 1e-5, 1e-5, 1e-3),
          "rot90": (np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]]), 1.0, (128, 0, 0), 1e-5, 1e-5, 1e-3),
          "half": (np.eye(3), 2.0, (0, 0, 0), 0.1, 0.05, 6.0)}


@pytest.mark.parametrize("case", ["shift", "rot90", "half"])
def test_match_keys_on_extractions(built, aorc, extractions, case):
    fixed, moving = extractions[0], extractions[1][case]
    got, want = built.match_keys(fixed, moving), aorc.match_keys(fixed, moving)
    _same(got, want)
    R, s, t, tr, ts, tt = EXPECT[case]
    assert got["winner"] >= 0 and got["inliers"] >= got["n_matches"] // 2
    assert np.abs(got["rot"] - R).max() < tr and abs(float(got["scale"]) - s) < ts and np.abs(got["trans"] - np.array(t)).max() < tt


def _cli_expect(built, aorc, tmp_path, names, sets, stdout):
    for i in range(1, len(names)):
        r = aorc.match_keys(sets[0], sets[i])
        stdout.append("%s: inliers %d\t0\t0\t%f" % (names[i], r["inliers"], float(r["scale"])))
        base = str(tmp_path / ("want_%d" % i))
        aorc.write_matches(base, names[0], names[i], sets[0], sets[i], r)
        aorc.write_matrix(base + ".trans.txt", r)
        inv = aorc.invert(r)
        aorc.write_matrix(base + ".trans-inverse.txt", dict(r, scale=inv[0], rot=inv[1], trans=inv[2]))
        built.write_key(base + ".update.key", sets[i], eig_thres=-1.0)
    stdout.append("")


@pytest.mark.parametrize("s2", [False, True])
def test_featmatchmultiple_align(built, aorc, extractions, tmp_path, s2):
    fixed, moving = extractions
    names = ["k0.key", "k1.key", "k2.key"]
    for name, f in zip(names, [fixed, moving["shift"], moving["rot90"]]):
        built.write_key(str(tmp_path / name), f, eig_thres=-1.0)
    argv = [built.FEATMATCH, "-a"] + (["-s2"] if s2 else []) + names
    run = subprocess.run(argv, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    read = [built.match_filter(built.read_key(str(tmp_path / n)), 1, 4) for n in names]
    passes = [read] + ([[built.match_filter(f, 1, 0) for f in read], [built.match_filter(f, 1, 1) for f in read]] if s2 else [])
    stdout = []
    for sets in passes:   # each pass overwrites the files: the last one's are what remain
        _cli_expect(built, aorc, tmp_path, names, sets, stdout)
    lines = [l for l in run.stdout.splitlines() if ": inliers " in l or l == ""]
    assert lines == stdout
    for i in range(1, len(names)):
        for suf in (".matches.info.txt", ".matches.img1.txt", ".matches.img2.txt", ".trans.txt", ".trans-inverse.txt", ".update.key"):
            got = (tmp_path / (names[i] + suf)).read_bytes()
            want = (tmp_path / ("want_%d" % i + suf)).read_bytes()
            assert got == want, names[i] + suf
    # the default path is untouched by -a's existence: no alignment files without it
    for p in tmp_path.iterdir():
        p.unlink() if p.name.endswith(".trans.txt") else None
    run = subprocess.run([built.FEATMATCH] + names, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and not any(p.name.endswith(".trans.txt") for p in tmp_path.iterdir())
    assert os.path.exists(tmp_path / "matching_votes.txt")
