"""CPU tests of the alignment path (featMatchMultiple -a): the oracle's transform recovery, the
product's ratio interval against a brute-force logf sweep, the product's writers against the oracle's bytes, and the
host-level edge cases.  No GPU needed."""
import numpy as np
import pytest

import align_cases as ac


@pytest.fixture(scope="module")
def aorc(tmp_path_factory):
    return ac.AlignOracle(tmp_path_factory.mktemp("align_oracle"))


@pytest.fixture(scope="module")
def alib(built):
    built.host_lib().sift3d_log_ratio_interval   # the product's host side of the alignment path must exist
    return built


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_oracle_recovers_a_similarity(alib, aorc, seed):
    fixed, moving, R, s, t, n, partner = ac.recovery_case(seed)
    r = aorc.match_keys(fixed, moving)
    assert r["winner"] >= 0 and r["n_matches"] == len(moving)
    assert np.abs(r["rot"] - R).max() < 1e-4
    assert abs(float(r["scale"]) - s) < 1e-4 * s
    assert np.abs(r["trans"] - t).max() < 1e-3
    # the inliers are exactly the true pairs, each matched to its partner
    mi, fi, fl = r["moving_idx"], r["fixed_idx"], r["inlier"]
    true = mi < n
    assert (fl[true] == 1).all() and (fl[~true] == 0).all()
    assert (fi[true] == partner[mi[true]]).all()
    assert r["inliers"] == n


@pytest.mark.parametrize("t", [ac.LOG_1_5, 1.0])
def test_log_interval_equals_logf_sweep(alib, aorc, t):
    lo, hi = alib.log_ratio_interval(t)
    want = aorc.interval_sweep(t)
    assert lo.view(np.uint32) == want[0].view(np.uint32) and hi.view(np.uint32) == want[1].view(np.uint32)


def test_writers_match_the_oracle_bytes(alib, aorc, tmp_path):
    fixed, moving, R, s, t, n, _ = ac.recovery_case(4, n=120)
    moving["info"][::7] |= 0x10
    r = aorc.match_keys(fixed, moving)
    alib.write_similarity(tmp_path / "p.trans.txt", r)
    aorc.write_matrix(str(tmp_path / "o.trans.txt"), r)
    assert (tmp_path / "p.trans.txt").read_bytes() == (tmp_path / "o.trans.txt").read_bytes()
    pinv, oinv = alib.similarity_invert(r), aorc.invert(r)
    for a, b in zip(pinv, oinv):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    inv = dict(r, scale=pinv[0], rot=pinv[1], trans=pinv[2])
    alib.write_similarity(tmp_path / "p.inv.txt", inv)
    aorc.write_matrix(str(tmp_path / "o.inv.txt"), inv)
    assert (tmp_path / "p.inv.txt").read_bytes() == (tmp_path / "o.inv.txt").read_bytes()
    # the inverse undoes the transform
    p = np.stack([moving["x"], moving["y"], moving["z"]], 1).astype(np.float64)
    fwd = float(r["scale"]) * p @ r["rot"].astype(np.float64).T + r["trans"]
    back = float(pinv[0]) * fwd @ pinv[1].astype(np.float64).T + pinv[2]
    assert np.abs(back - p).max() < 1e-5 * max(1.0, np.abs(p).max())
    names = ("dir/fixed.key", "dir/moving.v2.key")
    alib.write_alignment_matches(str(tmp_path / "p"), names[0], names[1], fixed, moving, r)
    aorc.write_matches(str(tmp_path / "o"), names[0], names[1], fixed, moving, r)
    for suf in (".matches.info.txt", ".matches.img1.txt", ".matches.img2.txt"):
        a, b = (tmp_path / ("p" + suf)).read_bytes(), (tmp_path / ("o" + suf)).read_bytes()
        assert a == b, suf
    head = (tmp_path / "p.matches.img1.txt").read_text().splitlines()
    assert head[0] == "# Img1: dir/fixed.hdr" and head[1] == "# Img2: dir/moving.v2.hdr" and head[2] == "# Matches: %d" % n


def test_edge_cases_at_the_host_level(alib, aorc, tmp_path):
    rng = np.random.default_rng(9)
    fixed = ac.random_records(rng, 50)
    # an empty moving set and a single fixed record: the identity, no matches
    for f, m in ((fixed, fixed[:0]), (fixed[:1], fixed[:10])):
        r = aorc.match_keys(f, m)
        assert r["n_matches"] == 0 and r["inliers"] == 0 and r["winner"] == -1
        assert float(r["scale"]) == 1.0 and (r["rot"] == np.eye(3, dtype=np.float32)).all() and (r["trans"] == 0).all()
    # at most three matches: the identity, inliers = the match count
    for k in (1, 2, 3):
        r = aorc.match_keys(fixed, fixed[:k])
        assert r["n_matches"] == k and r["inliers"] == k and r["winner"] == -1 and float(r["scale"]) == 1.0
        alib.write_similarity(tmp_path / "id.txt", r)
        assert (tmp_path / "id.txt").read_text() == ("1.000000\t0.000000\t0.000000\t0.000000\n0.000000\t1.000000\t0.000000\t0.000000\n"
                                                      "0.000000\t0.000000\t1.000000\t0.000000\n0.0\t0.0\t0.0\t1.0\n")
    # degenerate hypotheses (zero scale: the three points coincide) are skipped; all degenerate: no winner
    m = 6
    p = rng.uniform(0, 50, (m, 3)).astype(np.float32)
    o = np.tile(np.eye(3, dtype=np.float32).ravel(), (m, 1))
    s = np.full(m, 3.0, np.float32)
    s0 = s.copy()
    s0[[0, 2]] = 0.0
    h = aorc.hough(p, p, s0, s, o, o)
    assert h["counts"][0] == -1 and h["counts"][2] == -1 and h["winner"] == 1
    h = aorc.hough(p, p, np.zeros(m, np.float32), s, o, o)
    assert (h["counts"] == -1).all() and h["winner"] == -1 and (h["flags"] == 0).all()


def _same_keys(a, b):
    for k in ("scale", "rot", "trans", "center0", "center1"):
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    for k in ("n_matches", "inliers", "winner"):
        assert a[k] == b[k], k
    for k in ("moving_idx", "fixed_idx", "inlier", "dist2"):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("seed,n,max_matches", [(5, 300, 3000), (6, 400, 150), (7, 2, 3000), (8, 3, 3000), (9, 60, 4)])
def test_match_keys_from_ratio_equals_match_keys(alib, aorc, seed, n, max_matches):
    """orc_match_keys_from_ratio (the GPU scale tests feed it the GPU's ratio arrays) is orc_match_keys with the ratio search
    taken out: fed orc_ratio's own arrays it must give the same result, bit for bit -- here also with duplicated descriptors
    (0 / 0 ratios sorted last), a cut at max_matches, and too few matches for a Hough"""
    fixed, moving, R, s, t, _n, _p = ac.recovery_case(seed, n=n)
    rng = np.random.default_rng(seed)
    moving["desc"][::5] = fixed["desc"][rng.integers(0, len(fixed), len(moving[::5]))]
    fixed["desc"][1::9] = fixed["desc"][0]
    ratio = aorc.ratio(fixed, moving)
    _same_keys(aorc.match_keys_from_ratio(fixed, moving, ratio, max_matches=max_matches), aorc.match_keys(fixed, moving, max_matches=max_matches))
    for f, m in ((fixed[:1], moving), (fixed, moving[:0])):   # no ratio search at all: the centre and the identity
        empty = [np.zeros(len(m), np.int32)] * 4
        _same_keys(aorc.match_keys_from_ratio(f, m, empty), aorc.match_keys(f, m))
    bad = [a.copy() for a in ratio[:4]]
    bad[0][len(moving) // 2] = len(fixed)
    with pytest.raises(AssertionError):
        aorc.match_keys_from_ratio(fixed, moving, bad)
