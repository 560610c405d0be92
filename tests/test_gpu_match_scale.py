"""GPU suite: the matcher and alignment kernels at the sizes the product is used for -- sift3d_knn64, sift3d_match_ratio,
sift3d_match_keys / sift3d_hough_similarity, sift3d_guided_search / sift3d_refine_similarity and featMatchMultiple's default
path on the records of 512^3 extractions (about 185 k per set, 1.3 M concatenated), above 2^24 rows and queries, and on both
sides of the knn search's segment plan.

The CPU oracles cannot search sets of this size in full, but in every one of these searches a query's result depends only on
the database and that one query.  So the GPU searches all queries, the oracle searches a sample of them (sample_rows), and
the sampled rows must agree bit for bit."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import align_cases as ac
from refine_cases import RefineOracle, interval
from test_gpu_align import _same
from test_gpu_refine import _same_refine

pytestmark = pytest.mark.gpu

TILE, QBLOCK = 256, 128          # database rows per LDS tile, queries per workgroup (kernels_match.hip, kernels_align.hip)
BIG = 1 << 24                    # the first integer a float cannot tell from its neighbour
PLAN_BLOCKS, PLAN_TILES, PLAN_SEGMENTS = 600, 16, 8   # sift3d_knn_plan's limits (kernels_match.hip)


def sample_rows(n, n_random, seed, edge=64, boundaries=16):
    """The query rows a scale test checks against its oracle, ascending and unique: the first and last `edge`; every row of the
    last partial block of 128 queries; rows 256 t - 1 and 256 t on both sides of database-tile boundaries (where the queries
    are the database, the two rows sit in different tiles and query blocks; `boundaries` of them, the first and last
    included, seeded); and n_random seeded random rows."""
    rows = [np.arange(min(edge, n)), np.arange(max(0, n - edge), n), np.arange(n - n % QBLOCK, n)]
    cuts = np.arange(TILE, n, TILE)
    if len(cuts) > boundaries:
        pick = np.random.default_rng(seed).choice(len(cuts) - 2, boundaries - 2, replace=False) + 1
        cuts = cuts[np.concatenate([[0, len(cuts) - 1], pick])]
    rows += [cuts - 1, cuts, np.random.default_rng(seed + 1).integers(0, n, n_random)]
    return np.unique(np.concatenate(rows).astype(np.int64))


def assert_rows(rows, got, want, names):
    """got: arrays over all queries; want: the oracle's arrays over `rows` only.  Reports the first differing row."""
    for name, g, w in zip(names, got, want):
        g, w = np.asarray(g)[rows], np.asarray(w)
        assert g.shape == w.shape, (name, g.shape, w.shape)
        diff = (g != w).reshape(len(rows), -1).any(1)
        if diff.any():
            j = int(np.argmax(diff))
            raise AssertionError("%s: %d of %d sampled rows differ; first: row %d, got %s, want %s"
                                 % (name, int(diff.sum()), len(rows), rows[j], g[j].tolist(), w[j].tolist()))


def assert_knn_order(idx, d2, n_db):
    """the contract of every list: real rows, ascending distance, ties to the lower index (all rows, in chunks)"""
    for a in range(0, len(idx), 1 << 21):
        i, d = idx[a:a + (1 << 21)].astype(np.int64), d2[a:a + (1 << 21)].astype(np.int64)
        dd, di = np.diff(d, axis=1), np.diff(i, axis=1)
        bad = ~(((dd > 0) | ((dd == 0) & (di > 0))).all(1) & (i >= 0).all(1) & (i < n_db).all(1))
        if bad.any():
            j = int(np.argmax(bad))
            raise AssertionError("row %d breaks the order: idx %s dist2 %s" % (a + j, i[j].tolist(), d[j].tolist()))


def knn_check(built, oracle, db, q, k, rows, want=None):
    """the GPU's lists of all queries; the sampled rows against oracle.knn64 (or its given lists over `rows`, k or more wide:
    the order is total, so the first k of a longer list are the k nearest)"""
    got_i, got_d, _ = built.knn64(db, q, k)
    assert_knn_order(got_i, got_d, len(db))
    wi, wd = oracle.knn64(db, q[rows], k) if want is None else want
    assert_rows(rows, (got_i, got_d), (wi[:, :k], wd[:, :k]), ("idx", "dist2"))
    return got_i, got_d


# ---- the record sets: one 512^3 volume and cheap rigid variants of it, extracted on the GPU ----------------------------------
N = 512
ROLL = (3, -5, 7)     # np.roll shifts along (z, y, x): a record at fixed (x, y, z) sits at moving (x + 7, y - 5, z + 3)
VARIANTS = {"fixed": lambda v: v, "flip_x": lambda v: v[:, :, ::-1], "flip_y": lambda v: v[:, ::-1], "flip_z": lambda v: v[::-1],
            "roll": lambda v: np.roll(v, ROLL, axis=(0, 1, 2)), "rot90_xy": lambda v: np.rot90(v, 1, axes=(1, 2)),
            "rot90_zx": lambda v: np.rot90(v, 1, axes=(0, 2))}


@pytest.fixture(scope="module")
def sets(built):
    v = built.synth_blobs(N, N, N, seed=512)
    out = {}
    with built.Context(N, N, N, device=0) as ctx:
        for name, make in VARIANTS.items():
            ctx.set_volume(np.ascontiguousarray(make(v)))
            out[name] = ctx.extract()
    half = np.ascontiguousarray(v[::2, ::2, ::2])
    del v
    with built.Context(N // 2, N // 2, N // 2, device=0) as ctx:
        ctx.set_volume(half)
        out["half"] = ctx.extract()
    for name in VARIANTS:
        assert len(out[name]) > 150_000, (name, len(out[name]))
    return out


@pytest.fixture(scope="module")
def aorc(tmp_path_factory):
    return ac.AlignOracle(tmp_path_factory.mktemp("align_oracle"))


@pytest.fixture(scope="module")
def rorc(tmp_path_factory):
    return RefineOracle(tmp_path_factory.mktemp("refine_oracle"))


# ---- sift3d_knn64 ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def concat(built, oracle, sets):
    """every set's descriptors in one array (cut to 45 past a multiple of 128: a ragged last query block inside the last 64
    rows), the sampled rows and the oracle's 32 nearest of each"""
    desc = built.match_descriptors(np.concatenate(list(sets.values())))
    n = len(desc) - (len(desc) % QBLOCK - 45) % QBLOCK
    desc = np.ascontiguousarray(desc[:n])
    rows = sample_rows(n, 160, seed=1)
    return desc, rows, oracle.knn64(desc, desc[rows], 32)


@pytest.mark.parametrize("k", [5, 8, 9, 16, 17, 32])
def test_knn_all_records_against_all(built, oracle, concat, k):
    """every record of every set as database and as query: each list length (8, 16, 32) and the k on both sides of a change"""
    desc, rows, want = concat
    assert len(desc) > 1_000_000 and len(desc) % QBLOCK == 45
    got_i, got_d = knn_check(built, oracle, desc, desc, k, rows, want)
    # a query that is in the database finds itself at distance 0 (or k lower-indexed copies of itself)
    zero = got_d[rows] == 0
    assert zero[:, 0].all()
    assert all(r in got_i[r][zero[j]] or zero[j].all() for j, r in enumerate(rows))


@pytest.mark.parametrize("kind", ["one_norm", "mixed_norms"])
def test_knn_neighbours_above_2_24(built, oracle, kind):
    """A database of 2^24 + 4097 rows whose queries' neighbours all sit above row 2^24: the lower 2^24 rows are 4096 random
    rank descriptors, tiled; the upper 4097 are clustered rows near the queries -- rank descriptors too (one norm: the
    constant-norm kernel, many ties) or bytes with varied norms (the general kernel).  The oracle searches the upper rows;
    the lower ones are shown to be farther than every query's k-th neighbour there, so its lists, shifted by 2^24, are the
    answer over the whole database."""
    from test_match import clustered
    rng = np.random.default_rng(24 if kind == "one_norm" else 25)
    far = np.argsort(rng.random((4096, 64)), axis=1).astype(np.int8)
    if kind == "one_norm":
        near = clustered(rng, 4097, 16, 2)
        q = near[rng.integers(0, 4097, 300)]
        for row in q[100:]:                                                 # one transposition away from a database row
            a, b = rng.integers(0, 64, 2)
            row[a], row[b] = row[b], row[a]
    else:
        centres = rng.integers(8, 120, (40, 64))
        near = np.clip(centres[rng.integers(0, 40, 4097)] + rng.integers(-6, 7, (4097, 64)), 0, 127).astype(np.int8)
        q = near[rng.integers(0, 4097, 300)]
        q[100:] = np.clip(q[100:].astype(np.int64) + rng.integers(-3, 4, (200, 64)), 0, 127)
    db = np.empty((BIG + 4097, 64), np.int8)
    db[:BIG].reshape(BIG // 4096, 4096, 64)[:] = far[None]
    db[BIG:] = near
    qi = q.astype(np.int64)
    d_far = ((qi[:, None, :] - far.astype(np.int64)[None]) ** 2).sum(-1).min(1)
    for k in (5, 17, 32):
        wi, wd = oracle.knn64(near, q, k)
        assert (d_far > wd[:, -1]).all(), "the construction failed: a lower row is as near as a k-th neighbour"
        got_i, got_d, _ = built.knn64(db, q, k)
        rows = np.arange(len(q))
        assert_rows(rows, (got_i, got_d), (wi + BIG, wd), ("idx", "dist2"))
    assert (got_d[:100, 0] == 0).all()


def test_knn_more_than_2_24_queries(built, oracle):
    """2^24 + 129 queries against 300 rows: the grid's x dimension, the scratch lists and the merge kernel's query index
    above 2^24 (a ragged last block of one query)"""
    n_q = BIG + 129
    rng = np.random.default_rng(129)
    q = (np.frombuffer(rng.bytes(n_q * 64), np.uint8) & 127).astype(np.int8).reshape(n_q, 64)
    db = rng.integers(0, 128, (300, 64)).astype(np.int8)
    q[n_q - 300:] = db                                                      # the last queries find themselves
    rows = sample_rows(n_q, 4096, seed=3, boundaries=64)
    got_i, got_d = knn_check(built, oracle, db, q, 8, rows)
    assert (got_d[n_q - 300:, 0] == 0).all() and (got_i[n_q - 300:, 0] == np.arange(300)).all()


def plan_segments(n_db, n_q):
    """sift3d_knn_plan restated: database segments only while the query blocks alone give the chip fewer than 600 workgroups,
    at most 8, each at least 16 tiles"""
    ntiles, qblocks = -(-n_db // TILE), -(-n_q // QBLOCK)
    sg = 1
    while sg < PLAN_SEGMENTS and qblocks * sg < PLAN_BLOCKS and ntiles // (sg + 1) >= PLAN_TILES:
        sg += 1
    return sg


def library_plan(built, n_db, n_q):
    """the library's own sift3d_knn_plan (a C++ symbol of libsift3d_hip.so)"""
    fn = getattr(built.hip_lib(), "_Z15sift3d_knn_planlliPiS_")
    g, s = C.c_int(0), C.c_int(0)
    fn(C.c_int64(n_db), C.c_int64(n_q), C.c_int(5), C.byref(g), C.byref(s))
    return s.value


def _plan_switches():
    """(n_db, n_q) on both sides of every switch of the plan: along n_db with one query block, along n_q with a database of
    160 tiles"""
    cases = []
    for s in range(2, PLAN_SEGMENTS + 1):           # the first n_db whose tiles allow s segments, and the one before it
        n = TILE * (PLAN_TILES * s - 1) + 1
        cases += [(n - 1, 100), (n, 100)]
    n_db = TILE * 160 - 17
    prev = plan_segments(n_db, 1)
    for qb in range(2, PLAN_BLOCKS + 2):
        cur = plan_segments(n_db, QBLOCK * qb)
        if cur != prev:                              # the last n_q with the old plan, the first with the new one
            cases += [(n_db, QBLOCK * (qb - 1)), (n_db, QBLOCK * (qb - 1) + 1)]
        prev = cur
    return cases


def test_knn_both_sides_of_the_segment_plan(built, oracle):
    cases = _plan_switches()
    assert len(cases) == 28
    for a, b in zip(cases[::2], cases[1::2]):
        assert plan_segments(*a) != plan_segments(*b), (a, b)
    rng = np.random.default_rng(600)
    from test_match import clustered
    pool = clustered(rng, TILE * 160, 53, 4)
    for j, (n_db, n_q) in enumerate(cases):
        assert library_plan(built, n_db, n_q) == plan_segments(n_db, n_q), (n_db, n_q)
        db = pool[:n_db]
        q = np.concatenate([db[rng.integers(0, n_db, n_q // 2)], clustered(rng, n_q - n_q // 2, 53, 4)])
        rows = sample_rows(n_q, 16, seed=j, edge=8, boundaries=4)
        knn_check(built, oracle, db, q, (9, 16)[j // 2 % 2], rows)   # one k on both sides of a switch


# ---- sift3d_match_ratio, sift3d_match_keys, sift3d_hough_similarity -------------------------------------------------------
@pytest.fixture(scope="module")
def ratio_512(built, aorc, sets):
    """the GPU's ratio search of every moving (rolled) record over the fixed set, and the oracle's over a sample of them"""
    f, m = sets["fixed"], sets["roll"]
    got = built.match_ratio(f, m)[:4]
    rows = sample_rows(len(m), 3000, seed=5)
    return got, rows, aorc.ratio(f, m[rows])


def test_match_ratio_512(sets, ratio_512):
    got, rows, want = ratio_512
    assert len(sets["fixed"]) > 150_000 and len(sets["roll"]) > 150_000
    assert_rows(rows, got, want[:4], ("i1", "d1", "i2", "d2"))
    print("ratio 512: %d x %d, %d rows checked; branches (closer / closer compatible / second / second compatible): %s"
          % (len(sets["fixed"]), len(sets["roll"]), len(rows), want[4].tolist()))
    assert want[4][0] >= len(rows) and want[4][2] >= len(rows)   # the rare path, several times per query


def test_match_ratio_database_above_2_24(built, aorc, sets):
    """few queries over 2^24 + 4097 records: the lower 2^24 are 4096 records of the fixed set tiled, the upper ones the next
    4097; half of the queries are copies of upper records (their best match sits above 2^24)"""
    f = sets["fixed"]
    db = np.empty(BIG + 4097, f.dtype)
    db[:BIG].reshape(BIG // 4096, 4096)[:] = f[None, :4096]
    db[BIG:] = f[4096:4096 + 4097]
    rng = np.random.default_rng(7)
    q = np.concatenate([f[4096 + rng.integers(0, 4097, 6)], sets["roll"][rng.integers(0, len(sets["roll"]), 6)]])
    got = built.match_ratio(db, q)[:4]
    want = aorc.ratio(db, q)
    assert_rows(np.arange(len(q)), got, want[:4], ("i1", "d1", "i2", "d2"))
    assert (want[1][:6] == 0).all() and (want[0][:6] >= BIG).sum() >= 3


def test_match_keys_512(built, aorc, sets, ratio_512):
    """the whole sift3d_match_keys against MatchKeys restated from the GPU's ratio arrays (sampled above): sort, cut, Hough"""
    got_r, rows, want_r = ratio_512
    assert_rows(rows, got_r, want_r[:4], ("i1", "d1", "i2", "d2"))
    f, m = sets["fixed"], sets["roll"]
    got = built.match_keys(f, m)
    _same(got, aorc.match_keys_from_ratio(f, m, got_r))
    assert got["winner"] >= 0 and got["inliers"] >= got["n_matches"] // 2
    assert np.abs(got["trans"] - np.float32([-ROLL[2], -ROLL[1], -ROLL[0]])).max() < 1.0


def test_hough_similarity_12000(built, aorc, sets, ratio_512):
    """sift3d_hough_similarity on the 12 000 best ratio matches of the 512^3 pair (MatchKeys' default cut is 3 000)"""
    (i1, d1, i2, d2), _rows, _want = ratio_512
    f, m = sets["fixed"], sets["roll"]
    ratio = d1.astype(np.float32) / d2.astype(np.float32)
    order = np.lexsort((np.arange(len(m)), ratio))[:12_000]
    a, b = m[order], f[i1[order]]
    args = (np.stack([a["x"], a["y"], a["z"]], 1), np.stack([b["x"], b["y"], b["z"]], 1), a["scale"], b["scale"], a["ori"], b["ori"])
    got, want = built.hough_similarity(*args), aorc.hough(*args)
    assert (got["counts"] == want["counts"]).all()
    assert got["winner"] == want["winner"] >= 0
    assert (got["flags"] == want["flags"]).all() and want["flags"].sum() > 6_000
    assert got["rot"].tobytes() == want["rot"].tobytes() and got["scale"].tobytes() == want["scale"].tobytes()


# ---- sift3d_guided_search, sift3d_refine_similarity -----------------------------------------------------------------------
ROLL_T = {"scale": np.float32(1), "rot": np.eye(3, dtype=np.float32), "trans": np.float32([-ROLL[2], -ROLL[1], -ROLL[0]]),
          "center0": np.zeros(3, np.float32), "center1": np.float32([-ROLL[2], -ROLL[1], -ROLL[0]])}


def _snap(recs):
    """positions on the half-voxel lattice: under the exact integer shift ROLL_T many squared distances then equal the
    squared radius exactly (0.25, 16, 256), where the test `< radius^2` decides"""
    r = recs.copy()
    for ax in "xyz":
        r[ax] = np.round(r[ax] * 2) / 2
    return r


@pytest.fixture(scope="module")
def hough_512(built, sets):
    return built.match_keys(sets["fixed"], sets["roll"])


@pytest.mark.parametrize("geometry", ["hough", "lattice"])
@pytest.mark.parametrize("radius", [0.5, 4.0, 16.0])
def test_guided_search_512(built, rorc, sets, hough_512, geometry, radius):
    """Both index forms over 185 k fixed records (at radius 0.5 the dense table would need 10^9 cells: the sorted keys are the
    default there); sampled moving rows against the brute-force oracle, the two forms against each other on every row"""
    f, m = sets["fixed"], sets["roll"]
    t = hough_512
    if geometry == "lattice":
        f, m, t = _snap(f), _snap(m), ROLL_T
    lo, hi = interval()
    got = built.guided_search(f, m, t, radius)
    keyed = built.guided_search(f, m, t, radius, index_cells_max=1)
    for name, g, w in zip(("i1", "d1", "i2", "d2", "visited"), got[:5], keyed[:5]):
        assert np.array_equal(g, w), name
    rows = sample_rows(len(m), 4000, seed=int(radius * 8) + (geometry == "lattice"), boundaries=32)
    want = rorc.search(f, m[rows], t, radius, lo, hi)
    assert_rows(rows, got[:4], want, ("i1", "d1", "i2", "d2"))
    assert (got[4] >= 0).all() and (got[4][rows][want[2] >= 0] >= 2).all()
    if radius >= 4.0:
        assert (got[0] >= 0).mean() > 0.5 and (got[2] >= 0).any()


@pytest.mark.parametrize("cells_max", [None, 1])
def test_refine_similarity_512(built, rorc, sets, hough_512, cells_max):
    """the loop's bookkeeping at 185 k records: sift3d_refine_similarity against the loop restated on the host, its search the
    GPU's guided search (each round's sampled against the oracle)"""
    f, m = sets["fixed"], sets["roll"]
    lo, hi = interval()

    def search(t, r):
        res = built.guided_search(f, m, t, r)[:4]
        rows = sample_rows(len(m), 300, seed=int(r * 1000) % 9973, edge=16, boundaries=4)
        assert_rows(rows, res, rorc.search(f, m[rows], t, r, lo, hi), ("i1", "d1", "i2", "d2"))
        return res
    params = {} if cells_max is None else {"index_cells_max": cells_max}
    got, rep = built.refine_similarity(f, m, hough_512, **params)
    want = _same_refine(built, got, rep, f, m, hough_512, rorc, search=search)
    assert want["rounds"] >= 1 and got["n_matches"] > 1_000


# ---- featMatchMultiple, default path ---------------------------------------------------------------------------------------
def test_featmatchmultiple_default_path_512(built, oracle, sets, tmp_path):
    """test_match.py::test_matcher_command_line on the eight 512^3 key files: matching_votes.txt and vote_count.txt equal the
    oracle's votes over the GPU's lists of the same filtered records, and a sample of those lists equals the oracle's search"""
    names = []
    for name, f in sets.items():
        built.write_key(str(tmp_path / (name + ".key")), f)
        names.append(name + ".key")
    r = subprocess.run([built.FEATMATCH, "-n", "5"] + names, cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    sel = [built.match_filter(built.read_key(str(tmp_path / n)), reoriented=1, peaks=4) for n in names]
    first = np.concatenate([[0], np.cumsum([len(s) for s in sel])]).astype(np.int64)
    desc = built.match_descriptors(np.concatenate(sel))
    assert len(desc) > 500_000
    rows = sample_rows(len(desc), 64, seed=9, edge=16, boundaries=4)
    idx, d2 = knn_check(built, oracle, desc, desc, 5, rows)
    n = len(names)
    votes, counts = oracle.match_votes(first, np.arange(n, dtype=np.int32), n, idx, d2)
    lines = (tmp_path / "matching_votes.txt").read_text().split("\n")
    assert lines[0] == "Peak and Valley"
    got_v = np.array([[float(x) for x in l.split("\t") if x] for l in lines[1:n + 1]], np.float64)
    want_v = np.array([[float("%f" % x) for x in row] for row in votes])
    assert (got_v == want_v).all() and got_v.sum() > 0
    cl = (tmp_path / "vote_count.txt").read_text().split("\n")
    got_c = np.array([[int(x) for x in l.split("\t") if x] for l in cl[1:n + 1]])
    assert (got_c == counts).all() and counts.sum() > 0
    fc = (tmp_path / "feature_count.txt").read_text().split()
    assert [int(x) for x in fc[1::2]] == [len(s) for s in sel]
