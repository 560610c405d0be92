"""Shared pieces of the alignment-path tests (test_align_cpu.py, test_gpu_align.py): the CPU oracle tests/align_oracle.c,
built with cc -O2 -ffp-contract=off into a temporary directory and bound with ctypes, and the constructed record sets."""
import ctypes as C
import os

import numpy as np

from _helpers import c_oracle

FEAT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("scale", "<f4"), ("ori", "<f4", (9,)), ("eigs", "<f4", (3,)),
                 ("info", "<u4"), ("desc", "<f4", (64,))])
LINE = 0x100
LOG_1_5 = 0.4054651


class Sim(C.Structure):
    _fields_ = [("scale", C.c_float), ("rot", C.c_float * 9), ("trans", C.c_float * 3), ("c0", C.c_float * 3), ("c1", C.c_float * 3),
                ("n_matches", C.c_int32), ("inliers", C.c_int32), ("winner", C.c_int32), ("capacity", C.c_int32),
                ("moving_idx", C.c_void_p), ("fixed_idx", C.c_void_p), ("inlier", C.c_void_p), ("dist2", C.c_void_p)]


class AlignOracle:
    def __init__(self, tmpdir):
        L = c_oracle("align_oracle", tmpdir)
        P, I64, I = C.c_void_p, C.c_int64, C.c_int
        for name, res, args in [("orc_ratio", I, [P, I64, P, I64, P, P, P, P, P]),
                                ("orc_hough", I, [P, P, P, P, P, P, I, P, P, P, P, P]),
                                ("orc_match_keys", I, [P, I64, P, I64, I, P]),
                                ("orc_match_keys_from_ratio", I, [P, I64, P, I64, I, P, P, P, P, P]),
                                ("orc_invert", None, [P, P]),
                                ("orc_write_matrix", I, [C.c_char_p, P]),
                                ("orc_write_matches", I, [C.c_char_p, C.c_char_p, C.c_char_p, P, I64, P, P]),
                                ("orc_interval_sweep", I, [C.c_double, P, P])]:
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        self.L = L

    def ratio(self, db, q):
        db, q = np.ascontiguousarray(db, FEAT), np.ascontiguousarray(q, FEAT)
        out = [np.empty(len(q), np.int32) for _ in range(4)]
        br = np.zeros(4, np.int64)
        assert self.L.orc_ratio(db.ctypes.data, len(db), q.ctypes.data, len(q), *[o.ctypes.data for o in out], br.ctypes.data) == 0
        return tuple(out) + (br,)

    def hough(self, p0, p1, s0, s1, o0, o1):
        arr = [np.ascontiguousarray(a, np.float32) for a in (p0, p1, s0, s1, o0, o1)]
        m = len(arr[2])
        counts, flags, rot = np.empty(m, np.int32), np.empty(m, np.int32), np.zeros(9, np.float32)
        w, s = C.c_int32(-1), C.c_float(0)
        self.L.orc_hough(*[a.ctypes.data for a in arr], m, counts.ctypes.data, C.byref(w), rot.ctypes.data, C.byref(s), flags.ctypes.data)
        return {"counts": counts, "winner": w.value, "rot": rot.reshape(3, 3), "scale": np.float32(s.value), "flags": flags}

    def match_keys(self, fixed, moving, max_matches=3000):
        f, m = np.ascontiguousarray(fixed, FEAT), np.ascontiguousarray(moving, FEAT)
        cap = max(1, min(len(m), max_matches))
        arrays = {k: np.zeros(cap, np.int32) for k in ("moving_idx", "fixed_idx", "inlier", "dist2")}
        t = Sim()
        t.capacity = cap
        for k, a in arrays.items():
            setattr(t, k, a.ctypes.data)
        self.L.orc_match_keys(f.ctypes.data, len(f), m.ctypes.data, len(m), int(max_matches), C.byref(t))
        return sim_dict(t, arrays)

    def match_keys_from_ratio(self, fixed, moving, ratio, max_matches=3000):
        """match_keys with the ratio search replaced by given (i1, d1, i2, d2) of every moving record (test only: for record
        sets whose CPU ratio search is too slow, fed with GPU ratio results that were sample-checked against ratio())"""
        f, m = np.ascontiguousarray(fixed, FEAT), np.ascontiguousarray(moving, FEAT)
        r = [np.ascontiguousarray(a, np.int32) for a in ratio[:4]]
        assert all(len(a) == len(m) for a in r)
        cap = max(1, min(len(m), max_matches))
        arrays = {k: np.zeros(cap, np.int32) for k in ("moving_idx", "fixed_idx", "inlier", "dist2")}
        t = Sim()
        t.capacity = cap
        for k, a in arrays.items():
            setattr(t, k, a.ctypes.data)
        assert self.L.orc_match_keys_from_ratio(f.ctypes.data, len(f), m.ctypes.data, len(m), int(max_matches), *[a.ctypes.data for a in r],
                                                C.byref(t)) == 0
        return sim_dict(t, arrays)

    def _struct(self, d):
        t = Sim()
        t.scale = float(d["scale"])
        t.rot[:] = [float(v) for v in np.asarray(d["rot"], np.float32).ravel()]
        t.trans[:] = [float(v) for v in np.asarray(d["trans"], np.float32)]
        t.n_matches, t.inliers, t.winner = int(d.get("n_matches", 0)), int(d.get("inliers", 0)), int(d.get("winner", -1))
        keep = [np.ascontiguousarray(d.get(k, np.zeros(0)), np.int32) for k in ("moving_idx", "fixed_idx", "inlier", "dist2")]
        t.moving_idx, t.fixed_idx, t.inlier, t.dist2 = [a.ctypes.data if len(a) else None for a in keep]
        t.capacity = min(len(a) for a in keep)
        return t, keep

    def invert(self, d):
        t, _k = self._struct(d)
        o = Sim()
        self.L.orc_invert(C.byref(t), C.byref(o))
        return np.float32(o.scale), np.array(o.rot, np.float32).reshape(3, 3), np.array(o.trans, np.float32)

    def write_matrix(self, path, d):
        t, _k = self._struct(d)
        self.L.orc_write_matrix(os.fsencode(path), C.byref(t))

    def write_matches(self, base, name1, name2, fixed, moving, d):
        f, m = np.ascontiguousarray(fixed, FEAT), np.ascontiguousarray(moving, FEAT)
        t, _k = self._struct(d)
        self.L.orc_write_matches(os.fsencode(base), os.fsencode(name1), os.fsencode(name2), f.ctypes.data, len(f), m.ctypes.data, C.byref(t))

    def interval_sweep(self, t):
        lo, hi = C.c_float(0), C.c_float(0)
        self.L.orc_interval_sweep(float(t), C.byref(lo), C.byref(hi))
        return np.float32(lo.value), np.float32(hi.value)


def sim_dict(t, arrays):
    n = t.n_matches
    d = {"scale": np.float32(t.scale), "rot": np.array(t.rot, np.float32).reshape(3, 3), "trans": np.array(t.trans, np.float32),
         "center0": np.array(t.c0, np.float32), "center1": np.array(t.c1, np.float32), "n_matches": n, "inliers": t.inliers,
         "winner": t.winner}
    for k, a in arrays.items():
        d[k] = a[:n].copy()
    return d


def random_rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def random_records(rng, n, box=200.0):
    f = np.zeros(n, FEAT)
    f["x"], f["y"], f["z"] = (rng.uniform(0, box, n) for _ in range(3))
    f["scale"] = rng.uniform(2.0, 5.0, n)
    for i in range(n):
        f["ori"][i] = random_rotation(rng).ravel()
    f["desc"] = rng.integers(0, 64, (n, 64))
    f["info"] = 0x20
    return f


def transform_records(f, R, s, t):
    """the records as the similarity x -> s R x + t maps them: points, scales, and every frame row rotated"""
    g = f.copy()
    p = np.stack([f["x"], f["y"], f["z"]], 1).astype(np.float64)
    q = s * p @ R.T + t
    g["x"], g["y"], g["z"] = q[:, 0], q[:, 1], q[:, 2]
    g["scale"] = f["scale"] * s
    o = f["ori"].reshape(-1, 3, 3).astype(np.float64)
    g["ori"] = (o @ R.T).reshape(-1, 9)
    return g


def recovery_case(seed, n=400, extra=0.3):
    """(fixed, moving, R, s, t, n): moving = n records plus 30 % unrelated ones; fixed = the n mapped by a random similarity
    plus 30 % unrelated ones, shuffled so the true partner of moving record i is not fixed record i"""
    rng = np.random.default_rng(seed)
    R, s, t = random_rotation(rng), float(rng.uniform(0.8, 1.25)), rng.uniform(-20, 20, 3)
    base = random_records(rng, n)
    fixed = np.concatenate([transform_records(base, R, s, t), random_records(rng, int(extra * n))])
    perm = rng.permutation(len(fixed))
    fixed = fixed[perm]
    moving = np.concatenate([base, random_records(rng, int(extra * n))])
    partner = np.full(len(moving), -1)
    partner[:n] = np.argsort(perm)[:n]
    return fixed, moving, R, s, t, n, partner
