"""Shared pieces of the displacement field tests (test_field_cpu.py, test_gpu_field.py): the CPU oracle tests/field_oracle.c (built
with cc -O2 -ffp-contract=off into a temporary directory and bound with ctypes), a numpy restatement of the fit, the field stage
of DESIGN.md section 7e restated on the CPU, the sample sets, and the nonrigid scenario."""
import ctypes as C
import os
import subprocess

import numpy as np

from _helpers import c_oracle
from refine_cases import pos

SEARCH_RADIUS, SPACING, RADIUS, LAMBDA, MIN_TOL = 8.0, 4.0, 20.0, 0.1, 1.0   # sift3d_field_defaults


class FieldOracle:
    def __init__(self, tmpdir):
        L = c_oracle("field_oracle", tmpdir)
        P, I64, F = C.c_void_p, C.c_int64, C.c_float
        L.ofd_fit.restype = C.c_int
        L.ofd_fit.argtypes = [P, P, I64, P, F, P, F, F, P]
        L.ofd_eval.restype = None
        L.ofd_eval.argtypes = [P, P, P, F, P, I64, P]
        L.ofd_warp.restype = C.c_int
        L.ofd_warp.argtypes = [P, I64, I64, I64, P, I64, I64, I64, P, P, P, P, P, P, F, C.c_int, F, I64, I64]
        self.L = L

    def fit(self, y, v, grid, radius=RADIUS, lam=LAMBDA):
        """a field dict on grid (n, origin, spacing) from samples y, v (n x 3)"""
        y = np.ascontiguousarray(y, np.float32).reshape(-1, 3)
        v = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
        n = np.array(grid["n"], np.int64)
        o = np.ascontiguousarray(grid["origin"], np.float32)
        disp = np.empty(3 * int(np.prod(n)), np.float32)
        assert self.L.ofd_fit(y.ctypes.data, v.ctypes.data, len(y), o.ctypes.data, float(grid["spacing"]), n.ctypes.data, float(radius), float(lam),
                              disp.ctypes.data) == 0
        return {"n": tuple(int(x) for x in n), "origin": o.copy(), "spacing": np.float32(grid["spacing"]), "disp": disp.reshape(3, n[2], n[1], n[0])}

    def eval(self, field, y):
        y = np.ascontiguousarray(y, np.float32).reshape(-1, 3)
        n = np.array(field["n"], np.int64)
        o = np.ascontiguousarray(field["origin"], np.float32)
        d = np.ascontiguousarray(field["disp"], np.float32)
        out = np.empty_like(y)
        self.L.ofd_eval(d.ctypes.data, n.ctypes.data, o.ctypes.data, float(field["spacing"]), y.ctypes.data, len(y), out.ctypes.data)
        return out

    def warp(self, vol, out_shape, A, Cm, K, field, interp="linear", fill=0.0, z0=0, z1=None):
        v = np.ascontiguousarray(vol, np.float32)
        nz, ny, nx = v.shape
        oz, oy, ox = out_shape
        z1 = oz if z1 is None else z1
        out = np.empty((z1 - z0, oy, ox), np.float32)
        a, c, k = (np.ascontiguousarray(m, np.float32).reshape(-1) for m in (A, Cm, K))
        n = np.array(field["n"], np.int64)
        o = np.ascontiguousarray(field["origin"], np.float32)
        d = np.ascontiguousarray(field["disp"], np.float32)
        assert self.L.ofd_warp(v.ctypes.data, nx, ny, nz, out.ctypes.data, ox, oy, oz, a.ctypes.data, c.ctypes.data, k.ctypes.data, d.ctypes.data,
                               n.ctypes.data, o.ctypes.data, float(field["spacing"]), {"linear": 0, "nearest": 1}[interp], float(fill), z0, z1) == 0
        return out


def grid_numpy(y, h=SPACING, R=RADIUS):
    """the grid rule restated: o = (float)(min - R) in double, n = floor((max - min + 2R) / h) + 2"""
    y = np.asarray(y, np.float32).reshape(-1, 3)
    y = y[np.isfinite(y).all(1)].astype(np.float64)
    mn = y.min(0) if len(y) else np.zeros(3)
    mx = y.max(0) if len(y) else np.zeros(3)
    n = tuple(int(np.floor((mx[k] - mn[k] + 2.0 * float(np.float32(R))) / float(np.float32(h)))) + 2 for k in range(3))
    return {"n": n, "origin": (mn - float(np.float32(R))).astype(np.float32), "spacing": np.float32(h)}


def fit_numpy(y, v, grid, radius=RADIUS, lam=LAMBDA):
    """the fit restated in numpy, node by node block over all samples (float32 arithmetic, int64 sums)"""
    y = np.asarray(y, np.float32).reshape(-1, 3)
    v = np.asarray(v, np.float32).reshape(-1, 3)
    ok = np.isfinite(y).all(1) & np.isfinite(v).all(1)
    y, v = y[ok], v[ok]
    n0, n1, n2 = grid["n"]
    o, h = np.asarray(grid["origin"], np.float32), np.float32(grid["spacing"])
    c, b, a = np.meshgrid(np.arange(n2), np.arange(n1), np.arange(n0), indexing="ij")
    P = np.stack([o[0] + a.ravel().astype(np.float32) * h, o[1] + b.ravel().astype(np.float32) * h, o[2] + c.ravel().astype(np.float32) * h], 1)
    rr = np.float32(radius) * np.float32(radius)
    one, s24 = np.float32(1.0), np.float32(16777216.0)
    W = np.zeros(len(P), np.int64)
    V = np.zeros((len(P), 3), np.int64)
    for s in range(len(y)):
        d = y[s] - P
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        m = d2 < rr
        t = one - d2[m] / rr
        w = (t * t) * t
        W[m] += np.rint(w * s24).astype(np.int64)
        for k in range(3):
            V[m, k] += np.rint((w * v[s, k]) * s24).astype(np.int64)
    den = W.astype(np.float64) + float(np.float32(lam)) * 16777216.0
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(den[:, None] == 0, 0.0, V.astype(np.float64) / den[:, None]).astype(np.float32)
    return out.T.reshape(3, n2, n1, n0)


def sample_set(kind, seed, n, box=60.0):
    """(y, v) n x 3 float32: random (uniform), clustered (few centres), lattice (integer points, duplicates)"""
    rng = np.random.default_rng(seed)
    if kind == "random":
        y = rng.uniform(0, box, (n, 3))
    elif kind == "clustered":
        c = rng.uniform(0, box, (6, 3))
        y = c[rng.integers(0, 6, n)] + rng.normal(0, 2.0, (n, 3))
    else:
        y = rng.integers(0, 12, (n, 3)) * 3.0
    v = rng.uniform(-4, 4, (n, 3))
    return y.astype(np.float32), v.astype(np.float32)


def accept(i1, d1, i2, d2, ratio_num=4, ratio_den=5):
    """the accept rule of the guided re-matching restated (refine_cases.cpu_refine's): (moving, fixed) index arrays"""
    ok = (i1 >= 0) & ((i2 < 0) | (np.int64(ratio_num) * d2.astype(np.int64) > np.int64(ratio_den) * d1.astype(np.int64)))
    best = {}
    for m in np.nonzero(ok)[0]:
        f = int(i1[m])
        if f not in best or d1[m] < d1[best[f]]:
            best[f] = int(m)
    pm = np.array([m for m in np.nonzero(ok)[0] if best[int(i1[m])] == m], np.int64)
    return pm, i1[pm].astype(np.int64)


def local_residuals(fo, field, y, v):
    fit = fo.eval(field, y).astype(np.float64)
    d = np.asarray(v, np.float64) - fit
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def trim(e, min_tol=MIN_TOL):
    """keep e <= max(min_tol, 3 x the lower median)"""
    thr = max(float(min_tol), 3.0 * float(np.sort(e)[(len(e) - 1) // 2])) if len(e) else float(min_tol)
    return e <= thr


def cpu_field(pkg, fo, fixed, moving, t, search, spacing=SPACING, radius=RADIUS, lam=LAMBDA, min_tol=MIN_TOL, search_radius=SEARCH_RADIUS):
    """sift3d_refine_field restated: search(t, radius) -> (i1, d1, i2, d2); the product's sample helper, the oracle's fit and
    interpolation.  Returns (field dict, report dict without times)."""
    from refine_cases import rms
    i1, d1, i2, d2 = search(t, np.float32(search_radius))
    pm, pf = accept(i1, d1, i2, d2)
    y, v = pkg.field_samples(t, pos(fixed, pf), pos(moving, pm))
    grid = pkg.field_size(y, spacing=spacing, radius=radius)
    assert grid["n"] == grid_numpy(y, spacing, radius)["n"]
    f1 = fo.fit(y, v, grid, radius, lam)
    e = local_residuals(fo, f1, y, v)
    k = trim(e, min_tol)
    f2 = fo.fit(y[k], v[k], grid, radius, lam)
    e2 = local_residuals(fo, f2, y[k], v[k])
    folds, big = pkg.field_folds(t, f2)
    rep = {"accepted": len(pm), "kept": int(k.sum()), "rms_before": rms(e), "rms_after": rms(e2), "folds": folds, "max_disp": big}
    return f2, rep, (y, v, k)


# ---- the nonrigid scenario: the 20-degree case of refine_cases.scenario_volumes with a smooth warp of the content ---------------
AMP, WAVE = 3.0, 80.0


def warp_d(z):
    """d(z) in fixed voxels, z (..., 3) as (x, y, z)"""
    s = 2 * np.pi / WAVE
    return AMP * np.stack([np.sin(s * z[..., 1]), np.sin(s * z[..., 2]), np.sin(s * z[..., 0])], -1)


def trilinear(V, p):
    """V (nz, ny, nx) at positions p (..., 3) as (x, y, z), float64 arithmetic, 0 outside"""
    nz, ny, nx = V.shape
    out = np.zeros(p.shape[:-1])
    inside = (p[..., 0] >= 0) & (p[..., 0] <= nx - 1) & (p[..., 1] >= 0) & (p[..., 1] <= ny - 1) & (p[..., 2] >= 0) & (p[..., 2] <= nz - 1)
    q = p[inside]
    f = np.floor(q)
    w = q - f
    i0 = f.astype(np.int64)
    i1 = np.minimum(i0 + 1, np.array([nx - 1, ny - 1, nz - 1]))
    acc = 0.0
    for cz in (0, 1):
        for cy in (0, 1):
            for cx in (0, 1):
                ix = i1[:, 0] if cx else i0[:, 0]
                iy = i1[:, 1] if cy else i0[:, 1]
                iz = i1[:, 2] if cz else i0[:, 2]
                wt = (w[:, 0] if cx else 1 - w[:, 0]) * (w[:, 1] if cy else 1 - w[:, 1]) * (w[:, 2] if cz else 1 - w[:, 2])
                acc = acc + wt * V[iz, iy, ix]
    out[inside] = acc
    return out


def nonrigid_volumes(pkg, tmp, world):
    """(fixed path, moving path, V, M, A_true, vox_v, vox_m, hv, hm): scenario_volumes' fixed image and headers; the moving image
    M(x) = V(z + d(z)), z = A_true x, by numpy's trilinear interpolation"""
    from refine_cases import scenario_volumes
    from resample_cases import ResampleOracle
    fixed, moving, V, _M, A_true, vox_v, vox_m, hv, hm = scenario_volumes(pkg, ResampleOracle(tmp), tmp, world)
    N = _M.shape[0]
    M = np.empty((N, N, N), np.float32)
    y, x = np.meshgrid(np.arange(N, dtype=np.float64), np.arange(N, dtype=np.float64), indexing="ij")
    for k in range(N):
        p = np.stack([x, y, np.full_like(x, k)], -1)
        z = p @ A_true[:3, :3].T + A_true[:3, 3]
        M[k] = trilinear(V.astype(np.float64), z + warp_d(z)).astype(np.float32)
    pkg.write_nifti(moving, M, voxel=vox_m, qform=hm_q(world))
    return fixed, moving, V, M, A_true, vox_v, vox_m, hv, hm


def hm_q(world):
    return (-0.2, 0.05, 0.1, 10.0, -40.0, 25.0, -1.0) if world else None


def true_map(A_true, g):
    """x_true (moving voxels) of fixed voxels g (n x 3): z + d(z) = g by 40 fixed-point steps, x = A_true^-1 z"""
    z = g.astype(np.float64).copy()
    for _ in range(40):
        z = g - warp_d(z)
    inv = np.linalg.inv(A_true)
    return z @ inv[:3, :3].T + inv[:3, 3]


def lattice(n):
    return np.stack(np.meshgrid(*[np.arange(5, n - 5, 6)] * 3, indexing="ij"), -1).reshape(-1, 3)[:, ::-1].astype(np.float64)


def nonrigid_score(pkg, V, out, A, A_true, field=None, fv=None, mv=None):
    """(interior correlation, RMS map error, largest map error) over the lattice of scenario_score; the estimated map is
    A g + K v(C g) with the field, A g without"""
    n = V.shape[0]
    s = (slice(5, -5),) * 3
    c = np.corrcoef(out[s].ravel(), V[s].ravel())[0, 1]
    g = lattice(n)
    est = g @ np.asarray(A, np.float64)[:, :3].T + np.asarray(A, np.float64)[:, 3]
    if field is not None:
        Cm, K = pkg.field_warp_terms(fv, mv)
        kap = (g @ Cm[:, :3].astype(np.float64).T + Cm[:, 3].astype(np.float64)).astype(np.float32)
        est = est + pkg.field_eval(field, kap).astype(np.float64) @ K.astype(np.float64).T
    err = np.linalg.norm(est - true_map(A_true, g), axis=1)
    return float(c), float(np.sqrt(np.mean(err * err))), float(err.max())


def nonrigid_cpu(pkg, tmp, world):
    """The nonrigid scenario on the CPU alone: the oracle extraction, align_oracle's MatchKeys, refine_cases.cpu_refine, the
    field stage with the oracle search and fit, the warp oracle.  Returns {"refined": score, "field": score, "report": ...,
    "field_dict": ..., "T": ...}."""
    import _oracle
    from align_cases import AlignOracle
    from refine_cases import RefineOracle, cpu_refine, interval, scenario_map
    from resample_cases import ResampleOracle
    _oracle.build()
    ao, ro, rs, fo = AlignOracle(tmp), RefineOracle(tmp), ResampleOracle(tmp), FieldOracle(tmp)
    fixed, moving, V, M, A_true, vox_v, vox_m, hv, hm = nonrigid_volumes(pkg, tmp, world)
    opt = ["-w"] if world else []
    keys = []
    for src, name in ((fixed, "fixed.key"), (moving, "moving.key")):
        path = os.path.join(str(tmp), name)
        subprocess.run([_oracle.CLI] + opt + [src, path], check=True, capture_output=True)
        keys.append(pkg.match_filter(pkg.read_key(path)))
    F, Mk = keys
    lo, hi = interval()
    search = lambda t, r: ro.search(F, Mk, t, r, lo, hi)
    T, _kept, _rep = cpu_refine(F, Mk, ao.match_keys(F, Mk), search, pkg.fit_similarity)
    field, rep, _ = cpu_field(pkg, fo, F, Mk, T, search)
    fv = pkg.key_vox2key(vox_v, hv["qto_xyz"] if world else None)
    mv = pkg.key_vox2key(vox_m, hm["qto_xyz"] if world else None)
    A = scenario_map(pkg, pkg.similarity_matrix(T), world, vox_v, vox_m, hv, hm)
    Cm, K = pkg.field_warp_terms(fv, mv)
    res = {"report": rep, "field_dict": field, "T": T, "keys": (F, Mk)}
    res["refined"] = nonrigid_score(pkg, V, rs.resample(M, V.shape, A), A, A_true)
    res["field"] = nonrigid_score(pkg, V, fo.warp(M, V.shape, A, Cm, K, field), A, A_true, field, fv, mv)
    return res
