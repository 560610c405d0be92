"""Shared pieces of the guided re-matching tests (test_refine_cpu.py, test_gpu_refine.py): the CPU oracle tests/refine_oracle.c
(a brute-force guided search, built with cc -O2 -ffp-contract=off into a temporary directory and bound with ctypes), a
restatement of the refinement loop of DESIGN.md section 7d in float64 numpy, and the constructed record sets."""
import ctypes as C
import os
import subprocess

import numpy as np

from _helpers import c_oracle
from align_cases import FEAT, LOG_1_5

INT32_MAX = 2 ** 31 - 1


class RefineOracle:
    def __init__(self, tmpdir):
        L = c_oracle("refine_oracle", tmpdir)
        P, I64, F = C.c_void_p, C.c_int64, C.c_float
        L.orf_search.restype = C.c_int
        L.orf_search.argtypes = [P, I64, P, I64, P, P, P, F, F, F, F, P, P, P, P]
        L.orf_predict.restype = None
        L.orf_predict.argtypes = [P, P, P, P, F, P]
        self.L = L

    def search(self, fixed, moving, t, radius, lo, hi):
        """(i1, d1, i2, d2) of every moving record; t: a dict with center0, center1, rot, scale"""
        f, m = np.ascontiguousarray(fixed, FEAT), np.ascontiguousarray(moving, FEAT)
        c0, c1 = (np.ascontiguousarray(t[k], np.float32).reshape(3) for k in ("center0", "center1"))
        rot = np.ascontiguousarray(t["rot"], np.float32).reshape(9)
        out = [np.empty(len(m), np.int32) for _ in range(4)]
        self.L.orf_search(f.ctypes.data, len(f), m.ctypes.data, len(m), c0.ctypes.data, c1.ctypes.data, rot.ctypes.data, float(t["scale"]),
                          float(radius), float(lo), float(hi), *[o.ctypes.data for o in out])
        return tuple(out)


def apply_d(t, p):
    """x_fixed = s rot (p - c0) + c1 in float64, each row summed ((r0 d0 + r1 d1) + r2 d2): the loop's host arithmetic"""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    R = np.asarray(t["rot"], np.float32).astype(np.float64).reshape(3, 3)
    c0 = np.asarray(t["center0"], np.float32).astype(np.float64)
    c1 = np.asarray(t["center1"], np.float32).astype(np.float64)
    s = float(np.float32(t["scale"]))
    d = p - c0
    q = np.empty_like(d)
    for r in range(3):
        q[:, r] = c1[r] + s * ((R[r, 0] * d[:, 0] + R[r, 1] * d[:, 1]) + R[r, 2] * d[:, 2])
    return q


def pos(recs, idx=None):
    r = recs if idx is None else recs[np.asarray(idx, np.int64)]
    return np.stack([r["x"], r["y"], r["z"]], 1).astype(np.float32)


def residuals(t, moving, fixed, pm, pf):
    q = apply_d(t, pos(moving, pm))
    f = pos(fixed, pf).astype(np.float64)
    d = q - f
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def rms(r):
    """sqrt(sum / n) with the sum taken in order (np.add.accumulate is sequential, as the C loop)"""
    r = np.asarray(r, np.float64)
    return float(np.sqrt(np.add.accumulate(r * r)[-1] / len(r))) if len(r) else 0.0


def corners(moving):
    p = pos(moving).astype(np.float64)
    p = p[np.isfinite(p).all(1)]
    if not len(p):
        return None
    mn, mx = p.min(0), p.max(0)
    return np.array([[mx[0] if c & 1 else mn[0], mx[1] if c & 2 else mn[1], mx[2] if c & 4 else mn[2]] for c in range(8)])


def cpu_refine(fixed, moving, init, search, fit, max_rounds=3, min_radius=1.0, max_radius=16.0, ratio_num=4, ratio_den=5, stop_shift=0.01):
    """The loop of DESIGN.md section 7d restated: search(t, radius) -> (i1, d1, i2, d2); fit(p_moving, p_fixed, center0) ->
    dict or None.  Returns (transform dict, kept (moving, fixed, dist2) arrays or None, report dict)."""
    cur = {k: init[k] for k in ("scale", "rot", "trans", "center0", "center1")}
    rep = {"rounds": 0, "stop": "rounds", "round": []}
    inl = np.asarray(init["inlier"], bool)
    r0 = residuals(cur, moving, fixed, np.asarray(init["moving_idx"])[inl], np.asarray(init["fixed_idx"])[inl]) if inl.any() else np.zeros(0)
    m0 = rms(r0)
    radius = max_radius if (not len(r0) or not np.isfinite(m0)) else min(max(3.0 * m0, min_radius), max_radius)
    if len(fixed) == 0 or len(moving) == 0:
        rep["stop"] = "none"
        return cur, None, rep
    box = corners(moving)
    kept = None
    for rnd in range(max_rounds):
        rad = np.float32(radius)
        R = {"radius": rad, "accepted": 0, "kept": 0, "rms": 0.0, "shift": 0.0}
        rep["round"].append(R)
        rep["rounds"] = rnd + 1
        i1, d1, i2, d2 = search(cur, rad)
        ok = (i1 >= 0) & ((i2 < 0) | (np.int64(ratio_num) * d2.astype(np.int64) > np.int64(ratio_den) * d1.astype(np.int64)))
        best = {}
        for m in np.nonzero(ok)[0]:
            f = int(i1[m])
            if f not in best or d1[m] < d1[best[f]]:
                best[f] = int(m)
        pm = np.array([m for m in np.nonzero(ok)[0] if best[int(i1[m])] == m], np.int64)
        pf, pd = i1[pm], d1[pm]
        R["accepted"] = len(pm)
        t1 = fit(pos(moving, pm), pos(fixed, pf), cur["center0"]) if len(pm) else None
        if t1 is None:
            rep["stop"] = "fit"
            break
        res = residuals(t1, moving, fixed, pm, pf)
        thr = 3.0 * np.sort(res)[(len(res) - 1) // 2]
        k = res <= thr
        t2 = fit(pos(moving, pm[k]), pos(fixed, pf[k]), cur["center0"])
        if t2 is None:
            rep["stop"] = "fit"
            break
        R["kept"] = int(k.sum())
        R["rms"] = rms(residuals(t2, moving, fixed, pm[k], pf[k]))
        if box is not None:
            a, b = apply_d(cur, box), apply_d(t2, box)
            d = b - a
            R["shift"] = float(np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).max())
        cur = t2
        kept = (pm[k].astype(np.int32), pf[k].astype(np.int32), pd[k].astype(np.int32))
        radius = min(float(rad), max(min_radius, 3.0 * R["rms"]))
        if R["shift"] < stop_shift:
            rep["stop"] = "converged"
            break
    return cur, kept, rep


def map_error(t, moving, R, s, tr):
    """largest displacement from the true map x -> s R x + tr at the eight corners of the moving records' box"""
    box = corners(moving)
    return float(np.abs(np.linalg.norm(apply_d(t, box) - (s * box @ np.asarray(R).T + tr), axis=1)).max())


def noisy_case(seed, n=400, sigma=0.3, extra=0.3):
    """align_cases.recovery_case with Gaussian position noise (sigma key units) on the fixed side"""
    from align_cases import recovery_case
    fixed, moving, R, s, t, n, partner = recovery_case(seed, n=n, extra=extra)
    rng = np.random.default_rng(seed + 1000)
    for k in ("x", "y", "z"):
        fixed[k] = fixed[k] + rng.normal(0, sigma, len(fixed)).astype(np.float32)
    return fixed, moving, R, s, t


def interval():
    """[lo, hi] of the ratio search (LOG_1_5) from the product's host helper"""
    import importlib
    return importlib.import_module("3d_sift_cuda_amd").log_ratio_interval(LOG_1_5)


# ---- the 20-degree oblique scenario of tests/test_gpu_resample.py::_end_to_end ------------------------------------------------
def scenario_volumes(pkg, rs, tmp, world):
    """(fixed path, moving path, V, M, A_true, vox_v, vox_m, hv, hm): the fixed blobs at 128^3 and the moving image, the fixed
    content moved by 20 degrees about an oblique axis and shifted (192^3, or 256^3 with -w headers); as _end_to_end"""
    from resample_cases import rot
    n, N = 128, 192
    V = pkg.synth_blobs(n, n, n, seed=31)
    if world:
        vox_v, q_v = (1.0, 1.25, 1.5), (0.1, 0.2, 0.3, -30.0, 20.0, 5.0, -1.0)
        vox_m, q_m = (1.0, 1.0, 1.0), (-0.2, 0.05, 0.1, 10.0, -40.0, 25.0, -1.0)
        N = 256
    else:
        vox_v = vox_m = (1.0, 1.0, 1.0)
        q_v = q_m = None
    fixed, moving = os.path.join(str(tmp), "fixed.nii"), os.path.join(str(tmp), "moving.nii")
    pkg.write_nifti(fixed, V, voxel=vox_v, qform=q_v)
    pkg.write_nifti(moving, np.zeros((1, 1, 1), np.float32), voxel=vox_m, qform=q_m)
    _, hv = pkg.read_nifti(fixed)
    _, hm = pkg.read_nifti(moving)
    Wv = hv["qto_xyz"].astype(np.float64) if world else np.eye(4)
    Wm = hm["qto_xyz"].astype(np.float64) if world else np.eye(4)
    R = rot((1, 2, 3), 20.0)
    cV = (Wv @ np.append(np.full(3, (n - 1) / 2), 1))[:3]
    cM = (Wm @ np.append(np.full(3, (N - 1) / 2), 1))[:3]
    G = np.eye(4)
    G[:3, :3] = R
    G[:3, 3] = cV + np.array([3.5, -2.25, 4.0]) - R @ cM
    A_true = np.linalg.inv(Wv) @ G @ Wm
    M = rs.resample(V, (N, N, N), A_true[:3].astype(np.float32))
    pkg.write_nifti(moving, M, voxel=vox_m, qform=q_m)
    return fixed, moving, V, M, A_true, vox_v, vox_m, hv, hm


def scenario_score(pkg, V, out, A, A_true):
    """(interior correlation, largest map error in voxels over the interior lattice), as _end_to_end measures them"""
    n = V.shape[0]
    s = (slice(5, -5),) * 3
    c = np.corrcoef(out[s].ravel(), V[s].ravel())[0, 1]
    inv = np.linalg.inv(A_true)
    g = np.stack(np.meshgrid(*[np.arange(5, n - 5, 6)] * 3, indexing="ij"), -1).reshape(-1, 3)[:, ::-1].astype(np.float64)
    g1 = np.concatenate([g, np.ones((len(g), 1))], 1)
    err = np.abs(g1 @ np.asarray(A, np.float64).T - (g1 @ inv.T)[:, :3]).max()
    return float(c), float(err)


def scenario_map(pkg, T, world, vox_v, vox_m, hv, hm):
    fv = pkg.key_vox2key(vox_v, hv["qto_xyz"] if world else None)
    mv = pkg.key_vox2key(vox_m, hm["qto_xyz"] if world else None)
    return pkg.resample_map(T, fv, mv)


def scenario_cpu(pkg, tmp, world):
    """The scenario on the CPU alone: the oracle's extraction (_oracle.CLI, which the GPU's extraction equals bit for bit),
    the command line's record filter, align_oracle's MatchKeys, the loop with the oracle search and the product's host fit,
    and the resample oracle.  Returns {"hough": (corr, err), "refined": (corr, err), "report": ...}."""
    import _oracle
    from align_cases import AlignOracle
    from resample_cases import ResampleOracle
    _oracle.build()
    ao, ro, rs = AlignOracle(tmp), RefineOracle(tmp), ResampleOracle(tmp)
    fixed, moving, V, M, A_true, vox_v, vox_m, hv, hm = scenario_volumes(pkg, rs, tmp, world)
    opt = ["-w"] if world else []
    keys = []
    for src, name in ((fixed, "fixed.key"), (moving, "moving.key")):
        path = os.path.join(str(tmp), name)
        subprocess.run([_oracle.CLI] + opt + [src, path], check=True, capture_output=True)
        keys.append(pkg.match_filter(pkg.read_key(path)))
    F, Mk = keys
    lo, hi = interval()
    init = ao.match_keys(F, Mk)
    cur, kept, rep = cpu_refine(F, Mk, init, lambda t, r: ro.search(F, Mk, t, r, lo, hi), pkg.fit_similarity)
    res = {"report": rep}
    for name, T in (("hough", init), ("refined", cur)):
        A = scenario_map(pkg, pkg.similarity_matrix(T), world, vox_v, vox_m, hv, hm)
        res[name] = scenario_score(pkg, V, rs.resample(M, V.shape, A), A, A_true)
    return res
