"""Times the guided re-matching on the records of two 512^3 extractions: synth_blobs seed 12345 and a
20-degree oblique copy of it made on the device with sift3d_resample_affine (about the centre, plus a shift); all records,
as tools/bench_align.py takes them (featMatchMultiple filters first, to about 80 %).  After a warm-up, sift3d_match_keys,
sift3d_refine_similarity and one sift3d_guided_search call (index build + one search, the fixed cost of a refinement) are
run alternately --reps times; the wall times (host clock around calls that end in a device synchronise) are medians.
Per round: the guided-search kernel's device time, the candidates it visited, and visited x 64 B of candidate rows over the
kernel time (only the rows of the candidates that pass the geometric test are read: an upper figure of the row traffic).  Prints one JSON line; --out also writes it."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def oblique_map(n, deg=20.0, axis=(1.0, 2.0, 3.0), shift=(3.5, -2.25, 4.0)):
    """output voxel -> source voxel: a rotation by deg about axis through the centre, then a shift"""
    a = np.asarray(axis, np.float64)
    a /= np.linalg.norm(a)
    t = np.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K
    c = np.full(3, (n - 1) / 2.0)
    A = np.zeros((3, 4))
    A[:, :3] = R
    A[:, 3] = c - R @ c + np.asarray(shift)
    return A.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("3d_sift_cuda_amd")
    n = a.size
    v = pkg.synth_blobs(n, n, n, seed=12345)
    w = pkg.resample_affine(v, v.shape, oblique_map(n))
    feats = []
    with pkg.Context(n, n, n, device=0) as ctx:
        for vol in (v, w):
            ctx.set_volume(vol)
            feats.append(ctx.extract())
    del v, w
    fixed, moving = feats
    init = pkg.match_keys(fixed, moving)        # warm-up of both paths
    pkg.refine_similarity(fixed, moving, init)
    keys_ms, refine_ms, search_ms = [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        init = pkg.match_keys(fixed, moving)
        keys_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        ref, rep = pkg.refine_similarity(fixed, moving, init)
        refine_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        pkg.guided_search(fixed, moving, init, 4.0)
        search_ms.append((time.perf_counter() - t0) * 1e3)
    rounds = [{"radius": float(r["radius"]), "kernel_ms": r["kernel_ms"], "visited": r["visited"], "accepted": r["accepted"], "kept": r["kept"],
               "rms": r["rms"], "shift": r["shift"], "row_bytes_per_s_upper": r["visited"] * 64.0 / (r["kernel_ms"] * 1e-3) if r["kernel_ms"] > 0 else None}
              for r in rep["round"]]
    km, rm = float(np.median(keys_ms)), float(np.median(refine_ms))
    res = {"size": n, "n_fixed": len(fixed), "n_moving": len(moving), "match_keys_wall_ms": km, "match_keys_wall_ms_all": keys_ms,
           "refine_wall_ms": rm, "refine_wall_ms_all": refine_ms, "refine_over_match_keys": rm / km,
           "guided_search_call_ms": float(np.median(search_ms)), "guided_search_call_ms_all": search_ms, "rounds": rounds, "stop": rep["stop"],
           "search_kernel_ms_max": max(r["kernel_ms"] for r in rounds), "hough_inliers": init["inliers"], "refined_kept": ref["inliers"],
           "hough_scale": float(init["scale"]), "refined_scale": float(ref["scale"])}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
