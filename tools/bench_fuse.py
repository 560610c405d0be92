"""Times the kernels of the label fusion in one process: a 256^3 target (synth_blobs seed 12345), K = 8
atlases, b = 2, both similarities.  Every atlas is the target's 20-degree oblique copy with a 3-voxel sinusoidal warp (the pair of
bench_blockmatch.py) under its own gain and offset, its labels four bands of its intensities, and its field a 1-voxel sine: equal
work per atlas, which is what a time needs.
Device events around each kernel alone, median of --reps launches after a warm-up, min and max beside it:
  field_warp_kernel<0>, <1>                  one atlas' intensities (linear) and labels (nearest) onto the target grid: what the new
                                             kernels are held against, in this run
  fuse_weight_kernel<2, 0>, <2, 1>           the sliding form, SSD and NCC
  fuse_weight_kernel<0, 0>, <0, 1>           the form for any b, at b = 2 and (NCC) at b = 6
  fuse_vote_kernel                           K = 8, powers 0 and 2
with the bytes each kernel has to move (its inputs once, its outputs once), and sift3d_fuse_labels under both similarities: wall time
and the report's device times.  Prints one JSON line; --out also writes it."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_field import sinus_field  # noqa: E402
from bench_refine import oblique_map  # noqa: E402


def timed(fn, reps):
    fn()
    ms = [fn()[1] for _ in range(reps)]
    return {"kernel_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms), "kernel_ms_all": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--atlases", type=int, default=8)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--generic-reps", type=int, default=3)
    ap.add_argument("--stage-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("3d_sift_cuda_amd")
    n, K = a.size, a.atlases
    nv = n ** 3
    v = pkg.synth_blobs(n, n, n, seed=12345)
    A = oblique_map(n)
    m = pkg.resample_field(v, v.shape, A, sinus_field(n))
    T4 = np.vstack([np.asarray(A, np.float64).reshape(3, 4), [0, 0, 0, 1]]).astype(np.float32)   # m(x) = v(A x): moving x sits at fixed A x
    lab = np.digitize(m, np.quantile(m, [0.25, 0.5, 0.75])).astype(np.float32)
    field = sinus_field(n, amp=1.0)
    amap = pkg.resample_map(T4)
    res = {"size": n, "atlases": K, "block": 2}
    warp = {"linear": timed(lambda: pkg.resample_field(m, v.shape, amap, field, interp="linear", fill=np.nan, return_ms=True), a.reps),
            "nearest": timed(lambda: pkg.resample_field(lab, v.shape, amap, field, interp="nearest", fill=np.nan, return_ms=True), a.reps)}
    for w in warp.values():
        w["bytes"] = 8 * nv + 16 * int(np.prod(field["n"]))   # the source once, the output once, the nodes once
    res["field_warp"] = warp
    w = pkg.resample_field(m, v.shape, amap, field, interp="linear", fill=np.nan)
    ml = pkg.resample_field(lab, v.shape, amap, field, interp="nearest", fill=np.nan)
    us = {}
    for name, metric, block, generic, reps in (("weight_2_ssd", "ssd", 2, 0, a.reps), ("weight_2_ncc", "ncc", 2, 0, a.reps),
                                               ("weight_any_ssd", "ssd", 2, 1, a.reps), ("weight_any_ncc", "ncc", 2, 1, a.reps),
                                               ("weight_any_ncc_b6", "ncc", 6, 1, a.generic_reps)):
        res[name] = timed(lambda: pkg.fuse_weights(v, w, block=block, metric=metric, generic=generic, return_ms=True), reps)
        res[name].update(block=block, bytes=6 * nv)   # qT and qW in, u out: 2 bytes each
        us[name] = pkg.fuse_weights(v, w, block=block, metric=metric, generic=generic)
        res[name]["mean_u"] = float(us[name].mean())
    for metric in ("ssd", "ncc"):
        res["weight_any_%s" % metric]["same_u_as_weight_2"] = bool(np.array_equal(us["weight_any_%s" % metric], us["weight_2_%s" % metric]))
    for power in (0, 2):
        res["vote_p%d" % power] = timed(lambda: pkg.fuse_vote([us["weight_2_ssd"]] * K, [ml] * K, power=power, return_ms=True), a.reps)
        res["vote_p%d" % power].update(bytes=(4 * K + 8) * nv)   # K planes of u and of labels in, two words out
    gains = [(1.0 + 0.1 * k, 25.0 * k) for k in range(K)]
    for metric in ("ssd", "ncc"):
        atlases = [{"image": (g * m + o).astype(np.float32) if metric == "ncc" else m, "labels": lab, "t": T4, "field": field} for g, o in gains]
        pkg.fuse_labels(v, atlases, metric=metric)   # warm-up
        wall = []
        for _ in range(a.stage_reps):
            t0 = time.perf_counter()
            words, rep = pkg.fuse_labels(v, atlases, metric=metric)
            wall.append((time.perf_counter() - t0) * 1e3)
        kernels = sum(r["warp_ms"] + r["weight_ms"] for r in rep["atlas"]) + rep["vote_ms"]
        res["stage_" + metric] = {"wall_ms": float(np.median(wall)), "wall_ms_all": wall, "kernel_ms": kernels, "vote_ms": rep["vote_ms"],
                                  "warp_ms_per_atlas": float(np.median([r["warp_ms"] for r in rep["atlas"]])),
                                  "weight_ms_per_atlas": float(np.median([r["weight_ms"] for r in rep["atlas"]])),
                                  "none": rep["none"], "fallback": rep["fallback"], "mean_conf": float(words[..., 1].mean() / 65535.0)}
    line = json.dumps(res, default=float)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
