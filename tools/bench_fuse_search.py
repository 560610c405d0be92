"""Times the local search of the label fusion in one process on bench_fuse.py's workload: a 256^3 target
(synth_blobs seed 12345), the atlas its 20-degree oblique copy with a 3-voxel sinusoidal warp brought back through a 1-voxel sine
field, its labels four bands of its intensities, b = 2.
Device events around each kernel alone, median of the launches after a warm-up, min and max beside it:
  fuse_weight_kernel<2, 0>, <2, 1>            section 7j's sliding form, SSD and NCC: the yardstick, in this run
  fuse_search_kernel<2, r, 0>, <2, r, 1>      the forms with b and r at compile time, r = 1, 2, 3
  fuse_search_kernel<0, 0, 0>, <0, 0, 1>      the form for any b, r at the same (b, r)
with the patch products per voxel each has to form, whether both forms gave the same words, and how far the search moved; then
sift3d_fuse_labels_search with K atlases (each under its own gain and offset for NCC) at r = 2 under both similarities beside
sift3d_fuse_labels: wall time and the reports' device times.  Prints one JSON line; --out also writes it."""
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
    ms = [fn()[-1] for _ in range(reps)]
    return {"kernel_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms), "kernel_ms_all": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--atlases", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--generic-reps", type=int, default=2)
    ap.add_argument("--stage-radius", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("3d_sift_cuda_amd")
    n, K = a.size, a.atlases
    v = pkg.synth_blobs(n, n, n, seed=12345)
    A = oblique_map(n)
    m = pkg.resample_field(v, v.shape, A, sinus_field(n))
    T4 = np.vstack([np.asarray(A, np.float64).reshape(3, 4), [0, 0, 0, 1]]).astype(np.float32)   # m(x) = v(A x): moving x sits at fixed A x
    lab = np.digitize(m, np.quantile(m, [0.25, 0.5, 0.75])).astype(np.float32)
    field = sinus_field(n, amp=1.0)
    amap = pkg.resample_map(T4)
    w = pkg.resample_field(m, v.shape, amap, field, interp="linear", fill=np.nan)
    ml = pkg.resample_field(lab, v.shape, amap, field, interp="nearest", fill=np.nan)
    res = {"size": n, "atlases": K, "block": 2}
    for metric in ("ssd", "ncc"):
        res["weight_2_" + metric] = timed(lambda: pkg.fuse_weights(v, w, block=2, metric=metric, return_ms=True), a.reps)
        for r in (1, 2, 3):
            words = {}
            for form, generic, reps in (("2_%d" % r, 0, a.reps), ("any", 1, a.generic_reps)):
                name = "search_%s_r%d_%s" % ("2" if generic == 0 else "any", r, metric)
                res[name] = timed(lambda: pkg.fuse_search(v, w, ml, block=2, radius=r, metric=metric, generic=generic, return_ms=True), reps)
                words[generic] = pkg.fuse_search(v, w, ml, block=2, radius=r, metric=metric, generic=generic)
                print("%s: %.3f ms" % (name, res[name]["kernel_ms"]), file=sys.stderr, flush=True)
                res[name].update(radius=r, products_per_voxel=(2 * r + 1) ** 3 * 125,
                                 against_weight_2=res[name]["kernel_ms"] / res["weight_2_" + metric]["kernel_ms"])
            u, shift, picked = words[0]
            voters, moved, d2 = pkg.fuse_shift_stats(r, shift)
            res["search_2_r%d_%s" % (r, metric)].update(voters=voters, moved=moved, mean_dist2=d2 / max(voters, 1),
                                                        mean_u=float(u[shift != pkg.FUSE_NO_SHIFT].mean()))
            res["search_any_r%d_%s" % (r, metric)]["same_words_as_search_2"] = bool(
                np.array_equal(words[1][0], u) and np.array_equal(words[1][1], shift) and np.array_equal(words[1][2], picked, equal_nan=True))
    gains = [(1.0 + 0.1 * k, 25.0 * k) for k in range(K)]
    for metric in ("ssd", "ncc"):
        atlases = [{"image": (g * m + o).astype(np.float32) if metric == "ncc" else m, "labels": lab, "t": T4, "field": field} for g, o in gains]
        for search in (0, a.stage_radius):
            pkg.fuse_labels(v, atlases, metric=metric, search=search)   # warm-up
            t0 = time.perf_counter()
            words, rep = pkg.fuse_labels(v, atlases, metric=metric, search=search)
            wall = (time.perf_counter() - t0) * 1e3
            out = {"wall_ms": wall, "kernel_ms": sum(x["warp_ms"] + x["weight_ms"] for x in rep["atlas"]) + rep["vote_ms"], "vote_ms": rep["vote_ms"],
                   "weight_ms_per_atlas": float(np.median([x["weight_ms"] for x in rep["atlas"]])), "none": rep["none"], "fallback": rep["fallback"],
                   "mean_conf": float(words[..., 1].mean() / 65535.0)}
            if search:
                out.update(search_ms_per_atlas=float(np.median([x["search_ms"] for x in rep["search"]["atlas"]])),
                           moved_per_atlas=float(np.median([x["moved"] for x in rep["search"]["atlas"]])))
            res["stage_%s_s%d" % (metric, search)] = out
    line = json.dumps(res, default=float)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
