"""Times the correlation cost of the block search against the SSD cost in one process, on the 512^3 pair
of bench_blockmatch.py (synth_blobs seed 12345; a 20-degree oblique copy with a 3-voxel sinusoidal warp, resampled through T).
For the correlation cost the warped volume's intensities are remapped (0.45 w + 310), which changes no time.
Device events around the search kernel alone, median of --reps launches after a warm-up, min and max beside it:
  block_match_kernel<4, 3, 1>      the SSD default form: what the others are held against, in this run
  block_match_ncc_kernel<4, 3>     the correlation cost, rows in registers, at the defaults
  block_match_kernel<4, 4, 1>, block_match_ncc_kernel<4, 4>   the same pair at r = 4
  block_match_ncc_kernel<0, 0>     the form for any b, r (--generic-reps launches)
and sift3d_refine_field_intensity_metric under both costs: wall time and the report's kernel times per round.
Prints one JSON line; --out also writes it."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--generic-reps", type=int, default=5)
    ap.add_argument("--stage-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("3d_sift_cuda_amd")
    n = a.size
    v = pkg.synth_blobs(n, n, n, seed=12345)
    A = oblique_map(n)
    m = pkg.resample_field(v, v.shape, A, sinus_field(n))
    T4 = np.vstack([np.asarray(A, np.float64).reshape(3, 4), [0, 0, 0, 1]]).astype(np.float32)   # m(x) = v(A x): moving x sits at fixed A x
    w = pkg.resample_affine(m, v.shape, pkg.resample_map(T4), fill=np.nan)
    w2, m2 = 0.45 * w + 310.0, 0.45 * m + 310.0   # float32; NaN stays NaN
    p = pkg.blockmatch_params()
    res = {"size": n, "stride": p.stride, "block": p.block}
    forms = (("ssd_4_3_1", pkg.block_match, w, 3, 0, a.reps), ("ncc_4_3", pkg.block_match_ncc, w2, 3, 0, a.reps),
             ("ssd_4_4_1", pkg.block_match, w, 4, 0, a.reps), ("ncc_4_4", pkg.block_match_ncc, w2, 4, 0, a.reps),
             ("ncc_0_0", pkg.block_match_ncc, w2, 3, 1, a.generic_reps))
    for name, fn, vol, search, generic, reps in forms:
        first, count = pkg.blockmatch_lattice(v.shape, search=search)
        words, _ = fn(v, vol, first, p.stride, count, p.block, search, generic=generic, return_ms=True)
        ms = [fn(v, vol, first, p.stride, count, p.block, search, generic=generic, return_ms=True)[1] for _ in range(reps)]
        res[name] = {"search": search, "nodes": int(np.prod(count)), "unflagged": int((words[..., 3] == 0).sum()), "kernel_ms": float(np.median(ms)),
                     "min_ms": min(ms), "max_ms": max(ms), "kernel_ms_all": ms}
        if name == "ncc_0_0":
            res[name]["same_words_as_ncc_4_3"] = bool(words.tobytes() == keep.tobytes())
        if name == "ncc_4_3":
            keep = words
    for r in ("3", "4"):
        res["ratio_ncc_over_ssd_r" + r] = res["ncc_4_" + r]["kernel_ms"] / res["ssd_4_%s_1" % r]["kernel_ms"]
    for metric, vol in (("ssd", m), ("ncc", m2)):
        pkg.refine_field_intensity(v, vol, T4, metric=metric)   # warm-up
        wall = []
        for _ in range(a.stage_reps):
            t0 = time.perf_counter()
            f, rep = pkg.refine_field_intensity(v, vol, T4, metric=metric)
            wall.append((time.perf_counter() - t0) * 1e3)
        rounds = rep["round"][:rep["rounds"]]
        kernels = sum(r["warp_ms"] + r["match_ms"] + r["fit_ms"][0] + r["fit_ms"][1] for r in rounds)
        res["stage_" + metric] = {"wall_ms": float(np.median(wall)), "wall_ms_all": wall, "kernel_ms": kernels,
                                  "host_ms": float(np.median(wall)) - kernels, "rounds": rounds}
    line = json.dumps(res, default=float)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
