"""Times the intensity refinement on the 512^3 pair of bench_field.py: synth_blobs seed 12345 and a
20-degree oblique copy of it with a 3-voxel sinusoidal warp added.  T is the oblique map itself (keys in voxel units), so
the sinusoid is what the stage has to find.
1. block_match_kernel at the defaults (stride 4, b 4, r 3) on the fixed volume and the moving volume resampled through T:
   device events, median of --reps launches after a warm-up, for the three forms of the kernel (specialised with packed differences,
   specialised with one multiply-add per instruction, and the form for any b, r); beside it the
   integer multiply-adds it performs (unflagged nodes x (2r + 1)^3 x (2b + 1)^3) as a rate and as a share of the plain and the
   packed 16-bit integer peaks (256 CUs x 128 lanes x 2.4 GHz x 1 or 2 multiply-adds per lane and clock).
2. sift3d_refine_field_intensity at the defaults: wall time (a host clock around a call that ends in a device synchronise,
   median of --stage-reps after a warm-up) and the report's kernel times per round (warp, quantise + search, the two fits).
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

PEAK_MAC_PLAIN = 256 * 128 * 2.4e9   # v_mad_i32_i24: one multiply-add per lane and clock
PEAK_MAC_PACKED16 = 2 * PEAK_MAC_PLAIN   # v_dot2_i32_i16: two


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=21)
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
    p = pkg.blockmatch_params()
    first, count = pkg.blockmatch_lattice(v.shape)
    res = {"size": n, "stride": p.stride, "block": p.block, "search": p.search, "nodes": int(np.prod(count))}
    for name, generic in (("specialised_packed", 0), ("specialised_plain", 2), ("generic", 1)):
        words, _ = pkg.block_match(v, w, first, p.stride, count, p.block, p.search, generic=generic, return_ms=True)
        ms = [pkg.block_match(v, w, first, p.stride, count, p.block, p.search, generic=generic, return_ms=True)[1] for _ in range(a.reps)]
        live = int((words[..., 3] == 0).sum())
        macs = live * (2 * p.search + 1) ** 3 * (2 * p.block + 1) ** 3
        t = float(np.median(ms)) * 1e-3
        res[name] = {"kernel_ms": float(np.median(ms)), "kernel_ms_all": ms, "unflagged": live, "macs": macs, "mac_per_s": macs / t,
                     "share_of_plain_peak": macs / t / PEAK_MAC_PLAIN, "share_of_packed16_peak": macs / t / PEAK_MAC_PACKED16}
    pkg.refine_field_intensity(v, m, T4)   # warm-up
    wall = []
    for _ in range(a.stage_reps):
        t0 = time.perf_counter()
        f, rep = pkg.refine_field_intensity(v, m, T4)
        wall.append((time.perf_counter() - t0) * 1e3)
    rounds = rep["round"][:rep["rounds"]]
    kernels = sum(r["warp_ms"] + r["match_ms"] + r["fit_ms"][0] + r["fit_ms"][1] for r in rounds)
    res["stage"] = {"wall_ms": float(np.median(wall)), "wall_ms_all": wall, "kernel_ms": kernels, "host_ms": float(np.median(wall)) - kernels,
                    "field_nodes": list(f["n"]), "rounds": rounds}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
