"""Times the alignment path on the records of two 512^3 synthetic extractions, one shifted by (3, 9, 5) voxels:
sift3d_match_ratio (kernel time of the ratio search), the whole sift3d_match_keys (wall), and sift3d_knn64 with k = 2 on
the same descriptor sets, with the int8 rate of each (2 * 64 * n_q * n_db operations).  Prints one JSON line; --out also
writes it to a file (profiles/)."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("3d_sift_cuda_amd")
    n = a.size
    big = pkg.synth_blobs(n + 16, n + 16, n + 16, seed=2024)
    vols = [np.ascontiguousarray(big[:n, :n, :n]), np.ascontiguousarray(big[5:n + 5, 9:n + 9, 3:n + 3])]
    del big
    feats = []
    with pkg.Context(n, n, n, device=0) as ctx:
        for v in vols:
            ctx.set_volume(v)
            feats.append(ctx.extract())
    fixed, moving = feats
    ops = 2.0 * 64 * len(fixed) * len(moving)
    ratio_ms = []
    for _ in range(a.repeats):
        out = pkg.match_ratio(fixed, moving)
        ratio_ms.append(out[4])
    keys_ms = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        r = pkg.match_keys(fixed, moving)
        keys_ms.append((time.perf_counter() - t0) * 1e3)
    db, q = pkg.match_descriptors(fixed), pkg.match_descriptors(moving)
    knn_ms = pkg.knn64(db, q, 2, repeats=a.repeats + 1)[2]
    rm = float(np.median(ratio_ms))
    res = {"size": n, "n_fixed": len(fixed), "n_moving": len(moving), "ratio_kernel_ms": rm, "ratio_kernel_ms_all": ratio_ms,
           "ratio_tops": ops / rm / 1e9, "knn2_kernel_ms": knn_ms, "knn2_tops": ops / knn_ms / 1e9, "ratio_over_knn2": rm / knn_ms,
           "match_keys_wall_ms": float(np.median(keys_ms)), "match_keys_wall_ms_all": keys_ms, "n_matches": r["n_matches"],
           "inliers": r["inliers"], "scale": float(r["scale"]), "trans": [float(v) for v in r["trans"]]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
