"""Times sift3d_resample_affine_dev in its three modes -- label-aware linear, linear and nearest -- at
512^3 -> 512^3 under the identity map and a 20-degree oblique rotation about the centre, on one label volume (labels 0 .. 4 in blobs).
Device events on one stream, a warm-up of every case, then the three modes alternated in one process, the median of --reps runs
each with its minimum and maximum.  The yardstick of label mode is the linear kernel of the same run: both issue eight gathers per
output voxel.  Prints one JSON line and a table; --out also writes them (profiles/)."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MODES = ("label", "linear", "nearest")
TARGET = 1.25   # label <= TARGET x linear, set before the first measurement


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from resample_cases import about_centre, rot
    pkg = importlib.import_module("3d_sift_cuda_amd")
    n = a.size
    shape = (n, n, n)
    maps = {"identity": about_centre(np.eye(3), shape, shape), "oblique": about_centre(rot((1, 2, 3), 20.0), shape, shape, (0.3, -0.7, 0.2))}
    blobs = pkg.synth_blobs(n, n, n, seed=2024)
    edges = np.quantile(blobs[::4, ::4, ::4], [0.5, 0.7, 0.85, 0.95])
    labels = np.digitize(blobs, edges).astype(np.float32)
    src = torch.from_numpy(labels).cuda()
    dst = torch.empty_like(src)
    stream = torch.cuda.Stream()
    times = {(k, m): [] for k in maps for m in MODES}
    with pkg.Context(64, 64, 64) as ctx, torch.cuda.stream(stream):
        ctx.set_stream(stream.cuda_stream)

        def once(k, m):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            ctx.resample_affine_dev(src.data_ptr(), shape, dst.data_ptr(), shape, maps[k], m, 0.0)
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        for key in times:   # warm-up
            for _ in range(3):
                once(*key)
        for _ in range(a.reps):
            for key in times:
                times[key].append(once(*key))
        ctx.set_stream(0)
    res = {"size": n, "reps": a.reps, "labels": int(labels.max()) + 1, "target": TARGET, "cases": {}}
    lines = ["map       mode     median ms   min ms   max ms   x linear"]
    for k in maps:
        lin = float(np.median(times[k, "linear"]))
        res["cases"][k] = {}
        for m in MODES:
            t = times[k, m]
            res["cases"][k][m] = {"ms": float(np.median(t)), "ms_min": float(np.min(t)), "ms_max": float(np.max(t)), "of_linear": float(np.median(t)) / lin}
            lines.append("%-9s %-8s %9.3f %8.3f %8.3f %9.3f" % (k, m, np.median(t), np.min(t), np.max(t), np.median(t) / lin))
        res["cases"][k]["target_met"] = bool(res["cases"][k]["label"]["of_linear"] <= TARGET)
        lines.append("%-9s label <= %.2f x linear: %s" % (k, TARGET, "met" if res["cases"][k]["target_met"] else "MISSED"))
    text = json.dumps(res) + "\n" + "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
