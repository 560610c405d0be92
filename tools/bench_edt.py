"""Times the exact distance map and the surface distances in one process.
The map: the sites are the surface of label 1 of bench_fuse.py's labels (four bands of the intensities of synth_blobs seed 12345) at
256^3 and at 512^3, for the spacings (1000, 1000, 1000) and (700, 700, 3000) um.  Device events around each of the three passes and
around all three, medians of --reps launches after a warm-up, min and max beside them, and the bytes each pass has to move (its input
once, its output once): x 1 + 2, y 2 + 8, z 8 + 8 bytes per voxel.  The yardstick, in the same run: a device-to-device copy of the
8 bytes per voxel map (torch, device events), which moves 16 bytes per voxel.
The stage: sift3d_surface_distances of the labels that two of bench_fuse.py's atlases fuse to against the target's own bands at 256^3,
wall time and the device time of its transform kernels.  Prints text lines and one JSON line; --out also writes them."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch  # before the library: one HIP runtime in the process

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_field import sinus_field  # noqa: E402
from bench_refine import oblique_map  # noqa: E402


def bands(vol):
    return np.digitize(vol, np.quantile(vol, [0.25, 0.5, 0.75])).astype(np.float32)


def surface(lab, l):
    """the surface voxels of the label l with numpy (section 7l's rule)"""
    c = np.pad(lab == l, 1)
    inner = c[1:-1, 1:-1, 1:-1]
    return inner & ~(c[:-2, 1:-1, 1:-1] & c[2:, 1:-1, 1:-1] & c[1:-1, :-2, 1:-1] & c[1:-1, 2:, 1:-1] & c[1:-1, 1:-1, :-2] & c[1:-1, 1:-1, 2:])


def copy_ms(nv, reps):
    """a device-to-device copy of nv 64-bit words: median, min, max in ms"""
    src = torch.arange(nv, dtype=torch.int64, device="cuda")
    dst = torch.empty_like(src)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps + 1):
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = ms[1:]
    return float(np.median(ms)), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--stage-size", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("3d_sift_cuda_amd")
    lines, res = [], {"reps": a.reps, "map": [], "copy": {}}

    def say(text):
        print(text, flush=True)
        lines.append(text)

    per_voxel = {"x": 3, "y": 10, "z": 16}
    for n in a.sizes:
        nv = n ** 3
        sites = surface(bands(pkg.synth_blobs(n, n, n, seed=12345)), 1)
        c = copy_ms(nv, a.reps)
        res["copy"][str(n)] = {"ms": c[0], "min_ms": c[1], "max_ms": c[2], "bytes": 16 * nv}
        rate = 16 * nv / c[0] / 1e6   # GB/s: bytes per ms / 10^6
        say("%d^3: %d sites (%.1f %%); copy of the 8 B/voxel map %.3f ms (%.3f - %.3f), %.0f GB/s" % (n, int(sites.sum()), 100.0 * sites.mean(), c[0], c[1], c[2], rate))
        for spacing in ((1000, 1000, 1000), (700, 700, 3000)):
            pkg.distance_map(sites, spacing)   # warm-up
            ms = np.array([pkg.distance_map(sites, spacing, return_ms=True)[1] for _ in range(a.reps)])
            med, lo, hi = np.median(ms, 0), ms.min(0), ms.max(0)
            row = {"size": n, "spacing_um": spacing, "total_ms": med[0], "x_ms": med[1], "y_ms": med[2], "z_ms": med[3], "min_ms": list(lo), "max_ms": list(hi)}
            res["map"].append(row)
            say("  spacing %s: all %.3f ms (%.3f - %.3f) = %.2f x the copy" % (spacing, med[0], lo[0], hi[0], med[0] / c[0]))
            for k, name in enumerate("xyz", 1):
                gbs = per_voxel[name] * nv / med[k] / 1e6
                say("    %s pass %.3f ms (%.3f - %.3f), %d B/voxel, %.0f GB/s = %.1f %% of the copy's rate" % (name, med[k], lo[k], hi[k], per_voxel[name], gbs,
                                                                                                              100.0 * gbs / rate))
    # the stage on fused labels against the target's own bands
    n = a.stage_size
    v = pkg.synth_blobs(n, n, n, seed=12345)
    A = oblique_map(n)
    m = pkg.resample_field(v, v.shape, A, sinus_field(n))
    T4 = np.vstack([np.asarray(A, np.float64).reshape(3, 4), [0, 0, 0, 1]]).astype(np.float32)
    field = sinus_field(n, amp=1.0)
    atlases = [{"image": m, "labels": bands(m), "t": T4, "field": field}] * 2
    words, _ = pkg.fuse_labels(v, atlases)
    fused = np.where(words[..., 0] & pkg.FUSE_NONE, np.float32(np.nan), (words[..., 0] & 0xffff).astype(np.float32)).astype(np.float32)
    truth = bands(v)
    pkg.surface_distances(fused, truth)   # warm-up
    wall, dev = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        rec, ms = pkg.surface_distances(fused, truth, return_ms=True)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(ms)
    res["stage"] = {"size": n, "labels": [r["label"] for r in rec], "wall_ms": float(np.median(wall)), "wall_ms_all": wall, "transform_ms": float(np.median(dev)),
                    "surface_voxels": [(r["n_a"], r["n_b"]) for r in rec], "hd95_mm": [r["hd95_mm"] for r in rec], "assd_mm": [r["assd_mm"] for r in rec]}
    say("stage at %d^3, labels %s: wall %.1f ms (%s), transform kernels %.2f ms for %d maps" % (n, res["stage"]["labels"], res["stage"]["wall_ms"],
                                                                                                 " ".join("%.1f" % w for w in wall), res["stage"]["transform_ms"], 2 * len(rec)))
    line = json.dumps(res, default=float)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write("\n".join(lines) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
