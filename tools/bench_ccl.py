"""Times the connected components and the island removal in one process.
The volumes, at 256^3 and at 512^3: the labels that two of bench_fuse.py's atlases fuse to (four bands of the intensities of
synth_blobs seed 12345, warped by an oblique map and a sine field), and the volume of one label alone, in which every brick border
joins what lies on its two sides: the border merge's worst case.  sift3d_label_components under connectivity 6: device events around
each of its five steps and around all of them, medians of --reps calls after a warm-up, min and max beside them.
sift3d_clean_labels at -v8 -c6 -r4: the device time of all its rounds, likewise, and the wall time of the call.  The yardstick, in the
same run: a device-to-device copy of the uint32 plane (torch, device events), which moves 8 bytes per voxel.  Prints text lines and
one JSON line; --out also writes them."""
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

from bench_edt import bands  # noqa: E402
from bench_field import sinus_field  # noqa: E402
from bench_refine import oblique_map  # noqa: E402

STEPS = ("all", "label plane", "brick pass", "border merge", "flatten", "numbers and records")


def copy_ms(nv, reps):
    """a device-to-device copy of nv 32-bit words: median, min, max in ms"""
    src = torch.arange(nv, dtype=torch.int32, device="cuda")
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


def fused_labels(pkg, n):
    v = pkg.synth_blobs(n, n, n, seed=12345)
    A = oblique_map(n)
    m = pkg.resample_field(v, v.shape, A, sinus_field(n))
    T4 = np.vstack([np.asarray(A, np.float64).reshape(3, 4), [0, 0, 0, 1]]).astype(np.float32)
    atlases = [{"image": m, "labels": bands(m), "t": T4, "field": sinus_field(n, amp=1.0)}] * 2
    words, _ = pkg.fuse_labels(v, atlases)
    return np.where(words[..., 0] & pkg.FUSE_NONE, np.float32(np.nan), (words[..., 0] & 0xffff).astype(np.float32)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("3d_sift_cuda_amd")
    lines, res = [], {"reps": a.reps, "components": [], "clean": [], "copy": {}}

    def say(text):
        print(text, flush=True)
        lines.append(text)

    for n in a.sizes:
        nv = n ** 3
        c = copy_ms(nv, a.reps)
        res["copy"][str(n)] = {"ms": c[0], "min_ms": c[1], "max_ms": c[2], "bytes": 8 * nv}
        say("%d^3: copy of the 4 B/voxel plane %.3f ms (%.3f - %.3f), %.0f GB/s" % (n, c[0], c[1], c[2], 8 * nv / c[0] / 1e6))
        for name, vol in (("fused", fused_labels(pkg, n)), ("one label", np.ones((n, n, n), np.float32))):
            _, rec = pkg.label_components(vol, 6)   # warm-up; it also tells the room the records need
            ms = np.array([pkg.label_components(vol, 6, max_records=len(rec), return_ms=True)[2] for _ in range(a.reps)])
            med, lo, hi = np.median(ms, 0), ms.min(0), ms.max(0)
            res["components"].append({"size": n, "volume": name, "components": len(rec), "largest": int(rec["voxels"].max()), "steps": STEPS, "ms": list(med),
                                      "min_ms": list(lo), "max_ms": list(hi)})
            say("  %s, %d components (largest %d voxels), connectivity 6: all %.3f ms (%.3f - %.3f) = %.2f x the copy, %.2f Gvoxel/s"
                % (name, len(rec), int(rec["voxels"].max()), med[0], lo[0], hi[0], med[0] / c[0], nv / med[0] / 1e6))
            for k in range(1, len(STEPS)):
                say("    %-19s %.3f ms (%.3f - %.3f) = %.2f x the copy" % (STEPS[k], med[k], lo[k], hi[k], med[k] / c[0]))
            pkg.clean_labels(vol)                   # warm-up
            dev, wall = [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                _, rep, t = pkg.clean_labels(vol, return_ms=True)
                wall.append((time.perf_counter() - t0) * 1e3)
                dev.append(t)
            res["clean"].append({"size": n, "volume": name, "rounds_run": rep["rounds_run"], "total": rep["total"], "ms": float(np.median(dev)), "min_ms": min(dev),
                                 "max_ms": max(dev), "wall_ms": float(np.median(wall))})
            say("    cleaning -v8 -c6 -r4: %d rounds, %d components resolved (%d voxels): %.3f ms (%.3f - %.3f) = %.2f x the copy; wall %.0f ms"
                % (rep["rounds_run"], rep["total"]["resolved"], rep["total"]["resolved_voxels"], np.median(dev), min(dev), max(dev), np.median(dev) / c[0], np.median(wall)))
    line = json.dumps(res, default=float)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write("\n".join(lines) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
