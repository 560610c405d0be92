"""Times the joint histogram of the image similarity in one process, at 512^3 by default.
The pairs: iid (two independent white-noise volumes: the lanes of a wave scatter over the cells), smooth (products of a few sines and
the same moved by one voxel along x on a scale of its own: the lanes of a wave land in a handful of cells) and one cell (one value but
for the two corner voxels that give the range: every add of the volume meets one LDS word and one result word).  Bins 64 and 32, both
flush forms, without labels and with 16 blocks of labels.  sift3d_image_similarity's kernel_ms: device events around its launches (the
result's memset, the kernel and, for the slices, the sum kernel).  After a warm-up of every case the cases and the yardstick are
alternated --reps times; medians with min - max.  The yardstick, in the same process: a device-to-device copy (torch, device events)
that moves the bytes the kernel must read, 8 per voxel without labels and 12 with them.  Prints text lines and one JSON line; --out
also writes them."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch  # before the library: one HIP runtime in the process

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sines(n, shift=0):
    """float32 (n, n, n): 1000 sin(0.0061 x) cos(0.0043 y) + 500 sin(0.0037 z) cos(0.0023 x), from 1-D factors: at 512^3 the 256 voxels of a wave span
    about a third of the range"""
    t = np.arange(n, dtype=np.float64)
    x = t + shift
    v = (np.sin(0.0061 * x) * 1000.0)[None, None, :] * np.cos(0.0043 * t)[None, :, None] + (500.0 * np.sin(0.0037 * t))[:, None, None] * np.cos(0.0023 * x)[None, None, :]
    return np.ascontiguousarray(np.broadcast_to(v, (n, n, n)), np.float32)


def pairs(n):
    rng = np.random.default_rng(24)
    iid = (rng.standard_normal((n, n, n), np.float32) * np.float32(30) + np.float32(100), rng.standard_normal((n, n, n), np.float32))
    smooth = (sines(n), (np.float32(0.37) * sines(n, 1) - np.float32(55)).astype(np.float32))
    one = np.full((n, n, n), 3.25, np.float32)
    one[0, 0, 0], one[-1, -1, -1] = 0.0, 10.0
    return {"iid": iid, "smooth": smooth, "one cell": (one, one.copy())}


def blocks_of_labels(n):
    """16 blocks: 4 along z, 2 along y, 2 along x"""
    z, y, x = np.arange(n)[:, None, None], np.arange(n)[None, :, None], np.arange(n)[None, None, :]
    return np.ascontiguousarray(np.broadcast_to((z * 4 // n) * 4 + (y * 2 // n) * 2 + x * 2 // n, (n, n, n)), np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("3d_sift_cuda_amd")
    n, nv = a.size, a.size ** 3
    vols, labels = pairs(n), blocks_of_labels(n)
    cases = {}
    for name in vols:
        for bins in (64, 32):
            for flush in ("slices", "atomics"):
                cases[(name, bins, flush, False)] = []
                cases[(name, bins, flush, True)] = []
    src, dst = torch.zeros(3 * nv // 2, dtype=torch.float32, device="cuda"), torch.empty(3 * nv // 2, dtype=torch.float32, device="cuda")
    copies = {8: [], 12: []}

    def copy_ms(bytes_per_voxel):
        k = nv * bytes_per_voxel // 8
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst[:k].copy_(src[:k])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def once(case):
        name, bins, flush, lab = case
        A, B = vols[name]
        return pkg.image_similarity(A, B, labels if lab else None, bins=bins, flush=flush)

    checks = {}
    print("warm-up of %d cases" % len(cases), flush=True)
    for case in cases:                       # warm-up; the two flush forms must agree to the last integer
        r = once(case)
        key = (case[0], case[1])
        if key in checks:
            assert np.array_equal(r["hist"], checks[key]["hist"]) and r["sums"] == checks[key]["sums"], case
        checks[key] = r
    for b in copies:
        copy_ms(b)
    for rep in range(a.reps):
        print("rep %d of %d" % (rep + 1, a.reps), flush=True)
        for case in cases:
            cases[case].append(once(case)["kernel_ms"])
        for b in copies:
            copies[b].append(copy_ms(b))

    lines, res = [], {"size": n, "reps": a.reps, "copy": {}, "cases": []}

    def say(text):
        print(text, flush=True)
        lines.append(text)

    stat = lambda ms: (float(np.median(ms)), float(min(ms)), float(max(ms)))
    for b, ms in copies.items():
        c = stat(ms)
        res["copy"][str(b)] = {"ms": c[0], "min_ms": c[1], "max_ms": c[2], "bytes": b * nv}
        say("%d^3: copy moving %d B/voxel %.3f ms (%.3f - %.3f), %.0f GB/s" % (n, b, c[0], c[1], c[2], b * nv / c[0] / 1e6))
    med = {}
    for case, ms in cases.items():
        name, bins, flush, lab = case
        m = stat(ms)
        med[case] = m[0]
        yard = res["copy"]["12" if lab else "8"]["ms"]
        r = checks[(name, bins)]
        res["cases"].append({"pair": name, "bins": bins, "flush": flush, "labels": lab, "ms": m[0], "min_ms": m[1], "max_ms": m[2], "of_copy": m[0] / yard,
                             "cells_filled": int((r["hist"] > 0).sum()), "mi": r["mi"], "rho": r["rho"]})
        say("  %-8s bins %2d %-7s %s: %.3f ms (%.3f - %.3f) = %.2f x the copy, %.2f Gvoxel/s; %d cells filled"
            % (name, bins, flush, "labels" if lab else "      ", m[0], m[1], m[2], m[0] / yard, nv / m[0] / 1e6, int((r["hist"] > 0).sum())))
    for bins in (64, 32):
        for flush in ("slices", "atomics"):
            for other in ("smooth", "one cell"):
                ratio = med[(other, bins, flush, False)] / med[("iid", bins, flush, False)]
                res.setdefault("ratios", []).append({"bins": bins, "flush": flush, "pair": other, "to_iid": ratio})
                say("  %s to iid, bins %d, %s: %.2f" % (other, bins, flush, ratio))
    line = json.dumps(res, default=float)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write("\n".join(lines) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
