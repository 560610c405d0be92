"""Times the two launches of the intensity matching in one process, 256^3 volumes by default (--size 512 for 512^3).
Images: products of a few sines; the image is the reference with a gain, an offset and a roll.  Legs of the histogram launch
(sift3d_overlap_histograms' kernel_ms: device events around the one launch): "identity" (no field), "oblique" (a rotation by 20 degrees
about an oblique axis through the centre) and "oblique+field" (the same with a sine field of 1 voxel amplitude on a grid of spacing 4);
"background": the identity and the oblique leg again with a constant background over about 60 % of both volumes, where most waves
hold one bin and add once; and "noise": the two again on white noise, where neighbouring voxels share no bin, so that no thread merges a
run and every add is an LDS atomic of its own (what the merging and the one-bin path save shows as the textured legs against these).
The yardsticks, in the same process on the same arrays: one launch of the resampling kernel (identity, oblique) and one of the field
warp kernel (oblique+field), each by its own kernel_ms: they do the same sampling and also write a volume.
The apply launch (sift3d_apply_transfer's kernel_ms) with a table of 2 knots (linear), 65 (hist, Q = 64) and 257 (Q = 256), against a
device-to-device copy of the same bytes (torch, device events), 8 bytes per voxel either way.
After a warm-up of every case the cases and the yardsticks are alternated --reps times; medians with min - max.  Prints text lines and
one JSON line; --out also writes them."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_average import rotation, sine_field, sines  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch                                   # loaded first: the process keeps ONE HIP runtime, torch's
    pkg = importlib.import_module("3d_sift_cuda_amd")
    if pkg.device_count() <= 0:
        raise SystemExit("no HIP device: nothing is measured without one")
    n, shape = a.size, (a.size,) * 3
    R = sines(n)
    B = np.ascontiguousarray(np.float32(0.7) * np.roll(R, (3, -2, 5), (0, 1, 2)) + np.float32(150.0))
    Rb, Bb = R.copy(), B.copy()
    cut = int(round(n * (1 - 0.4 ** 0.5) / 2))      # a frame of that width on the y and x faces leaves 40 % of the volume textured
    for v, c in ((Rb, R.min()), (Bb, B.min())):
        v[:, :cut, :], v[:, n - cut:, :], v[:, :, :cut], v[:, :, n - cut:] = c, c, c, c
    rng = np.random.default_rng(7)
    Rn, Bn = rng.normal(0.0, 300.0, shape).astype(np.float32), rng.normal(150.0, 200.0, shape).astype(np.float32)
    grid = pkg.blockmatch_grid(shape, None, spacing=4.0)
    t, field = rotation(n, 20.0, 0.0), sine_field(grid, 1.0, 30.0, 0.1)
    eye = np.eye(4, dtype=np.float32)
    legs = {"identity": (R, {"image": B}), "oblique": (R, {"image": B, "t": t}), "oblique+field": (R, {"image": B, "t": t, "field": field}),
            "background identity": (Rb, {"image": Bb}), "background oblique": (Rb, {"image": Bb, "t": t}),
            "noise identity": (Rn, {"image": Bn}), "noise oblique": (Rn, {"image": Bn, "t": t})}
    ranges = {k: (pkg.blockmatch_range(r), pkg.blockmatch_range(im["image"])) for k, (r, im) in legs.items()}
    ha, hb, sums, _ = pkg.overlap_histograms(R, legs["oblique"][1], *ranges["oblique"])
    tables = {"linear, 2 knots": pkg.normalize_transfer("linear", ha, hb, sums, *ranges["oblique"]), "hist, 65 knots": pkg.normalize_transfer("hist", ha, hb, sums, *ranges["oblique"], 64),
              "hist, 257 knots": pkg.normalize_transfer("hist", ha, hb, sums, *ranges["oblique"], 256)}
    ca = torch.from_numpy(B).cuda()
    cb = torch.empty_like(ca)

    def hist(leg):
        r, im = legs[leg]
        return pkg.overlap_histograms(r, im, *ranges[leg], return_ms=True)

    def yardstick(leg):
        r, im = legs[leg]
        m = pkg.resample_map(im.get("t", eye), None, None)
        if "field" in im:
            return pkg.resample_field(im["image"], shape, m, im["field"], None, None, "linear", float("nan"), return_ms=True)[1]
        return pkg.resample_affine(im["image"], shape, m, "linear", float("nan"), return_ms=True)[1]

    def copy():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        cb.copy_(ca)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    yards = ("identity", "oblique", "oblique+field")
    times = {("hist", k): [] for k in legs}
    times.update({("yardstick", k): [] for k in yards})
    times.update({("apply", k): [] for k in tables})
    times["copy", ""] = []
    print("warm-up of %d cases" % len(times), flush=True)
    for kind, k in times:       # warm-up; every histogram leg counts a good part of the volume
        if kind == "hist":
            got = hist(k)
            assert got[2][0] > 0.3 * n ** 3, (k, got[2][0])
        elif kind == "yardstick":
            yardstick(k)
        elif kind == "apply":
            out = pkg.apply_transfer(B, tables[k])
            assert np.isfinite(out).all()
        else:
            copy()
    for r in range(a.reps):
        print("rep %d of %d" % (r + 1, a.reps), flush=True)
        for kind, k in times:
            times[kind, k].append(hist(k)[4] if kind == "hist" else yardstick(k) if kind == "yardstick" else pkg.apply_transfer(B, tables[k], return_ms=True)[1] if kind == "apply" else copy())

    lines, res = [], {"size": n, "reps": a.reps, "cases": []}

    def say(text):
        print(text, flush=True)
        lines.append(text)

    stat = lambda ms: (float(np.median(ms)), float(min(ms)), float(max(ms)))
    med = {key: stat(ms) for key, ms in times.items()}
    for (kind, k), (m, lo, hi) in med.items():
        row = {"kind": kind, "case": k, "ms": m, "min_ms": lo, "max_ms": hi}
        if kind == "hist":
            base = k.replace("background ", "").replace("noise ", "")
            row["of_yardstick"] = m / med["yardstick", base][0]
            if base != k:
                row["of_textured"] = m / med["hist", base][0]
            say("%d^3 hist      %-20s %8.3f ms (%.3f - %.3f); %.2f x its warp launch%s" % (n, k, m, lo, hi, row["of_yardstick"],
                                                                                        "; %.2f x the textured leg" % row["of_textured"] if "of_textured" in row else ""))
        elif kind == "yardstick":
            say("%d^3 yardstick %-20s %8.3f ms (%.3f - %.3f)" % (n, k, m, lo, hi))
        elif kind == "apply":
            row["of_copy"] = m / med["copy", ""][0]
            row["gb_per_s"] = 8 * n ** 3 / m / 1e6
            say("%d^3 apply     %-20s %8.3f ms (%.3f - %.3f); %.2f x the copy; %.0f GB/s" % (n, k, m, lo, hi, row["of_copy"], row["gb_per_s"]))
        else:
            row["gb_per_s"] = 8 * n ** 3 / m / 1e6
            say("%d^3 copy      %-20s %8.3f ms (%.3f - %.3f); %.0f GB/s" % (n, "device to device", m, lo, hi, row["gb_per_s"]))
        res["cases"].append(row)
    line = json.dumps(res, default=float)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write("\n".join(lines) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
