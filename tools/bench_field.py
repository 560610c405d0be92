"""Times the displacement field on two 512^3 extractions: synth_blobs seed 12345 and a 20-degree oblique
copy of it (bench_refine.py's map) with a 3-voxel sinusoidal warp added, made on the device with sift3d_resample_field.
1. sift3d_refine_field at the defaults (h = 4, R = 20) over sift3d_refine_similarity's transform: wall time (a host clock around
   calls that end in a device synchronise, median of --reps after a warm-up) and the fit kernel's device time per pass.
2. The linear warp 512^3 -> 512^3 through that field against sift3d_resample_affine on the same map: device events, runs
   alternated, medians of 25 after a warm-up.
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

from bench_refine import oblique_map  # noqa: E402


def sinus_field(n, amp=3.0, wave=80.0, h=4.0):
    """a field in voxel key units over the whole volume: v(y) = amp (sin 2pi y_y / wave, sin 2pi y_z / wave, sin 2pi y_x / wave)"""
    m = int(np.ceil((n + 16) / h)) + 1
    g = -8.0 + np.arange(m) * h
    s = 2 * np.pi / wave
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    d = amp * np.stack([np.sin(s * y), np.sin(s * z), np.sin(s * x)]).astype(np.float32)
    return {"n": (m, m, m), "origin": np.full(3, -8.0, np.float32), "spacing": np.float32(h), "disp": d}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warp-reps", type=int, default=25)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("3d_sift_cuda_amd")
    n = a.size
    v = pkg.synth_blobs(n, n, n, seed=12345)
    A = oblique_map(n)
    w = pkg.resample_field(v, v.shape, A, sinus_field(n))
    feats = []
    with pkg.Context(n, n, n, device=0) as ctx:
        for vol in (v, w):
            ctx.set_volume(vol)
            feats.append(ctx.extract())
    fixed, moving = feats
    t = pkg.refine_similarity(fixed, moving, pkg.match_keys(fixed, moving))[0]
    pkg.refine_field(fixed, moving, t)   # warm-up
    wall, fit0, fit1, search = [], [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        f, rep = pkg.refine_field(fixed, moving, t)
        wall.append((time.perf_counter() - t0) * 1e3)
        fit0.append(rep["fit_ms"][0])
        fit1.append(rep["fit_ms"][1])
        search.append(rep["search_ms"])
    # the warp against the affine resampler on the same map
    pkg.resample_field(w, v.shape, A, f, return_ms=True)
    pkg.resample_affine(w, v.shape, A, return_ms=True)
    warp_ms, aff_ms = [], []
    for _ in range(a.warp_reps):
        warp_ms.append(pkg.resample_field(w, v.shape, A, f, return_ms=True)[1])
        aff_ms.append(pkg.resample_affine(w, v.shape, A, return_ms=True)[1])
    med = lambda x: float(np.median(x))
    res = {"size": n, "n_fixed": len(fixed), "n_moving": len(moving), "nodes": list(f["n"]), "accepted": rep["accepted"], "kept": rep["kept"],
           "rms_before": rep["rms_before"], "rms_after": rep["rms_after"], "max_disp": rep["max_disp"], "folds": rep["folds"],
           "refine_field_wall_ms": med(wall), "refine_field_wall_ms_all": wall, "fit_kernel_ms_pass1": med(fit0), "fit_kernel_ms_pass2": med(fit1),
           "fit_kernel_ms_all": [fit0, fit1], "search_kernel_ms": med(search), "warp_linear_ms": med(warp_ms), "affine_linear_ms": med(aff_ms),
           "warp_over_affine": med(warp_ms) / med(aff_ms), "warp_ms_all": warp_ms, "affine_ms_all": aff_ms}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
