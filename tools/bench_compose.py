"""Times the composition of two alignments on the 512^3 pair of bench_invert.py: synth_blobs seed 12345 and
a 20-degree oblique copy of it with a 3-voxel sinusoidal warp added.  The forward pair is (T, v): T the oblique map (keys in voxel
units), v the field sift3d_refine_field_intensity finds at the defaults (139^3 nodes); the inverse pair is (M', u) from
sift3d_invert_field.  The composite is Phi = phi o psi: pair 1 is the inverse pair (M', u), pair 2 the forward pair (T, v), on the
inverse's grid over the moving image (139^3 nodes): the inverse-consistency check of section 7h's inverse.
1. field_compose_kernel and compose_residual_kernel against field_invert_kernel on the same forward field, alternated in one
   loop: device events, medians of --reps launches after a warm-up.
2. sift3d_compose_field: wall time (a host clock around a call that ends in a device synchronise, median of --stage-reps after a
   warm-up) and its report.
--synthetic skips the 512^3 pair: sine fields on the same 139^3 grids (no block matching; for a quick look).
Prints one JSON line; --out also writes it."""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def sine_field(grid, amp=3.0, wave=80.0):
    n0, n1, n2 = grid["n"]
    o, h = np.asarray(grid["origin"], np.float64), float(grid["spacing"])
    z, y, x = np.meshgrid(o[2] + h * np.arange(n2), o[1] + h * np.arange(n1), o[0] + h * np.arange(n0), indexing="ij")
    s = 2 * np.pi / wave
    return dict(grid, disp=(amp * np.stack([np.sin(s * y), np.sin(s * z), np.sin(s * x)])).astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--stage-reps", type=int, default=3)
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("3d_sift_cuda_amd")
    n = a.size
    from bench_refine import oblique_map
    A = oblique_map(n)
    T4 = np.vstack([np.asarray(A, np.float64).reshape(3, 4), [0, 0, 0, 1]]).astype(np.float32)   # moving x sits at fixed A x
    if a.synthetic:
        field = sine_field(pkg.blockmatch_grid((n, n, n)))
    else:
        from bench_field import sinus_field
        v = pkg.synth_blobs(n, n, n, seed=12345)
        m = pkg.resample_field(v, v.shape, A, sinus_field(n))
        field, _ = pkg.refine_field_intensity(v, m, T4)
    res = {"size": n, "synthetic": bool(a.synthetic), "forward_nodes": list(field["n"])}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "m.trans.txt")
        pkg.write_matrix(path, pkg.affine_invert(T4))
        m_inv = pkg.read_similarity(path)
        igrid = pkg.invert_grid((n, n, n), None, spacing=float(field["spacing"]))
        inverse, irep = pkg.invert_field(T4, m_inv, field, igrid)
        # Phi = phi o psi on the inverse's grid: pair 1 = (M', u), pair 2 = (M, v)
        pkg.write_matrix(path, pkg.compose_matrix(m_inv, T4))
        mr = pkg.read_similarity(path)
        grid = pkg.compose_grid((n, n, n), None, inverse, field)
        # 1. the kernels, alternated with the inverse
        _, st, _, _ = pkg.compose_nodes(m_inv, T4, mr, inverse, field, grid, return_ms=True)
        pkg.invert_nodes(T4, m_inv, field, igrid)
        t = {"field_compose": [], "compose_residual": [], "field_invert": []}
        for _ in range(a.reps):
            ms = pkg.compose_nodes(m_inv, T4, mr, inverse, field, grid, return_ms=True)[3]
            t["field_compose"].append(ms[0])
            t["compose_residual"].append(ms[1])
            t["field_invert"].append(pkg.invert_nodes(T4, m_inv, field, igrid, return_ms=True)[3])
        res["kernels"] = {k: {"kernel_ms": float(np.median(x)), "kernel_ms_all": x} for k, x in t.items()}
        for k in ("field_compose", "compose_residual"):
            res["kernels"][k]["ratio_to_field_invert"] = res["kernels"][k]["kernel_ms"] / res["kernels"]["field_invert"]["kernel_ms"]
        res["grid"] = list(grid["n"])
        res["status_bits"] = [int(((st & b) != 0).sum()) for b in (1, 2, 4)]
        res["invert_report"] = irep
        # 2. the stage
        pkg.compose_field(m_inv, T4, mr, inverse, field, grid)
        wall = []
        for _ in range(a.stage_reps):
            t0 = time.perf_counter()
            _, rep = pkg.compose_field(m_inv, T4, mr, inverse, field, grid)
            wall.append((time.perf_counter() - t0) * 1e3)
        res["stage"] = {"wall_ms": float(np.median(wall)), "wall_ms_all": wall, "report": rep}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
