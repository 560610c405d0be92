"""Times the reverse direction on the 512^3 pair of bench_blockmatch.py: synth_blobs seed 12345 and a
20-degree oblique copy of it with a 3-voxel sinusoidal warp added; T is the oblique map itself (keys in voxel units) and the
forward field is what sift3d_refine_field_intensity finds at the defaults.
1. field_invert_kernel on the default inverse grid: device events, median of --reps launches after a warm-up, and the
   distribution of the steps the nodes used.
2. sift3d_invert_field: wall time (a host clock around a call that ends in a device synchronise, median of --stage-reps after a
   warm-up) and its report.
3. both forms of jacobian_map_kernel against field_warp_kernel<0> (sift3d_resample_field) at the same size and through the same
   field, alternated in one loop: device events, medians.
4. with --cli: featResample -r -u against featResample -u on the same files, alternated, wall time of the processes (they read
   and write 512 MB images, so most of either is file work).
Prints one JSON line; --out also writes it."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import tempfile
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
    ap.add_argument("--stage-reps", type=int, default=3)
    ap.add_argument("--cli", type=int, default=0, help="repetitions of the two command lines (0: skip them)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("3d_sift_cuda_amd")
    n = a.size
    v = pkg.synth_blobs(n, n, n, seed=12345)
    A = oblique_map(n)
    m = pkg.resample_field(v, v.shape, A, sinus_field(n))
    T4 = np.vstack([np.asarray(A, np.float64).reshape(3, 4), [0, 0, 0, 1]]).astype(np.float32)   # m(x) = v(A x): moving x sits at fixed A x
    field, frep = pkg.refine_field_intensity(v, m, T4)
    res = {"size": n, "forward_nodes": list(field["n"]), "forward_rounds": frep["rounds"]}
    with tempfile.TemporaryDirectory() as tmp:
        inv_path = os.path.join(tmp, "inv.trans.txt")
        pkg.write_matrix(inv_path, pkg.affine_invert(T4))
        m_inv = pkg.read_similarity(inv_path)
        grid = pkg.invert_grid(m.shape, None, spacing=float(field["spacing"]))
        # 1. the kernel
        _, st, _, _ = pkg.invert_nodes(T4, m_inv, field, grid, return_ms=True)
        ms = [pkg.invert_nodes(T4, m_inv, field, grid, return_ms=True)[3] for _ in range(a.reps)]
        steps, state = (st & 0xffff).ravel(), (st >> 16).ravel()
        res["invert_kernel"] = {"nodes": int(st.size), "grid": list(grid["n"]), "kernel_ms": float(np.median(ms)), "kernel_ms_all": ms,
                                "steps_histogram": np.bincount(steps).tolist(), "steps_mean": float(steps.mean()),
                                "states": np.bincount(state, minlength=3).tolist()}
        # 2. the stage
        pkg.invert_field(T4, m_inv, field, grid)
        wall = []
        for _ in range(a.stage_reps):
            t0 = time.perf_counter()
            inv, rep = pkg.invert_field(T4, m_inv, field, grid)
            wall.append((time.perf_counter() - t0) * 1e3)
        res["stage"] = {"wall_ms": float(np.median(wall)), "wall_ms_all": wall, "report": rep}
        # 3. the Jacobian map's two forms and the warp, alternated
        Amap = pkg.resample_map(T4)
        for form in (0, 1):
            pkg.jacobian_map(v.shape, Amap, None, None, field, form=form)
        pkg.resample_field(m, v.shape, Amap, field)
        t = {"jacobian_plain": [], "jacobian_shared": [], "field_warp": []}
        for _ in range(a.reps):
            t["jacobian_plain"].append(pkg.jacobian_map(v.shape, Amap, None, None, field, form=0, return_ms=True)[1])
            t["jacobian_shared"].append(pkg.jacobian_map(v.shape, Amap, None, None, field, form=1, return_ms=True)[1])
            t["field_warp"].append(pkg.resample_field(m, v.shape, Amap, field, return_ms=True)[1])
        res["jacobian"] = {k: {"kernel_ms": float(np.median(x)), "kernel_ms_all": x} for k, x in t.items()}
        for k in ("jacobian_plain", "jacobian_shared"):
            res["jacobian"][k]["ratio_to_field_warp"] = res["jacobian"][k]["kernel_ms"] / res["jacobian"]["field_warp"]["kernel_ms"]
        # 4. the command lines
        if a.cli > 0:
            fixed, moving, fpath, trans = (os.path.join(tmp, x) for x in ("fixed.nii", "moving.nii", "fwd.field.nii", "fwd.trans.txt"))
            pkg.write_nifti(fixed, v)
            pkg.write_nifti(moving, m)
            # keys in voxel units sit at x + 0.5: T4 acts on voxel indices, the file's matrix on keys
            half = np.eye(4)
            half[:3, 3] = 0.5
            pkg.write_matrix(trans, (half @ T4.astype(np.float64) @ np.linalg.inv(half)).astype(np.float32))
            shifted = dict(field, origin=np.asarray(field["origin"], np.float32) + np.float32(0.5))
            pkg.write_field(fpath, shifted)
            cl = {"forward_u": [], "reverse_u": []}
            for _ in range(a.cli + 1):   # the first pair is the warm-up
                for name, opt, out in (("forward_u", [], "out_u.nii"), ("reverse_u", ["-r"], "out_r.nii")):
                    t0 = time.perf_counter()
                    subprocess.run([pkg.FEATRESAMPLE, "-d0"] + opt + ["-u", fpath, fixed, moving, trans, os.path.join(tmp, out)], check=True,
                                   capture_output=True, timeout=900)
                    cl[name].append((time.perf_counter() - t0) * 1e3)
            res["cli"] = {k: {"wall_ms": float(np.median(x[1:])), "wall_ms_all": x} for k, x in cl.items()}
            res["cli"]["ratio_reverse_to_forward"] = res["cli"]["reverse_u"]["wall_ms"] / res["cli"]["forward_u"]["wall_ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
