"""Times sift3d_resample_affine_dev (linear) at 512^3 -> 512^3 for four maps -- identity, an oblique rotation, scale 1/2 and
scale 2, each about the centre -- against a device-to-device copy in the same process.  Device events on one stream, a
warm-up of every case, then the cases and the copy alternated, the median of --reps runs each.

Compulsory bytes of a case: 4 B per output voxel written, plus 4 B per source voxel the map reaches (counted on the host:
source voxels whose preimage lies within one voxel of the output grid), read once.  The copy moves the same byte count:
hipMemcpyDtoD of half of it (read once, written once).  Prints one JSON line; --out also writes it (profiles/)."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def reached(A, src_shape, out_shape):
    """source voxels whose preimage under the 3 x 4 map A is within one voxel of the output box"""
    A4 = np.eye(4)
    A4[:3] = A.astype(np.float64)
    B = np.linalg.inv(A4)[:3]
    nz, ny, nx = src_shape
    oz, oy, ox = out_shape
    y, x = np.meshgrid(np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    n = 0
    for z in range(nz):
        p = [B[r, 0] * x + B[r, 1] * y + B[r, 2] * z + B[r, 3] for r in range(3)]
        n += int(((p[0] >= -1) & (p[0] <= ox) & (p[1] >= -1) & (p[1] <= oy) & (p[2] >= -1) & (p[2] <= oz)).sum())
    return n


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
    maps = {"identity": about_centre(np.eye(3), shape, shape), "oblique": about_centre(rot((1, 2, 3), 20.0), shape, shape, (0.3, -0.7, 0.2)),
            "scale_half": about_centre(0.5 * np.eye(3), shape, shape), "scale_2": about_centre(2.0 * np.eye(3), shape, shape)}
    byts = {k: 4 * n ** 3 + 4 * reached(A, shape, shape) for k, A in maps.items()}
    src = torch.from_numpy(pkg.synth_blobs(n, n, n, seed=2024)).cuda()
    dst = torch.empty_like(src)
    cbytes = max(byts.values()) // 2
    ca = torch.empty(cbytes // 4, dtype=torch.float32, device="cuda")
    cb = torch.empty_like(ca)
    stream = torch.cuda.Stream()
    times = {k: [] for k in list(maps) + ["copy"]}
    with pkg.Context(64, 64, 64) as ctx, torch.cuda.stream(stream):
        ctx.set_stream(stream.cuda_stream)

        def once(k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            if k == "copy":
                cb.copy_(ca)
            else:
                ctx.resample_affine_dev(src.data_ptr(), shape, dst.data_ptr(), shape, maps[k], "linear", 0.0)
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        for k in times:   # warm-up
            for _ in range(3):
                once(k)
        for _ in range(a.reps):
            for k in times:
                times[k].append(once(k))
        ctx.set_stream(0)
    med = {k: float(np.median(v)) for k, v in times.items()}
    copy_gbs = 2 * cbytes / med["copy"] / 1e6
    res = {"size": n, "reps": a.reps, "copy_bytes_moved": 2 * cbytes, "copy_ms": med["copy"], "copy_gbs": copy_gbs, "cases": {}}
    for k in maps:
        gbs = byts[k] / med[k] / 1e6
        res["cases"][k] = {"ms": med[k], "ms_min": float(np.min(times[k])), "ms_max": float(np.max(times[k])), "compulsory_bytes": byts[k],
                           "gbs": gbs, "of_copy_rate": gbs / copy_gbs}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
