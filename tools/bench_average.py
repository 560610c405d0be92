"""Times the template from warped images in one process, K images of 256^3 onto a 256^3 grid by default.
Images: products of a few sines, each with a gain, an offset and a roll of its own, so that their order by value changes from voxel
to voxel.  Legs: "identity" (every image under the identity, no field) and "oblique" (every image under a rotation by 20 degrees
about an oblique axis through the centre, jittered per image, with a sine field of 1 voxel amplitude on a grid of spacing 4).
K = 8 and 32, trim 0, 1 and 15.  sift3d_average_warped's kernel_ms: device events around the one launch; wall_ms: the whole call,
uploads and downloads included.
The yardstick, in the same process on the same arrays: the K launches of the resampling kernel (identity leg) or of the field warp
kernel (oblique leg) that the unfused route needs before it has averaged anything, each by its own kernel_ms.  It is a lower bound of
that route, which also reads K volumes back and averages them.
After a warm-up of every case the cases and the yardstick are alternated --reps times; medians with min - max.  Bytes: every source
voxel and every field node once, three output planes once.  Prints text lines and one JSON line; --out also writes them."""
import argparse
import importlib
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COUNTS = (8, 32)
TRIMS = (0, 1, 15)


def sines(n):
    t = np.arange(n, dtype=np.float64) * (512.0 / n)
    v = (np.sin(0.0061 * 4 * t) * 1000.0)[None, None, :] * np.cos(0.0043 * 4 * t)[None, :, None] + (500.0 * np.sin(0.0037 * 4 * t))[:, None, None] * np.cos(0.0023 * 4 * t)[None, None, :]
    return np.ascontiguousarray(np.broadcast_to(v, (n, n, n)), np.float32)


def rotation(n, degrees, jitter):
    """4 x 4 moving -> fixed in voxel keys: a rotation about the axis (1, 2, 3) through the volume's centre, plus jitter (3 x 4)"""
    a, ax = math.radians(degrees), np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)
    c = np.full(3, (n - 1) / 2.0)
    M = np.vstack([np.concatenate([R, (c - R @ c)[:, None]], 1) + jitter, [0, 0, 0, 1]])
    return M.astype(np.float32)


def sine_field(grid, amp, wave, phase):
    n0, n1, n2 = (int(x) for x in grid["n"])
    o, h = np.asarray(grid["origin"], np.float64), float(grid["spacing"])
    z, y, x = np.meshgrid(o[2] + h * np.arange(n2), o[1] + h * np.arange(n1), o[0] + h * np.arange(n0), indexing="ij")
    s = 2 * np.pi / wave
    d = amp * np.stack([np.sin(s * y + phase), np.sin(s * z + phase), np.sin(s * x + phase)])
    return dict(grid, disp=np.ascontiguousarray(d, np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("3d_sift_cuda_amd")
    if pkg.device_count() <= 0:
        raise SystemExit("no HIP device: nothing is measured without one")
    n, shape = a.size, (a.size,) * 3
    rng = np.random.default_rng(3)
    base = sines(n)
    kmax = max(COUNTS)
    vols = [np.ascontiguousarray(np.float32(1.0 + 0.05 * rng.normal()) * np.roll(base, (int(rng.integers(-9, 10)), int(rng.integers(-9, 10)), int(rng.integers(-9, 10))), (0, 1, 2))
                                 + np.float32(40.0 * rng.normal())) for _ in range(kmax)]
    grid = pkg.blockmatch_grid(shape, None, spacing=4.0)
    legs = {"identity": [{"image": v} for v in vols],
            "oblique": [{"image": v, "t": rotation(n, 20.0, rng.normal(0, 1, (3, 4)) * [1e-3, 1e-3, 1e-3, 0.25]), "field": sine_field(grid, 1.0, 30.0 + k, 0.1 * k)}
                        for k, v in enumerate(vols)]}
    nodes = int(np.prod(grid["n"]))
    eye = np.eye(4, dtype=np.float32)
    cases = {(leg, K, trim): [] for leg in legs for K in COUNTS for trim in TRIMS}
    walls = {case: [] for case in cases}
    yard = {leg: [] for leg in legs}

    def once(case):
        leg, K, trim = case
        return pkg.average_warped(shape, legs[leg][:K], trim=trim)

    def yardstick(leg, keep=False):
        """kernel_ms of each image's own warp launch (and the warped volumes where they are kept)"""
        ms, out = [], []
        for im in legs[leg]:
            m = pkg.resample_map(im.get("t", eye), None, None)
            if "field" in im:
                w, t = pkg.resample_field(im["image"], shape, m, im["field"], None, None, "linear", float("nan"), return_ms=True)
            else:
                w, t = pkg.resample_affine(im["image"], shape, m, "linear", float("nan"), return_ms=True)
            ms.append(t)
            if keep and len(out) < min(COUNTS):
                out.append(w)
        return ms, out

    print("warm-up of %d cases" % (len(cases) + len(yard)), flush=True)
    for leg in legs:            # warm-up, and the mean of the smaller group held to the unfused route's volumes, averaged in float64 in image order
        _, warped = yardstick(leg, keep=True)
        for case in cases:
            if case[0] != leg:
                continue
            avg, var, mask, rep = once(case)
            if case[1] == min(COUNTS) and case[2] == 0:
                full = mask == (1 << case[1]) - 1
                S = np.zeros(shape, np.float64)
                for w in warped:
                    S = S + np.where(np.isfinite(w), w, 0).astype(np.float64)
                want = (S / float(case[1])).astype(np.float32)
                assert full.any() and np.array_equal(avg[full].view(np.uint32), want[full].view(np.uint32)), case
        del warped
    for r in range(a.reps):
        print("rep %d of %d" % (r + 1, a.reps), flush=True)
        for case in cases:
            rep = once(case)[3]
            cases[case].append(rep["kernel_ms"])
            walls[case].append(rep["wall_ms"])
        for leg in yard:
            yard[leg].append(yardstick(leg)[0])

    lines, res = [], {"size": n, "reps": a.reps, "yardstick": [], "cases": []}

    def say(text):
        print(text, flush=True)
        lines.append(text)

    stat = lambda ms: (float(np.median(ms)), float(min(ms)), float(max(ms)))
    ysum = {}
    for leg, runs in yard.items():
        for K in COUNTS:
            s = stat([sum(r[:K]) for r in runs])
            ysum[leg, K] = s[0]
            res["yardstick"].append({"leg": leg, "K": K, "sum_ms": s[0], "sum_min_ms": s[1], "sum_max_ms": s[2], "per_launch_ms": s[0] / K})
            say("%d^3 %-8s K %2d yardstick: %d warp launches = %.3f ms (%.3f - %.3f), %.3f ms each" % (n, leg, K, K, s[0], s[1], s[2], s[0] / K))
    for case, ms in cases.items():
        leg, K, trim = case
        m, w = stat(ms), stat(walls[case])
        nbytes = 4 * K * n ** 3 + 12 * n ** 3 + (16 * nodes * K if leg == "oblique" else 0)
        row = {"leg": leg, "K": K, "trim": trim, "ms": m[0], "min_ms": m[1], "max_ms": m[2], "of_yardstick": m[0] / ysum[leg, K], "bytes": nbytes,
               "gb_per_s": nbytes / m[0] / 1e6, "wall_ms": w[0]}
        res["cases"].append(row)
        say("  %-8s K %2d trim %2d: %8.3f ms (%.3f - %.3f); %.2f x the yardstick; %.1f MB, %.0f GB/s; the stage %.0f ms wall"
            % (leg, K, trim, m[0], m[1], m[2], row["of_yardstick"], nbytes / 1e6, row["gb_per_s"], w[0]))
    line = json.dumps(res, default=float)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write("\n".join(lines) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
