"""Times the joint histograms under K maps of the affine registration in one process, 256^3 into 256^3 by default.
The pair: products of a few sines and the same through a fold on a scale of its own.  Maps: the identity and a rotation by 7 degrees
about an oblique axis through the centre.  Bins 32 and 64, K = 1 and K = 24 (the rotation and 23 maps a small step away from it, as one
iteration of the search launches them), strides 1, 2 and 4, and the four forms: workgroups ordered by brick or by map, F read and
quantised per map or from an int16 lattice plane made once per call.  sift3d_warp_histogram's kernel_ms: device events around the
call's launches (the plane's kernel where there is one, the result's memset and the kernel).
The yardstick, in the same process on the same arrays: what a user had to run for ONE evaluation before this entry point --
sift3d_resample_affine's kernel (linear, fill NaN) plus sift3d_joint_histogram's kernel on its output, each by its own kernel_ms.  It has
no strided form: every stride is held against the whole-volume sum.
After a warm-up of every case the cases and the yardstick are alternated --reps times; medians with min - max.  Then the wall time of
a default 12-parameter registration of a 256^3 pair (blobs, folded, moved by a known 12-parameter map).  Prints text lines and one JSON
line; --out also writes them."""
import argparse
import importlib
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = ("by_brick", "by_map", "by_brick_plane", "by_map_plane")


def sines(n):
    t = np.arange(n, dtype=np.float64) * (512.0 / n)
    v = (np.sin(0.0061 * 4 * t) * 1000.0)[None, None, :] * np.cos(0.0043 * 4 * t)[None, :, None] + (500.0 * np.sin(0.0037 * 4 * t))[:, None, None] * np.cos(0.0023 * 4 * t)[None, None, :]
    return np.ascontiguousarray(np.broadcast_to(v, (n, n, n)), np.float32)


def rotation_map(n, degrees, jitter=None):
    """3 x 4: a rotation about the axis (1, 2, 3) through the volume's centre, plus jitter (3 x 4) where given"""
    a, ax = math.radians(degrees), np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)
    c = np.full(3, (n - 1) / 2.0)
    A = np.concatenate([R, (c - R @ c)[:, None]], 1)
    return (A if jitter is None else A + jitter).astype(np.float32)


def blobs_pair(pkg, n, seed=7):
    """(F, M, the true map): 60 separable Gaussian blobs; M = the fold |F - mid| resampled through the inverse of a known 12-parameter
    map (the product's resampler makes the test data, nothing that is timed)"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    F = np.zeros((n, n, n))
    for _ in range(60):
        c, s, a = rng.uniform(0, n - 1, 3), rng.uniform(2.5, 6.0) * n / 44.0, rng.uniform(0.4, 1.0)
        g = [np.exp(-(t - c[k]) ** 2 / (2 * s * s)) for k in range(3)]
        F += a * g[2][:, None, None] * g[1][None, :, None] * g[0][None, None, :]
    fold = np.abs(F - 0.5 * (F.min() + F.max()))
    F = (1000.0 * F + rng.normal(0, 10.0, F.shape)).astype(np.float32)
    theta = np.array([2.0, -1.5, 1.0, 0.04, -0.03, 0.05, 0.05, -0.04, 0.03, 0.03, -0.02, 0.015])
    theta[:3] *= n / 44.0
    true = pkg.register_map(theta, F.shape)                       # fixed voxel -> moving voxel
    inv = np.linalg.inv(np.vstack([true.astype(np.float64), [0, 0, 0, 1]]))[:3]
    M = pkg.resample_affine((1000.0 * fold).astype(np.float32), F.shape, inv, fill=0.0)
    M = (M + rng.normal(0, 10.0, M.shape)).astype(np.float32)
    return F, M, true


def corner_error(a, b, n):
    c = np.array([[x, y, z, 1.0] for x in (0, n - 1) for y in (0, n - 1) for z in (0, n - 1)])
    return float(np.sqrt((((np.asarray(a, np.float64) - np.asarray(b, np.float64)) @ c.T) ** 2).sum(0)).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("3d_sift_cuda_amd")
    if pkg.device_count() <= 0:
        raise SystemExit("no HIP device: nothing is measured without one")
    n = a.size
    F = sines(n)
    M = (np.float32(0.37) * np.abs(np.roll(F, 3, 2) - np.float32(100.0)) - np.float32(55.0)).astype(np.float32)
    fr, mr = pkg.blockmatch_range(F), pkg.blockmatch_range(M)
    rng = np.random.default_rng(3)
    maps = {"identity": np.stack([rotation_map(n, 0.0)] + [rotation_map(n, 0.0, rng.normal(0, 1, (3, 4)) * [1e-3, 1e-3, 1e-3, 0.25]) for _ in range(23)]),
            "rotated": np.stack([rotation_map(n, 7.0)] + [rotation_map(n, 7.0, rng.normal(0, 1, (3, 4)) * [1e-3, 1e-3, 1e-3, 0.25]) for _ in range(23)])}
    cases = {(kind, bins, K, stride, form): [] for kind in maps for bins in (32, 64) for K in (1, 24) for stride in (1, 2, 4) for form in FORMS}
    yard = {(kind, bins): [] for kind in maps for bins in (32, 64)}

    def once(case):
        kind, bins, K, stride, form = case
        return pkg.warp_histogram(F, M, maps[kind][:K], fr, mr, stride, bins, form=form, return_ms=True)

    def yardstick(key):
        kind, bins = key
        W, ms_warp = pkg.resample_affine(M, F.shape, maps[kind][0], fill=float("nan"), return_ms=True)
        out = pkg.joint_histogram(F, W, fr, mr, bins, return_ms=True)
        return out, ms_warp, out[3]

    print("warm-up of %d cases" % (len(cases) + len(yard)), flush=True)
    first = {}
    for case in cases:                        # warm-up; every form must give the same integers, and the yardstick's where it computes the same
        r = once(case)
        key = case[:4]
        if key in first:
            assert np.array_equal(r[0], first[key][0]) and r[1] == first[key][1] and r[3] == first[key][3], case
        first[key] = r
    for key in yard:
        out, _, _ = yardstick(key)
        r = first[(key[0], key[1], 1, 1)]
        assert np.array_equal(out[0], r[0][0]) and out[1] == r[1][0], key
    for rep in range(a.reps):
        print("rep %d of %d" % (rep + 1, a.reps), flush=True)
        for case in cases:
            cases[case].append(once(case)[4])
        for key in yard:
            _, w, h = yardstick(key)
            yard[key].append((w, h))

    lines, res = [], {"size": n, "reps": a.reps, "yardstick": [], "cases": []}

    def say(text):
        print(text, flush=True)
        lines.append(text)

    stat = lambda ms: (float(np.median(ms)), float(min(ms)), float(max(ms)))
    ysum = {}
    for key, ms in yard.items():
        w, h, s = stat([x[0] for x in ms]), stat([x[1] for x in ms]), stat([x[0] + x[1] for x in ms])
        ysum[key] = s[0]
        res["yardstick"].append({"map": key[0], "bins": key[1], "resample_ms": w[0], "joint_hist_ms": h[0], "sum_ms": s[0], "sum_min_ms": s[1], "sum_max_ms": s[2]})
        say("%d^3 %-8s bins %2d yardstick: resample %.3f ms + joint histogram %.3f ms = %.3f ms (%.3f - %.3f)" % (n, key[0], key[1], w[0], h[0], s[0], s[1], s[2]))
    med = {}
    for case, ms in cases.items():
        med[case] = stat(ms)
    for case, m in med.items():
        kind, bins, K, stride, form = case
        per_map = m[0] / K
        one = med[(kind, bins, 1, stride, form)][0]
        row = {"map": kind, "bins": bins, "K": K, "stride": stride, "form": form, "ms": m[0], "min_ms": m[1], "max_ms": m[2], "per_map_of_yardstick": per_map / ysum[(kind, bins)],
               "of_K_single_launches": m[0] / (K * one)}
        res["cases"].append(row)
        say("  %-8s bins %2d K %2d stride %d %-14s: %8.3f ms (%.3f - %.3f); per map %.2f x the two-step yardstick; %.2f x K single-map launches"
            % (kind, bins, K, stride, form, m[0], m[1], m[2], row["per_map_of_yardstick"], row["of_K_single_launches"]))

    # the wall time of a default registration
    Fb, Mb, true = blobs_pair(pkg, n)
    pkg.register_affine(Fb, Mb, levels=[(8, 1.0, 1.0)], max_iterations=1)          # warm-up
    t0 = time.perf_counter()
    r = pkg.register_affine(Fb, Mb)
    wall = time.perf_counter() - t0
    before, after = corner_error(true, pkg.register_map(np.zeros(12), Fb.shape), n), corner_error(true, r["map"], n)
    res["registration"] = {"wall_s": wall, "device_ms": sum(l["device_ms"] for l in r["levels"]), "corner_before": before, "corner_after": after,
                           "levels": [{k: l[k] for k in ("stride", "n_lattice", "iterations", "evaluations", "score_in", "score_out", "device_ms")} for l in r["levels"]]}
    say("%d^3 default 12-parameter registration: %.2f s wall, %.1f ms on the device; corner error %.2f -> %.2f voxels; %s"
        % (n, wall, res["registration"]["device_ms"], before, after,
           ", ".join("stride %d: %d iterations, %d evaluations, %.1f ms" % (l["stride"], l["iterations"], l["evaluations"], l["device_ms"]) for l in r["levels"])))
    line = json.dumps(res, default=float)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write("\n".join(lines) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
