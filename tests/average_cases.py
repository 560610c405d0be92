"""Shared pieces of the template tests (test_average_cpu.py, test_gpu_average.py): the CPU oracle
tests/average_oracle.c, the contract restated with float64 numpy, the stage sift3d_average_warped restated on the oracle, the image
groups of the kernel tests, the shapes with what kernels_average.hip's #defines make of them, and the five-image scenario."""
import ctypes as C
import math
import os
import re

import numpy as np

from _helpers import c_oracle
from blockmatch_cases import volume
from invert_cases import forward_field
from register_cases import BIG, holes, map_of

KERNEL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3d_sift_cuda_amd", "csrc", "kernels_average.hip")
NAMES = ("AVG_THREADS", "AVG_MAX_BLOCKS", "AVG_MAX_IMAGES", "AVG_GROUP4_MAX", "AVG_GROUP2_MAX")
BRICK = (4, 8, 32)                # warp_device.h's brick of output voxels (z, y, x)
CAP = 1024                        # workgroups of a launch
SHAPES = [(1, 1, 1), (2, 3, 4), (5, 9, 33), (11, 19, 70)]     # nz, ny, nx: 1 voxel; 24; a brick plus one voxel per axis; several partial bricks
COUNTS = (1, 2, 5, 32)
GROUP_EDGES = (8, 9, 16, 17)      # the image counts either side of the two thresholds between the kernel's three instantiations
TRIMS = (0, 1, 15)
MAP_KINDS = ("identity", "shift", "half", "rotation", "outside")   # register_cases.map_of; a NaN entry cannot pass sift3d_resample_map: a refusal
FV = np.array([[0.0, -0.9, 0.0, 12.5], [1.1, 0.0, 0.0, -3.0], [0.0, 0.0, 1.25, 7.25], [0, 0, 0, 1]], np.float32)   # a permutation, anisotropic voxels
assert BIG == (33, 257, 253)


def kernel_constants(path=KERNEL):
    """{name: int} of NAMES: each `#define NAME integer` of the kernel file"""
    text = open(path).read()
    out = {}
    for name in NAMES:
        m = re.findall(r"^#define[ \t]+%s[ \t]+(\d+)[ \t]*(?:/\*.*)?$" % name, text, re.M)
        assert len(m) == 1, "%s is defined %d times in %s" % (name, len(m), path)
        out[name] = int(m[0])
    return out


def bricks(shape):
    return math.prod(-(-n // b) for n, b in zip(shape, BRICK))


def bits32(x):
    return np.ascontiguousarray(x).view(np.uint32)


class AverageOracle:
    def __init__(self, tmpdir):
        L = c_oracle("average_oracle", tmpdir)
        P, I64, F, I = C.c_void_p, C.c_int64, C.c_float, C.c_int
        L.oav_warp.restype = I
        L.oav_warp.argtypes = [P, I64, I64, I64, P, I64, I64, I64, P, P, P, P, P, P, F]
        L.oav_average.restype = I
        L.oav_average.argtypes = [I, P, I64, I, I, F, P, P, P]
        L.oav_counts.restype = None
        L.oav_counts.argtypes = [P, I64, I, I, P]
        L.oav_mean_field.restype = None
        L.oav_mean_field.argtypes = [I, P, I64, P]
        self.L = L

    def warp(self, vol, out_shape, A, Cm=None, K=None, field=None):
        """one image on the grid out_shape (nz, ny, nx): linear, fill NaN; through the field where one is given"""
        v = np.ascontiguousarray(vol, np.float32)
        nz, ny, nx = v.shape
        oz, oy, ox = out_shape
        out = np.empty(out_shape, np.float32)
        a = np.ascontiguousarray(A, np.float32).reshape(12)
        if field is None:
            rc = self.L.oav_warp(v.ctypes.data, nx, ny, nz, out.ctypes.data, ox, oy, oz, a.ctypes.data, None, None, None, None, None, 1.0)
        else:
            c, k = np.ascontiguousarray(Cm, np.float32).reshape(12), np.ascontiguousarray(K, np.float32).reshape(9)
            n, o = np.array(field["n"], np.int64), np.ascontiguousarray(field["origin"], np.float32)
            d = np.ascontiguousarray(field["disp"], np.float32)
            rc = self.L.oav_warp(v.ctypes.data, nx, ny, nz, out.ctypes.data, ox, oy, oz, a.ctypes.data, c.ctypes.data, k.ctypes.data, d.ctypes.data, n.ctypes.data,
                                 o.ctypes.data, float(field["spacing"]))
        assert rc == 0
        return out

    def average(self, planes, trim=0, min_count=1, fill=np.nan):
        """(avg, var, mask) of K warped planes of one shape"""
        p = np.ascontiguousarray(np.stack([np.asarray(a, np.float32) for a in planes]))
        shape = p.shape[1:]
        avg, var, mask = np.empty(shape, np.float32), np.empty(shape, np.float32), np.empty(shape, np.uint32)
        rc = self.L.oav_average(len(p), p.ctypes.data, int(np.prod(shape)), int(trim), int(min_count), float(fill), avg.ctypes.data, var.ctypes.data, mask.ctypes.data)
        assert rc == 0, rc
        return avg, var, mask

    def counts(self, mask, K, min_count=1):
        """the report's counts of a mask plane: a dict with none, below, count, contributing"""
        m, out = np.ascontiguousarray(mask, np.uint32), np.zeros(67, np.int64)
        self.L.oav_counts(m.ctypes.data, m.size, int(K), int(min_count), out.ctypes.data)
        return {"none": int(out[0]), "below": int(out[1]), "count": [int(v) for v in out[2:3 + K]], "contributing": [int(v) for v in out[35:35 + K]]}

    def mean_field(self, fields):
        d = np.ascontiguousarray(np.stack([np.asarray(f["disp"], np.float32).reshape(-1) for f in fields]))
        out = np.empty(d.shape[1], np.float32)
        self.L.oav_mean_field(len(d), d.ctypes.data, d.shape[1], out.ctypes.data)
        return out.reshape(np.asarray(fields[0]["disp"]).shape)


def warped_planes(pkg, ao, shape, images, grid_vox2key=None):
    """every image of an average_warped call on the grid, by the oracle: the maps are the host code's, as the stage takes them"""
    eye = np.eye(4, dtype=np.float32)
    out = []
    for a in images:
        A = pkg.resample_map(eye if a.get("t") is None else a["t"], grid_vox2key, a.get("vox2key"))
        Cm, K = pkg.field_warp_terms(grid_vox2key, a.get("vox2key"))
        out.append(ao.warp(a["image"], shape, A, Cm, K, a.get("field")))
    return out


def cpu_average(pkg, ao, shape, images, grid_vox2key=None, trim=0, min_count=1, fill=np.nan):
    """sift3d_average_warped restated: (avg, var, mask)"""
    return ao.average(warped_planes(pkg, ao, shape, images, grid_vox2key), trim, min_count, fill)


def same_planes(got, want):
    """every word of avg, var and mask equal"""
    for name, g, w in zip(("avg", "var", "mask"), got[:3], want[:3]):
        assert g.shape == w.shape and g.dtype == w.dtype, (name, g.shape, w.shape, g.dtype, w.dtype)
        diff = bits32(g) != bits32(w)
        assert not diff.any(), (name, int(diff.sum()), g[diff][:4], w[diff][:4])


# ---- the contract with float64 numpy: shares no code with the oracle ----------------------------------------------------------------
def average_numpy(planes, trim=0, min_count=1, fill=np.nan):
    """(avg, var, mask): sums added array by array, in image order and in rank order"""
    v = [np.asarray(p, np.float32) for p in planes]
    K, shape = len(v), v[0].shape
    inn = [np.isfinite(p) for p in v]
    d = [np.where(i, p, np.float32(0)).astype(np.float64) for i, p in zip(inn, v)]
    n = np.zeros(shape, np.int64)
    mask = np.zeros(shape, np.uint32)
    S = np.zeros(shape, np.float64)
    for k in range(K):
        n += inn[k]
        mask |= (inn[k].astype(np.uint32) << np.uint32(k))
        S = np.where(inn[k], S + d[k], S)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = S / n.astype(np.float64)
        V = np.zeros(shape, np.float64)
        for k in range(K):
            V = np.where(inn[k], V + (d[k] - m) * (d[k] - m), V)
        var = np.where(n > 1, V / (n - 1).astype(np.float64), 0.0).astype(np.float32)
        if trim == 0:
            avg = m.astype(np.float32)
        else:
            rank = []
            for k in range(K):
                r = np.zeros(shape, np.int64)
                for j in range(K):
                    r += inn[j] & ((v[j] < v[k]) | ((v[j] == v[k]) & (j < k)))
                rank.append(np.where(inn[k], r, -1))
            t = np.minimum(trim, (n - 1) // 2)
            T = np.zeros(shape, np.float64)
            for r in range(K):
                val = np.zeros(shape, np.float64)
                for k in range(K):
                    val = np.where(rank[k] == r, d[k], val)
                T = np.where((r >= t) & (r <= n - 1 - t), T + val, T)
            avg = (T / (n - 2 * t).astype(np.float64)).astype(np.float32)
    short = n < min_count
    return np.where(short, np.float32(fill), avg).astype(np.float32), np.where(short, np.float32(fill), var).astype(np.float32), mask


# ---- the groups of the kernel tests ------------------------------------------------------------------------------------------------
def matrix_of_map(A):
    """the moving -> fixed 4 x 4 whose sift3d_resample_map, under identity vox2key matrices, is (nearly) the 3 x 4 map A: its inverse"""
    M = np.vstack([np.asarray(A, np.float64).reshape(3, 4), [0, 0, 0, 1]])
    T = np.linalg.inv(M).astype(np.float32)
    T[3] = [0, 0, 0, 1]
    return T


def source_shape(shape, k):
    """the shape of image k of a group on the grid `shape`: the grid's, or one a few voxels off per axis"""
    off = [(0, 0, 0), (1, 2, -3), (-1, 3, 2), (2, -2, 5), (3, 1, -1)][k % 5]
    return tuple(max(1, n + o) for n, o in zip(shape, off))


def group(pkg, shape, K, fields="none", seed=0, kinds=MAP_KINDS, grid_vox2key=None, with_holes=True):
    """K images for pkg.average_warped on the grid `shape`: smooth volumes of differing shapes and scales with NaN and infinite voxels,
    the map kinds in turn (each later round moved a little), and fields: "none", "all", or "mixed" (spacing 4 for k % 3 == 0, spacing
    6 for k % 3 == 1, none for the others); every third image of a round with featExtract's voxel + 0.5 keys"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(K):
        s = source_shape(shape, k)
        v = (np.float32(1.0 + 0.1 * (k % 7)) * volume("smooth", s, seed + k) + np.float32(10.0 * k)).astype(np.float32)
        if with_holes and v.size > 1:
            v = holes(v, seed + 100 + k, 0.03)
        A = map_of(kinds[k % len(kinds)], shape, s).astype(np.float64)
        if k >= len(kinds):
            A = A + rng.normal(0, 0.02, (3, 4))
        a = {"image": v, "t": None if (kinds[k % len(kinds)] == "identity" and k < len(kinds)) else matrix_of_map(A)}
        if k % 3 == 2 and grid_vox2key is None:
            a["vox2key"] = pkg.key_vox2key()
        want = fields == "all" or (fields == "mixed" and k % 3 != 2)
        if want:
            grid = pkg.blockmatch_grid(shape, grid_vox2key, spacing=4.0 if k % 3 == 0 else 6.0)
            a["field"] = forward_field("smooth", grid, seed=seed + k, amp=1.5, wave=25.0)
        out.append(a)
    return out


# ---- the scenario: section 7j's world, one of five images wrong in every slab ------------------------------------------------------
def scenario(pkg, ro, tmp):
    """fuse_cases.scenario's world and five atlases, each keeping its 3-voxel displacement only in the FIRST of its wrong slabs, so that
    in every one of the target's five z slabs exactly one of the five images is misregistered.  Returns (target, grid vox2key, images)."""
    import fuse_cases
    s = fuse_cases.scenario(pkg, ro, tmp)
    grid = pkg.blockmatch_grid(fuse_cases.SHAPE, s["vox2key"], spacing=4.0)
    node_z = np.float64(grid["origin"][2]) + np.float64(grid["spacing"]) * np.arange(grid["n"][2])
    node_slab = np.clip(np.floor((node_z - 0.5) / (fuse_cases.SHAPE[0] / fuse_cases.SLABS)), 0, fuse_cases.SLABS - 1).astype(int)
    images = []
    for k, a in enumerate(s["atlases"]):
        field = forward_field("sine", grid, amp=0.4, wave=30.0 + 5.0 * k)
        field["disp"] = field["disp"].copy()
        wrong = node_slab == a["wrong_slabs"][0]
        for c in range(3):
            field["disp"][c, wrong] += np.float32(fuse_cases.WRONG[k][c])
        images.append({"image": a["image"], "t": a["t"], "vox2key": a["vox2key"], "field": field})
    assert sorted(a["wrong_slabs"][0] for a in s["atlases"]) == list(range(fuse_cases.SLABS))
    return s["target"], s["vox2key"], images


def rms(a, b, where):
    d = a.astype(np.float64)[where] - b.astype(np.float64)[where]
    return float(np.sqrt((d * d).mean()))
