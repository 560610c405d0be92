"""Shared pieces of the distance map and surface distance tests (test_edt_cpu.py, test_gpu_edt.py): the CPU
oracle tests/edt_oracle.c, the site patterns, the label pairs, the figures of a label restated in Python, and the stage
sift3d_surface_distances restated on the oracle's lists."""
import ctypes as C
import math

import numpy as np

from _helpers import c_oracle

NONE = 0xffffffffffffffff
SPACINGS = [(1000, 1000, 1000), (700, 1300, 3000), (1, 1, 65535), (65535, 65535, 65535)]
PATTERNS = ["none", "corner", "all", "plane", "random1", "random50"]


class EdtOracle:
    def __init__(self, tmpdir):
        L = c_oracle("edt_oracle", tmpdir)
        P, I64, I = C.c_void_p, C.c_int64, C.c_int
        L.oed_map.restype = I
        L.oed_map.argtypes = [P, I64, I64, I64, P, P]
        L.oed_surface.restype = I64
        L.oed_surface.argtypes = [P, I64, I64, I64, C.c_int32, P]
        L.oed_lists.restype = I
        L.oed_lists.argtypes = [P, P, I64, I64, I64, P, C.c_int32, P, P, P, P]
        self.L = L

    def map(self, sites, spacing):
        """the squared distances of sites (nz, ny, nx), uint64"""
        s = np.ascontiguousarray(np.asarray(sites) != 0, np.uint8)
        nz, ny, nx = s.shape
        d2 = np.empty(s.shape, np.uint64)
        assert self.L.oed_map(s.ctypes.data, nx, ny, nz, (C.c_uint32 * 3)(*spacing), d2.ctypes.data) == 0
        return d2

    def surface(self, labels, l):
        """the surface flags of the label l, uint8 (nz, ny, nx)"""
        v = np.ascontiguousarray(labels, np.float32)
        nz, ny, nx = v.shape
        flags = np.empty(v.shape, np.uint8)
        assert self.L.oed_surface(v.ctypes.data, nx, ny, nz, int(l), flags.ctypes.data) == int(flags.sum())
        return flags

    def lists(self, a, b, spacing, l):
        """(list a -> b, list b -> a) of the label l in voxel order, uint64"""
        a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
        nz, ny, nx = a.shape
        ab, ba = np.empty(a.size, np.uint64), np.empty(a.size, np.uint64)
        na, nb = C.c_int64(0), C.c_int64(0)
        assert self.L.oed_lists(a.ctypes.data, b.ctypes.data, nx, ny, nz, (C.c_uint32 * 3)(*spacing), int(l), ab.ctypes.data, C.byref(na), ba.ctypes.data,
                                C.byref(nb)) == 0
        return ab[:na.value].copy(), ba[:nb.value].copy()


# ---- the site patterns -------------------------------------------------------------------------------------------------------------
def sites(shape, pattern, seed=0):
    """uint8 (nz, ny, nx): none; one site in the last corner; every voxel; the middle plane across the longest axis; random at 1 %
    (at least one site) and at 50 %"""
    rng = np.random.default_rng(seed + 17 * shape[0] + 5 * shape[1] + shape[2])
    s = np.zeros(shape, np.uint8)
    if pattern == "corner":
        s[-1, -1, -1] = 1
    elif pattern == "all":
        s[:] = 1
    elif pattern == "plane":
        axis = int(np.argmax(shape))
        s[tuple(slice(None) if c != axis else shape[c] // 2 for c in range(3))] = 1
    elif pattern == "random1":
        s[rng.random(shape) < 0.01] = 1
        s.reshape(-1)[int(rng.integers(s.size))] = 1
    elif pattern == "random50":
        s[rng.random(shape) < 0.5] = 1
    else:
        assert pattern == "none"
    return s


def map_numpy(s, spacing):
    """the squared distances with numpy: every voxel against every site, in int64 (every value is below 2^58)"""
    s = np.asarray(s) != 0
    z, y, x = (c.astype(np.int64) for c in np.nonzero(np.ones(s.shape, bool)))
    sz, sy, sx = (c.astype(np.int64) for c in np.nonzero(s))
    if len(sx) == 0:
        return np.full(s.shape, NONE, np.uint64)
    d = (spacing[0] * (x[:, None] - sx[None])) ** 2 + (spacing[1] * (y[:, None] - sy[None])) ** 2 + (spacing[2] * (z[:, None] - sz[None])) ** 2
    return d.min(1).astype(np.uint64).reshape(s.shape)


# ---- the figures of one label ----------------------------------------------------------------------------------------------------------
def stats_python(ab, ba):
    """sift3d_surface_stats in Python integers and floats (IEEE double, one operation at a time; math.sqrt is correctly rounded)"""
    ab, ba = sorted(int(v) for v in ab), sorted(int(v) for v in ba)
    r = {"n_a": len(ab), "n_b": len(ba)}
    if not ab or not ba:
        r.update({k: NONE for k in ("max_ab", "max_ba", "p95_ab", "p95_ba")})
        r.update({k: math.nan for k in ("sum_ab", "sum_ba", "hausdorff_mm", "hd95_mm", "assd_mm")})
        return r
    for name, lst in (("ab", ab), ("ba", ba)):
        r["max_" + name], r["p95_" + name] = lst[-1], lst[(95 * len(lst) + 99) // 100 - 1]
        total = 0.0
        for v in lst:
            total += math.sqrt(float(v))
        r["sum_" + name] = total
    r["hausdorff_mm"] = math.sqrt(float(max(r["max_ab"], r["max_ba"]))) / 1000.0
    r["hd95_mm"] = math.sqrt(float(max(r["p95_ab"], r["p95_ba"]))) / 1000.0
    r["assd_mm"] = (r["sum_ab"] + r["sum_ba"]) / float(len(ab) + len(ba)) / 1000.0
    return r


def bits(v):
    """a double by its 64 bits, so that NaN compares equal to itself and -0.0 differs from 0.0"""
    return int(np.float64(v).view(np.uint64))


def same_record(got, want):
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for k, w in want.items():
        if isinstance(w, float):
            assert bits(got[k]) == bits(w), (k, got[k], w)
        else:
            assert int(got[k]) == int(w), (k, got[k], w)


def oracle_records(pkg, ed, a, b, spacing, first_label=1):
    """sift3d_surface_distances restated: the labels >= first_label of either volume, the oracle's lists of each pushed through the
    product's host helper sift3d_surface_stats (test_edt_cpu.py holds that one to stats_python)"""
    labels, ca, cb, _ = pkg.label_overlap(a, b)
    out = []
    for l, na, nb in zip(labels, ca, cb):
        if l < first_label:
            continue
        ab, ba = ed.lists(a, b, spacing, l)
        r = {"label": int(l), "voxels_a": int(na), "voxels_b": int(nb)}
        r.update(pkg.surface_stats(ab, ba))
        out.append(r)
    return out


def means(records):
    """(mean Hausdorff, mean HD95, mean ASSD, count) over the labels both volumes have"""
    both = [r for r in records if r["n_a"] > 0 and r["n_b"] > 0]
    if not both:
        return 0.0, 0.0, 0.0, 0
    return tuple(sum(r[k] for r in both) / len(both) for k in ("hausdorff_mm", "hd95_mm", "assd_mm")) + (len(both),)


def distance_block(records, spacing):
    """the distance block of <out>.fuse.txt and of featOverlap as label_report.c writes it"""
    t = "# spacing_um %d %d %d\n# label surf_fused surf_truth hausdorff_mm hd95_mm assd_mm\n" % tuple(spacing)
    for r in records:
        t += "%d\t%d\t%d\t%.6f\t%.6f\t%.6f\n" % (r["label"], r["n_a"], r["n_b"], r["hausdorff_mm"], r["hd95_mm"], r["assd_mm"])
    hd, hd95, assd, n = means(records)
    return t + "# mean hausdorff_mm %.6f hd95_mm %.6f assd_mm %.6f over %d labels\n" % (hd, hd95, assd, n)


# ---- the label pairs -------------------------------------------------------------------------------------------------------------------
def cube_pair():
    """label 1 on [4, 9]^3 of 16^3 and the same cube two voxels further along x"""
    a, b = np.zeros((16, 16, 16), np.float32), np.zeros((16, 16, 16), np.float32)
    a[4:10, 4:10, 4:10] = 1
    b[4:10, 4:10, 6:12] = 1
    return a, b


def blocky_pair(shape=(11, 19, 70), seed=5):
    """two label volumes of the labels 0, 1, 2, 7 and 65535 in blocks of 3 x 4 x 5 voxels, the second with its blocks one or two voxels
    off and some of them relabelled; NaN and infinite voxels scattered in both"""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    values = np.array([0, 1, 2, 7, 65535], np.float32)
    a = values[(x // 5 + 2 * (y // 4) + 3 * (z // 3)) % 5]
    b = values[((x + 2) // 5 + 2 * ((y + 1) // 4) + 3 * (z // 3)) % 5]
    b[rng.random(shape) < 0.05] = 2
    for vol in (a, b):
        at = rng.random(shape) < 0.03
        vol[at] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), int(at.sum()))
    return np.ascontiguousarray(a), np.ascontiguousarray(b)
