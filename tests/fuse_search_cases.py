"""Shared pieces of the tests of the label fusion's local search (test_fuse_search_cpu.py, test_gpu_fuse_search.py; DESIGN.md
section 7k): the CPU oracle tests/fuse_search_oracle.c, sift3d_fuse_search and the stage sift3d_fuse_labels_search restated on the
CPU, and the small volumes of the kernel tests.  Everything of section 7j comes from fuse_cases.py as it is."""
import ctypes as C

import numpy as np

from _helpers import c_oracle
from fuse_cases import ENDS_SHAPE, METRICS, NONE, FALLBACK, SUM_MAX_B6, FuseOracle, bright_pair, lattice3, pair, speckled_pair, stripes   # noqa: F401

NO_SHIFT = 0xffff


class FuseSearchOracle(FuseOracle):
    """tests/fuse_search_oracle.c: fuse_oracle.c's functions (it includes that file) and the search"""

    def __init__(self, tmpdir):
        FuseOracle.__init__(self, tmpdir)
        S = c_oracle("fuse_search_oracle", tmpdir)
        P, I64, I = C.c_void_p, C.c_int64, C.c_int
        S.ofs_shift_code.restype = I
        S.ofs_shift_code.argtypes = [I] * 4
        S.ofs_search.restype = I
        S.ofs_search.argtypes = [P, P, P, I64, I64, I64, I, I, I, P, P, P, P]
        S.ofs_search_sat.restype = I
        S.ofs_search_sat.argtypes = [P, P, P, I64, I64, I64, I, I, I, P, P, P]
        self.S = S

    def code(self, r, t):
        return int(self.S.ofs_shift_code(int(r), int(t[0]), int(t[1]), int(t[2])))

    def search_q(self, qt, qw, labels, b, r, metric, sums=False, sat=False):
        """(u, shift, picked or None) of quantised volumes, each (nz, ny, nx); sums=True appends the chosen candidate's six sums;
        sat=True: through the summed-area tables"""
        qt, qw = np.ascontiguousarray(qt, np.int16), np.ascontiguousarray(qw, np.int16)
        lb = None if labels is None else np.ascontiguousarray(labels, np.float32)
        nz, ny, nx = qt.shape
        u, shift = np.empty(qt.shape, np.uint16), np.empty(qt.shape, np.uint16)
        picked = None if lb is None else np.empty(qt.shape, np.float32)
        ptr = lambda a: None if a is None else a.ctypes.data
        if sat:
            assert not sums
            assert self.S.ofs_search_sat(qt.ctypes.data, qw.ctypes.data, ptr(lb), nx, ny, nz, int(b), int(r), METRICS[metric], u.ctypes.data,
                                         shift.ctypes.data, ptr(picked)) == 0
            return u, shift, picked
        s = np.empty(qt.shape + (6,), np.int64) if sums else None
        assert self.S.ofs_search(qt.ctypes.data, qw.ctypes.data, ptr(lb), nx, ny, nz, int(b), int(r), METRICS[metric], u.ctypes.data, shift.ctypes.data,
                                 ptr(picked), ptr(s)) == 0
        return (u, shift, picked, s) if sums else (u, shift, picked)

    def quantised(self, T, W, metric, w_range=None):
        """(qT, qW) as sift3d_fuse_search quantises them: a W without a range is not finite everywhere"""
        rt = self.range(T)
        rw = w_range if w_range is not None else (rt if metric == "ssd" else self.range(W))
        qt = self.quantize(T, *rt)
        if rw is None or not rw[1] > rw[0]:
            return qt, np.full(np.shape(T), -1, np.int16)
        return qt, self.quantize(W, *rw)

    def search(self, T, W, labels, b, r, metric, w_range=None, sat=False):
        """sift3d_fuse_search restated"""
        qt, qw = self.quantised(T, W, metric, w_range)
        return self.search_q(qt, qw, labels, b, r, metric, sat=sat)


def shift_stats(shift, r):
    """(moved, dist2_sum) of a plane of codes, in Python integers"""
    s = np.asarray(shift).astype(np.int64).reshape(-1)
    s = s[s != NO_SHIFT]
    w = 2 * r + 1
    d2 = (s % w - r) ** 2 + (s // w % w - r) ** 2 + (s // (w * w) - r) ** 2
    return int((d2 > 0).sum()), int(d2.sum())


def warped_planes(pkg, fs, ro, fo, target, atlases, target_vox2key=None, metric="ssd"):
    """what the stage has before it weighs: (T's range, qT, [(qW or None where the atlas' range is empty, M)]), the warps by the
    resampling and field oracles.  ro, fo: a ResampleOracle and a FieldOracle; atlases: dicts as pkg.fuse_labels takes them."""
    target = np.ascontiguousarray(target, np.float32)
    rt = fs.range(target)
    assert rt is not None
    planes = []
    for a in atlases:
        t = pkg.similarity_matrix(a["t"]) if isinstance(a["t"], dict) else a["t"]
        A = pkg.resample_map(t, target_vox2key, a.get("vox2key"))
        Cm, K = pkg.field_warp_terms(target_vox2key, a.get("vox2key"))
        field = a.get("field")

        def warp(vol, interp):
            if field is not None:
                return fo.warp(vol, target.shape, A, Cm, K, field, interp=interp, fill=np.nan)
            return ro.resample(vol, target.shape, A, interp=interp, fill=np.nan)

        rw = rt if metric == "ssd" else fs.range(a["image"])
        planes.append((None if rw is None else fs.quantize(warp(a["image"], "linear"), *rw), warp(a["labels"], "nearest")))
    return rt, fs.quantize(target, *rt), planes


def fuse_planes(fs, rt, qt, planes, block=2, metric="ssd", power=2, search=0):
    """the stage after the warps, restated: (words (nz, ny, nx, 2), report dict without times, with "search" where search >= 1).
    search 0 is section 7j (fuse_oracle.c's weights); search >= 1 goes through the oracle's summed-area tables, which
    test_fuse_search_cpu.py holds to its brute force."""
    assert power > 0
    us, Ms, rep = [], [], {"lo": rt[0], "hi": rt[1], "atlas": [], "search": {"radius": search, "atlas": []}}
    for qw, M in planes:
        moved, d2 = 0, 0
        if qw is None:      # nothing to weigh or to search by: the atlas votes with the labels it has at the voxel and u = 0
            u = np.zeros(qt.shape, np.uint16)
        elif search == 0:
            u = fs.weights_q(qt, qw, block, metric)
        else:
            u, shift, M = fs.search_q(qt, qw, M, block, search, metric, sat=True)
            moved, d2 = shift_stats(shift, search)
        us.append(u)
        Ms.append(M)
        rep["atlas"].append({"empty_range": int(qw is None)})
        rep["search"]["atlas"].append({"moved": moved, "dist2_sum": d2})
    words = fs.vote(us, Ms, power)
    rep["none"] = int(((words[..., 0] & NONE) != 0).sum())
    rep["fallback"] = int(((words[..., 0] & FALLBACK) != 0).sum())
    for u, M, r in zip(us, Ms, rep["atlas"]):
        votes = np.isfinite(M)
        r["voters"] = int(votes.sum())
        r["support"] = int((votes & (np.where(votes, M, -1) == (words[..., 0] & 0xffff))).sum())
        r["mean_u"] = float(int(u[votes].astype(np.int64).sum())) / r["voters"] if r["voters"] else 0.0
    return words, rep


def cpu_fuse_search(pkg, fs, ro, fo, target, atlases, target_vox2key=None, block=2, metric="ssd", power=2, search=1):
    """sift3d_fuse_labels_search restated"""
    rt, qt, planes = warped_planes(pkg, fs, ro, fo, target, atlases, target_vox2key, metric)
    return fuse_planes(fs, rt, qt, planes, block, metric, power, search)


def same_search_report(got, want):
    assert got["search"]["radius"] == want["search"]["radius"] and len(got["search"]["atlas"]) == len(want["search"]["atlas"])
    for g, w in zip(got["search"]["atlas"], want["search"]["atlas"]):
        for k in ("moved", "dist2_sum"):
            assert g[k] == w[k], (k, g[k], w[k])


# ---- the kernel tests' volumes -----------------------------------------------------------------------------------------------------
def shifted_pair(shape, seed, t=(1, -1, 1), holes=False):
    """fuse_cases.pair whose W is moved by t = (tx, ty, tz) voxels (W(x + t) resembles T(x), cyclically), so that the search has
    something to find; holes: pair's NaN and infinite voxels"""
    T, W = pair(shape, seed, holes)
    return T, np.ascontiguousarray(np.roll(W, (t[2], t[1], t[0]), (0, 1, 2)))


def block_labels(shape, seed, nan_block=True):
    """a label volume of a few labels in blocks of 3 x 4 x 5 voxels, 65535 among them; nan_block: a box of NaN wider than any search
    radius (7 voxels and more along every axis it can, from the first corner) and single NaN and infinite voxels"""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    lab = np.array([0, 1, 2, 7, 65535], np.float32)[(x // 5 + 2 * (y // 4) + 3 * (z // 3)) % 5]
    if nan_block:
        lab[:min(nz, 9), :min(ny, 10), :min(nx, 12)] = np.nan
        at = rng.random(shape) < 0.02
        lab[at] = rng.choice(np.array([np.nan, np.inf], np.float32), int(at.sum()))
    return np.ascontiguousarray(lab)


# ---- volumes at the ends of the integer sums (blockmatch_cases.py) ------------------------------------------------------------------
SEARCH_ENDS = ["speckled", "speckled_holes", "bright"]
SEARCH_ENDS_BR = [(2, 1), (2, 3), (3, 3), (5, 1), (6, 0)]   # the forms with b and r at compile time, the largest tiles, the widest sums


def ends_search_volumes(kind, shape, seed):
    """(T, W) of 0 and 1 alone: speckled (every candidate's D near n 1023^2), speckled_holes (NaN and infinite voxels in both: which
    pairs count changes with the shift), bright (W is T moved by (tx, ty, tz) = (-1, 1, 0) with 3 % of its voxels flipped: Sff, Sww and
    Sfw beyond 2^31 at b = 6, and a shift to find)"""
    if kind == "bright":
        return bright_pair(shape, seed)
    return speckled_pair(shape, seed, holes=kind == "speckled_holes")


def tie_pick(shape, axis=None):
    """the shift codes (as (tx, ty, tz) per voxel, int, shape + (3,)) that the contract picks on lattice3 (axis None) or stripes
    (axis 0: z, 1: y, 2: x) against the complement: of the shortest shifts that cost nothing the one with the least tz, then ty,
    then tx, among those that stay inside the volume"""
    zyx = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    t = np.zeros(tuple(shape) + (3,), np.int64)
    done = np.zeros(shape, bool)
    for ax in ((0, 1, 2) if axis is None else (axis,)):          # -1 along z, then y, then x, where the voxel has a neighbour there
        take = ~done & (zyx[ax] > 0)
        t[..., 2 - ax][take] = -1
        done |= take
    for ax in ((2, 1, 0) if axis is None else (axis,)):          # else +1: tz = ty = 0 and tx = 1 comes before ty = 1, and that before tz = 1
        take = ~done & (zyx[ax] < shape[ax] - 1)
        t[..., 2 - ax][take] = 1
        done |= take
    assert done.all()
    return t


def shift_vectors(shift, r):
    """(tx, ty, tz) per voxel of a plane of codes without NO_SHIFT"""
    s = np.asarray(shift).astype(np.int64)
    w = 2 * r + 1
    return np.stack([s % w - r, s // w % w - r, s // (w * w) - r], -1)
