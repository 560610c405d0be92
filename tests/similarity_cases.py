"""Shared pieces of the image similarity tests (test_similarity_cpu.py, test_gpu_similarity.py): the CPU oracle
tests/similarity_oracle.c, the contract restated with numpy and Python integers, the image pairs, the label volumes, and the shapes
with what kernels_similarity.hip's #defines make of them."""
import ctypes as C
import math
import os
import re

import numpy as np

from _helpers import c_oracle
from blockmatch_cases import quantize_numpy, volume

KERNEL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3d_sift_cuda_amd", "csrc", "kernels_similarity.hip")
NAMES = ("SIM_THREADS", "SIM_VPT", "SIM_MAX_BLOCKS", "SIM_MAX_BINS", "SIM_MAX_LABELS")
BINS = (8, 16, 32, 64)
MEASURES = ("mi", "nmi", "rho", "rms", "h_a", "h_b", "h_ab")


def kernel_constants(path=KERNEL):
    """{name: int} of NAMES: each `#define NAME integer` of the kernel file, as grid_loop_cases.header_constants reads its header"""
    text = open(path).read()
    out = {}
    for name in NAMES:
        m = re.findall(r"^#define[ \t]+%s[ \t]+(\d+)[ \t]*(?:/\*.*)?$" % name, text, re.M)
        assert len(m) == 1, "%s is defined %d times in %s" % (name, len(m), path)
        out[name] = int(m[0])
    return out


# ---- the shapes (nz, ny, nx): literals, held to the kernel file's #defines by test_similarity_cpu.py -------------------------------
VPT, STRETCH, CAP, EXCESS = 4, 1024, 2048, 32   # voxels per thread, per workgroup and trip, workgroups per launch; workgroups' worth beyond the cap
# 1 voxel; 24; 1485 = 1, 630 = 2, 195 = 3 mod 4; one below, exactly at and one above a workgroup's stretch; several workgroups
COUNT_SHAPES = [(1, 1, 1), (2, 3, 4), (5, 9, 33), (7, 9, 10), (3, 5, 13), (3, 11, 31), (4, 16, 16), (5, 5, 41), (11, 19, 70)]
PAIR_SHAPES = [(2, 3, 4), (5, 9, 33), (11, 19, 70)]
BIG = (33, 257, 253)                            # 2145693 voxels: past the cap by more than EXCESS stretches, and no multiple of 4
LABEL_SHAPE = (11, 19, 70)


class SimilarityOracle:
    def __init__(self, tmpdir):
        L = c_oracle("similarity_oracle", tmpdir)
        P, I64, F, I = C.c_void_p, C.c_int64, C.c_float, C.c_int
        L.osim_range.restype = I
        L.osim_range.argtypes = [P, I64, P, P]
        L.osim_q.restype = I
        L.osim_q.argtypes = [F, F, F]
        L.osim_count.restype = I64
        L.osim_count.argtypes = [P, P, P, I64, F, F, F, F, I, P, P, P]
        L.osim_rho_rms.restype = None
        L.osim_rho_rms.argtypes = [P, F, F, I, P]
        L.osim_measures.restype = None
        L.osim_measures.argtypes = [P, I, P, F, F, I, P]
        self.L = L

    def range(self, v):
        """(lo, hi) float32, or None where v has no two distinct finite values"""
        v = np.ascontiguousarray(v, np.float32)
        lo, hi = C.c_float(0), C.c_float(0)
        ok = self.L.osim_range(v.ctypes.data, v.size, C.byref(lo), C.byref(hi))
        return (np.float32(lo.value), np.float32(hi.value)), bool(ok)

    def count(self, a, b, a_range, b_range, bins, labels=None):
        """(hist int64 bins x bins, the six sums as Python integers, excluded, {label: its six sums} of the labels with n > 0)"""
        a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
        lb = None if labels is None else np.ascontiguousarray(labels, np.float32)
        hist, sums = np.zeros((bins, bins), np.int64), np.zeros(6, np.int64)
        ls = None if lb is None else np.zeros((65536, 6), np.int64)
        excluded = self.L.osim_count(a.ctypes.data, b.ctypes.data, None if lb is None else lb.ctypes.data, a.size, float(a_range[0]), float(a_range[1]),
                                     float(b_range[0]), float(b_range[1]), bins, hist.ctypes.data, sums.ctypes.data, None if ls is None else ls.ctypes.data)
        rows = {} if ls is None else {int(l): [int(v) for v in ls[l]] for l in np.nonzero(ls[:, 0])[0]}
        return hist, [int(v) for v in sums], int(excluded), rows

    def measures(self, hist, sums, lo, hi, same_scale):
        h, s, out = np.ascontiguousarray(hist, np.int64), np.array(sums, np.int64), np.zeros(7, np.float64)
        self.L.osim_measures(h.ctypes.data, h.shape[0], s.ctypes.data, float(lo), float(hi), int(same_scale), out.ctypes.data)
        return dict(zip(MEASURES, (float(v) for v in out)))

    def rho_rms(self, sums, lo, hi, same_scale):
        s, out = np.array(sums, np.int64), np.zeros(2, np.float64)
        self.L.osim_rho_rms(s.ctypes.data, float(lo), float(hi), int(same_scale), out.ctypes.data)
        return float(out[0]), float(out[1])

    def similarity(self, a, b, labels=None, bins=64, same_scale=False):
        """the stage restated on the oracle's functions: a dict with the keys same_result compares"""
        a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
        ra, ok_a = self.range(a)
        rb, ok_b = (ra, True) if same_scale else self.range(b)
        out = {"bins": bins, "same_scale": int(same_scale), "empty_range": (0 if ok_a else 1) | (0 if ok_b else 2), "range_a": ra, "range_b": rb}
        if out["empty_range"]:
            hist, sums, excluded, rows = np.zeros((bins, bins), np.int64), [0] * 6, a.size, {}
        else:
            hist, sums, excluded, rows = self.count(a, b, ra, rb, bins, labels)
        out.update(hist=hist, sums=sums, n=sums[0], excluded=excluded)
        out.update(self.measures(hist, sums, ra[0], ra[1], same_scale))
        if labels is not None:
            out["labels"] = [dict(zip(("rho", "rms"), self.rho_rms(rows[l], ra[0], ra[1], same_scale)), label=l, sums=rows[l], n=rows[l][0]) for l in sorted(rows)]
        return out


def bits(x):
    return np.array([x], np.float64).view(np.uint64)[0]


def same_measure(got, want):
    """equal bits, or both NaN"""
    return bits(got) == bits(want) or (math.isnan(got) and math.isnan(want))


def same_result(got, want):
    """what the product's image_similarity returned against the oracle's similarity: every integer equal, every range the same bits,
    every derived value the same bits (they are host arithmetic on equal integers)"""
    for k in ("bins", "same_scale", "empty_range", "excluded", "n", "sums"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert np.array_equal(got["hist"], want["hist"]), int((got["hist"] != want["hist"]).sum())
    assert int(got["hist"].sum()) == want["n"]
    for k in ("range_a", "range_b"):
        assert np.array_equal(np.array(got[k], np.float32).view(np.uint32), np.array(want[k], np.float32).view(np.uint32)), (k, got[k], want[k])
    for k in MEASURES:
        assert same_measure(got[k], want[k]), (k, got[k], want[k])
    assert ("labels" in got) == ("labels" in want)
    for g, w in zip(got.get("labels", []), want.get("labels", [])):
        assert (g["label"], g["sums"], g["n"]) == (w["label"], w["sums"], w["n"]), (g, w)
        assert same_measure(g["rho"], w["rho"]) and same_measure(g["rms"], w["rms"]), (g, w)
    assert len(got.get("labels", [])) == len(want.get("labels", []))


# ---- the contract with numpy and Python integers: shares no code with the oracle ----------------------------------------------------
def count_numpy(a, b, a_range, b_range, bins):
    """(hist, sums, excluded): quantize_numpy, np.add.at and Python integers"""
    qa = quantize_numpy(a, *a_range).astype(np.int64).reshape(-1)
    qb = quantize_numpy(b, *b_range).astype(np.int64).reshape(-1)
    ok = (qa >= 0) & (qb >= 0)
    qa, qb = qa[ok], qb[ok]
    s = 10 - int(math.log2(bins))
    hist = np.zeros((bins, bins), np.int64)
    np.add.at(hist, (qa >> s, qb >> s), 1)
    la, lb = [int(v) for v in qa], [int(v) for v in qb]
    sums = [len(la), sum(la), sum(lb), sum(v * v for v in la), sum(v * v for v in lb), sum(v * w for v, w in zip(la, lb))]
    return hist, sums, int((~ok).sum())


def rho_rms_python(sums, lo, hi, same_scale):
    n, sa, sb, saa, sbb, sab = (int(v) for v in sums)
    rho = rms = math.nan
    if n <= 0:
        return rho, rms
    cov, va, vb = n * sab - sa * sb, n * saa - sa * sa, n * sbb - sb * sb
    if va > 0 and vb > 0:
        rho = float(cov) / (math.sqrt(float(va)) * math.sqrt(float(vb)))   # float(int) rounds to nearest, as the conversion from 128 bits does
    if same_scale:
        rms = math.sqrt(float(saa - 2 * sab + sbb) / float(n)) * ((float(np.float32(hi)) - float(np.float32(lo))) / 1023.0)
    return rho, rms


def measures_python(hist, sums, lo, hi, same_scale):
    """the derived values with math.log and big integers"""
    h = np.asarray(hist, np.int64)
    n = int(sums[0])
    out = dict.fromkeys(MEASURES, math.nan)
    if n <= 0:
        return out
    out["rho"], out["rms"] = rho_rms_python(sums, lo, hi, same_scale)

    def entropy(cells):
        s = 0.0
        for c in cells:
            if c > 0:
                s += float(c) * math.log(float(c))
        return math.log(float(n)) - s / float(n)
    out["h_a"], out["h_b"], out["h_ab"] = entropy([int(v) for v in h.sum(1)]), entropy([int(v) for v in h.sum(0)]), entropy([int(v) for v in h.reshape(-1)])
    out["mi"] = (out["h_a"] + out["h_b"]) - out["h_ab"]
    if out["h_ab"] > 0:
        out["nmi"] = (out["h_a"] + out["h_b"]) / out["h_ab"]
    return out


# ---- the image pairs ------------------------------------------------------------------------------------------------------------------
PAIRS = ("iid", "smooth", "smooth_holes", "binary", "equal", "constant")


def holes(v, rng, fraction=0.03):
    at = rng.random(v.shape) < fraction
    v[at] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), int(at.sum()))
    return v


def pair(kind, shape, seed=3):
    """(A, B) float32 (nz, ny, nx).  iid: independent white noise.  smooth: blockmatch_cases' sines and the same moved by one voxel along
    x on a scale of its own.  smooth_holes: that with 3 % NaN and infinite voxels in each.  binary: 0.0 and 1.0 only (q is 0 or 1023).
    equal: B is A.  constant: one value but for the two corner voxels that give a range, B on a scale of its own."""
    rng = np.random.default_rng(seed + 101 * shape[0] + 7 * shape[1] + shape[2])
    if kind == "iid":
        return volume("random", shape, seed), volume("random", shape, seed + 1)
    if kind in ("smooth", "smooth_holes"):
        A = volume("smooth", shape, seed)
        B = (np.float32(0.37) * np.roll(A, 1, 2) - np.float32(55.0)).astype(np.float32)
        return (holes(A, rng), holes(B, rng)) if kind == "smooth_holes" else (A, B)
    if kind == "binary":
        return rng.integers(0, 2, shape).astype(np.float32), rng.integers(0, 2, shape).astype(np.float32)
    if kind == "equal":
        A = volume("smooth", shape, seed)
        return A, A.copy()
    assert kind == "constant"
    A = volume("constant", shape, seed)
    return A, (np.float32(2.0) * A + np.float32(1.0)).astype(np.float32)


# ---- the label volumes ---------------------------------------------------------------------------------------------------------------
def labels_of(kind, shape, seed=4):
    """blobby: label_interp_cases.blobby_labels (NaN, +-inf, -0 sprinkled); iid: 0 .. 6 per voxel, no wave is uniform; one: label 3
    everywhere, every wave is uniform; top: two halves, 0 and 65535; n64, n65: 64 and 65 labels in runs along x, from 1000 on in steps of
    1000 (n64) or 1 (n65)"""
    from label_interp_cases import blobby_labels
    rng = np.random.default_rng(seed)
    if kind == "blobby":
        return blobby_labels(shape, seed)
    if kind == "iid":
        return rng.integers(0, 7, shape).astype(np.float32)
    if kind == "one":
        return np.full(shape, 3, np.float32)
    if kind == "top":
        v = np.zeros(shape, np.float32)
        v[shape[0] // 2:] = 65535
        return v
    count = {"n64": 64, "n65": 65}[kind]
    step = 1000 if kind == "n64" else 1
    idx = (np.arange(int(np.prod(shape))) // 5) % count
    return (1000 + step * idx).astype(np.float32).reshape(shape)
