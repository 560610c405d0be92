"""Shared pieces of the label fusion tests (test_fuse_cpu.py, test_gpu_fuse.py): the CPU oracle
tests/fuse_oracle.c, the stage sift3d_fuse_labels restated on the CPU (the resampling and field oracles' warps, this oracle's
quantisation, weights and vote), the small volumes of the kernel tests and the five-atlas scenario."""
import ctypes as C
import os

import numpy as np

from _helpers import c_oracle
from blockmatch_cases import SUM_MAX_B6, bright, bright_pair, lattice3, speckled_pair, stripes, volume   # noqa: F401 (the fusion tests take them from here)
from invert_cases import forward_field
from resample_cases import affine, rot

METRICS = {"ssd": 0, "ncc": 1}
U_ONE, FALLBACK, NONE = 32768, 0x40000000, 0x80000000


class FuseOracle:
    def __init__(self, tmpdir):
        L = c_oracle("fuse_oracle", tmpdir)
        P, I64, F, I = C.c_void_p, C.c_int64, C.c_float, C.c_int
        L.ofu_range.restype = I
        L.ofu_range.argtypes = [P, I64, P, P]
        L.ofu_quantize.restype = None
        L.ofu_quantize.argtypes = [P, I64, F, F, P]
        L.ofu_similarity.restype = C.c_uint32
        L.ofu_similarity.argtypes = [I] + [I64] * 6
        L.ofu_weights.restype = I
        L.ofu_weights.argtypes = [P, P, I64, I64, I64, I, I, P, P]
        L.ofu_vote.restype = I
        L.ofu_vote.argtypes = [I, P, P, I64, I, P]
        L.ofu_overlap.restype = I
        L.ofu_overlap.argtypes = [P, P, I64, P, P, P]
        self.L = L

    def range(self, vol):
        v = np.ascontiguousarray(vol, np.float32)
        lo, hi = C.c_float(0), C.c_float(0)
        ok = self.L.ofu_range(v.ctypes.data, v.size, C.byref(lo), C.byref(hi))
        return (np.float32(lo.value), np.float32(hi.value)) if ok else None

    def quantize(self, vol, lo, hi):
        v = np.ascontiguousarray(vol, np.float32)
        q = np.empty(v.shape, np.int16)
        self.L.ofu_quantize(v.ctypes.data, v.size, float(lo), float(hi), q.ctypes.data)
        return q

    def similarity(self, metric, n, sf, sff, sw, sww, sfw):
        return int(self.L.ofu_similarity(METRICS[metric], int(n), int(sf), int(sff), int(sw), int(sww), int(sfw)))

    def weights_q(self, qt, qw, b, metric, sums=False):
        """u (nz, ny, nx) uint16 of quantised volumes; sums=True: (u, the six int64 sums per voxel)"""
        qt, qw = np.ascontiguousarray(qt, np.int16), np.ascontiguousarray(qw, np.int16)
        nz, ny, nx = qt.shape
        u = np.empty(qt.shape, np.uint16)
        s = np.empty(qt.shape + (6,), np.int64) if sums else None
        assert self.L.ofu_weights(qt.ctypes.data, qw.ctypes.data, nx, ny, nz, int(b), METRICS[metric], u.ctypes.data,
                                  s.ctypes.data if sums else None) == 0
        return (u, s) if sums else u

    def weights(self, T, W, b, metric, w_range=None):
        """sift3d_fuse_weights restated: T quantised with its range, W with w_range (None: T's under ssd, W's own under ncc); u = 0
        everywhere where W's range is empty"""
        rt = self.range(T)
        rw = w_range if w_range is not None else (rt if metric == "ssd" else self.range(W))
        if rw is None or not rw[1] > rw[0]:
            return np.zeros(np.shape(T), np.uint16)
        return self.weights_q(self.quantize(T, *rt), self.quantize(W, *rw), b, metric)

    def vote(self, u, labels, power):
        """words, the shape of one plane + (2,); u, labels: K arrays of one shape"""
        us = np.ascontiguousarray(np.stack([np.asarray(a, np.uint16) for a in u]))
        ls = np.ascontiguousarray(np.stack([np.asarray(a, np.float32) for a in labels]))
        words = np.empty(us.shape[1:] + (2,), np.uint32)
        assert self.L.ofu_vote(len(us), us.ctypes.data, ls.ctypes.data, int(us[0].size), int(power), words.ctypes.data) == 0
        return words

    def overlap(self, a, b):
        a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
        ca, cb, cc = (np.zeros(65536, np.int64) for _ in range(3))
        assert self.L.ofu_overlap(a.ctypes.data, b.ctypes.data, a.size, ca.ctypes.data, cb.ctypes.data, cc.ctypes.data) == 0
        return ca, cb, cc


def fused_labels(words, fill=np.nan):
    """the label volume of the words: float32, fill where no atlas votes"""
    w0 = np.asarray(words)[..., 0]
    return np.where(w0 & NONE, np.float32(fill), (w0 & 0xffff).astype(np.float32)).astype(np.float32)


def mean_dice(fz, a, b):
    """the mean over the labels either volume has of 2 both / (a + b), and the per-label values"""
    ca, cb, cc = fz.overlap(a, b)
    present = (ca > 0) | (cb > 0)
    d = 2.0 * cc[present] / (ca[present] + cb[present])
    return float(d.mean()), d


def cpu_fuse(pkg, fz, ro, fo, target, atlases, target_vox2key=None, block=2, metric="ssd", power=2):
    """sift3d_fuse_labels restated: (words (nz, ny, nx, 2), report dict without times).  ro, fo: a ResampleOracle and a FieldOracle;
    atlases: dicts as pkg.fuse_labels takes them."""
    target = np.ascontiguousarray(target, np.float32)
    rt = fz.range(target)
    assert rt is not None
    qt = fz.quantize(target, *rt)
    us, Ms, rep = [], [], {"lo": rt[0], "hi": rt[1], "atlas": []}
    for a in atlases:
        t = pkg.similarity_matrix(a["t"]) if isinstance(a["t"], dict) else a["t"]
        A = pkg.resample_map(t, target_vox2key, a.get("vox2key"))
        Cm, K = pkg.field_warp_terms(target_vox2key, a.get("vox2key"))
        field = a.get("field")

        def warp(vol, interp):
            if field is not None:
                return fo.warp(vol, target.shape, A, Cm, K, field, interp=interp, fill=np.nan)
            return ro.resample(vol, target.shape, A, interp=interp, fill=np.nan)

        M = warp(a["labels"], "nearest")
        u, empty = np.zeros(target.shape, np.uint16), 0
        if power > 0:
            rw = rt if metric == "ssd" else fz.range(a["image"])
            empty = int(rw is None)
            if rw is not None:
                u = fz.weights_q(qt, fz.quantize(warp(a["image"], "linear"), *rw), block, metric)
        us.append(u)
        Ms.append(M)
        rep["atlas"].append({"empty_range": empty})
    words = fz.vote(us, Ms, power)
    rep["none"] = int(((words[..., 0] & NONE) != 0).sum())
    rep["fallback"] = int(((words[..., 0] & FALLBACK) != 0).sum())
    for u, M, r in zip(us, Ms, rep["atlas"]):
        votes = np.isfinite(M)
        r["voters"] = int(votes.sum())
        r["support"] = int((votes & (np.where(votes, M, -1) == (words[..., 0] & 0xffff))).sum())
        r["mean_u"] = float(int(u[votes].astype(np.int64).sum())) / r["voters"] if r["voters"] else 0.0
    return words, rep


def same_report(got, want):
    for k in ("lo", "hi", "none", "fallback"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert len(got["atlas"]) == len(want["atlas"])
    for g, w in zip(got["atlas"], want["atlas"]):
        for k in ("voters", "support", "mean_u", "empty_range"):
            assert g[k] == w[k], (k, g[k], w[k])


# ---- the kernel tests' volumes -----------------------------------------------------------------------------------------------------
def pair(shape, seed, holes=False):
    """(T, W) float32 (nz, ny, nx): a smooth volume, and it with a slightly different gain, an offset and some noise (a few
    quantisation steps, so that neither similarity saturates); holes: NaN and infinite voxels scattered in both"""
    rng = np.random.default_rng(seed)
    T = volume("smooth", shape, seed)
    W = (0.98 * T + 15.0 + rng.normal(0, 12.0, shape)).astype(np.float32)
    if holes:
        for vol in (T, W):
            at = rng.random(shape) < 0.03
            vol[at] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), int(at.sum()))
    return T, W


ZERO_SHIFT_SHAPE = (9, 11, 37)   # more than one brick of the fusion kernels along x, one brick and a voxel along y and z


def assert_zero_shift_identity(metric, u, words, first):
    """u: fuse_weights of (T, W) at b = 2; words: the block matcher's of the same pair at b = 2 on a lattice of stride 1 from first
    (x, y, z).  An unflagged node's patch is whole, n = N = 125, and word 5 is the cost at the zero shift from the same sums: u is
    (2^31 - cost) >> 16 under "ncc" and (125 << 15) // (cost + 125) under "ssd".  Not vacuously: more than 100 unflagged nodes, more
    than one value on both sides."""
    cz, cy, cx = words.shape[:3]
    at = u[first[2]:first[2] + cz, first[1]:first[1] + cy, first[0]:first[0] + cx].astype(np.int64)
    node = words[..., 3] == 0
    got, cost = at[node], words[..., 5][node].astype(np.int64)
    want = ((1 << 31) - cost) >> 16 if metric == "ncc" else (125 << 15) // (cost + 125)
    print("zero shift %s: %d unflagged nodes, cost %d .. %d, u %d .. %d" % (metric, node.sum(), cost.min(), cost.max(), got.min(), got.max()))
    assert node.sum() > 100 and len(np.unique(got)) > 1 and len(np.unique(cost)) > 1
    assert np.array_equal(got, want), (metric, int((got != want).sum()))


def ends_volumes(kind, shape, seed):
    """(T, W) of 0 and 1 alone, at the ends of the integer sums (blockmatch_cases.py): speckled (nearly every pair differs by the full
    range: D near n 1023^2, u = 0), speckled_holes (with NaN and infinite voxels in both), bright (Sff, Sww and Sfw beyond 2^31 at
    b = 6, patches that are not flat; the bright pair with W moved back, so that the patches correspond at the zero shift, the one
    the weights look at), bright_same (W = T: D = Sff - 2 Sfw + Sww = 0 from three sums beyond 2^31, u = 32768)"""
    if kind == "bright_same":
        T = bright(shape, seed)
        return T, T.copy()
    if kind == "bright":
        T, W = bright_pair(shape, seed)
        return T, np.ascontiguousarray(np.roll(W, (0, -1, 1), (0, 1, 2)))
    return speckled_pair(shape, seed, holes=kind == "speckled_holes")


ENDS = ["speckled", "speckled_holes", "bright", "bright_same"]
ENDS_SHAPE = (15, 17, 37)   # every extent >= 2 * 6 + 3: some patches are unclipped at b = 6; more than one 32 x 8 x 4 brick per axis, partial ones


# ---- the scenario ------------------------------------------------------------------------------------------------------------------
SHAPE, BIG, ATLAS, PAD, SLABS = (40, 40, 40), (64, 64, 64), (48, 48, 48), 12, 5
WRONG = [(3.0, 0.0, 0.0), (0.0, 3.0, 0.0), (-3.0, 0.0, 0.0), (0.0, -3.0, 0.0), (2.0, 2.0, 1.0)]   # atlas voxels, where an atlas is misregistered
GAINS = [(1.0, 0.0), (0.6, 250.0), (1.5, -400.0), (0.8, 120.0), (1.25, 60.0)]                     # the -c leg's gain and offset per atlas


def scenario(pkg, ro, tmp):
    """One world of 64^3 voxels with a label map of 6^3 cubes (labels 1 .. 4 inside a ball, 0 outside) and intensities that follow
    a smooth texture plus a step per label.  The target is its central 40^3.  Five atlases of 48^3 are the world resampled through
    oblique similarities (a few degrees, scales near 1), so each atlas' transform to the target is known exactly; the matrix is
    taken as a .trans.txt holds it.  Each atlas' field is a small smooth one (forward_field "sine", 0.4 key units: an honest
    registration error) plus, in three of the target's five z slabs -- a different three per atlas, so that in every slab three
    of five atlases are wrong -- a displacement of three atlas voxels.  Keys are featExtract's (voxel + 0.5).  Returns a dict:
    target, truth, vox2key, atlases (image, remapped, labels, t, vox2key, field)."""
    rng = np.random.default_rng(40)
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in BIG), indexing="ij")
    cube = (x // 6 + 2 * (y // 6) + 3 * (z // 6)) % 4 + 1
    ball = (x - 31.5) ** 2 + (y - 31.5) ** 2 + (z - 31.5) ** 2 < 27.0 ** 2
    labels_big = np.where(ball, cube, 0).astype(np.float32)
    image_big = (volume("smooth", BIG, 4).astype(np.float64) * 0.4 + 160.0 * labels_big + rng.normal(0, 8.0, BIG)).astype(np.float32)
    crop = (slice(PAD, PAD + SHAPE[0]),) * 3
    vk = pkg.key_vox2key()
    grid = pkg.blockmatch_grid(SHAPE, vk, spacing=4.0)
    n0, n1, n2 = grid["n"]
    node_z = np.float64(grid["origin"][2]) + np.float64(grid["spacing"]) * np.arange(n2)          # key z of the node planes
    node_slab = np.clip(np.floor((node_z - 0.5) / (SHAPE[0] / SLABS)), 0, SLABS - 1).astype(int)
    atlases = []
    for k in range(5):
        axis = [(0.3, -0.5, 0.8), (1, 0.2, 0.1), (-0.4, 0.9, 0.2), (0.1, 0.1, -1), (0.7, 0.7, 0.1)][k]
        R, s = rot(axis, [7.0, -6.0, 8.0, 5.0, -7.5][k]), [1.03, 0.98, 1.0, 1.04, 0.97][k]
        ca, cb = (np.array(ATLAS[::-1], np.float64) - 1) / 2, (np.array(BIG[::-1], np.float64) - 1) / 2
        B = affine(R, cb - s * R @ ca + np.array([1.5, -1.0, 0.5]) * (k - 2), s)                    # atlas voxel -> world voxel
        image = ro.resample(image_big, ATLAS, B[:3].astype(np.float32), "linear", fill=0.0)
        lab = ro.resample(labels_big, ATLAS, B[:3].astype(np.float32), "nearest", fill=np.nan)
        T = affine(np.eye(3), [0.5 - PAD] * 3) @ B @ affine(np.eye(3), [-0.5] * 3)                    # atlas key -> target key
        path = os.path.join(str(tmp), "atlas%d.trans.txt" % k)
        pkg.write_matrix(path, T.astype(np.float32))
        t = pkg.read_similarity(path)
        field = forward_field("sine", grid, amp=0.4, wave=30.0 + 5.0 * k)
        wrong = np.isin(node_slab, [(k + j) % SLABS for j in range(3)])
        field["disp"] = field["disp"].copy()
        for c in range(3):
            field["disp"][c, wrong] += np.float32(WRONG[k][c])
        g, o = GAINS[k]
        atlases.append({"image": image, "remapped": (g * image.astype(np.float64) + o).astype(np.float32), "labels": lab, "t": t, "vox2key": vk,
                        "field": field, "wrong_slabs": [(k + j) % SLABS for j in range(3)]})
    return {"target": np.ascontiguousarray(image_big[crop]), "truth": np.ascontiguousarray(labels_big[crop]), "vox2key": vk, "atlases": atlases}


def leg(s, metric):
    """the scenario's atlases as pkg.fuse_labels takes them: the remapped intensities under "ncc" """
    return [{"image": a["remapped"] if metric == "ncc" else a["image"], "labels": a["labels"], "t": a["t"], "vox2key": a["vox2key"], "field": a["field"]}
            for a in s["atlases"]]
