"""Shared pieces of the label-aware interpolation tests (test_label_interp_cpu.py, test_gpu_label_interp.py):
the CPU oracle tests/label_interp_oracle.c, a numpy restatement of the contract that shares no code with it, the label volumes and
maps of the tests, stand-ins that hand fuse_cases.cpu_fuse the label oracle where it asks for a nearest-neighbour warp, and the
analytic world of the resampling scenario."""
import ctypes as C

import numpy as np

from _helpers import c_oracle
from resample_cases import about_centre, rot, special_volume

QUARTER = {"qz": np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float64),
           "qx": np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], np.float64),
           "qy": np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], np.float64)}


class LabelOracle:
    def __init__(self, tmpdir):
        L = c_oracle("label_interp_oracle", tmpdir)
        P, I64, F = C.c_void_p, C.c_int64, C.c_float
        L.orc_label_resample.restype = C.c_int
        L.orc_label_resample.argtypes = [P, I64, I64, I64, P, I64, I64, I64, P, F, I64, I64]
        L.orc_label_warp.restype = C.c_int
        L.orc_label_warp.argtypes = [P, I64, I64, I64, P, I64, I64, I64, P, P, P, P, P, P, F, F, I64, I64]
        L.orc_label_scores.restype = I64
        L.orc_label_scores.argtypes = [P, I64, I64, I64, I64, I64, I64, P, P, P]
        self.L = L

    def resample(self, vol, out_shape, A, fill=0.0, z0=0, z1=None):
        """output planes [z0, z1) of out_shape = (oz, oy, ox)"""
        v = np.ascontiguousarray(vol, np.float32)
        nz, ny, nx = v.shape
        oz, oy, ox = out_shape
        z1 = oz if z1 is None else z1
        out = np.empty((z1 - z0, oy, ox), np.float32)
        a = np.ascontiguousarray(A, np.float32).reshape(12)
        assert self.L.orc_label_resample(v.ctypes.data, nx, ny, nz, out.ctypes.data, ox, oy, oz, a.ctypes.data, float(fill), z0, z1) == 0
        return out

    def warp(self, vol, out_shape, A, Cm, K, field, fill=0.0, z0=0, z1=None):
        v = np.ascontiguousarray(vol, np.float32)
        nz, ny, nx = v.shape
        oz, oy, ox = out_shape
        z1 = oz if z1 is None else z1
        out = np.empty((z1 - z0, oy, ox), np.float32)
        a, c, k = (np.ascontiguousarray(m, np.float32).reshape(-1) for m in (A, Cm, K))
        n = np.array(field["n"], np.int64)
        o = np.ascontiguousarray(field["origin"], np.float32)
        d = np.ascontiguousarray(field["disp"], np.float32)
        assert self.L.orc_label_warp(v.ctypes.data, nx, ny, nz, out.ctypes.data, ox, oy, oz, a.ctypes.data, c.ctypes.data, k.ctypes.data, d.ctypes.data,
                                     n.ctypes.data, o.ctypes.data, float(field["spacing"]), float(fill), z0, z1) == 0
        return out

    def scores(self, vol, out_shape, A):
        """(top, second, inside count): per output voxel the winner's score and the best other class' (-1 for none; both -1 outside)"""
        v = np.ascontiguousarray(vol, np.float32)
        nz, ny, nx = v.shape
        oz, oy, ox = out_shape
        top, second = np.empty(out_shape, np.float32), np.empty(out_shape, np.float32)
        a = np.ascontiguousarray(A, np.float32).reshape(12)
        n = self.L.orc_label_scores(v.ctypes.data, nx, ny, nz, ox, oy, oz, a.ctypes.data, top.ctypes.data, second.ctypes.data)
        assert n >= 0
        return top, second, int(n)


class LabelForNearest:
    """A ResampleOracle or FieldOracle for fuse_cases.cpu_fuse whose "nearest" is the label oracle: the stage restated with
    label_interp = SIFT3D_INTERP_LABEL, every other warp as it was."""

    def __init__(self, lo, inner):
        self.lo, self.inner = lo, inner

    def resample(self, vol, out_shape, A, interp="linear", fill=0.0):
        return self.lo.resample(vol, out_shape, A, fill) if interp == "nearest" else self.inner.resample(vol, out_shape, A, interp=interp, fill=fill)

    def warp(self, vol, out_shape, A, Cm, K, field, interp="linear", fill=0.0):
        if interp == "nearest":
            return self.lo.warp(vol, out_shape, A, Cm, K, field, fill)
        return self.inner.warp(vol, out_shape, A, Cm, K, field, interp=interp, fill=fill)


def same(got, want):
    """equal bits where the result is a number, NaN where NaN"""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    gn, wn = np.isnan(got), np.isnan(want)
    assert (gn == wn).all(), "NaN at %d voxels vs %d" % (gn.sum(), wn.sum())
    g, w = got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, "%d voxels differ, first %r vs %r" % (bad.size, got[~gn][bad[:4]], want[~wn][bad[:4]])


# ---- the contract in numpy ------------------------------------------------------------------------------------------------------------
def label_numpy(vol, out_shape, A, fill=0.0):
    """Section 7n with float32 arrays, one operation at a time: the score of every corner's class as the masked sum over the eight
    corners in order, then one pass over the corners in which a later corner takes over only where its class is strictly before."""
    v = np.ascontiguousarray(vol, np.float32)
    nz, ny, nx = v.shape
    oz, oy, ox = out_shape
    A = np.asarray(A, np.float32).reshape(3, 4)
    k, j, i = (g.astype(np.float32).reshape(-1) for g in np.meshgrid(np.arange(oz), np.arange(oy), np.arange(ox), indexing="ij"))
    with np.errstate(all="ignore"):
        q = [((A[r, 0] * i + A[r, 1] * j) + A[r, 2] * k) + A[r, 3] for r in range(3)]
        n = (nx, ny, nz)
        inside = np.ones(i.shape, bool)
        for r in range(3):
            inside &= (q[r] >= np.float32(0)) & (q[r] <= np.float32(n[r] - 1))
        q = [np.where(inside, x, np.float32(0)) for x in q]
        f = [np.floor(x) for x in q]
        w = [(x - y).astype(np.float32) for x, y in zip(q, f)]
        u = [(np.float32(1) - x).astype(np.float32) for x in w]
        lo = [y.astype(np.int64) for y in f]
        hi = [np.minimum(x + 1, m - 1) for x, m in zip(lo, n)]
        L, W = [], []
        for c in range(8):
            a, b, d = c & 1, (c >> 1) & 1, c >> 2
            L.append(v[(hi if d else lo)[2], (hi if b else lo)[1], (hi if a else lo)[0]])
            W.append((((w if a else u)[0] * (w if b else u)[1]).astype(np.float32) * (w if d else u)[2]).astype(np.float32))
        fin = [np.isfinite(x) for x in L]
        zero = np.zeros(i.shape, np.float32)
        best = best_s = best_fin = None
        for c in range(8):
            s = None
            for e in range(8):
                one = (fin[c] & fin[e] & (L[c] == L[e])) | (~fin[c] & ~fin[e])
                t = np.where(one, W[e], zero)
                s = t if s is None else (s + t).astype(np.float32)
            if c == 0:
                best, best_s, best_fin = L[0].copy(), s, fin[0].copy()
                continue
            better = (s > best_s) | ((s == best_s) & fin[c] & (~best_fin | (L[c] < best)))
            best, best_s, best_fin = np.where(better, L[c], best), np.where(better, s, best_s), np.where(better, fin[c], best_fin)
    out = np.where(best_fin, best, np.float32(np.nan)).astype(np.float32)
    out = np.where(inside, out, np.float32(fill)).astype(np.float32)
    # np.where keeps the bits of -0; the winner's bits are its corner's
    return out.reshape(out_shape)


# ---- volumes and maps -----------------------------------------------------------------------------------------------------------------
def iid_labels(shape, seed):
    """labels 0 .. 3, independent and equally likely"""
    return np.random.default_rng(seed).integers(0, 4, shape).astype(np.float32)


def blobby_labels(shape, seed):
    """labels 0 .. 4 in blobs a few voxels across, with NaN, +inf, -inf and -0 sprinkled, 1 - 2 % each"""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    ph = rng.uniform(0, 6.28, 6)
    s = np.sin(x * 0.45 + ph[0]) + np.sin(y * 0.6 + ph[1]) + np.sin(z * 0.5 + ph[2]) + np.sin((x + y) * 0.3 + ph[3]) + np.sin((y - z) * 0.35 + ph[4])
    v = np.clip(np.floor((s + 5.0) / 2.0), 0, 4).astype(np.float32)
    flat = v.reshape(-1)
    for val, frac in ((np.nan, 0.015), (np.inf, 0.01), (-np.inf, 0.01), (np.float32(-0.0), 0.02)):
        flat[rng.choice(flat.size, max(1, int(flat.size * frac)), replace=False)] = val
    return v


def source(kind, shape, seed):
    return {"iid": iid_labels, "blobby": blobby_labels, "special": special_volume}[kind](shape, seed)


def shift_map(t):
    A = np.zeros((3, 4), np.float32)
    A[:, :3] = np.eye(3)
    A[:, 3] = t
    return A


def a_map(kind, src, out):
    """3 x 4 float32, output voxel -> source voxel, for shapes (nz, ny, nx)"""
    if kind == "identity":
        return shift_map((0, 0, 0))
    if kind == "half_x":
        return shift_map((0.5, 0, 0))
    if kind == "half_xyz":
        return shift_map((0.5, 0.5, 0.5))
    if kind in QUARTER:
        return about_centre(QUARTER[kind], src, out)
    if kind == "scale_half":
        return about_centre(0.5 * np.eye(3), src, out)
    if kind == "scale_2":
        return about_centre(2.0 * np.eye(3), src, out)
    if kind == "oblique":
        return about_centre(rot((1, 2, 3), 20.0), src, out, (0.7, -1.3, 2.1))
    if kind == "oblique2":
        return about_centre(1.1 * rot((-3, 1, 0.5), 47.0), src, out, (-0.4, 0.25, 0.0))
    if kind == "outside":
        return about_centre(np.eye(3), src, out, (1e4, 0, 0))
    raise ValueError(kind)


# ---- the tie cases (test_label_interp_cpu.py holds them to their share of exact ties) ------------------------------------------------
TIE_SHAPE, TIE_SEED = (129, 5, 37), 7   # every extent n has (n - 1) / 4 whole: the scale-1/2 map about the centre lands on half voxels
TIE_MAPS = ("half_x", "scale_half")


def tie_case(kind):
    """(volume, output shape, map): iid labels under the half shift (two corners of weight 1/2: a tie wherever they differ, 3/4 of
    the voxels) and under the scale-1/2 map about the centre onto a grid of the same shape (q = o / 2 + (n - 1) / 4: every second
    position along an axis is a half voxel, so two, four or eight corners share the weight equally)"""
    vol = iid_labels(TIE_SHAPE, TIE_SEED)
    return vol, TIE_SHAPE, a_map(kind, TIE_SHAPE, TIE_SHAPE)


# ---- the resampling scenario: an analytic world ---------------------------------------------------------------------------------------
WORLD = 48.0


def world_labels(p):
    """the label at world positions p (..., 3) as (x, y, z), 0 .. 4: two nested balls, an off-centre ball and a box, 48 units wide"""
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    lab = np.zeros(x.shape, np.float32)
    lab[(x - 24) ** 2 + (y - 24) ** 2 + (z - 24) ** 2 < 18.0 ** 2] = 1
    lab[(x - 24) ** 2 + (y - 24) ** 2 + (z - 24) ** 2 < 9.0 ** 2] = 2
    lab[(x - 35) ** 2 + (y - 30) ** 2 + (z - 15) ** 2 < 7.0 ** 2] = 3
    lab[(np.abs(x - 11) < 5.0) & (np.abs(y - 14) < 6.0) & (np.abs(z - 34) < 6.0)] = 4
    return lab


def world_case(n_atlas, n_target, degrees):
    """(atlas labels n_atlas^3, map target voxel -> atlas voxel, truth n_target^3): the atlas samples the world at its voxel centres
    under a rotation about the axis (1, 2, 3) through the world's centre; the target's voxel centres are the world's own axes"""
    R = rot((1, 2, 3), degrees)
    sa, st = WORLD / n_atlas, WORLD / n_target
    c = np.full(3, WORLD / 2)

    def grid(n):
        z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64),) * 3, indexing="ij")
        return np.stack([x, y, z], -1)
    atlas_world = ((grid(n_atlas) + 0.5) * sa - c) @ R.T + c             # atlas voxel -> world
    atlas = world_labels(atlas_world)
    truth = world_labels((grid(n_target) + 0.5) * st)
    # target voxel t -> world (t + 0.5) st -> atlas voxel R^T (world - c) / sa + c / sa - 0.5
    M = R.T * (st / sa)
    A = np.zeros((3, 4))
    A[:, :3] = M
    A[:, 3] = (R.T @ (0.5 * st - c)) / sa + c / sa - 0.5
    return atlas, A.astype(np.float32), truth


def dice_per_label(got, truth, labels=range(5)):
    """2 both / (a + b) per label over the voxels where got is finite (the warp reached the atlas)"""
    at = np.isfinite(got)
    g, t = got[at], truth[at]
    return [2.0 * float(((g == l) & (t == l)).sum()) / float((g == l).sum() + (t == l).sum()) for l in labels]
