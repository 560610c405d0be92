"""Shared pieces of the registration tests (test_register_cpu.py, test_gpu_register.py): the CPU oracle
tests/register_oracle.c, the kernel's contract restated with float32 numpy, the maps, the shapes with what kernels_register.hip's
#defines make of them, and the scenario pair."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np

from _helpers import c_oracle
from blockmatch_cases import quantize_numpy, volume

KERNEL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3d_sift_cuda_amd", "csrc", "kernels_register.hip")
NAMES = ("REG_THREADS", "REG_MAX_BLOCKS", "REG_MAX_MAPS", "REG_MAX_BINS", "REG_WORDS")
BINS = (8, 16, 32, 64)
STRIDES = (1, 2, 4, 8)
DOFS = (3, 6, 7, 9, 12)
DEFAULT_LEVELS = ((4, 4.0, 1.0), (2, 1.0, 0.25), (1, 0.25, 0.0625))


def kernel_constants(path=KERNEL):
    """{name: int} of NAMES: each `#define NAME integer` of the kernel file"""
    text = open(path).read()
    out = {}
    for name in NAMES:
        m = re.findall(r"^#define[ \t]+%s[ \t]+(\d+)[ \t]*(?:/\*.*)?$" % name, text, re.M)
        assert len(m) == 1, "%s is defined %d times in %s" % (name, len(m), path)
        out[name] = int(m[0])
    return out


# ---- the shapes (nz, ny, nx): literals, held to the kernel file's #defines by test_register_cpu.py -----------------------------------
BRICK = (4, 8, 32)            # warp_device.h's brick of lattice points (z, y, x)
CAP = 512                     # workgroups per map of a launch
# 1 voxel; 24; a brick plus one in x; the pair of odd shapes every stride runs on
SMALL_PAIRS = [((1, 1, 1), (1, 1, 1)), ((2, 3, 4), (2, 3, 4)), ((5, 9, 33), (5, 9, 33))]
ODD_PAIR = ((13, 17, 31), (11, 19, 29))
BIG = (33, 257, 253)          # 2145693 lattice points at stride 1: 9 x 33 x 8 = 2376 bricks, more than four trips of CAP workgroups


def bricks(shape, stride=1):
    return math.prod(-(-((n - 1) // stride + 1) // b) for n, b in zip(shape, BRICK))


class RegisterOracle:
    def __init__(self, tmpdir):
        L = c_oracle("register_oracle", tmpdir)
        P, I64, F, I, D = C.c_void_p, C.c_int64, C.c_float, C.c_int, C.c_double
        L.oreg_warp_hist.restype = I64
        L.oreg_warp_hist.argtypes = [P, I64, I64, I64, P, I64, I64, I64, P, I, I, F, F, F, F, I, P, P, P, P]
        L.oreg_map.restype = I
        L.oreg_map.argtypes = [P, I64, I64, I64, P, P, P, P]
        L.oreg_result.restype = I
        L.oreg_result.argtypes = [P, I64, I64, I64, P, P, P]
        L.oreg_candidates.restype = I
        L.oreg_candidates.argtypes = [P, I, D, D, P]
        L.oreg_lattice.restype = I64
        L.oreg_lattice.argtypes = [I64, I64, I64, I, P, P, P, P]
        L.oreg_register.restype = I
        L.oreg_register.argtypes = [P, I64, I64, I64, P, I64, I64, I64, P, P, P, I, I, I, I, P, P, P, I, D] + [P] * 8
        L.osim_range.restype = I
        L.osim_range.argtypes = [P, I64, P, P]
        L.osim_measures.restype = None
        L.osim_measures.argtypes = [P, I, P, F, F, I, P]
        self.L = L

    @staticmethod
    def _m(m):
        return None if m is None else np.ascontiguousarray(m, np.float32).reshape(16)

    def range(self, v):
        v = np.ascontiguousarray(v, np.float32)
        lo, hi = C.c_float(0), C.c_float(0)
        ok = self.L.osim_range(v.ctypes.data, v.size, C.byref(lo), C.byref(hi))
        return (np.float32(lo.value), np.float32(hi.value)) if ok else None

    def warp_hist(self, F, M, maps, fr, mr, stride=1, bins=64):
        """(hist int64 K x bins x bins, sums K lists, excluded K, outside K), as the product's warp_histogram returns them"""
        F, M = np.ascontiguousarray(F, np.float32), np.ascontiguousarray(M, np.float32)
        a = np.ascontiguousarray(maps, np.float32).reshape(-1, 12)
        K = len(a)
        hist, sums, ex, out = np.zeros((K, bins, bins), np.int64), np.zeros((K, 6), np.int64), np.zeros(K, np.int64), np.zeros(K, np.int64)
        (nz, ny, nx), (mz, my, mx) = F.shape, M.shape
        self.N = self.L.oreg_warp_hist(F.ctypes.data, nx, ny, nz, M.ctypes.data, mx, my, mz, a.ctypes.data, K, stride, float(fr[0]), float(fr[1]), float(mr[0]),
                                       float(mr[1]), bins, hist.ctypes.data, sums.ctypes.data, ex.ctypes.data, out.ctypes.data)
        return hist, [[int(v) for v in r] for r in sums], [int(v) for v in ex], [int(v) for v in out]

    def map(self, theta, shape, fv=None, mv=None, m0=None):
        t, out = np.ascontiguousarray(theta, np.float64), np.zeros(12, np.float32)
        nz, ny, nx = shape
        ms = [self._m(m) for m in (fv, mv, m0)]
        rc = self.L.oreg_map(t.ctypes.data, nx, ny, nz, *[None if m is None else m.ctypes.data for m in ms], out.ctypes.data)
        return out.reshape(3, 4) if rc == 0 else None

    def result(self, theta, shape, fv=None, m0=None):
        t, out = np.ascontiguousarray(theta, np.float64), np.zeros(16, np.float32)
        nz, ny, nx = shape
        ms = [self._m(m) for m in (fv, m0)]
        rc = self.L.oreg_result(t.ctypes.data, nx, ny, nz, *[None if m is None else m.ctypes.data for m in ms], out.ctypes.data)
        return out.reshape(4, 4) if rc == 0 else None

    def candidates(self, theta, dof, u, rho):
        t, out = np.ascontiguousarray(theta, np.float64), np.zeros((24, 12), np.float64)
        n = self.L.oreg_candidates(t.ctypes.data, dof, u, rho, out.ctypes.data)
        return None if n < 0 else out[:n].copy()

    def lattice(self, shape, stride, fv=None):
        nz, ny, nx = shape
        n, h, rho, m = (C.c_int64 * 3)(), C.c_double(0), C.c_double(0), self._m(fv)
        N = self.L.oreg_lattice(nx, ny, nz, stride, None if m is None else m.ctypes.data, n, C.byref(h), C.byref(rho))
        return int(N), tuple(int(v) for v in n), h.value, rho.value

    def measures(self, hist, sums):
        h, s, out = np.ascontiguousarray(hist, np.int64), np.array(sums, np.int64), np.zeros(7, np.float64)
        self.L.osim_measures(h.ctypes.data, h.shape[0], s.ctypes.data, 0.0, 1.0, 0, out.ctypes.data)
        return {"mi": float(out[0]), "nmi": float(out[1]), "rho": float(out[2]), "h_a": float(out[4]), "h_b": float(out[5]), "h_ab": float(out[6])}

    def register(self, F, M, fv=None, mv=None, m0=None, dof=12, metric="nmi", bins=32, levels=DEFAULT_LEVELS, max_iterations=200, min_overlap=0.25):
        """the stage: a dict with the keys same_registration compares, or the negative code"""
        F, M = np.ascontiguousarray(F, np.float32), np.ascontiguousarray(M, np.float32)
        (nz, ny, nx), (mz, my, mx) = F.shape, M.shape
        n = len(levels)
        strides, first, last = (C.c_int * n)(*[l[0] for l in levels]), (C.c_double * n)(*[l[1] for l in levels]), (C.c_double * n)(*[l[2] for l in levels])
        theta, result = np.zeros(12, np.float64), np.zeros(16, np.float32)
        it, ev, stop = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        s_in, s_out, step = np.zeros(n), np.zeros(n), np.zeros(n)
        ms = [self._m(m) for m in (fv, mv, m0)]
        rc = self.L.oreg_register(F.ctypes.data, nx, ny, nz, M.ctypes.data, mx, my, mz, *[None if m is None else m.ctypes.data for m in ms], dof,
                                  {"mi": 0, "nmi": 1}[metric], bins, n, strides, first, last, max_iterations, min_overlap, theta.ctypes.data, result.ctypes.data,
                                  it.ctypes.data, ev.ctypes.data, stop.ctypes.data, s_in.ctypes.data, s_out.ctypes.data, step.ctypes.data)
        if rc != 0:
            return rc
        return {"theta": theta, "result": result.reshape(4, 4),
                "levels": [{"stride": levels[l][0], "iterations": int(it[l]), "evaluations": int(ev[l]), "stop": int(stop[l]), "score_in": float(s_in[l]),
                            "score_out": float(s_out[l]), "last_step": float(step[l])} for l in range(n)]}


def bits64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def bits32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def same_histograms(got, want):
    """the product's warp_histogram against the oracle's warp_hist: every integer equal"""
    assert got[0].dtype == np.int64 and got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), int((got[0] != want[0]).sum())
    assert got[1] == want[1] and got[2] == want[2] and got[3] == want[3], (got[1:], want[1:])


def same_registration(got, want):
    """the product's register_affine against the oracle's register: equal bits of theta and M1, every level's counts and every score"""
    assert np.array_equal(bits64(got["theta"]), bits64(want["theta"])), (got["theta"], want["theta"])
    assert np.array_equal(bits32(got["result"]), bits32(want["result"])), (got["result"], want["result"])
    assert len(got["levels"]) == len(want["levels"])
    for g, w in zip(got["levels"], want["levels"]):
        for k in ("stride", "iterations", "evaluations", "stop"):
            assert g[k] == w[k], (k, g, w)
        for k in ("score_in", "score_out", "last_step"):
            assert bits64(g[k]) == bits64(w[k]), (k, g, w)


# ---- the contract with float32 numpy: shares no code with the oracle ---------------------------------------------------------------
def warp_hist_numpy(F, M, A, fr, mr, stride=1, bins=64):
    """one map: (hist, sums, excluded, outside).  Every operation on float32 arrays in the contract's order"""
    F, M = np.asarray(F, np.float32), np.asarray(M, np.float32)
    A = np.asarray(A, np.float32).reshape(3, 4)
    nz, ny, nx = F.shape
    top = [np.float32(d - 1) for d in M.shape[::-1]]       # x, y, z
    k, j, i = np.meshgrid(np.arange(0, nz, stride), np.arange(0, ny, stride), np.arange(0, nx, stride), indexing="ij")
    p = [i.astype(np.float32), j.astype(np.float32), k.astype(np.float32)]
    with np.errstate(invalid="ignore", over="ignore"):
        q = [((A[r, 0] * p[0] + A[r, 1] * p[1]) + A[r, 2] * p[2]) + A[r, 3] for r in range(3)]
        assert all(v.dtype == np.float32 for v in q)
        inside = np.ones(i.shape, bool)
        for r in range(3):
            inside &= (q[r] >= 0) & (q[r] <= top[r])
        lo, hi, w = [], [], []
        for r in range(3):
            qs = np.where(inside, q[r], np.float32(0))
            f = np.floor(qs)
            w.append(qs - f)
            lo.append(f.astype(np.int64))
            hi.append(np.minimum(lo[r] + 1, M.shape[2 - r] - 1))
        one = np.float32(1)
        lerp = lambda a, b, t: (one - t) * a + t * b
        at = lambda x, y, z: M[z, y, x]
        e00, e10 = lerp(at(lo[0], lo[1], lo[2]), at(hi[0], lo[1], lo[2]), w[0]), lerp(at(lo[0], hi[1], lo[2]), at(hi[0], hi[1], lo[2]), w[0])
        e01, e11 = lerp(at(lo[0], lo[1], hi[2]), at(hi[0], lo[1], hi[2]), w[0]), lerp(at(lo[0], hi[1], hi[2]), at(hi[0], hi[1], hi[2]), w[0])
        v = lerp(lerp(e00, e10, w[1]), lerp(e01, e11, w[1]), w[2])
        assert v.dtype == np.float32
        v = np.where(inside, v, np.float32(np.nan))
    qa = quantize_numpy(F[::stride, ::stride, ::stride], *fr).astype(np.int64).reshape(-1)
    qb = quantize_numpy(v, *mr).astype(np.int64).reshape(-1)
    ok = (qa >= 0) & (qb >= 0)
    qa, qb = qa[ok], qb[ok]
    s = 10 - int(math.log2(bins))
    hist = np.zeros((bins, bins), np.int64)
    np.add.at(hist, (qa >> s, qb >> s), 1)
    la, lb = [int(x) for x in qa], [int(x) for x in qb]
    sums = [len(la), sum(la), sum(lb), sum(x * x for x in la), sum(x * x for x in lb), sum(x * y for x, y in zip(la, lb))]
    return hist, sums, int((~ok).sum()), int((~inside).sum())


# ---- the maps -------------------------------------------------------------------------------------------------------------------------
MAP_KINDS = ("identity", "shift", "half", "rotation", "scale", "outside", "nan")


def map_of(kind, fshape, mshape):
    """3 x 4 float32, fixed voxel -> moving voxel: the identity; an integer shift (2, -1, 1); a half-voxel shift; a 20 degree rotation
    about z through the fixed centre onto the moving centre, a part of the lattice outside; a 1.3 x 1.0 x 0.8 scale about the centre;
    everything outside; a NaN entry"""
    cf = np.array([(d - 1) / 2.0 for d in fshape[::-1]])
    cm = np.array([(d - 1) / 2.0 for d in mshape[::-1]])
    L, t = np.eye(3), np.zeros(3)
    if kind == "shift":
        t = np.array([2.0, -1.0, 1.0])
    elif kind == "half":
        t = np.array([0.5, 0.5, 0.5])
    elif kind == "rotation":
        a = math.radians(20.0)
        L = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1.0]])
        t = cm - L @ cf
    elif kind == "scale":
        L = np.diag([1.3, 1.0, 0.8])
        t = cm - L @ cf
    elif kind == "outside":
        t = np.array([5000.0, 0.0, 0.0])
    A = np.concatenate([L, t[:, None]], 1).astype(np.float32)
    if kind == "nan":
        A[1, 2] = np.nan
    return A


def all_maps(fshape, mshape):
    return np.stack([map_of(k, fshape, mshape) for k in MAP_KINDS])


def holes(v, seed, fraction=0.04):
    """NaN and +-inf sprinkled into a copy of v"""
    rng = np.random.default_rng(seed)
    v = v.copy()
    at = rng.random(v.shape) < fraction
    v[at] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), int(at.sum()))
    return v


def image_pair(fshape, mshape, seed=2, with_holes=True):
    """(F, M, F's range, M's range): smooth volumes on scales of their own, with non-finite voxels; a single voxel gets given ranges"""
    F = volume("smooth", fshape, seed)
    M = (np.float32(-0.4) * volume("smooth", mshape, seed) + np.float32(30.0)).astype(np.float32)
    if with_holes and F.size > 1:
        F, M = holes(F, seed + 10), holes(M, seed + 11)
        F.flat[0], M.flat[0] = 1.0, 2.0     # a finite corner each
    return F, M, (np.float32(-900.0), np.float32(1100.0)), (np.float32(-500.0), np.float32(400.0))


# ---- the scenario: a 12-parameter map and an intensity relation that is not monotone -----------------------------------------------
SCENARIO_SHAPE = (48, 44, 40)       # nz, ny, nx
SCENARIO_THETA = np.array([2.0, -1.5, 1.0, 0.04, -0.03, 0.05, 0.05, -0.04, 0.03, 0.03, -0.02, 0.015])


def corner_error(map_a, map_b, shape):
    """the largest distance between the images of the fixed volume's eight corners under two maps, in moving voxels"""
    nz, ny, nx = shape
    c = np.array([[x, y, z, 1.0] for x in (0, nx - 1) for y in (0, ny - 1) for z in (0, nz - 1)])
    a, b = np.asarray(map_a, np.float64).reshape(3, 4), np.asarray(map_b, np.float64).reshape(3, 4)
    return float(np.sqrt((((a - b) @ c.T) ** 2).sum(0)).max())


@functools.lru_cache(maxsize=None)
def scenario(true_map_key, shape=SCENARIO_SHAPE, blobs=60, seed=7):
    """(F, M): F = `blobs` random Gaussian blobs plus noise on `shape`; M = the same blobs through the fold |v - mid| and through the
    map fixed voxel -> moving voxel given as a tuple of 12 numbers, plus noise of its own, on the same grid.  Read-only arrays."""
    A = np.array(true_map_key, np.float64).reshape(3, 4)
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    centre = rng.uniform([0, 0, 0], [nx - 1, ny - 1, nz - 1], (blobs, 3))
    sigma, amp = rng.uniform(2.5, 6.0, blobs), rng.uniform(0.4, 1.0, blobs)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    grid = np.stack([x, y, z], -1).astype(np.float64)

    def f(pos):
        v = np.zeros(pos.shape[:-1])
        for c, s, a in zip(centre, sigma, amp):
            v += a * np.exp(-((pos - c) ** 2).sum(-1) / (2 * s * s))
        return v
    F = f(grid)
    mid = 0.5 * (F.min() + F.max())
    Ainv = np.linalg.inv(np.vstack([A, [0, 0, 0, 1]]))
    back = grid @ Ainv[:3, :3].T + Ainv[:3, 3]     # the fixed position whose content a moving voxel holds
    M = np.abs(f(back) - mid)
    F = (1000.0 * F + rng.normal(0, 10.0, shape)).astype(np.float32)
    M = (1000.0 * M + rng.normal(0, 10.0, shape)).astype(np.float32)
    F.setflags(write=False)
    M.setflags(write=False)
    return F, M
