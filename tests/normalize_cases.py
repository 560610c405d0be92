"""Shared pieces of the intensity-matching tests (test_normalize_cpu.py, test_gpu_normalize.py): the CPU oracle
tests/normalize_oracle.c, the contract restated with float64 numpy, the stage sift3d_normalize_intensity restated on the oracle, the
pairs of the kernel tests, the shapes with what kernels_normalize.hip's #defines make of them, and the scenario."""
import ctypes as C
import math
import os
import re

import numpy as np

from _helpers import c_oracle
from average_cases import FV, SHAPES, matrix_of_map, source_shape
from blockmatch_cases import quantize_numpy, volume
from invert_cases import forward_field
from register_cases import holes, map_of

KERNEL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3d_sift_cuda_amd", "csrc", "kernels_normalize.hip")
NAMES = ("NORM_THREADS", "NORM_MAX_BLOCKS", "NORM_BINS", "NORM_WORDS", "APPLY_THREADS", "APPLY_VPT", "APPLY_MAX_BLOCKS", "APPLY_MAX_KNOTS")
BRICK = (4, 8, 32)                  # warp_device.h's brick of reference voxels (z, y, x)
HIST_CAP = 1024                     # workgroups of the histogram launch
APPLY_CAP, APPLY_STRETCH = 2048, 1024   # workgroups of the apply launch; voxels of a workgroup per trip
BIG_REF = (33, 257, 253)            # 9 x 33 x 8 = 2376 bricks: the third trip of HIST_CAP workgroups is a partial one
BIG_IMAGE = (35, 311, 393)          # 4277805 voxels = 4177.5 stretches: the third trip of APPLY_CAP workgroups is a partial one, the last stretch too;
                                    # it holds BIG_REF moved by half a voxel, so that the reference's last plane (the third trip's) is counted
MAP_KINDS = ("identity", "shift", "half", "rotation", "outside")
MODES = ("linear", "hist")
KNOTS = (2, 3, 64, 65, 255, 256)    # Q: m = Q + 1 kept knots at most, either side of the powers of two that set the apply kernel's bisection steps
REFUSALS = {-2: "at least 2 are needed", -3: "of the reference all fall", -4: "of the image all fall"}
assert SHAPES == [(1, 1, 1), (2, 3, 4), (5, 9, 33), (11, 19, 70)]


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
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def bits64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


class Refused(Exception):
    """the oracle's transfer refuses: .code is onm_transfer's, .text what the product's message holds"""

    def __init__(self, code):
        Exception.__init__(self, REFUSALS[code])
        self.code, self.text = code, REFUSALS[code]


class NormalizeOracle:
    def __init__(self, tmpdir):
        L = c_oracle("normalize_oracle", tmpdir)
        P, I64, F, I, D = C.c_void_p, C.c_int64, C.c_float, C.c_int, C.c_double
        L.onm_range.restype = I
        L.onm_range.argtypes = [P, I64, P, P]
        L.onm_overlap.restype = I
        L.onm_overlap.argtypes = [P, I64, I64, I64, P, P, I64, I64, I64, P, P, P, P, P, P, F, F, F, F, F, P, P, P, P]
        L.onm_transfer.restype = I
        L.onm_transfer.argtypes = [I, I, P, P, P, F, F, P, P, P, P, P, P]
        L.onm_apply.restype = None
        L.onm_apply.argtypes = [P, I64, I, P, P, P, D, D, F, F, F, P]
        self.L = L

    def range(self, v):
        v = np.ascontiguousarray(v, np.float32)
        lo, hi = C.c_float(0), C.c_float(0)
        ok = self.L.onm_range(v.ctypes.data, v.size, C.byref(lo), C.byref(hi))
        return (np.float32(lo.value), np.float32(hi.value)) if ok else None

    def overlap(self, pkg, ref, image, ar, br, ref_vox2key=None, mask=None):
        """(hist_a, hist_b, sums, counts) as pkg.overlap_histograms returns them; the map's terms are the host code's, as the stage takes them"""
        R, B = np.ascontiguousarray(ref, np.float32), np.ascontiguousarray(image["image"], np.float32)
        M = None if mask is None else np.ascontiguousarray(mask, np.float32)
        A = np.ascontiguousarray(pkg.resample_map(np.eye(4, dtype=np.float32) if image.get("t") is None else image["t"], ref_vox2key, image.get("vox2key")), np.float32).reshape(12)
        Cm, K = (np.ascontiguousarray(a, np.float32).reshape(-1) for a in pkg.field_warp_terms(ref_vox2key, image.get("vox2key")))
        f = image.get("field")
        ha, hb, sums, counts = np.zeros(1024, np.int64), np.zeros(1024, np.int64), np.zeros(6, np.int64), np.zeros(3, np.int64)
        (nz, ny, nx), (mz, my, mx) = R.shape, B.shape
        if f is None:
            fa = (None, None, None, 1.0)
        else:
            d, n, o = np.ascontiguousarray(f["disp"], np.float32), np.array(f["n"], np.int64), np.ascontiguousarray(f["origin"], np.float32)
            fa = (d.ctypes.data, n.ctypes.data, o.ctypes.data, float(f["spacing"]))
        rc = self.L.onm_overlap(R.ctypes.data, nx, ny, nz, None if M is None else M.ctypes.data, B.ctypes.data, mx, my, mz, A.ctypes.data, Cm.ctypes.data, K.ctypes.data,
                                *fa, float(ar[0]), float(ar[1]), float(br[0]), float(br[1]), ha.ctypes.data, hb.ctypes.data, sums.ctypes.data, counts.ctypes.data)
        assert rc == 0
        return ha, hb, [int(v) for v in sums], dict(zip(("masked", "outside", "excluded"), (int(v) for v in counts)))

    def transfer(self, mode, ha, hb, sums, ar, br, knots=64):
        """the table dict, as pkg.normalize_transfer returns it (without its struct); raises Refused"""
        ha, hb, s = (np.ascontiguousarray(v, np.int64) for v in (ha, hb, sums))
        xb, xa, slope = np.zeros(257), np.zeros(257), np.zeros(257)
        m, tail, wa = C.c_int(0), C.c_double(0), C.c_double(0)
        rc = self.L.onm_transfer({"linear": 0, "hist": 1}[mode], int(knots), ha.ctypes.data, hb.ctypes.data, s.ctypes.data, float(ar[0]), float(ar[1]), C.byref(m),
                                 xb.ctypes.data, xa.ctypes.data, slope.ctypes.data, C.byref(tail), C.byref(wa))
        if rc != 0:
            raise Refused(rc)
        return {"mode": {"linear": 0, "hist": 1}[mode], "m": m.value, "a_range": (np.float32(ar[0]), np.float32(ar[1])), "b_range": (np.float32(br[0]), np.float32(br[1])),
                "wa": wa.value, "tail": tail.value, "xb": xb[:m.value].copy(), "xa": xa[:m.value].copy(), "slope": slope[:m.value - 1].copy()}

    def apply(self, v, t):
        v = np.ascontiguousarray(v, np.float32)
        out = np.empty(v.shape, np.float32)
        xb, xa, slope = (np.ascontiguousarray(t[k], np.float64) for k in ("xb", "xa", "slope"))
        self.L.onm_apply(v.ctypes.data, v.size, int(t["m"]), xb.ctypes.data, xa.ctypes.data, slope.ctypes.data, float(t["tail"]), float(t["wa"]), float(t["a_range"][0]),
                         float(t["b_range"][0]), float(t["b_range"][1]), out.ctypes.data)
        return out

    def stage(self, pkg, ref, image, ref_vox2key=None, mask=None, mode="linear", knots=64):
        """sift3d_normalize_intensity restated: (out, {hist_a, hist_b, sums, counts, table}); raises Refused where the transfer refuses"""
        ar, br = self.range(ref), self.range(image["image"])
        assert ar is not None and br is not None
        ha, hb, sums, counts = self.overlap(pkg, ref, image, ar, br, ref_vox2key, mask)
        t = self.transfer(mode, ha, hb, sums, ar, br, knots)
        return self.apply(image["image"], t), {"hist_a": ha, "hist_b": hb, "sums": sums, "counts": counts, "table": t}


def same_tables(got, want):
    """two table dicts: every double and every range equal in bits"""
    assert got["m"] == want["m"] and got["mode"] == want["mode"], (got["m"], want["m"])
    for k in ("xb", "xa", "slope", "tail", "wa"):
        assert np.array_equal(bits64(got[k]), bits64(want[k])), (k, got[k], want[k])
    for k in ("a_range", "b_range"):
        assert np.array_equal(bits32(got[k]), bits32(want[k])), k


def same_words(got, want):
    """(hist_a, hist_b, sums, counts) of the product against the oracle's"""
    for k in (0, 1):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))
    assert got[2] == want[2] and got[3] == want[3], (got[2:], want[2:])


def same_stage(got, want):
    """pkg.normalize_intensity's (out, report) against NormalizeOracle.stage's (out, info): every output word, sum, count and table double"""
    out, rep = got
    assert out.shape == want[0].shape and np.array_equal(bits32(out), bits32(want[0])), int((bits32(out) != bits32(want[0])).sum())
    assert rep["sums"] == want[1]["sums"] and rep["counts"] == want[1]["counts"], (rep["sums"], rep["counts"], want[1]["sums"], want[1]["counts"])
    same_tables(rep["table"], want[1]["table"])


# ---- the contract with float64 numpy: shares no code with the oracle ----------------------------------------------------------------
def inside_numpy(A, shape, mshape):
    """the sampler's inside test of an affine map on the grid `shape`, in float32 in the contract's order"""
    A = np.asarray(A, np.float32).reshape(3, 4)
    k, j, i = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    p = [i.astype(np.float32), j.astype(np.float32), k.astype(np.float32)]
    ok = np.ones(shape, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(3):
            q = ((A[r, 0] * p[0] + A[r, 1] * p[1]) + A[r, 2] * p[2]) + A[r, 3]
            assert q.dtype == np.float32
            ok &= (q >= 0) & (q <= np.float32(mshape[2 - r] - 1))
    return ok


def words_numpy(ref, warped, ar, br, mask=None, inside=None):
    """(hist_a, hist_b, sums, counts) from the reference and the image warped onto its grid with fill NaN: np.bincount histograms, Python
    integer sums.  inside (bool plane) separates outside from excluded; without it counts["outside"] is None and excluded holds both"""
    R, W = np.asarray(ref, np.float32), np.asarray(warped, np.float32)
    masked = np.zeros(R.shape, bool) if mask is None else ~np.isfinite(mask) | (np.asarray(mask, np.float32) == 0)
    qa, qb = quantize_numpy(R, *ar).astype(np.int64), quantize_numpy(W, *br).astype(np.int64)
    out = np.zeros(R.shape, bool) if inside is None else ~inside & ~masked
    counted = ~masked & ~out & (qa >= 0) & (qb >= 0)
    a, b = qa[counted], qb[counted]
    la, lb = [int(x) for x in a], [int(x) for x in b]
    sums = [len(la), sum(la), sum(lb), sum(x * x for x in la), sum(x * x for x in lb), sum(x * y for x, y in zip(la, lb))]
    rest = int((~masked & ~out & ~counted).sum())
    return (np.bincount(a, minlength=1024).astype(np.int64), np.bincount(b, minlength=1024).astype(np.int64), sums,
            {"masked": int(masked.sum()), "outside": None if inside is None else int(out.sum()), "excluded": rest})


def knots_numpy(h, n, Q):
    """x_j, j = 0 .. Q, of one histogram: float64 arrays"""
    h = np.asarray(h, np.int64)
    r = (np.arange(Q + 1, dtype=np.int64) * (n - 1)) // Q
    cum = np.cumsum(h)
    i = np.searchsorted(cum, r, side="right")            # the smallest bin with cum_i > r
    below = cum[i] - h[i]
    return (i.astype(np.float64) - 0.5) + ((r - below).astype(np.float64) + 0.5) / h[i].astype(np.float64)


def transfer_numpy(mode, ha, hb, sums, ar, br, knots=64):
    """the table dict, or raises Refused"""
    n, Sa, Sb, Saa, Sbb = (int(v) for v in sums[:5])
    if n < 2:
        raise Refused(-2)
    if mode == "linear":
        Va, Vb = n * Saa - Sa * Sa, n * Sbb - Sb * Sb                 # Python integers: exact
        if Va <= 0:
            raise Refused(-3)
        if Vb <= 0:
            raise Refused(-4)
        ma, mb = np.float64(Sa) / np.float64(n), np.float64(Sb) / np.float64(n)
        g = np.sqrt(np.float64(float(Va))) / np.sqrt(np.float64(float(Vb)))
        xb = np.array([0.0, 1023.0])
        xa = np.array([ma + (np.float64(0.0) - mb) * g, ma + (np.float64(1023.0) - mb) * g])
    else:
        ka, kb = knots_numpy(ha, n, knots), knots_numpy(hb, n, knots)
        keep = [0]
        for j in range(1, knots + 1):
            if kb[j] > kb[keep[-1]]:
                keep.append(j)
        xa, xb = ka[keep], kb[keep]
        if len(keep) < 2:
            raise Refused(-4)
        if xa[0] == xa[-1]:
            raise Refused(-3)
    return {"mode": {"linear": 0, "hist": 1}[mode], "m": len(xb), "a_range": (np.float32(ar[0]), np.float32(ar[1])), "b_range": (np.float32(br[0]), np.float32(br[1])),
            "wa": (np.float64(np.float32(ar[1])) - np.float64(np.float32(ar[0]))) / np.float64(1023.0), "tail": (xa[-1] - xa[0]) / (xb[-1] - xb[0]), "xb": xb, "xa": xa,
            "slope": (xa[1:] - xa[:-1]) / (xb[1:] - xb[:-1])}


def apply_numpy(v, t):
    v = np.asarray(v, np.float32)
    xb, xa, slope, m = t["xb"], t["xa"], t["slope"], t["m"]
    blo, bhi, alo = (np.float64(np.float32(x)) for x in (t["b_range"][0], t["b_range"][1], t["a_range"][0]))
    fin = np.isfinite(v)
    with np.errstate(invalid="ignore", over="ignore"):
        u = ((np.where(fin, v, np.float32(0)).astype(np.float64) - blo) / (bhi - blo)) * np.float64(1023.0)
        k = np.clip(np.searchsorted(xb, u, side="right") - 1, 0, m - 2)      # the largest index with xb[k] <= u, where there is a segment
        seg = np.minimum(xa[k] + (u - xb[k]) * slope[k], xa[k + 1])
        low, high = xa[0] + (u - xb[0]) * np.float64(t["tail"]), xa[m - 1] + (u - xb[m - 1]) * np.float64(t["tail"])
        y = np.where(u < xb[0], low, np.where(u >= xb[m - 1], high, seg))
        out = (alo + y * np.float64(t["wa"])).astype(np.float32)
    return np.where(fin, bits32(out).reshape(v.shape), bits32(v).reshape(v.shape)).astype(np.uint32).view(np.float32)


# ---- the pairs of the kernel tests --------------------------------------------------------------------------------------------------
def pair(pkg, shape, kind="identity", field=False, ref_vox2key=None, seed=0, with_holes=True, k=1, masked=False):
    """(reference, image dict, mask or None) on the reference grid `shape`: smooth volumes on scales of their own, the image's shape a
    few voxels off per axis (source_shape's k), NaN and +-inf voxels in both, the map kind, a field with a NaN-free smooth displacement,
    and a mask with zeros, a NaN and other non-zero values"""
    rng = np.random.default_rng(seed)
    s = source_shape(shape, k)
    R = volume("smooth", shape, seed)
    B = (np.float32(-0.4) * volume("smooth", s, seed) + np.float32(30.0)).astype(np.float32)
    if with_holes and R.size > 1:
        R, B = holes(R, seed + 10), holes(B, seed + 11)
    if R.size > 1:
        R.flat[0], R.flat[-1] = -1200.0, 1300.0      # two distinct finite values each, whatever the holes took
    if B.size > 1:
        B.flat[0], B.flat[-1] = -500.0, 520.0
    a = {"image": B, "t": None if kind == "identity" else matrix_of_map(map_of(kind, shape, s))}
    if ref_vox2key is None and seed % 2:
        a["vox2key"] = pkg.key_vox2key()
    if field:
        a["field"] = forward_field("smooth", pkg.blockmatch_grid(shape, ref_vox2key, spacing=4.0), seed=seed, amp=1.5, wave=25.0)
    M = None
    if masked:
        M = rng.choice(np.array([0.0, -0.0, 1.0, -2.5, 1e-30], np.float32), shape, p=[0.2, 0.1, 0.5, 0.1, 0.1]).astype(np.float32)
        if M.size > 1:
            M.flat[1] = np.nan
            M.flat[-1] = np.inf
    return R, a, M


def one_bin_pair(shape, top):
    """(reference, image dict, mask): every counted voxel in bin 0 (top False) or in bin 1023 (top True) of both histograms: the images
    are constant but for their first voxel, which gives each its range; under the identity it is read at the reference's first voxel
    alone, which the mask takes out"""
    R, B = np.full(shape, 7.0 if top else 3.0, np.float32), np.full(shape, -2.0 if top else -6.0, np.float32)
    R.flat[0], B.flat[0] = (3.0, -6.0) if top else (7.0, -2.0)
    M = np.ones(shape, np.float32)
    M.flat[0] = 0.0
    return R, {"image": B}, M


# ---- the scenario: section 7r's, every atlas on a scale of its own ------------------------------------------------------------------
# The second leg's curves all bend one way (gamma above 1) and its atlases are registered as well as the first leg's good ones (the small sine
# field, no 3-voxel displacement).  With gammas on both sides of 1 (0.6, 0.9, 1.2, 1.5, 1.8) under the first leg's misregistration the bends
# cancel in the mean of five and the misregistration (clean: 103.0) dominates the RMS: linear came out at 101.5, BELOW clean, and the leg's
# condition had nothing to separate.  A gain and an offset cannot undo a bend; bends of one sign add up in the mean.
GAMMAS = (1.4, 1.5, 1.6, 1.7, 1.8)
# gain and offset per atlas, in fuse_cases.GAINS' ranges (0.6 .. 1.5, -400 .. 250).  fuse_cases.GAINS themselves average to a gain of 1.03 and an
# offset of 6: the MEAN of the five remapped images is then nearly the mean of the clean ones (RMS 100.9 against 103.0), and shows nothing
SCALES = [(0.6, 250.0), (0.75, -150.0), (1.5, -400.0), (0.8, 120.0), (0.65, 200.0)]


def gamma_curve(v, gamma):
    """v through a gamma curve on its own range: lo + (hi - lo) ((v - lo) / (hi - lo)) ^ gamma, float32"""
    d = np.asarray(v, np.float64)
    lo, hi = d.min(), d.max()
    return (lo + (hi - lo) * ((d - lo) / (hi - lo)) ** gamma).astype(np.float32)


def scenario(pkg, ro, tmp, gamma=False):
    """average_cases.scenario with each atlas image remapped as fuse_cases remaps it, by SCALES (gain 0.6 .. 1.5, offset -400 .. 250).  With
    gamma, the second leg: every atlas keeps only the small sine part of its field (0.4 key units, fuse_cases.scenario's honest registration
    error; no atlas is three voxels off anywhere) and goes through a gamma curve of its own (GAMMAS) before the remap.  Returns (target, grid
    vox2key, clean images, remapped images); the clean images carry the leg's fields."""
    import average_cases
    target, gv, clean = average_cases.scenario(pkg, ro, tmp)
    if gamma:
        grid = pkg.blockmatch_grid(target.shape, gv, spacing=4.0)
        clean = [dict(a, field=forward_field("sine", grid, amp=0.4, wave=30.0 + 5.0 * k)) for k, a in enumerate(clean)]
    out = []
    for k, a in enumerate(clean):
        g, o = SCALES[k]
        v = gamma_curve(a["image"], GAMMAS[k]) if gamma else a["image"]
        out.append(dict(a, image=(g * v.astype(np.float64) + o).astype(np.float32)))
    return target, gv, clean, out


def rms(a, b, where):
    d = a.astype(np.float64)[where] - b.astype(np.float64)[where]
    return float(np.sqrt((d * d).mean()))
