"""Shared pieces of the correlation-cost tests (test_blockmatch_ncc_cpu.py, test_gpu_blockmatch_ncc.py):
the CPU oracle tests/blockmatch_ncc_oracle.c, a numpy restatement of the search (int64 sums, Python floats), the stage restated
on the CPU under either cost, and the intensity remaps of the moving volume.  Everything section 7f's tests already have comes
from blockmatch_cases.py."""
import ctypes as C

import numpy as np

from _helpers import c_oracle
from blockmatch_cases import DEFAULTS, NONE, WORDS, BlockOracle, lattice_numpy, zero_field
from field_cases import local_residuals, trim

FLAT = 1 << 31   # the cost of an anticorrelated pair and of a flat block


class NccOracle:
    """oncc_match on quantised volumes; the range and the 10-bit map are blockmatch_oracle.c's (section 7f's)"""

    def __init__(self, tmpdir):
        self.ssd = BlockOracle(tmpdir)
        L = c_oracle("blockmatch_ncc_oracle", tmpdir)
        P, I64 = C.c_void_p, C.c_int64
        L.oncc_cost.restype = C.c_uint32
        L.oncc_cost.argtypes = [I64] * 6
        L.oncc_match.restype = C.c_int
        L.oncc_match.argtypes = [P, P, I64, I64, I64, P, I64, P, C.c_int, C.c_int, P]
        self.L = L
        self.range, self.quantize = self.ssd.range, self.ssd.quantize

    def cost(self, N, Sf, Sff, Sw, Sww, Sfw):
        return int(self.L.oncc_cost(N, Sf, Sff, Sw, Sww, Sfw))

    def match_q(self, qf, qw, first, stride, count, b, r):
        qf, qw = np.ascontiguousarray(qf, np.int16), np.ascontiguousarray(qw, np.int16)
        nz, ny, nx = qf.shape
        fi, cn = np.array(first, np.int64), np.array(count, np.int64)
        out = np.empty((int(cn[2]), int(cn[1]), int(cn[0]), WORDS), np.uint32)
        assert self.L.oncc_match(qf.ctypes.data, qw.ctypes.data, nx, ny, nz, fi.ctypes.data, int(stride), cn.ctypes.data, int(b), int(r),
                                 out.ctypes.data) == 0
        return out

    def match(self, F, W, first, stride, count, b, r):
        """the search of float volumes: F quantised with F's range, W with W's own"""
        return self.match_q(self.quantize(F, *self.range(F)), self.quantize(W, *self.range(W)), first, stride, count, b, r)


def cost_python(N, Sf, Sff, Sw, Sww, Sfw):
    """section 7g's cost in Python integers and floats (IEEE double, one operation at a time; round() is ties-to-even)"""
    A, Vf, Vw = N * Sfw - Sf * Sw, N * Sff - Sf * Sf, N * Sww - Sw * Sw
    rho2 = (float(A) * float(A)) / (float(Vf) * float(Vw)) if A > 0 and Vf > 0 and Vw > 0 else 0.0
    return round((1.0 - min(rho2, 1.0)) * 2147483648.0)


def match_numpy_ncc(qf, qw, first, stride, count, b, r):
    """the search restated with numpy: int64 sums per node and shift, the cost by cost_python"""
    qf, qw = np.asarray(qf, np.int64), np.asarray(qw, np.int64)
    nz, ny, nx = qf.shape
    c0, c1, c2 = (int(c) for c in count)
    out = np.zeros((c2, c1, c0, WORDS), np.uint32)
    S, side = 2 * r + 1, 2 * b + 1
    N = side ** 3
    g = np.arange(-r, r + 1)
    m2 = (g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2).ravel()
    gz, gy, gx = (np.broadcast_to(v, (S, S, S)).ravel() for v in (g[:, None, None], g[None, :, None], g[None, None, :]))
    for c in range(c2):
        for bb in range(c1):
            for a in range(c0):
                p = (first[0] + a * stride, first[1] + bb * stride, first[2] + c * stride)
                o = out[c, bb, a]
                if min(p) - b - r < 0 or p[0] + b + r > nx - 1 or p[1] + b + r > ny - 1 or p[2] + b + r > nz - 1:
                    o[3] = 1
                    continue
                fb = qf[p[2] - b:p[2] + b + 1, p[1] - b:p[1] + b + 1, p[0] - b:p[0] + b + 1]
                ww = qw[p[2] - b - r:p[2] + b + r + 1, p[1] - b - r:p[1] + b + r + 1, p[0] - b - r:p[0] + b + r + 1]
                if (fb < 0).any() or (ww < 0).any():
                    o[3] = 1
                    continue
                Sf, Sff = int(fb.sum()), int((fb * fb).sum())
                cost = np.empty((S, S, S), np.int64)
                for sz in range(S):
                    for sy in range(S):
                        for sx in range(S):
                            wb = ww[sz:sz + side, sy:sy + side, sx:sx + side]
                            cost[sz, sy, sx] = cost_python(N, Sf, Sff, int(wb.sum()), int((wb * wb).sum()), int((fb * wb).sum()))
                sz, sy, sx = np.unravel_index(np.lexsort((gx, gy, gz, m2, cost.ravel()))[0], cost.shape)
                o[0], o[1], o[2] = np.array([sx - r, sy - r, sz - r]).astype(np.int32).view(np.uint32)
                o[4], o[5] = cost[sz, sy, sx], cost[r, r, r]
                for k, (dz, dy, dx) in enumerate(((0, 0, -1), (0, 0, 1), (0, -1, 0), (0, 1, 0), (-1, 0, 0), (1, 0, 0))):
                    z, y, x = sz + dz, sy + dy, sx + dx
                    o[6 + k] = cost[z, y, x] if 0 <= z < S and 0 <= y < S and 0 <= x < S else NONE
                o[12], o[13] = Sf, Sff
    return out


def remap(vol, kind):
    """the moving volume's intensities remapped, in double and then rounded to float32; x is the last axis, y the middle one.
    Names: the planted-translation table's half, half_offset, bias; the scenario table's affine, smooth_bias."""
    v = np.asarray(vol, np.float64)
    nz, ny, nx = v.shape
    x = np.arange(nx, dtype=np.float64)[None, None, :]
    y = np.arange(ny, dtype=np.float64)[None, :, None]
    out = {"none": lambda: v,
           "half": lambda: 0.5 * v,
           "half_offset": lambda: 0.5 * v + 300.0,
           "bias": lambda: 1.7 * v * (1.0 + 0.35 * (x / nx - 0.5)) - 200.0,
           "affine": lambda: 0.45 * v + 310.0,
           "smooth_bias": lambda: v * (0.6 + 0.5 * x / nx + 0.3 * np.sin(2.0 * np.pi * y / ny)) + 120.0}[kind]()
    return np.ascontiguousarray(out, np.float32)


def cpu_refine_intensity_metric(pkg, no, fo, V, M, t, field=None, fv=None, mv=None, metric="ncc", **params):
    """sift3d_refine_field_intensity_metric restated, as blockmatch_cases.cpu_refine_intensity restates the SSD stage: the
    oracles' warp, quantisation, block search, fit and interpolation; the product's host helpers for the grid, the lattice, the
    gates and samples and the fold count.  no: an NccOracle.  Under "ncc" W is quantised with the moving volume's range and an
    empty moving range is an empty range.  Returns (field dict, report dict without times)."""
    from refine_cases import rms
    p = dict(DEFAULTS)
    p.update(params)
    t = np.asarray(t, np.float32).reshape(4, 4)
    grid = pkg.blockmatch_grid(V.shape, fv, **params)
    first, count = pkg.blockmatch_lattice(V.shape, **params)
    assert (first, count) == lattice_numpy(V.shape, p["stride"], p["block"], p["search"])
    A = pkg.resample_map(t, fv, mv)
    Cm, K = pkg.field_warp_terms(fv, mv)
    cur = field if field is not None else zero_field(grid)
    search = no.match_q if metric == "ncc" else no.ssd.match_q
    rng = no.range(V)
    wrng = no.range(M) if metric == "ncc" else rng
    rep = {"rounds": 0, "empty_range": int(rng is None or wrng is None), "round": []}
    if rng is not None:
        rep["lo"], rep["hi"] = rng
    if metric == "ncc" and wrng is not None:
        rep["moving_lo"], rep["moving_hi"] = wrng
    if rep["empty_range"]:
        return cur, rep
    qf = no.quantize(V, *rng)
    for _ in range(p["rounds"]):
        W = fo.warp(M, V.shape, A, Cm, K, cur, fill=np.nan)
        words = search(qf, no.quantize(W, *wrng), first, p["stride"], count, p["block"], p["search"])
        y, v, counts = pkg.blockmatch_samples(words, V.shape, t, cur, fv, **params)
        r = {"nodes": int(np.prod(count)), "flagged": counts[0], "gated_variance": counts[1], "gated_border": counts[2], "gated_cost": counts[3],
             "samples": len(y)}
        rep["round"].append(r)
        if len(y) == 0:
            break
        f1 = fo.fit(y, v, grid, p["radius"], p["lam"])
        e = local_residuals(fo, f1, y, v)
        k = trim(e, p["min_tol"])
        cur = fo.fit(y[k], v[k], grid, p["radius"], p["lam"])
        e2 = local_residuals(fo, cur, y[k], v[k])
        folds, big = pkg.blockmatch_folds(t, cur)
        r.update(kept=int(k.sum()), rms_before=rms(e), rms_after=rms(e2), folds=folds, max_disp=big)
        rep["rounds"] += 1
    return cur, rep


def same_report_ncc(got, want):
    """blockmatch_cases.same_report, and the range W was quantised with"""
    from blockmatch_cases import same_report
    same_report(got, want)
    for k in ("moving_lo", "moving_hi"):
        if k in want:
            assert got[k] == want[k], (k, got[k], want[k])
