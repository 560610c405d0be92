"""Shared pieces of the block matching tests (test_blockmatch_cpu.py, test_gpu_blockmatch.py): the CPU oracle
tests/blockmatch_oracle.c (built with cc -O2 -ffp-contract=off into a temporary directory and bound with ctypes), a numpy
restatement of the block search, the stage of DESIGN.md section 7f restated on the CPU (oracle block search, FieldOracle's
warp, fit and interpolation, the product's host helper for gates and samples), the volumes and the scenario; and the volumes of 0
and 1 alone on which the 32-bit sums of the quantised-integer kernels pass 2^31, with the quantiser's probe (test_gpu_integer_ends.py
and the CPU suites of sections 7f, 7g, 7j and 7k)."""
import ctypes as C

import numpy as np

from _helpers import c_oracle
from field_cases import FieldOracle, local_residuals, trim

WORDS, NONE = 16, 0xffffffff
DEFAULTS = dict(stride=4, block=4, search=3, rounds=2, variance_quantile=0.25, cost_fraction=0.8, spacing=4.0, radius=20.0, lam=0.1,
                min_tol=1.0)   # sift3d_blockmatch_defaults


class BlockOracle:
    def __init__(self, tmpdir):
        L = c_oracle("blockmatch_oracle", tmpdir)
        P, I64, F = C.c_void_p, C.c_int64, C.c_float
        L.obm_range.restype = C.c_int
        L.obm_range.argtypes = [P, I64, P, P]
        L.obm_quantize.restype = None
        L.obm_quantize.argtypes = [P, I64, F, F, P]
        L.obm_match.restype = C.c_int
        L.obm_match.argtypes = [P, P, I64, I64, I64, P, I64, P, C.c_int, C.c_int, P]
        self.L = L

    def range(self, vol):
        v = np.ascontiguousarray(vol, np.float32)
        lo, hi = C.c_float(0), C.c_float(0)
        ok = self.L.obm_range(v.ctypes.data, v.size, C.byref(lo), C.byref(hi))
        return (np.float32(lo.value), np.float32(hi.value)) if ok else None

    def quantize(self, vol, lo, hi):
        v = np.ascontiguousarray(vol, np.float32)
        q = np.empty(v.shape, np.int16)
        self.L.obm_quantize(v.ctypes.data, v.size, float(lo), float(hi), q.ctypes.data)
        return q

    def match_q(self, qf, qw, first, stride, count, b, r):
        """words (count z, count y, count x, 16) of quantised volumes (nz, ny, nx) int16"""
        qf, qw = np.ascontiguousarray(qf, np.int16), np.ascontiguousarray(qw, np.int16)
        nz, ny, nx = qf.shape
        fi, cn = np.array(first, np.int64), np.array(count, np.int64)
        out = np.empty((int(cn[2]), int(cn[1]), int(cn[0]), WORDS), np.uint32)
        assert self.L.obm_match(qf.ctypes.data, qw.ctypes.data, nx, ny, nz, fi.ctypes.data, int(stride), cn.ctypes.data, int(b), int(r),
                                out.ctypes.data) == 0
        return out

    def match(self, F, W, first, stride, count, b, r):
        """the block search of float volumes: the range of F, both quantised, the words"""
        lo, hi = self.range(F)
        return self.match_q(self.quantize(F, lo, hi), self.quantize(W, lo, hi), first, stride, count, b, r)


def quantize_numpy(vol, lo, hi):
    v = np.asarray(vol, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = ((v.astype(np.float64) - float(lo)) / (float(hi) - float(lo))) * 1023.0
        q = np.where(t <= 0, 0.0, np.where(t >= 1023.0, 1023.0, np.rint(t)))
    return np.where(np.isfinite(v), q, -1.0).astype(np.int16)


def match_numpy(qf, qw, first, stride, count, b, r):
    """the block search restated with numpy: int64 sums over whole-lattice slices, one shift at a time"""
    qf, qw = np.asarray(qf, np.int64), np.asarray(qw, np.int64)
    nz, ny, nx = qf.shape
    c0, c1, c2 = (int(c) for c in count)
    out = np.zeros((c2, c1, c0, WORDS), np.uint32)
    S = 2 * r + 1
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
                side = 2 * b + 1
                cost = np.empty((S, S, S), np.int64)
                for sz in range(S):
                    for sy in range(S):
                        for sx in range(S):
                            d = fb - ww[sz:sz + side, sy:sy + side, sx:sx + side]
                            cost[sz, sy, sx] = (d * d).sum()
                g = np.arange(-r, r + 1)
                m2 = g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2
                order = np.lexsort((np.broadcast_to(g[None, None, :], cost.shape).ravel(), np.broadcast_to(g[None, :, None], cost.shape).ravel(),
                                    np.broadcast_to(g[:, None, None], cost.shape).ravel(), m2.ravel(), cost.ravel()))
                sz, sy, sx = np.unravel_index(order[0], cost.shape)
                o[0], o[1], o[2] = np.array([sx - r, sy - r, sz - r]).astype(np.int32).view(np.uint32)
                o[4], o[5] = cost[sz, sy, sx], cost[r, r, r]
                for k, (dz, dy, dx) in enumerate(((0, 0, -1), (0, 0, 1), (0, -1, 0), (0, 1, 0), (-1, 0, 0), (1, 0, 0))):
                    z, y, x = sz + dz, sy + dy, sx + dx
                    o[6 + k] = cost[z, y, x] if 0 <= z < S and 0 <= y < S and 0 <= x < S else NONE
                o[12], o[13] = fb.sum(), (fb * fb).sum()
    return out


def lattice_numpy(shape, stride, b, r):
    """first = b + r, count = floor((n - 1 - 2 (b + r)) / stride) + 1 per axis, as (x, y, z)"""
    nz, ny, nx = shape
    return (b + r,) * 3, tuple((n - 1 - 2 * (b + r)) // stride + 1 for n in (nx, ny, nz))


def shifts(words):
    return np.ascontiguousarray(words[..., :3]).view(np.int32)


def volume(kind, shape, seed):
    """(nz, ny, nx) float32: random (white noise), smooth (a few sines plus a little noise), constant (every cost ties)"""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    if kind == "random":
        return rng.normal(100.0, 30.0, shape).astype(np.float32)
    if kind == "constant":   # but for two corner voxels, which give the quantisation a range and lie in no node's block
        v = np.full(shape, 3.25, np.float32)
        v[0, 0, 0], v[-1, -1, -1] = 0.0, 10.0
        return v
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    v = np.sin(0.31 * x + 0.2 * y) * np.cos(0.23 * y - 0.11 * z) + 0.5 * np.sin(0.17 * z + 0.05 * x * y / max(nx, ny))
    return (1000.0 * v + rng.normal(0, 5.0, shape)).astype(np.float32)


# ---- volumes at the ends of the integer sums -------------------------------------------------------------------------------------
# Float32 volumes of the two finite values 0.0 and 1.0: the range is (0, 1) and the quantised values are 0 and 1023 exactly.  A 13^3
# block of them reaches 13^3 1023^2 = 2 299 224 213, between 2^31 and 2^32 (test_gpu_integer_ends.py and the "oracle equals numpy"
# tests of the CPU suites).
SUM_MAX_B6 = 13 ** 3 * 1023 ** 2


def binary(shape, seed):
    """quantised volumes of 0 and 1023 alone: the widest sums and the extremes of A and the variances"""
    rng = np.random.default_rng(seed)
    qf = (1023 * rng.integers(0, 2, shape)).astype(np.int16)
    qw = np.roll(qf, (0, 1, -1), (0, 1, 2))
    flip = rng.random(shape) < 0.05
    qw[flip] = 1023 - qw[flip]
    return qf, qw


def _holes(vols, shape, rng):
    """NaN, +inf and -inf at a fraction 0.01 of the voxels of each volume.  fuse_cases.pair has 0.03; of two volumes with that many
    no 13^3 patch keeps the 2052 voxel pairs that a sum of 2^31 takes (2052 x 1023^2 >= 2^31 > 2051 x 1023^2)."""
    for vol in vols:
        at = rng.random(shape) < 0.01
        vol[at] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), int(at.sum()))


def speckled_pair(shape, seed, holes=False, fraction=0.015):
    """(F, W): F has a fraction 0.015 of its voxels at 1, W 0.985: nearly every voxel pair differs by the full range, and the
    costs still vary from shift to shift; holes: NaN, +inf and -inf voxels scattered in both, as fuse_cases.pair has them.
    fraction 0.033: the pairs of a 13^3 block that differ number 2056 +- 12, around the 2052 at which the cost is 2^31, so the
    costs of one node's shifts lie on both sides of 2^31 (ends_pair's "straddling")"""
    rng = np.random.default_rng(seed)
    F = (rng.random(shape) < fraction).astype(np.float32)
    W = (rng.random(shape) < 1.0 - fraction).astype(np.float32)
    if holes:
        _holes((F, W), shape, rng)
    for vol in (F, W):
        assert np.nanmin(np.where(np.isfinite(vol), vol, np.nan)) == 0.0 and np.nanmax(np.where(np.isfinite(vol), vol, np.nan)) == 1.0
    return F, W


def solid_pair(shape):
    """(F, W): F is 0 and W is 1 but for one corner voxel in each that completes the range (F's last voxel is 1, W's first is 0).
    F's lies in no unflagged node's block; W's lies in no window of solid_lattice's nodes.  Every cost there is the exact maximum
    (2b + 1)^3 1023^2."""
    F, W = np.zeros(shape, np.float32), np.ones(shape, np.float32)
    F[-1, -1, -1], W[0, 0, 0] = 1.0, 0.0
    return F, W


def solid_lattice(shape, stride, b, r):
    """lattice_numpy begun one voxel later along x: no window reaches the voxels of x = 0"""
    first, count = lattice_numpy(shape, stride, b, r)
    cx = (shape[2] - 2 - 2 * (b + r)) // stride + 1
    assert cx >= 1
    return (first[0] + 1, first[1], first[2]), (cx, count[1], count[2])


def bright(shape, seed):
    """a fraction 0.97 of the voxels at 1: sum q^2 of a 13^3 block exceeds 2^31 and the block is not flat"""
    v = (np.random.default_rng(seed).random(shape) < 0.97).astype(np.float32)
    assert v.min() == 0.0 and v.max() == 1.0
    return v


def bright_pair(shape, seed):
    """(bright, bright moved by (0, 1, -1) voxels along (z, y, x) with 3 % of its voxels flipped): Sf2, Sww and Sfw exceed 2^31 at
    b = 6, and Vf and Vw are small differences of large products"""
    F = bright(shape, seed)
    W = np.roll(F, (0, 1, -1), (0, 1, 2))
    flip = np.random.default_rng(seed + 1000).random(shape) < 0.03
    W[flip] = 1.0 - W[flip]
    assert W.min() == 0.0 and W.max() == 1.0
    return F, np.ascontiguousarray(W)


def lattice3(shape):
    """(F, W): the 3-D checkerboard (x + y + z) % 2 and its complement, which is the board moved by one voxel along any axis: the
    six unit shifts all reach cost 0 and the zero shift has the largest cost"""
    z, y, x = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    F = ((x + y + z) % 2).astype(np.float32)
    return F, (1.0 - F).astype(np.float32)


def stripes(shape, axis):
    """(F, W): stripes of period 2 along one axis (0: z, 1: y, 2: x) and their complement: only the shifts -1 and +1 along that axis
    tie at cost 0 among the shortest"""
    c = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")[axis]
    F = (c % 2).astype(np.float32)
    return F, (1.0 - F).astype(np.float32)


def ends_pair(kind, shape, seed, own_scale=False):
    """the pair of a family by name (speckled, straddling, solid, bright); own_scale: W's finite values on a scale of its own, 0.37 W - 55, for
    the correlation cost, which quantises W with W's range (the two values stay two values: 0 and 1023 again)"""
    F, W = {"speckled": lambda: speckled_pair(shape, seed), "straddling": lambda: speckled_pair(shape, seed, fraction=0.033), "solid": lambda: solid_pair(shape), "bright": lambda: bright_pair(shape, seed)}[kind]()
    if own_scale:
        W = (0.37 * W.astype(np.float64) - 55.0).astype(np.float32)
    return F, W


def ends_lattice(kind, shape, stride, b, r):
    return solid_lattice(shape, stride, b, r) if kind == "solid" else lattice_numpy(shape, stride, b, r)


def quantiser_probe(values, lo, hi):
    """(volume, first, count): a float32 volume that is constant over cells of 3 x 3 x 3 voxels, one of the values per cell (x
    fastest; the cells left over hold lo), inside a shell of one voxel at lo whose first voxel is lo and whose last is hi: the two
    range voxels.  The block search with b = 1, r = 1, stride 3 from first over count has one node per cell, on its centre, whose
    block is the cell: as F, the record's words 12 and 13 are 27 q and 27 q^2 of the cell's quantised value q; as W against an
    F of lo alone, word 5 (the cost of the zero shift) is 27 q^2."""
    values = np.asarray(values, np.float32)
    c = int(np.ceil(len(values) ** (1.0 / 3.0) - 1e-9))
    cells = np.full(c ** 3, lo, np.float32)
    cells[:len(values)] = values
    vol = np.full((3 * c + 2,) * 3, lo, np.float32)
    vol[1:-1, 1:-1, 1:-1] = np.repeat(np.repeat(np.repeat(cells.reshape(c, c, c), 3, 0), 3, 1), 3, 2)
    vol[-1, -1, -1] = hi
    return vol, (2, 2, 2), (c, c, c)


def half_way_values():
    """what a quantiser over 0 .. 1023 can get wrong: every exact half-way value k + 0.5 (rint goes to the even neighbour), the
    floats next to a few of them, both ends, -0.0, a denormal, a tiny value and the last float below 1023"""
    k = np.arange(1023, dtype=np.float32) + np.float32(0.5)
    near = np.array([0.5, 1.5, 2.5, 511.5, 512.5, 1021.5, 1022.5], np.float32)
    return np.concatenate([k, np.nextafter(near, np.float32(np.inf)), np.nextafter(near, np.float32(-np.inf)),
                           np.array([0.0, 1023.0, -0.0, 1e-45, 1e-30, 1022.99994], np.float32)]).astype(np.float32)


def probe_read(words, n, word=12):
    """the quantised value of the first n cells of a probe from the records' word 12 (27 q), 13 or 5 (27 q^2)"""
    w = np.asarray(words).reshape(-1, WORDS)[:n, word].astype(np.int64)
    assert (w % 27 == 0).all()
    if word == 12:
        return w // 27
    q = np.rint(np.sqrt(w // 27)).astype(np.int64)
    assert (27 * q * q == w).all()
    return q


def zero_field(grid):
    n = grid["n"]
    return {"n": n, "origin": np.asarray(grid["origin"], np.float32), "spacing": np.float32(grid["spacing"]),
            "disp": np.zeros((3, n[2], n[1], n[0]), np.float32)}


def cpu_refine_intensity(pkg, bo, fo, V, M, t, field=None, fv=None, mv=None, **params):
    """sift3d_refine_field_intensity restated: the oracle's warp, quantisation, block search, fit and interpolation; the
    product's host helpers for the grid, the lattice, the gates and samples and the fold count.  t: 4 x 4.  Returns (field dict,
    report dict without times)."""
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
    rng = bo.range(V)
    rep = {"rounds": 0, "empty_range": int(rng is None), "round": []}
    if rng is None:
        return cur, rep
    rep["lo"], rep["hi"] = rng
    qf = bo.quantize(V, *rng)
    for _ in range(p["rounds"]):
        W = fo.warp(M, V.shape, A, Cm, K, cur, fill=np.nan)
        words = bo.match_q(qf, bo.quantize(W, *rng), first, p["stride"], count, p["block"], p["search"])
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


def same_report(got, want):
    """the product's report dict against the restatement's: every count and figure of every round, bit for bit"""
    assert got["rounds"] == want["rounds"] and got["empty_range"] == want["empty_range"], (got["rounds"], want)
    if not want["empty_range"]:
        assert got["lo"] == want["lo"] and got["hi"] == want["hi"]
    for g, w in zip(got["round"], want["round"]):
        for k, x in w.items():
            assert g[k] == x, (k, g[k], x)


def same_field(a, b):
    assert tuple(a["n"]) == tuple(b["n"]) and np.float32(a["spacing"]) == np.float32(b["spacing"])
    assert (np.asarray(a["origin"], np.float32).view(np.uint32) == np.asarray(b["origin"], np.float32).view(np.uint32)).all()
    assert (np.ascontiguousarray(a["disp"], np.float32).view(np.uint32).ravel() == np.ascontiguousarray(b["disp"], np.float32).view(np.uint32).ravel()).all()


def scenario_setup(pkg, tmp, world):
    """The nonrigid scenario of field_cases with what the intensity stage needs: the CPU prediction of section 7e
    (nonrigid_cpu), the volumes, the 4 x 4 T, the vox2keys and the map."""
    from field_cases import nonrigid_cpu, nonrigid_volumes
    from refine_cases import scenario_map
    res = nonrigid_cpu(pkg, tmp, world)
    _f, _m, V, M, A_true, vox_v, vox_m, hv, hm = nonrigid_volumes(pkg, tmp, world)
    fv = pkg.key_vox2key(vox_v, hv["qto_xyz"] if world else None)
    mv = pkg.key_vox2key(vox_m, hm["qto_xyz"] if world else None)
    T4 = pkg.similarity_matrix(res["T"])
    A = scenario_map(pkg, T4, world, vox_v, vox_m, hv, hm)
    return {"parent": res, "V": V, "M": M, "A_true": A_true, "fv": fv, "mv": mv, "T4": T4, "A": A}


def scenario_score(pkg, fo, s, field):
    """(correlation, RMS map error, largest map error) of a field on the scenario, as field_cases.nonrigid_score"""
    from field_cases import nonrigid_score
    Cm, K = pkg.field_warp_terms(s["fv"], s["mv"])
    out = fo.warp(s["M"], s["V"].shape, s["A"], Cm, K, field)
    return nonrigid_score(pkg, s["V"], out, s["A"], s["A_true"], field, s["fv"], s["mv"])
