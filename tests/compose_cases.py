"""Shared pieces of the composition tests (test_compose_cpu.py, test_gpu_compose.py): the CPU oracle tests/compose_oracle.c (built
with cc -O2 -ffp-contract=off into a temporary directory and bound with ctypes), a numpy restatement of the composite field and of
its interpolation residual, the stage of DESIGN.md section 7i restated on the CPU, and the synthetic triple of images of the
end-to-end test."""
import ctypes as C
import os

import numpy as np

from _helpers import c_oracle
from invert_cases import _field_args, _rows, affine_inverse_numpy, field_at_numpy, node_positions, phi_numpy

MAX_DISP = 128.0                       # SIFT3D_FIELD_MAX_DISP
OUTSIDE1, OUTSIDE2, ZEROED = 1, 2, 4   # SIFT3D_COMPOSE_*
RADIUS = 20.0                          # sift3d_compose_defaults


class ComposeOracle:
    def __init__(self, tmpdir):
        L = c_oracle("compose_oracle", tmpdir)
        P, F = C.c_void_p, C.c_float
        L.ocp_matrix.restype = None
        L.ocp_matrix.argtypes = [P, P, P]
        L.ocp_compose.restype = C.c_int
        L.ocp_compose.argtypes = [P, P, P, P, P, P, F, P, P, P, F, P, P, F, P, P, P]
        self.L = L

    def matrix(self, m1, m2):
        a, b = (np.ascontiguousarray(x, np.float32).reshape(16) for x in (m1, m2))
        o = np.zeros(16, np.float32)
        self.L.ocp_matrix(a.ctypes.data, b.ctypes.data, o.ctypes.data)
        return o.reshape(4, 4)

    def compose(self, m1, m2, mc, field1, field2, grid, residual=True):
        """(w (3, n2, n1, n0) float32, status (n2, n1, n0) uint32, res2 (n2 - 1, n1 - 1, n0 - 1) float64 or None) over grid"""
        a, b, c = (np.ascontiguousarray(x, np.float32).reshape(16) for x in (m1, m2, mc))
        n = np.array(grid["n"], np.int64)
        o = np.ascontiguousarray(grid["origin"], np.float32)
        N, cn = int(np.prod(n)), tuple(int(x) - 1 for x in n)
        w, st = np.zeros(3 * N, np.float32), np.zeros(N, np.uint32)
        r2 = np.zeros(max(cn[0] * cn[1] * cn[2], 1), np.float64) if residual else None
        d1, n1, o1, h1, _k1 = _field_args(field1)
        d2, n2, o2, h2, _k2 = _field_args(field2)
        assert self.L.ocp_compose(a.ctypes.data, b.ctypes.data, c.ctypes.data, d1, n1, o1, h1, d2, n2, o2, h2, n.ctypes.data, o.ctypes.data,
                                  float(grid["spacing"]), w.ctypes.data, st.ctypes.data, None if r2 is None else r2.ctypes.data) == 0
        shape = (int(n[2]), int(n[1]), int(n[0]))
        return w.reshape((3,) + shape), st.reshape(shape), r2[:cn[0] * cn[1] * cn[2]].reshape(cn[2], cn[1], cn[0]) if residual else None


# ---- the numpy restatement ----------------------------------------------------------------------------------------------------
def compose_matrix_numpy(m1, m2):
    """Mc = M1 M2: float64 entries ((a0 b0 + a1 b1) + a2 b2), plus a3 in the last column, rounded to float32 once"""
    a, b = (np.asarray(x, np.float32).astype(np.float64).reshape(4, 4) for x in (m1, m2))
    o = np.zeros((4, 4), np.float32)
    for r in range(3):
        for c in range(4):
            s = (a[r, 0] * b[0, c] + a[r, 1] * b[1, c]) + a[r, 2] * b[2, c]
            o[r, c] = np.float32(s + a[r, 3] if c == 3 else s)
    o[3, 3] = 1.0
    return o


def cell_centres(grid):
    """(cells, 3) float32: origin + ((float)index + 0.5f) * h in float32, x fastest, n - 1 cells per axis"""
    n0, n1, n2 = (int(x) - 1 for x in grid["n"])
    o, h, half = np.asarray(grid["origin"], np.float32), np.float32(grid["spacing"]), np.float32(0.5)
    c, b, a = np.meshgrid(np.arange(n2), np.arange(n1), np.arange(n0), indexing="ij")
    return np.stack([o[0] + (a.ravel().astype(np.float32) + half) * h, o[1] + (b.ravel().astype(np.float32) + half) * h,
                     o[2] + (c.ravel().astype(np.float32) + half) * h], 1)


def _chain_numpy(P1, P2, Pc, field1, field2, yf):
    """(t, c, status bits 0 and 1) at float32 positions yf (n, 3): the contract's chain, float64 one operation at a time"""
    y = yf.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        a = _rows(P1, y)
        v1, in1 = field_at_numpy(field1, yf)
        s = a + v1.astype(np.float64)
        b = _rows(P2, s)
        v2, in2 = field_at_numpy(field2, s.astype(np.float32))
        t = b + v2.astype(np.float64)
        c = _rows(Pc, y)
    st = np.zeros(len(y), np.uint32)
    if field1 is not None:
        st |= np.where(in1, 0, OUTSIDE1).astype(np.uint32)
    if field2 is not None:
        st |= np.where(in2, 0, OUTSIDE2).astype(np.uint32)
    return t, c, st


def compose_numpy(m1, m2, mc, field1, field2, grid):
    """the composite nodes, their status words and the per-cell residual restated, all nodes at once"""
    P1, P2, Pc = affine_inverse_numpy(m1), affine_inverse_numpy(m2), affine_inverse_numpy(mc)
    n0, n1, n2 = (int(x) for x in grid["n"])
    t, c, st = _chain_numpy(P1, P2, Pc, field1, field2, node_positions(grid))
    with np.errstate(invalid="ignore", over="ignore"):
        w = t - c
        bad = ~((w <= MAX_DISP) & (w >= -MAX_DISP)).all(1)
    w[bad] = 0.0
    st[bad] |= ZEROED
    wf = w.astype(np.float32).T.reshape(3, n2, n1, n0).copy()
    z = cell_centres(grid)
    t, c, _ = _chain_numpy(P1, P2, Pc, field1, field2, z)
    wt, _ = field_at_numpy(dict(grid, disp=wf), z)
    with np.errstate(invalid="ignore", over="ignore"):
        e = t - (c + wt.astype(np.float64))
        r2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    return wf, st.reshape(n2, n1, n0), r2.reshape(n2 - 1, n1 - 1, n0 - 1)


def residual_numpy(status, res2, margin):
    """sift3d_compose_residual restated: (cells, rms, max) over the cells at least margin cells from the border none of whose
    corner nodes is zeroed; the sum in index order (np.add.accumulate is sequential); a NaN value never becomes the maximum"""
    z = (np.asarray(status) & ZEROED) != 0
    corner = (z[:-1, :-1, :-1] | z[:-1, :-1, 1:] | z[:-1, 1:, :-1] | z[:-1, 1:, 1:] | z[1:, :-1, :-1] | z[1:, :-1, 1:] | z[1:, 1:, :-1] | z[1:, 1:, 1:])
    keep = ~corner
    m = int(margin)
    inner = np.zeros_like(keep)
    c2, c1, c0 = keep.shape
    if c2 - 2 * m > 0 and c1 - 2 * m > 0 and c0 - 2 * m > 0:
        inner[m:c2 - m, m:c1 - m, m:c0 - m] = True
    vals = np.asarray(res2, np.float64)[keep & inner]   # boolean indexing keeps the index order
    if not len(vals):
        return 0, 0.0, 0.0
    return len(vals), float(np.sqrt(np.add.accumulate(vals)[-1] / len(vals))), float(np.sqrt(np.fmax.reduce(vals, initial=0.0)))


def default_margin(grid, radius=RADIUS):
    return int(np.ceil(float(np.float32(radius)) / float(np.float32(grid["spacing"]))))


# ---- the stage restated --------------------------------------------------------------------------------------------------------
def cpu_compose_field(pkg, co, m1, m2, mc, field1, field2, grid, radius=RADIUS, margin=-1):
    """sift3d_compose_field restated: the oracle's nodes and cells, the report from them, the product's host helper for the fold
    count.  Returns (field dict, report dict without the times)."""
    w, st, r2 = co.compose(m1, m2, mc, field1, field2, grid)
    field = dict(grid, disp=w)
    folds, big = pkg.blockmatch_folds(mc, field)
    cells, rms, worst = residual_numpy(st, r2, default_margin(grid, radius) if margin < 0 else margin)
    rep = {"nodes": int(st.size), "outside1": int(((st & OUTSIDE1) != 0).sum()), "outside2": int(((st & OUTSIDE2) != 0).sum()),
           "zeroed": int(((st & ZEROED) != 0).sum()), "max_disp": big, "folds": folds, "residual_cells": cells, "rms_residual": rms,
           "max_residual": worst}
    return field, rep


def same_compose_report(got, want):
    """the product's report dict against the restatement's: every count and figure, bit for bit"""
    for k, x in want.items():
        assert got[k] == x, (k, got[k], x)


# ---- cases ------------------------------------------------------------------------------------------------------------------------
def written(pkg, m, tmp, tag="m"):
    """m as a reader gets it back: sift3d_write_matrix, sift3d_read_similarity"""
    path = os.path.join(str(tmp), "%s_%d.trans.txt" % (tag, abs(hash(np.asarray(m, np.float32).tobytes())) % (1 << 30)))
    pkg.write_matrix(path, m)
    return pkg.read_similarity(path)


def chain_float64(m1, field1, m2, field2, y):
    """phi2(phi1(y)) in float64 with float64 trilinear weights (the check, not a restatement)"""
    return phi_numpy(m2, field2, phi_numpy(m1, field1, np.asarray(y, np.float64)))


def box_of(grid):
    lo = np.asarray(grid["origin"], np.float64)
    return lo, lo + float(grid["spacing"]) * (np.array(grid["n"]) - 1)


# ---- the synthetic triple of the end-to-end test ----------------------------------------------------------------------------------
WAVELENGTH = 9.0   # voxels of image C; test_compose_cpu.test_one_interpolation_beats_two holds the ratio this gives


def image_c(p, wavelength=WAVELENGTH):
    """image C in closed form at voxel positions p (n, 3), float64: a sum of sines along three oblique directions"""
    k = 2 * np.pi / wavelength
    d = np.array([[0.8, 0.6, 0.0], [-0.36, 0.48, 0.8], [0.48, -0.64, 0.6]])
    q = np.asarray(p, np.float64) @ d.T
    return 100.0 + 40.0 * (np.sin(k * q[:, 0]) + np.sin(k * q[:, 1] + 1.0) + np.sin(k * q[:, 2] + 2.0))


def triple(pkg):
    """Images A (40 x 44 x 48 voxels), B (56^3) and C (64^3) with voxel keys, pair 1 (B moving, A fixed) and pair 2 (C moving, B
    fixed) with sine fields on the grids featResample -i would give them, and the closed-form truth of C on A's grid:
    C(phi2(phi1(key of p)) as a voxel of C)."""
    from invert_cases import forward_field
    from resample_cases import affine, rot
    shape = {"A": (40, 44, 48), "B": (56, 56, 56), "C": (64, 64, 64)}
    vk = pkg.key_vox2key()
    centre = {k: np.asarray(vk, np.float64)[:3, :3] @ ((np.array(s[::-1]) - 1) / 2.0) + np.asarray(vk, np.float64)[:3, 3] for k, s in shape.items()}

    def about(R, s, src, dst, shift):   # moving key -> fixed key: the moving centre lands on the fixed centre plus shift
        m = affine(R, (0, 0, 0), s)
        m[:3, 3] = centre[dst] + np.asarray(shift) - m[:3, :3] @ centre[src]
        return np.array([[float("%f" % x) for x in row] for row in m.astype(np.float32)], np.float32)   # as a .trans.txt holds it
    m1 = about(rot((0.2, 0.9, -0.4), 5.0), 1.04, "B", "A", (1.5, -1.0, 0.5))
    m2 = about(rot((-0.6, 0.3, 0.7), -4.0), 0.97, "C", "B", (-1.0, 2.0, 1.0))
    f1 = forward_field("sine", pkg.blockmatch_grid(shape["A"], vk), amp=1.5, wave=45.0)
    f2 = forward_field("sine", pkg.blockmatch_grid(shape["B"], vk), amp=1.5, wave=50.0)
    nz, ny, nx = shape["C"]
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    vol_c = image_c(np.stack([i.ravel(), j.ravel(), k.ravel()], 1)).reshape(shape["C"]).astype(np.float32)
    nz, ny, nx = shape["A"]
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    pa = np.stack([i.ravel(), j.ravel(), k.ravel()], 1).astype(np.float64)
    vkd = np.asarray(vk, np.float64)
    t = chain_float64(m1, f1, m2, f2, pa @ vkd[:3, :3].T + vkd[:3, 3])
    pc = (t - vkd[:3, 3]) @ np.linalg.inv(vkd[:3, :3]).T
    truth = image_c(pc).reshape(shape["A"])
    interior = np.zeros(shape["A"], bool)
    interior[6:-6, 6:-6, 6:-6] = True
    assert (pc.reshape(shape["A"] + (3,))[interior] > 4).all() and (pc.reshape(shape["A"] + (3,))[interior] < 59).all()
    return {"shape": shape, "vk": vk, "m1": m1, "m2": m2, "f1": f1, "f2": f2, "C": vol_c, "truth": truth, "interior": interior}


def rms_error(img, s):
    d = (np.asarray(img, np.float64) - s["truth"])[s["interior"]]
    return float(np.sqrt(np.mean(d * d)))


def cpu_one_and_two_step(pkg, co, fo, s, tmp):
    """the one-step image (C through the composite pair, the oracle's nodes) and the two-step image (C onto B's grid through pair
    2, that onto A's through pair 1) by the warp oracle, and the composite pair"""
    mc = pkg.compose_matrix(s["m1"], s["m2"])
    mr = written(pkg, mc, tmp, "mc")
    grid = pkg.compose_grid(s["shape"]["A"], s["vk"], s["f1"], s["f2"])
    field, rep = cpu_compose_field(pkg, co, s["m1"], s["m2"], mr, s["f1"], s["f2"], grid)
    Cm, K = pkg.field_warp_terms(s["vk"], s["vk"])
    warp = lambda vol, out, m, f: fo.warp(vol, s["shape"][out], pkg.resample_map(m, s["vk"], s["vk"]), Cm, K, f)
    one = warp(s["C"], "A", mr, field)
    c_on_b = warp(s["C"], "B", s["m2"], s["f2"])
    two = warp(c_on_b, "A", s["m1"], s["f1"])
    return {"mc": mc, "mr": mr, "grid": grid, "field": field, "rep": rep, "one": one, "two": two, "c_on_b": c_on_b}
