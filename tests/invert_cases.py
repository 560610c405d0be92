"""Shared pieces of the reverse-direction tests (test_invert_cpu.py, test_gpu_invert.py): the CPU oracle tests/invert_oracle.c
(built with cc -O2 -ffp-contract=off into a temporary directory and bound with ctypes), a numpy restatement of the inversion and
of the Jacobian map, the stage of DESIGN.md section 7h restated on the CPU, the forward fields and the scenario's reverse score."""
import ctypes as C
import os

import numpy as np

from _helpers import c_oracle

MAX_ITER, TOL, MAX_DISP = 30, 1e-3, 128.0   # sift3d_invert_defaults, SIFT3D_FIELD_MAX_DISP
CONVERGED, NOT_CONVERGED, DIVERGED = 0, 1, 2


def steps(status):
    return np.asarray(status, np.uint32) & 0xffff


def state(status):
    return np.asarray(status, np.uint32) >> 16


def _field_args(field):
    if field is None:
        return None, None, None, 1.0, ()
    n = np.array(field["n"], np.int64)
    o = np.ascontiguousarray(field["origin"], np.float32)
    d = np.ascontiguousarray(field["disp"], np.float32)
    return d.ctypes.data, n.ctypes.data, o.ctypes.data, float(field["spacing"]), (n, o, d)


class InvertOracle:
    def __init__(self, tmpdir):
        L = c_oracle("invert_oracle", tmpdir)
        P, I64, F = C.c_void_p, C.c_int64, C.c_float
        L.oiv_affine_inverse.restype = C.c_int
        L.oiv_affine_inverse.argtypes = [P, P]
        L.oiv_invert.restype = C.c_int
        L.oiv_invert.argtypes = [P, P, P, P, P, F, P, P, F, C.c_int, F, P, P, P]
        L.oiv_jacobian.restype = None
        L.oiv_jacobian.argtypes = [I64, I64, I64, P, P, P, P, P, P, F, C.c_double, P]
        L.oiv_jacobian_planes.restype = None
        L.oiv_jacobian_planes.argtypes = [I64, I64, I64, P, P, P, P, P, P, F, C.c_double, I64, I64, P]
        self.L = L

    def affine_inverse(self, m):
        a = np.ascontiguousarray(m, np.float32).reshape(16)
        o = np.zeros(16, np.float64)
        return o.reshape(4, 4) if self.L.oiv_affine_inverse(a.ctypes.data, o.ctypes.data) == 0 else None

    def invert(self, m, m_inv, forward, grid, max_iter=MAX_ITER, tol=TOL):
        """(u (3, n2, n1, n0) float32, status (n2, n1, n0) uint32, res2 float64) of the inversion over grid"""
        a, b = (np.ascontiguousarray(x, np.float32).reshape(16) for x in (m, m_inv))
        n = np.array(grid["n"], np.int64)
        o = np.ascontiguousarray(grid["origin"], np.float32)
        N = int(np.prod(n))
        u, st, r2 = np.zeros(3 * N, np.float32), np.zeros(N, np.uint32), np.zeros(N, np.float64)
        fd, fn, fo, fh, _keep = _field_args(forward)
        assert self.L.oiv_invert(a.ctypes.data, b.ctypes.data, fd, fn, fo, fh, n.ctypes.data, o.ctypes.data, float(grid["spacing"]), int(max_iter),
                                 float(tol), u.ctypes.data, st.ctypes.data, r2.ctypes.data) == 0
        shape = (int(n[2]), int(n[1]), int(n[0]))
        return u.reshape((3,) + shape), st.reshape(shape), r2.reshape(shape)

    def jacobian(self, out_shape, A, Cm, K, field, factor, z0=0, z1=None):
        """the map on out_shape = (oz, oy, ox); with z0, z1: its planes [z0, z1) alone"""
        oz, oy, ox = (int(d) for d in out_shape)
        a, c, k = (np.ascontiguousarray(x, np.float32).reshape(-1) for x in (A, Cm, K))
        fd, fn, fo, fh, _keep = _field_args(field)
        if z0 == 0 and z1 is None:
            out = np.empty((oz, oy, ox), np.float32)
            self.L.oiv_jacobian(ox, oy, oz, a.ctypes.data, c.ctypes.data, k.ctypes.data, fd, fn, fo, fh, float(factor), out.ctypes.data)
            return out
        z0, z1 = max(int(z0), 0), oz if z1 is None else min(int(z1), oz)
        out = np.empty((z1 - z0, oy, ox), np.float32)
        self.L.oiv_jacobian_planes(ox, oy, oz, a.ctypes.data, c.ctypes.data, k.ctypes.data, fd, fn, fo, fh, float(factor), z0, z1, out.ctypes.data)
        return out


# ---- the numpy restatement ----------------------------------------------------------------------------------------------------
def affine_inverse_numpy(m):
    """adjugate over determinant, then t' = -((o0 t0 + o1 t1) + o2 t2), in float64 one operation at a time"""
    a = np.asarray(m, np.float32).astype(np.float64).reshape(16)
    c00, c01, c02 = a[5] * a[10] - a[6] * a[9], a[6] * a[8] - a[4] * a[10], a[4] * a[9] - a[5] * a[8]
    det = (a[0] * c00 + a[1] * c01) + a[2] * c02
    o = np.zeros(16)
    o[0], o[1], o[2] = c00 / det, (a[2] * a[9] - a[1] * a[10]) / det, (a[1] * a[6] - a[2] * a[5]) / det
    o[4], o[5], o[6] = c01 / det, (a[0] * a[10] - a[2] * a[8]) / det, (a[2] * a[4] - a[0] * a[6]) / det
    o[8], o[9], o[10] = c02 / det, (a[1] * a[8] - a[0] * a[9]) / det, (a[0] * a[5] - a[1] * a[4]) / det
    for r in range(3):
        o[4 * r + 3] = -((o[4 * r] * a[3] + o[4 * r + 1] * a[7]) + o[4 * r + 2] * a[11])
    o[15] = 1.0
    return o.reshape(4, 4)


def field_at_numpy(field, y):
    """(v (n, 3) float32, inside (n,)) of a field dict at key positions y (n, 3) float32: float32 arithmetic, x then y then z"""
    y = np.asarray(y, np.float32).reshape(-1, 3)
    v = np.zeros_like(y)
    if field is None:
        return v, np.zeros(len(y), bool)
    n = [int(x) for x in field["n"]]
    o, h = np.asarray(field["origin"], np.float32), np.float32(field["spacing"])
    d = np.asarray(field["disp"], np.float32).reshape(3, n[2], n[1], n[0])
    with np.errstate(invalid="ignore"):
        g = (y - o) / h
        inside = np.ones(len(y), bool)
        for r in range(3):
            inside &= (g[:, r] >= np.float32(0)) & (g[:, r] <= np.float32(n[r] - 1))
    g = g[inside]
    fl = np.floor(g)
    w = g - fl
    lo = fl.astype(np.int64)
    hi = np.minimum(lo + 1, np.array(n, np.int64) - 1)
    one = np.float32(1)
    u = one - w
    out = np.empty_like(g)
    for c in range(3):
        at = lambda x, yy, z: d[c][z, yy, x]
        e00 = u[:, 0] * at(lo[:, 0], lo[:, 1], lo[:, 2]) + w[:, 0] * at(hi[:, 0], lo[:, 1], lo[:, 2])
        e10 = u[:, 0] * at(lo[:, 0], hi[:, 1], lo[:, 2]) + w[:, 0] * at(hi[:, 0], hi[:, 1], lo[:, 2])
        e01 = u[:, 0] * at(lo[:, 0], lo[:, 1], hi[:, 2]) + w[:, 0] * at(hi[:, 0], lo[:, 1], hi[:, 2])
        e11 = u[:, 0] * at(lo[:, 0], hi[:, 1], hi[:, 2]) + w[:, 0] * at(hi[:, 0], hi[:, 1], hi[:, 2])
        a, b = u[:, 1] * e00 + w[:, 1] * e10, u[:, 1] * e01 + w[:, 1] * e11
        out[:, c] = u[:, 2] * a + w[:, 2] * b
    v[inside] = out
    return v, inside


def node_positions(grid):
    """(N, 3) float32: origin + (float)index * h in float32, x fastest"""
    n0, n1, n2 = (int(x) for x in grid["n"])
    o, h = np.asarray(grid["origin"], np.float32), np.float32(grid["spacing"])
    c, b, a = np.meshgrid(np.arange(n2), np.arange(n1), np.arange(n0), indexing="ij")
    return np.stack([o[0] + a.ravel().astype(np.float32) * h, o[1] + b.ravel().astype(np.float32) * h, o[2] + c.ravel().astype(np.float32) * h], 1)


def _rows(Mx, p):
    """((m0 p0 + m1 p1) + m2 p2) + m3 per row of a 3 x 4 (or 4 x 4) matrix, in p's precision"""
    return np.stack([((Mx[r, 0] * p[:, 0] + Mx[r, 1] * p[:, 1]) + Mx[r, 2] * p[:, 2]) + Mx[r, 3] for r in range(3)], 1)


def invert_numpy(m, m_inv, forward, grid, max_iter=MAX_ITER, tol=TOL):
    """the iteration restated, all nodes at once with a mask of those still running"""
    m = np.asarray(m, np.float32).reshape(4, 4)
    P, Q, A = affine_inverse_numpy(m_inv), affine_inverse_numpy(m), m[:3, :3].astype(np.float64)
    z = node_positions(grid).astype(np.float64)
    N = len(z)
    base = _rows(P, z)
    u, k = np.zeros((N, 3)), np.zeros(N, np.int64)
    st, rr_out = np.full(N, -1, np.int64), np.zeros(N)
    tol2 = float(np.float32(tol)) * float(np.float32(tol))
    run = np.arange(N)
    with np.errstate(invalid="ignore", over="ignore"):
        while len(run):
            y = base[run] + u[run]
            v, _ = field_at_numpy(forward, y.astype(np.float32))
            lin = _rows(Q, y)
            r = (lin + v.astype(np.float64)) - z[run]
            rr = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
            rr_out[run] = rr
            conv = rr <= tol2
            st[run[conv]] = CONVERGED
            last = ~conv & (k[run] == max_iter)
            st[run[last]] = NOT_CONVERGED
            go = ~conv & ~last
            run, r = run[go], r[go]
            u[run] = u[run] - np.stack([(A[c, 0] * r[:, 0] + A[c, 1] * r[:, 1]) + A[c, 2] * r[:, 2] for c in range(3)], 1)
            k[run] += 1
            bad = ~((u[run] <= MAX_DISP) & (u[run] >= -MAX_DISP)).all(1)
            u[run[bad]] = 0.0
            st[run[bad]] = DIVERGED
            run = run[~bad]
    n0, n1, n2 = (int(x) for x in grid["n"])
    status = (k.astype(np.uint32) | (st.astype(np.uint32) << 16)).reshape(n2, n1, n0)
    return u.astype(np.float32).T.reshape(3, n2, n1, n0).copy(), status, rr_out.reshape(n2, n1, n0)


def warp_q_numpy(p, A, Cm, K, field):
    """the warp's output voxel -> source voxel map at positions p (n, 3) float32, in float32"""
    A, Cm, K = (np.asarray(x, np.float32) for x in (A, Cm, K))
    with np.errstate(invalid="ignore", over="ignore"):
        q = _rows(A.reshape(3, 4), p)
        if field is not None:
            v, inside = field_at_numpy(field, _rows(Cm.reshape(3, 4), p))
            K = K.reshape(3, 3)
            add = np.stack([(K[r, 0] * v[:, 0] + K[r, 1] * v[:, 1]) + K[r, 2] * v[:, 2] for r in range(3)], 1)
            q[inside] = q[inside] + add[inside]
    return q


def jacobian_numpy(out_shape, A, Cm, K, field, factor):
    """J restated: q once on the grid widened by one voxel, central differences times 0.5 in float32, the determinant in float64"""
    oz, oy, ox = (int(d) for d in out_shape)
    k, j, i = np.meshgrid(np.arange(-1, oz + 1), np.arange(-1, oy + 1), np.arange(-1, ox + 1), indexing="ij")
    p = np.stack([i.ravel(), j.ravel(), k.ravel()], 1).astype(np.float32)
    q = warp_q_numpy(p, A, Cm, K, field).reshape(oz + 2, oy + 2, ox + 2, 3)
    half = np.float32(0.5)
    with np.errstate(invalid="ignore", over="ignore"):
        D = [((q[1:-1, 1:-1, 2:] - q[1:-1, 1:-1, :-2]) * half).astype(np.float64),     # column a = x: D[a][..., r]
             ((q[1:-1, 2:, 1:-1] - q[1:-1, :-2, 1:-1]) * half).astype(np.float64),
             ((q[2:, 1:-1, 1:-1] - q[:-2, 1:-1, 1:-1]) * half).astype(np.float64)]
        J = lambda r, a: D[a][..., r]
        det = (J(0, 0) * (J(1, 1) * J(2, 2) - J(1, 2) * J(2, 1)) - J(0, 1) * (J(1, 0) * J(2, 2) - J(1, 2) * J(2, 0))
               + J(0, 2) * (J(1, 0) * J(2, 1) - J(1, 1) * J(2, 0)))
        return (det * float(factor)).astype(np.float32)


# ---- cases ------------------------------------------------------------------------------------------------------------------------
def oblique(scale=1.07, deg=20.0, axis=(0.3, -0.5, 0.8), trans=(3.0, -2.0, 1.5)):
    """a forward 4 x 4 float32 (moving key -> fixed key): a similarity about an oblique axis with scale != 1"""
    from resample_cases import affine, rot
    return affine(rot(axis, deg), trans, scale).astype(np.float32)


def written_inverse(pkg, m, tmp):
    """M' as a reader gets it back: sift3d_affine_invert, sift3d_write_matrix, sift3d_read_similarity"""
    path = os.path.join(str(tmp), "inv_%d.trans.txt" % (abs(hash(np.asarray(m, np.float32).tobytes())) % (1 << 30)))
    pkg.write_matrix(path, pkg.affine_invert(m))
    return pkg.read_similarity(path)


def box_grid(pkg, lo, hi, spacing, radius=20.0):
    """sift3d_field_size over the two corners lo, hi"""
    return pkg.field_size(np.array([lo, hi], np.float32), spacing=spacing, radius=radius)


def forward_field(kind, grid, seed=0, amp=3.0, wave=80.0):
    """a field dict on grid: zero; sine (the scenario's kind: amp, wavelength wave); smooth (a few random long sines); random
    (white noise of standard deviation amp: rough, contraction factor above 1 for small spacings).  sine and smooth fall to 0
    over the outermost 10 key units of the grid, as a fitted field does: outside its grid a field reads 0, and a step at the border
    is a discontinuity of phi that no iteration inverts"""
    rng = np.random.default_rng(seed)
    n0, n1, n2 = (int(x) for x in grid["n"])
    pos = node_positions(grid).astype(np.float64)
    if kind == "zero":
        d = np.zeros((len(pos), 3))
    elif kind == "sine":
        s = 2 * np.pi / wave
        d = amp * np.stack([np.sin(s * pos[:, 1]), np.sin(s * pos[:, 2]), np.sin(s * pos[:, 0])], 1)
    elif kind == "smooth":
        d = np.zeros((len(pos), 3))
        for _ in range(4):
            kvec = rng.normal(0, 2 * np.pi / wave, 3)
            d += rng.normal(0, amp / 2, 3) * np.sin(pos @ kvec + rng.uniform(0, 6.28))[:, None]
    else:
        d = rng.normal(0, amp, (len(pos), 3))
    if kind in ("sine", "smooth"):
        lo = np.asarray(grid["origin"], np.float64)
        hi = lo + float(grid["spacing"]) * (np.array([n0, n1, n2]) - 1)
        d = d * np.clip(np.minimum(pos - lo, hi - pos) / 10.0, 0.0, 1.0).prod(1)[:, None]
    return dict(grid, disp=d.T.astype(np.float32).reshape(3, n2, n1, n0).copy())


def contraction(m, field):
    """the largest 2-norm over the nodes of A . (forward differences of v between neighbouring nodes) / h: above 1 the fixed-point
    step is no contraction somewhere"""
    A = np.asarray(m, np.float64).reshape(4, 4)[:3, :3]
    d = np.asarray(field["disp"], np.float64)
    h = float(field["spacing"])
    big = 0.0
    gx, gy, gz = (np.diff(d, axis=3) / h)[:, :-1, :-1, :], (np.diff(d, axis=2) / h)[:, :-1, :, :-1], (np.diff(d, axis=1) / h)[:, :, :-1, :-1]
    G = np.stack([gx, gy, gz], -1).reshape(3, -1, 3).transpose(1, 0, 2)   # (cells, component, axis)
    G = G[np.isfinite(G).all((1, 2))]
    if len(G):
        big = float(np.linalg.norm(A @ G, 2, axis=(1, 2)).max())
    return big


def phi_numpy(m, forward, y):
    """phi(y) = inv(M) y + v(y) in float64 with float64 trilinear weights (the check of the round trip, not a restatement)"""
    Q = np.linalg.inv(np.asarray(m, np.float64).reshape(4, 4))
    out = y @ Q[:3, :3].T + Q[:3, 3]
    if forward is not None:
        n = np.array(forward["n"], np.int64)
        g = (y - np.asarray(forward["origin"], np.float64)) / float(forward["spacing"])
        inside = ((g >= 0) & (g <= n - 1)).all(1)
        gi = g[inside]
        lo = np.floor(gi).astype(np.int64)
        w = gi - lo
        hi = np.minimum(lo + 1, n - 1)
        d = np.asarray(forward["disp"], np.float64)
        acc = np.zeros((len(gi), 3))
        for cz in (0, 1):
            for cy in (0, 1):
                for cx in (0, 1):
                    ix, iy, iz = (hi if cx else lo)[:, 0], (hi if cy else lo)[:, 1], (hi if cz else lo)[:, 2]
                    wt = (w[:, 0] if cx else 1 - w[:, 0]) * (w[:, 1] if cy else 1 - w[:, 1]) * (w[:, 2] if cz else 1 - w[:, 2])
                    acc += wt[:, None] * d[:, iz, iy, ix].T
        out[inside] += acc
    return out


# ---- the stage restated --------------------------------------------------------------------------------------------------------
def cpu_invert_field(pkg, io, m, m_inv, forward, grid, **params):
    """sift3d_invert_field restated: the oracle's nodes, the report from them, the product's host helper for the fold count.
    Returns (field dict, report dict without the time)."""
    u, st, r2 = io.invert(m, m_inv, forward, grid, params.get("max_iter", MAX_ITER), params.get("tol", TOL))
    field = dict(grid, disp=u)
    s, conv = state(st).ravel(), state(st).ravel() == CONVERGED
    folds, big = pkg.blockmatch_folds(m_inv, field)
    res = r2.ravel()[conv]
    rep = {"nodes": int(st.size), "converged": int(conv.sum()), "not_converged": int((s == NOT_CONVERGED).sum()), "diverged": int((s == DIVERGED).sum()),
           "max_steps": int(steps(st).max()), "rms_residual": float(np.sqrt(np.add.accumulate(res)[-1] / len(res))) if len(res) else 0.0,
           "max_residual": float(np.sqrt(res.max())) if len(res) else 0.0, "max_disp": big, "folds": folds}
    return field, rep


def same_invert_report(got, want):
    """the product's report dict against the restatement's: every count and figure, bit for bit (the sum of the residuals is
    taken in node order on both sides: np.add.accumulate is sequential)"""
    for k, x in want.items():
        assert got[k] == x, (k, got[k], x)


# ---- the scenario, reversed ------------------------------------------------------------------------------------------------------
def reverse_setup(pkg, s, tmp):
    """what the reverse direction of blockmatch_cases.scenario_setup's dict needs: M', the inverse grid at the forward field's
    spacing, the reverse map and the warp terms with the roles swapped"""
    m_inv = written_inverse(pkg, s["T4"], tmp)
    return {"m_inv": m_inv, "A": pkg.resample_map(m_inv, s["mv"], s["fv"]), "terms": pkg.field_warp_terms(s["mv"], s["fv"])}


def supported_grid(pkg, s, field):
    """The scenario's inverse grid.  Outside the fixed volume the forward field is the fit's extrapolation, and where the fit's
    weights fall to its lambda (15 to 20 key units from the nearest sample) it rolls off to 0 so steeply that A grad v exceeds 1:
    the fixed-point step is no contraction there, and nodes whose psi lands in that shell do not converge at any max_iter or
    sensible tol.  No image content constrains either map there.  So the scenario inverts on the largest cube of moving key space,
    centred on the image of the fixed volume's centre voxel and a multiple of the spacing in half-width, whose eight corners map
    through M into the fixed volume's interior (5 voxels from its faces, the region the forward direction is scored on) less
    the forward field's largest |v| plus 2 key units for the displacement itself."""
    n = s["V"].shape[0]
    fv, T = np.asarray(s["fv"], np.float64), np.asarray(s["T4"], np.float64)
    Q, fvi = np.linalg.inv(T), np.linalg.inv(fv)
    h = float(field["spacing"])
    centre = Q[:3, :3] @ (fv[:3, :3] @ np.full(3, (n - 1) / 2.0) + fv[:3, 3]) + Q[:3, 3]
    allowance = float(np.sqrt((np.asarray(field["disp"], np.float64) ** 2).sum(0)).max()) + 2.0
    pad = allowance / np.sqrt(np.abs(np.linalg.det(fv[:3, :3])) ** (2.0 / 3.0))   # the allowance in fixed voxels (isotropic keys)
    a = 0.0
    while True:
        c = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64) * (a + h) + centre
        vox = (c @ T[:3, :3].T + T[:3, 3]) @ fvi[:3, :3].T + fvi[:3, 3]
        if not ((vox >= 5 + pad) & (vox <= n - 6 - pad)).all():
            break
        a += h
    assert a >= 6 * h, a
    lo, hi = centre - a, centre + a
    return pkg.field_size(np.array([lo, hi], np.float32), spacing=h, radius=h / 4)


def reverse_lattice(s, grid):
    """moving voxels (n, 3) on the lattice of field_cases.lattice whose key position lies inside the inverse grid, and their true
    fixed positions x -> A_true x + d(A_true x)"""
    from field_cases import lattice, warp_d
    g = lattice(s["M"].shape[0])
    mv = np.asarray(s["mv"], np.float64)
    key = g @ mv[:3, :3].T + mv[:3, 3]
    lo = np.asarray(grid["origin"], np.float64)
    hi = lo + float(grid["spacing"]) * (np.array(grid["n"]) - 1)
    keep = ((key >= lo) & (key <= hi)).all(1)
    z = g @ s["A_true"][:3, :3].T + s["A_true"][:3, 3]
    return g[keep], (z + warp_d(z))[keep]


def reverse_score(pkg, s, rv, out, field, grid):
    """(correlation, RMS, largest reverse map error in fixed voxels) over the moving voxels inside the inverse grid `grid`: the
    estimated map is A' x + K' u(C' x) with the inverse field, A' x without; the correlation is between `out` (the fixed image on the
    moving grid) and the moving image over every second moving voxel inside the grid"""
    g, true = reverse_lattice(s, grid)
    A = np.asarray(rv["A"], np.float64)
    est = g @ A[:, :3].T + A[:, 3]
    if field is not None:
        Cm, K = rv["terms"]
        kap = (g @ Cm[:, :3].astype(np.float64).T + Cm[:, 3].astype(np.float64)).astype(np.float32)
        est = est + pkg.field_eval(field, kap).astype(np.float64) @ K.astype(np.float64).T
    err = np.linalg.norm(est - true, axis=1)
    N = s["M"].shape[0]
    k, j, i = np.meshgrid(*[np.arange(0, N, 2)] * 3, indexing="ij")
    mv = np.asarray(s["mv"], np.float64)
    key = np.stack([i.ravel(), j.ravel(), k.ravel()], 1).astype(np.float64) @ mv[:3, :3].T + mv[:3, 3]
    lo = np.asarray(grid["origin"], np.float64)
    hi = lo + float(grid["spacing"]) * (np.array(grid["n"]) - 1)
    m = ((key >= lo) & (key <= hi)).all(1)
    c = np.corrcoef(out[::2, ::2, ::2].ravel()[m], s["M"][::2, ::2, ::2].ravel()[m])[0, 1]
    return float(c), float(np.sqrt(np.mean(err * err))), float(err.max()), len(g)
