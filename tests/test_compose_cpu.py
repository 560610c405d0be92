"""CPU suite: the composition of two alignments of DESIGN.md section 7i without a GPU -- the oracle tests/compose_oracle.c against a
numpy restatement, the exact properties of the composite (the %f residue, pure translations, the accuracy of the sampled field
against the float64 chain, inverse consistency, NaN and oversized nodes), the host helpers, and the one-step against the two-step
resampling of the end-to-end triple."""
import numpy as np
import pytest

from compose_cases import (OUTSIDE1, OUTSIDE2, ZEROED, ComposeOracle, box_of, cell_centres, chain_float64, compose_matrix_numpy, compose_numpy,
                           cpu_compose_field, cpu_one_and_two_step, default_margin, residual_numpy, rms_error, triple, written)
from invert_cases import affine_inverse_numpy, box_grid, forward_field, node_positions, oblique


@pytest.fixture(scope="module")
def co(tmp_path_factory):
    return ComposeOracle(tmp_path_factory.mktemp("compose_oracle"))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


M1 = oblique(scale=1.07, deg=20.0, axis=(0.3, -0.5, 0.8), trans=(3.0, -2.0, 1.5))
M2 = oblique(scale=0.96, deg=-14.0, axis=(-0.7, 0.2, 0.4), trans=(-4.0, 2.5, 6.0))


def setup(built, tmp, h, m1=M1, m2=M2):
    """the composite grid over the A box 0 .. 40, grid 1 over the same box, grid 2 over that box's image in B key space; all at h"""
    mr = written(built, built.compose_matrix(m1, m2), tmp)
    g = box_grid(built, (0, 0, 0), (40, 40, 40), h, radius=5.0)
    g1 = box_grid(built, (0, 0, 0), (40, 40, 40), h, radius=12.0)
    c = np.array([[x, y, z] for x in (0, 40) for y in (0, 40) for z in (0, 40)], np.float64)
    Q = np.linalg.inv(np.asarray(m1, np.float64))
    img = c @ Q[:3, :3].T + Q[:3, 3]
    g2 = box_grid(built, img.min(0), img.max(0), h, radius=12.0)
    return mr, g, g1, g2


@pytest.mark.parametrize("fields", ["both", "first", "second", "none"])
@pytest.mark.parametrize("h", [1.0, 4.0, 7.5])
def test_oracle_equals_numpy(built, co, tmp_path, fields, h):
    mr, g, g1, g2 = setup(built, tmp_path, h)
    f1 = forward_field("smooth", g1, seed=3, amp=2.0, wave=30.0) if fields in ("both", "first") else None
    f2 = forward_field("sine", g2, seed=4, amp=2.0, wave=30.0) if fields in ("both", "second") else None
    w, st, r2 = co.compose(M1, M2, mr, f1, f2, g)
    wn, stn, r2n = compose_numpy(M1, M2, mr, f1, f2, g)
    assert (st == stn).all() and (bits(w) == bits(wn)).all() and (bits(r2) == bits(r2n)).all(), (fields, h)
    assert not (st & ZEROED).any() and (f1 is None or np.abs(w).max() > 0.5)
    assert co.compose(M1, M2, mr, f1, f2, g, residual=False)[2] is None


def test_no_fields_gives_the_written_matrix_residue(built, co, tmp_path):
    """no fields: Phi(y) = inv(Mc) y up to rounding, so w(y) = (inv(Mc) - inv(Mc')) y, the %f residue of the written matrix.  With
    E = Mc' - Mc (each entry within 5e-7 of %f plus half a float ulp of the value read back: 2^-24 relative), inv(Mc') - inv(Mc) =
    -inv(Mc') E inv(Mc), so |w|_inf <= |inv(Mc')|_inf |E|_inf (|inv(Mc) y|_inf + 1) over the grid's extent; the double
    arithmetic of the chain and the float of w add below 1e-6."""
    mc = built.compose_matrix(M1, M2)
    mr, g, _, _ = setup(built, tmp_path, 4.0)
    y = node_positions(g).astype(np.float64)
    e = 5e-7 + np.abs(mc.astype(np.float64)) * 2.0 ** -24
    assert (np.abs(mr.astype(np.float64) - mc.astype(np.float64)) <= e).all() and not np.array_equal(mr, mc)
    Pr, Pc = np.linalg.inv(mr.astype(np.float64)), np.linalg.inv(mc.astype(np.float64))
    reach = np.abs(y @ Pc[:3, :3].T + Pc[:3, 3]).max()
    bound = np.abs(Pr[:3, :3]).sum(1).max() * e[:3].sum(1).max() * (reach + 1.0) + 1e-6
    want = (y @ Pc[:3, :3].T + Pc[:3, 3]) - (y @ Pr[:3, :3].T + Pr[:3, 3])
    w, st, r2 = co.compose(M1, M2, mr, None, None, g)
    assert (st == 0).all() and np.abs(w).max() <= bound and 1e-6 < np.abs(want).max() <= bound
    assert np.abs(w.reshape(3, -1).T - want).max() < 1e-6
    assert np.sqrt(r2.max()) < 1e-6   # an affine w is reproduced by the trilinear interpolation up to its float rounding


def test_pure_translations(built, co, tmp_path):
    """M1, M2 translations and v1, v2 the constants c1, c2 around the nodes: Phi(y) = y - t1 + c1 - t2 + c2 and inv(Mc') y =
    y - (t1 + t2) with t1 + t2 representable in %f, so w = c1 + c2 exactly up to the double roundings of sums of magnitude 60
    (a few 1e-14) and the float of w (half an ulp at 2.75: 1.2e-7)."""
    m1, m2 = np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)
    m1[:3, 3], m2[:3, 3] = (3.5, -2.25, 1.0), (-1.5, 4.0, 0.75)
    mc = built.compose_matrix(m1, m2)
    assert np.array_equal(mc[:3, 3], np.array([2.0, 1.75, 1.75], np.float32)) and np.array_equal(written(built, mc, tmp_path), mc)
    c1, c2 = np.array([1.5, -2.25, 0.75], np.float32), np.array([-0.5, 0.5, 2.0], np.float32)
    g1 = box_grid(built, (-60, -60, -60), (100, 100, 100), 4.0, radius=4.0)
    f1 = dict(g1, disp=np.broadcast_to(c1[:, None, None, None], (3,) + g1["n"][::-1]).copy())
    f2 = dict(g1, disp=np.broadcast_to(c2[:, None, None, None], (3,) + g1["n"][::-1]).copy())
    g = box_grid(built, (0, 0, 0), (30, 30, 30), 4.0, radius=2.0)
    w, st, r2 = co.compose(m1, m2, mc, f1, f2, g)
    assert (st == 0).all() and np.abs(w.reshape(3, -1).T - (c1 + c2).astype(np.float64)).max() < 2e-7 and np.sqrt(r2.max()) < 1e-6
    w, _, _ = co.compose(m1, m2, mc, f1, None, g)
    assert np.abs(w.reshape(3, -1).T - c1.astype(np.float64)).max() < 2e-7


@pytest.mark.parametrize("h", [2.0, 4.0])
def test_accuracy_against_the_float64_chain(built, co, tmp_path, h):
    """Mc' + w read through sift3d_field_eval against phi2(phi1(y)) in float64 at random A-key points inside the margin.
    The fields are sines (amplitude a, wave number k, each component along one axis), taken where forward_field's border taper
    is 1.  The trilinear interpolant I of the composite grid obeys, for the norm of the vector (apply the scalar bound to u . w for
    every unit u),
      |I w - w| <= 3 h^2 / 8 max|d^2 w|,  max|d^2 w| <= (|P2| + a2 k2) a1 k1^2 + a2 k2^2 (|P1| + a1 k1)^2   (chain rule),
    |P| the spectral norm: h^2 / 8 times the second derivative along each of the three axes.  The float steps of the contract add:
    s rounded to float before field 2 is read (half an ulp below 128, 3.8e-6, times a2 k2), two float trilinear interpolations of
    values below 8 (7 roundings of 4.8e-7 each), w stored as float (2.4e-7) and read back by a third: below 2e-5 together.  The
    reported residual maximum is |I w - w| at the cell centres in the same arithmetic, so it respects the same bound.
    (v1 and v2 reach the chain as trilinear interpolants of the sines on grids of the same h, not as the sines, so w has kinks at
    their cell faces and the derivation is exact for the chain through the sines only; the fields' own interpolation error is of
    the same order h^2 a k^2 and is NOT added to the bound: the bound asserted is the sines' alone.)
    Figures of the oracle: h = 4 error 0.111, residual maximum 0.138, bound 0.174; h = 2 error 0.0143, residual maximum 0.0162,
    bound 0.0434."""
    a1, a2, wave1, wave2 = 2.0, 1.5, 80.0, 70.0
    k1, k2 = 2 * np.pi / wave1, 2 * np.pi / wave2
    mr, _, _, _ = setup(built, tmp_path, h)
    g1 = box_grid(built, (-30, -30, -30), (70, 70, 70), h, radius=4.0)
    Q1 = np.linalg.inv(M1.astype(np.float64))
    g2 = box_grid(built, Q1[:3, 3] - 90.0, Q1[:3, 3] + 90.0, h, radius=4.0)
    f1, f2 = forward_field("sine", g1, amp=a1, wave=wave1), forward_field("sine", g2, amp=a2, wave=wave2)
    g = box_grid(built, (0, 0, 0), (40, 40, 40), h, radius=8.0)
    n1, n2 = np.linalg.norm(Q1[:3, :3], 2), np.linalg.norm(np.linalg.inv(M2.astype(np.float64))[:3, :3], 2)
    bound = 3 * h * h / 8 * ((n2 + a2 * k2) * a1 * k1 * k1 + a2 * k2 * k2 * (n1 + a1 * k1) ** 2) + 2e-5
    field, rep = cpu_compose_field(built, co, M1, M2, mr, f1, f2, g, radius=8.0)
    assert rep["outside1"] == rep["outside2"] == rep["zeroed"] == 0 and rep["residual_cells"] == int(np.prod(np.array(g["n"]) - 1 - 2 * default_margin(g, 8.0)))
    lo, hi = box_of(g)
    y = np.random.default_rng(7).uniform(lo + 8.0, hi - 8.0, (4000, 3)).astype(np.float32)
    Pr = np.linalg.inv(mr.astype(np.float64))
    got = (y.astype(np.float64) @ Pr[:3, :3].T + Pr[:3, 3]) + built.field_eval(field, y).astype(np.float64)
    want = chain_float64(M1, f1, M2, f2, y)
    # every point and its image stay where the tapers are 1 and inside both grids
    s = y.astype(np.float64) @ Q1[:3, :3].T + Q1[:3, 3]
    for gr, p in ((g1, y), (g2, s)):
        l, u = box_of(gr)
        assert (p > l + 10 + a1).all() and (p < u - 10 - a1).all()
    err = np.linalg.norm(got - want, axis=1).max()
    print("h %g: largest |Mc' + w - chain| %.3g, reported residual max %.3g rms %.3g, bound %.3g" % (h, err, rep["max_residual"], rep["rms_residual"], bound))
    assert err <= bound and rep["max_residual"] <= bound and 0 < rep["rms_residual"] <= rep["max_residual"]
    assert err > 1e-4   # the grid's interpolation error is there to be seen: the residual reports something real


def test_inverse_consistency_on_the_scenario(built, co, tmp_path):
    """Compose the inverse pair (M', u) of test_invert_cpu.py's scenario (the refined field inverted by invert_oracle on
    supported_grid) with the forward pair (M, v): Phi = phi o psi is the identity of moving key space, so Mc' is the identity to %f
    and w is the inverse-consistency error.
    Mc = M' M with M' = inv(M) + D, |D_rc| <= 5e-7 (%f) + 2^-24 |M'_rc| (the float read back), so Mc = I + D M and
    |Mc - I|_rc <= sum_k |D_rk| |M_kc| (+ |D_r3| in the last column) plus the float of the entry; %f of Mc adds 5e-7 + 2^-24 |Mc_rc|
    again.
    At a node z whose inverse node converged, s = inv(M') z + (double)(float)u is the inverse's last iterate up to the float of u
    (half an ulp below 8: 2.4e-7, through |inv(M)| + |grad v| < 2), and the contract's chain from there is the inverse's residual:
    |phi(s) - z| <= tol + 2e-5 (test_invert_cpu.test_round_trip_at_converged_nodes derives the 2e-5).  w = (phi(s) - z) + (z -
    inv(Mc') z) and the second term is computed here from the matrix in float64."""
    from blockmatch_cases import BlockOracle, cpu_refine_intensity, scenario_setup
    from field_cases import FieldOracle
    from invert_cases import CONVERGED, TOL, InvertOracle, reverse_setup, state, supported_grid
    bo, fo, io = BlockOracle(tmp_path), FieldOracle(tmp_path), InvertOracle(tmp_path)
    s = scenario_setup(built, tmp_path, False)
    v, rep = cpu_refine_intensity(built, bo, fo, s["V"], s["M"], s["T4"], s["parent"]["field_dict"], s["fv"], s["mv"])
    m, m_inv = s["T4"], reverse_setup(built, s, tmp_path)["m_inv"]
    grid = supported_grid(built, s, v)
    u, st_inv, _ = io.invert(m, m_inv, v, grid)
    inverse = dict(grid, disp=u)
    mc = built.compose_matrix(m_inv, m)
    mr = written(built, mc, tmp_path)
    md, mi = m.astype(np.float64), m_inv.astype(np.float64)
    D = 5e-7 + 2.0 ** -24 * np.abs(mi[:3])
    lim = D[:, :3] @ np.abs(md[:3])
    lim[:, 3] += D[:, 3]
    lim = lim + 2.0 ** -24 * (np.eye(4)[:3] + lim)
    assert (np.abs(mc.astype(np.float64)[:3] - np.eye(4)[:3]) <= lim).all()
    assert (np.abs(mr.astype(np.float64)[:3] - np.eye(4)[:3]) <= lim + 5e-7 + 2.0 ** -24 * (np.eye(4)[:3] + lim)).all() and np.array_equal(mr[3], [0, 0, 0, 1])
    w, st, r2 = co.compose(m_inv, m, mr, inverse, v, grid)
    z = node_positions(grid).astype(np.float64)
    Pr = np.linalg.inv(mr.astype(np.float64))
    residue = z - (z @ Pr[:3, :3].T + Pr[:3, 3])
    ok = ((state(st_inv) == CONVERGED) & (st == 0)).ravel()
    err = np.linalg.norm(w.reshape(3, -1).T.astype(np.float64) - residue, axis=1)
    print("inverse consistency: %d of %d nodes, largest |w - residue| %.3g, largest |residue| %.3g" % (ok.sum(), ok.size, err[ok].max(), np.abs(residue).max()))
    assert ok.sum() > 0.9 * ok.size and err[ok].max() <= TOL + 2e-5 + 2 * 2.4e-7
    assert np.linalg.norm(w.reshape(3, -1).T, axis=1)[ok].max() <= TOL + 2e-5 + 2 * 2.4e-7 + np.linalg.norm(residue, axis=1).max()


def test_nan_nodes_zero_only_their_readers_and_oversized_fields_are_counted(built, co, tmp_path):
    """NaN nodes in v1 or v2: exactly the composite nodes whose gather reads one (any of the eight corners, weight 0 included) are
    zeroed with bit 2; the others keep the clean run's bits.  Who reads a node is restated here from the clean run's positions.
    A field above 128 sets bit 2 where the composite leaves +-128, and the report counts those nodes."""
    mr, g, g1, g2 = setup(built, tmp_path, 4.0)
    c1, c2 = forward_field("sine", g1, amp=2.0, wave=40.0), forward_field("sine", g2, amp=2.0, wave=40.0)
    w0, st0, _ = co.compose(M1, M2, mr, c1, c2, g)
    y = node_positions(g)
    P1 = affine_inverse_numpy(M1)
    from invert_cases import _rows, field_at_numpy
    s = (_rows(P1, y.astype(np.float64)) + field_at_numpy(c1, y)[0].astype(np.float64)).astype(np.float32)

    def readers(field, pos, spots):
        """the positions whose eight corners include one of the nodes `spots` (x, y, z)"""
        n = np.array(field["n"])
        gg = (pos - np.asarray(field["origin"], np.float32)) / np.float32(field["spacing"])
        inside = ((gg >= 0) & (gg <= (n - 1).astype(np.float32))).all(1)
        lo = np.floor(gg).astype(np.int64)
        hi = np.minimum(lo + 1, n - 1)
        hit = np.zeros(len(pos), bool)
        for sp in spots:
            hit |= inside & ((lo == sp) | (hi == sp)).all(1)
        return hit
    spots = [(5, 6, 7), (9, 9, 4), (7, 12, 10)]
    for which, pos in ((1, y), (2, s)):
        clean = c1 if which == 1 else c2
        bad = dict(clean, disp=clean["disp"].copy())
        for c, (a, b, d) in enumerate(spots):
            bad["disp"][c, d, b, a] = np.nan
        w, st, _ = co.compose(M1, M2, mr, bad if which == 1 else c1, bad if which == 2 else c2, g)
        z = ((st & ZEROED) != 0).ravel()
        want = readers(clean, pos, spots)
        assert 0 < want.sum() < 100 and np.array_equal(z, want), (which, z.sum(), want.sum())
        keep = ~z.reshape(st.shape)
        assert (w[:, ~keep] == 0).all() and (bits(w)[:, keep] == bits(w0)[:, keep]).all() and (st[keep] == st0[keep]).all() and np.isfinite(w).all()
    big = dict(c1, disp=(c1["disp"] * 100.0).astype(np.float32))
    field, rep = cpu_compose_field(built, co, M1, M2, mr, big, c2, g, radius=5.0)
    w, st, _ = co.compose(M1, M2, mr, big, c2, g)
    assert 0 < rep["zeroed"] < rep["nodes"] and rep["zeroed"] == int(((st & ZEROED) != 0).sum()) and (w[:, (st & ZEROED) != 0] == 0).all()
    assert np.abs(field["disp"]).max() <= 128.0 and rep["max_disp"] <= np.sqrt(3) * 128.0


def test_matrix_helpers_and_round_trips(built, co, tmp_path):
    for a, b in ((M1, M2), (M2, M1), (oblique(scale=0.83, trans=(123.456789, -0.0000004, 7.5)), M1)):
        mc = built.compose_matrix(a, b)
        assert mc.dtype == np.float32 and np.array_equal(mc, compose_matrix_numpy(a, b)) and np.array_equal(mc, co.matrix(a, b))
        assert np.allclose(mc.astype(np.float64), a.astype(np.float64) @ b.astype(np.float64), rtol=0, atol=1e-5)
        back = written(built, mc, tmp_path)
        assert np.array_equal(back, np.array([[float("%f" % x) for x in row] for row in mc], np.float32))
        assert np.array_equal(written(built, back, tmp_path), back)   # what a reader got writes the same file again
    bad = M1.copy()
    bad[3, 1] = 0.5
    for a, b in ((bad, M2), (M1, bad), (np.full((4, 4), np.inf, np.float32), M2)):
        with pytest.raises(built.Sift3DError):
            built.compose_matrix(a, b)
    p = built.compose_params()
    assert (p.spacing, p.radius, p.margin, p.max_nodes) == (0.0, 20.0, -1, 1 << 26)
    # the grid: the block matching grid's rule over image A, at field 1's spacing, else field 2's, else 4
    vk = built.key_vox2key((1.0, 1.0, 1.0))
    f1, f2 = dict(box_grid(built, (0, 0, 0), (8, 8, 8), 7.5), disp=None), dict(box_grid(built, (0, 0, 0), (8, 8, 8), 3.0), disp=None)
    for f in (f1, f2):
        f["disp"] = np.zeros((3,) + f["n"][::-1], np.float32)
    for kw, h in ((dict(field1=f1, field2=f2), 7.5), (dict(field2=f2), 3.0), ({}, 4.0), (dict(field1=f1, spacing=5.0), 5.0)):
        g, b = built.compose_grid((64, 100, 128), vk, **kw), built.blockmatch_grid((64, 100, 128), vk, spacing=h)
        assert g["n"] == b["n"] and np.array_equal(g["origin"], b["origin"]) and g["spacing"] == b["spacing"] == np.float32(h)
    with pytest.raises(built.Sift3DError):
        built.compose_grid((128, 128, 128), max_nodes=1000)
    # the reduction: the margin, the zeroed corners, the order
    rng = np.random.default_rng(2)
    n = (9, 8, 7)
    st = np.zeros(n[::-1], np.uint32)
    st[3, 4, 5] = ZEROED | OUTSIDE1
    st[1, 1, 1] = OUTSIDE2
    r2 = rng.uniform(0, 1, (n[2] - 1, n[1] - 1, n[0] - 1))
    for margin in (0, 1, 2, 3, 50):
        got, want = built.compose_residual(n, st, r2, margin), residual_numpy(st, r2, margin)
        assert got == want, (margin, got, want)
    assert built.compose_residual(n, st, r2, 0)[0] == 8 * 7 * 6 - 8 and built.compose_residual(n, st, r2, 3)[0] == 0


def test_one_interpolation_beats_two(built, co, tmp_path):
    """The end-to-end triple on the CPU: C resampled onto A through the composite pair (one interpolation of the image) against C
    resampled onto B and that onto A (two), each against the closed-form truth over A's interior.  The image wavelength of
    compose_cases.WAVELENGTH was chosen here so that the ratio of the two RMS errors is at most 0.8: the one-step image pays for the
    composite grid's interpolation residual (a position error, times the image gradient ~ 1 / wavelength), the two-step image for
    a second trilinear interpolation of the image (~ 1 / wavelength^2), so short wavelengths favour one step."""
    from field_cases import FieldOracle
    s = triple(built)
    r = cpu_one_and_two_step(built, co, FieldOracle(tmp_path), s, tmp_path)
    one, two = rms_error(r["one"], s), rms_error(r["two"], s)
    print("one step %.4f, two steps %.4f, ratio %.3f; composite report %s" % (one, two, one / two, r["rep"]))
    assert r["rep"]["zeroed"] == 0 and r["rep"]["max_residual"] < 0.5
    assert one / two <= 0.8 and two < 0.2 * 40.0   # both are resamplings of C, not noise: far below the sines' amplitude
