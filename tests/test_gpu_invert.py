"""GPU suite: the reverse direction of DESIGN.md section 7h -- field_invert_kernel and both forms of jacobian_map_kernel against the
CPU oracle tests/invert_oracle.c bit for bit, sift3d_invert_field against the stage restated in tests/invert_cases.py, and
featResample -r / -j end to end.  The serial oracle takes a few seconds on the 139^3-node grid and on the 256^3 Jacobian map."""
import numpy as np
import pytest

from _helpers import run as _run
from invert_cases import (CONVERGED, DIVERGED, MAX_ITER, NOT_CONVERGED, TOL, InvertOracle, box_grid, cpu_invert_field, forward_field, oblique,
                          reverse_setup, same_invert_report, state, steps, written_inverse)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def io(tmp_path_factory):
    return InvertOracle(tmp_path_factory.mktemp("invert_oracle"))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def check_invert(built, io, m, m_inv, field, grid, max_iter=MAX_ITER, tol=TOL):
    u, st, r2 = io.invert(m, m_inv, field, grid, max_iter, tol)
    gu, gst, gr2 = built.invert_nodes(m, m_inv, field, grid, max_iter=max_iter, tol=tol)
    assert gst.shape == st.shape and (gst == st).all(), (np.argwhere(gst != st)[:5], max_iter, tol)
    assert (bits(gu) == bits(u)).all() and (bits(gr2) == bits(r2)).all(), (np.argwhere(bits(gu) != bits(u))[:5], max_iter, tol)
    return u, st, r2


def grids(built, m, h, radius=12.0):
    """test_invert_cpu.grids: a forward grid over the fixed box 0 .. 40, an inverse grid over its image in moving key space"""
    fwd = box_grid(built, (0, 0, 0), (40, 40, 40), h, radius=radius)
    c = np.array([[x, y, z] for x in (0, 40) for y in (0, 40) for z in (0, 40)], np.float64)
    Q = np.linalg.inv(np.asarray(m, np.float64))
    img = c @ Q[:3, :3].T + Q[:3, 3]
    return fwd, box_grid(built, img.min(0), img.max(0), h, radius=5.0)


# ---- the inversion kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["smooth", "sine", "zero", "none", "random"])
@pytest.mark.parametrize("h", [1.0, 4.0, 7.5])
def test_invert_kernel_cpu_cases(built, io, tmp_path, kind, h):
    """the cases of test_invert_cpu.py (and a rough field whose nodes stop in all three states), max_iter 1 and 30, tol 1e-3 and 0"""
    m = oblique()
    m_inv = written_inverse(built, m, tmp_path)
    fwd, inv = grids(built, m, h)
    field = None if kind == "none" else forward_field(kind, fwd, seed=3, amp=6.0 if kind == "random" else 2.0, wave=30.0)
    for max_iter in (1, MAX_ITER):
        for tol in (TOL, 0.0):
            u, st, r2 = check_invert(built, io, m, m_inv, field, inv, max_iter, tol)
            if tol == 0.0:   # every node runs to max_iter, but for one whose residual is exactly 0 or that diverged on the way
                assert ((steps(st) == max_iter) | (r2 == 0) | (state(st) == DIVERGED)).all()
    if kind == "random" and h == 1.0:
        s = state(check_invert(built, io, m, m_inv, field, inv)[1])
        assert (s == CONVERGED).any() and (s == NOT_CONVERGED).any()


def test_invert_kernel_139_cubed(built, io, tmp_path):
    """139^3 nodes: no multiple of the 8 x 8 x 4 brick on any axis, 2.7 million nodes"""
    m = oblique(scale=0.96, deg=12.0)
    m_inv = written_inverse(built, m, tmp_path)
    fwd = box_grid(built, (-20, -20, -20), (150, 150, 150), 4.0, radius=8.0)
    field = forward_field("sine", fwd, amp=3.0, wave=80.0)
    inv = {"n": (139, 139, 139), "origin": np.array([-3.25, 1.5, -2.0], np.float32), "spacing": np.float32(1.0)}
    u, st, _ = check_invert(built, io, m, m_inv, field, inv)
    assert (state(st) == CONVERGED).all() and 3 <= steps(st).max() < MAX_ITER and np.abs(u).max() > 2.0


def test_invert_kernel_partial_overlap_and_nan(built, io, tmp_path):
    """an inverse grid of which only a corner maps into the forward grid, whose border is no zero (a step at the border); then NaN
    forward nodes"""
    m = oblique()
    m_inv = written_inverse(built, m, tmp_path)
    fwd = box_grid(built, (0, 0, 0), (40, 40, 40), 4.0, radius=4.0)
    field = forward_field("random", fwd, seed=6, amp=1.0)
    inv = {"n": (37, 21, 50), "origin": np.array([20.0, 25.0, 15.0], np.float32), "spacing": np.float32(2.5)}
    u, st, _ = check_invert(built, io, m, m_inv, field, inv)
    assert ((u != 0).any(0)).mean() < 0.5 and (u != 0).any()
    clean = forward_field("sine", fwd, amp=2.0, wave=40.0)
    spoiled = dict(clean, disp=clean["disp"].copy())
    rng = np.random.default_rng(1)
    for c in range(3):
        spoiled["disp"][c][tuple(rng.integers(1, n - 1, 5) for n in fwd["n"][::-1])] = np.nan
    _, inv2 = grids(built, m, 4.0)
    u, st, _ = check_invert(built, io, m, m_inv, spoiled, inv2)
    div = state(st) == DIVERGED
    assert 0 < div.sum() < div.size and (u[:, div] == 0).all() and np.isfinite(u).all()


def test_invert_refusals(built):
    m = oblique()
    g = {"n": (8, 8, 8), "origin": np.zeros(3, np.float32), "spacing": np.float32(4.0)}
    sing = m.copy()
    sing[:3, :3] = 0
    bad_row = m.copy()
    bad_row[3, 0] = 1
    for a, b, kw in ((sing, m, {}), (m, sing, {}), (bad_row, m, {}), (m, m, dict(max_iter=0)), (m, m, dict(max_iter=70000)), (m, m, dict(tol=-1.0)),
                     (m, m, dict(tol=float("nan"))), (m, m, dict(max_nodes=100))):
        for fn in (built.invert_nodes, built.invert_field):
            with pytest.raises(built.Sift3DError):
                fn(a, b, None, g, **kw)
    with pytest.raises(built.Sift3DError):
        built.invert_field(m, m, None, dict(g, n=(1, 8, 8)))
    with pytest.raises(built.Sift3DError):
        built.invert_nodes(m, m, None, dict(g, spacing=np.float32(0.0)))
    with pytest.raises(built.Sift3DError):
        built.invert_nodes(m, m, dict(g, n=(1, 8, 8), disp=np.zeros((3, 8, 8, 1), np.float32)), g)
    for kw in (dict(form=2), dict(form=-2)):
        with pytest.raises(built.Sift3DError):
            built.jacobian_map((4, 4, 4), m[:3], **kw)
    with pytest.raises(built.Sift3DError):
        built.jacobian_map((4, 0, 4), m[:3])
    with pytest.raises(built.Sift3DError):
        built.jacobian_map((4, 4, 4), m[:3], src_vox2key=sing)


# ---- the Jacobian kernel --------------------------------------------------------------------------------------------------------
def check_jacobian(built, io, shape, A, fv, mv, field):
    Cm, K = built.field_warp_terms(fv, mv)
    want = io.jacobian(shape, A, Cm, K, field, built.jacobian_factor(fv, mv))
    for form in (0, 1, -1):
        got = built.jacobian_map(shape, A, fv, mv, field, form=form)
        # a NaN J is NaN on both sides; which NaN (sign, payload) an invalid operation makes is the processor's choice, not IEEE's
        same = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))
        assert got.shape == want.shape and same.all(), (form, np.argwhere(~same)[:5])
    return want


WORLD_F = np.array([[0.9, 0.1, 0, -40], [-0.1, 0.9, 0.05, 20], [0, -0.05, 1.8, 10], [0, 0, 0, 1]], np.float32)
WORLD_M = np.array([[1.2, 0, 0.1, 5], [0, 1.1, 0, -30], [-0.1, 0, 0.7, 12], [0, 0, 0, 1]], np.float32)


@pytest.mark.parametrize("shape", [(1, 1, 1), (129, 5, 37), (33, 67, 130)])
@pytest.mark.parametrize("kind", ["random", "nan", "none"])
@pytest.mark.parametrize("world", [False, True])
def test_jacobian_kernel(built, io, shape, kind, world):
    """(nz, ny, nx) = 1^3, 37 x 5 x 129 and 130 x 67 x 33: bricks cut on every axis; random nodes, NaN nodes, no field; voxel keys
    and the -w geometry"""
    m = oblique()
    fv = built.key_vox2key((0.9, 0.9, 1.8), WORLD_F) if world else None
    mv = built.key_vox2key((1.2, 1.1, 0.7), WORLD_M) if world else None
    A = built.resample_map(m, fv, mv)
    field = None
    if kind != "none":
        corners = np.array([[x, y, z] for x in (0, shape[2] - 1) for y in (0, shape[1] - 1) for z in (0, shape[0] - 1)], np.float32)
        Cf = np.eye(4, dtype=np.float32) if fv is None else fv
        keys = corners @ Cf[:3, :3].T + Cf[:3, 3]
        grid = built.field_size(keys, spacing=4.0, radius=3.0)   # smaller than the volume's reach: voxels outside the grid too
        field = forward_field("random", grid, seed=2, amp=1.5)
        if kind == "nan":
            rng = np.random.default_rng(3)
            for c in range(3):
                field["disp"][c][tuple(rng.integers(0, n, 4) for n in grid["n"][::-1])] = np.nan
    J = check_jacobian(built, io, shape, A, fv, mv, field)
    if kind == "nan":
        assert np.isnan(J).any() and (shape == (1, 1, 1) or np.isfinite(J).any())
    if kind == "random" and shape != (1, 1, 1):
        assert (J <= 0).any() and (J > 0).any()


def test_jacobian_kernel_256_cubed(built, io):
    m = oblique()
    grid = box_grid(built, (0, 0, 0), (255, 255, 255), 4.0)
    field = forward_field("sine", grid, amp=3.0, wave=80.0)
    J = check_jacobian(built, io, (256, 256, 256), built.resample_map(m), None, None, field)
    assert (J > 0).all() and J.std() > 0.01


@pytest.mark.parametrize("shape", [(11, 19, 37), (8, 16, 40)])
def test_jacobian_no_field_equals_zero_field(built, shape):
    """(nz, ny, nx) = 11 x 19 x 37 (rows cut in x: the scalar store) and 8 x 16 x 40 (whole float4 rows): the map without a field
    has the bytes of the map through a zero field of two nodes per axis that covers part of the output, in both forms.  (The zero
    field adds +0 to a position, which changes bits only where the position is exactly -0; the oblique map has no such voxel.)"""
    A = built.resample_map(oblique())
    zero = {"n": (2, 2, 2), "origin": np.zeros(3, np.float32), "spacing": np.float32(20.0), "disp": np.zeros((3, 2, 2, 2), np.float32)}
    for form in (0, 1):
        none = built.jacobian_map(shape, A, None, None, None, form=form)
        got = built.jacobian_map(shape, A, None, None, zero, form=form)
        assert got.shape == none.shape and (bits(got) == bits(none)).all(), (form, np.argwhere(bits(got) != bits(none))[:5])


# ---- the stage ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [False, True])
def test_stage_equals_cpu_on_the_scenario(built, io, tmp_path, world):
    """sift3d_invert_field on the scenario's refined field (section 7f's stage on the GPU) against the restatement, node bits and
    report: on the default grid (where the nodes outside the fixed image's support are reported as not converged, see
    test_invert_cpu.test_reverse_scenario_cpu), with few steps, at another spacing, and on the CPU suite's grid, where every node
    converges"""
    from blockmatch_cases import same_field, scenario_setup
    from invert_cases import supported_grid
    s = scenario_setup(built, tmp_path, world)
    field, rep = built.refine_field_intensity(s["V"], s["M"], s["T4"], s["parent"]["field_dict"], s["fv"], s["mv"])
    assert rep["rounds"] == 2
    rv = reverse_setup(built, s, tmp_path)
    for kw in ({}, dict(max_iter=3, tol=1e-5), dict(spacing=7.5)):
        grid = built.invert_grid(s["M"].shape, s["mv"], **{k: v for k, v in kw.items() if k == "spacing"})
        got, grep = built.invert_field(s["T4"], rv["m_inv"], field, grid, **kw)
        want, wrep = cpu_invert_field(built, io, s["T4"], rv["m_inv"], field, grid, **kw)
        same_field(got, want)
        same_invert_report(grep, wrep)
        assert grep["kernel_ms"] > 0
        if not kw:
            assert grep["converged"] > 0.99 * grep["nodes"] and grep["diverged"] == 0
        if "max_iter" in kw:
            assert grep["not_converged"] > 0 and grep["max_steps"] == 3
    grid = supported_grid(built, s, field)
    got, grep = built.invert_field(s["T4"], rv["m_inv"], field, grid)
    want, wrep = cpu_invert_field(built, io, s["T4"], rv["m_inv"], field, grid)
    same_field(got, want)
    same_invert_report(grep, wrep)
    assert grep["converged"] == grep["nodes"] and grep["folds"] == 0 and grep["max_steps"] < MAX_ITER


# ---- the command line -------------------------------------------------------------------------------------------------------------
def _voxels(built, path):
    return built.read_nifti(str(path))[0]


@pytest.mark.parametrize("world", [False, True])
def test_end_to_end_reverse(built, io, tmp_path, world):
    """featExtract, featMatchMultiple -a -e -u, then featResample in every new form next to the old ones, in one run:
    -r alone = sift3d_resample_affine with the map of the written inverse; -r -u and -i -r -j = the CPU oracle's inverse of the field
    that was used, resampled through sift3d_resample_field, the Jacobian maps = the oracle's; the swapped command on the written
    .inv pair = -r's voxels; and -u and -i without -r and -j write what they wrote before (the voxels of the unchanged entry points,
    the same field files)."""
    from blockmatch_cases import same_field
    from field_cases import nonrigid_volumes
    fixed, moving, V, M, A_true, vox_v, vox_m, hv, hm = nonrigid_volumes(built, tmp_path, world)
    opt = ["-w"] if world else []
    _run([built.FEATEXTRACT, "-d0"] + opt + [fixed, "fixed.key"], tmp_path)
    _run([built.FEATEXTRACT, "-d0"] + opt + [moving, "moving.key"], tmp_path)
    _run([built.FEATMATCH, "-a", "-e", "-u", "fixed.key", "moving.key"], tmp_path)
    trans, fpath = str(tmp_path / "moving.key.trans.txt"), str(tmp_path / "moving.key.field.nii")
    R = [built.FEATRESAMPLE, "-d0"] + opt
    _run(R + ["-u", fpath, fixed, moving, trans, "out_u.nii"], tmp_path)
    _run(R + ["-i", "-u", fpath, fixed, moving, trans, "out_i.nii"], tmp_path)
    _run(R + ["-r", fixed, moving, trans, "rev.nii"], tmp_path)
    _run(R + ["-r", "-u", fpath, fixed, moving, trans, "rev_u.nii"], tmp_path)
    r = _run(R + ["-i", "-r", "-j", "-u", fpath, fixed, moving, trans, "rev_i.nii"], tmp_path)
    _run(R + ["-j", "-u", fpath, fixed, moving, trans, "fwd_j.nii"], tmp_path)
    _run(R + ["-j", "-r", fixed, moving, trans, "rev_j.nii"], tmp_path)
    _run(R + ["-u", str(tmp_path / "rev_u.nii.inv.field.nii"), moving, fixed, str(tmp_path / "rev_u.nii.inv.trans.txt"), "swapped.nii"], tmp_path)
    T4 = built.read_similarity(trans)
    fv = built.key_vox2key(vox_v, hv["qto_xyz"] if world else None)
    mv = built.key_vox2key(vox_m, hm["qto_xyz"] if world else None)
    A = built.resample_map(T4, fv, mv)
    field_u = built.read_field(fpath)
    # without -r and -j: what the commands wrote before
    assert _voxels(built, tmp_path / "out_u.nii").tobytes() == built.resample_field(M, V.shape, A, field_u, fv, mv).tobytes()
    field_i = built.read_field(str(tmp_path / "out_i.nii.field.nii"))
    same_field(field_i, built.refine_field_intensity(V, M, T4, field_u, fv, mv)[0])
    assert _voxels(built, tmp_path / "out_i.nii").tobytes() == built.resample_field(M, V.shape, A, field_i, fv, mv).tobytes()
    assert not (tmp_path / "out_u.nii.inv.trans.txt").exists() and not (tmp_path / "out_i.nii.jac.nii").exists()
    # -r alone: the written inverse, the affine resampler
    m_inv = built.read_similarity(str(tmp_path / "rev.nii.inv.trans.txt"))
    assert np.array_equal(m_inv, written_inverse(built, T4, tmp_path))
    rmap = built.resample_map(m_inv, mv, fv)
    out, hdr = built.read_nifti(str(tmp_path / "rev.nii"))
    assert hdr["dims"][:3] == M.shape[::-1] and out.tobytes() == built.resample_affine(V, M.shape, rmap).tobytes()
    assert not (tmp_path / "rev.nii.inv.field.nii").exists()
    # -r -u, and -i -r -j (the forward field refined first, still written)
    same_field(built.read_field(str(tmp_path / "rev_i.nii.field.nii")), field_i)
    Cm, K = built.field_warp_terms(mv, fv)
    fac = built.jacobian_factor(mv, fv)
    for name, fwd in (("rev_u.nii", field_u), ("rev_i.nii", field_i)):
        assert np.array_equal(built.read_similarity(str(tmp_path / (name + ".inv.trans.txt"))), m_inv)
        inv = built.read_field(str(tmp_path / (name + ".inv.field.nii")))
        grid = built.invert_grid(M.shape, mv, spacing=float(fwd["spacing"]))
        want, wrep = cpu_invert_field(built, io, T4, m_inv, fwd, grid)
        same_field(inv, want)
        assert _voxels(built, tmp_path / name).tobytes() == built.resample_field(V, M.shape, rmap, inv, mv, fv).tobytes()
        last = (tmp_path / (name + ".inv.field.txt")).read_text().splitlines()[-1].split("\t")
        assert last[:5] == [str(wrep[k]) for k in ("nodes", "converged", "not_converged", "diverged", "max_steps")] and last[8] == str(wrep["folds"])
        if name == "rev_i.nii":   # a warning line with the counts where nodes stopped short, and exit status 0 all the same
            stopped = wrep["not_converged"] + wrep["diverged"]
            assert ("Warning: the inverse field did not converge everywhere: %d of %d nodes not converged, %d diverged"
                    % (wrep["not_converged"], wrep["nodes"], wrep["diverged"]) in r.stdout) == (stopped > 0)
    inv_i = built.read_field(str(tmp_path / "rev_i.nii.inv.field.nii"))
    J, jh = built.read_nifti(str(tmp_path / "rev_i.nii.jac.nii"))
    assert jh["dims"][:3] == M.shape[::-1] and (bits(J) == bits(io.jacobian(M.shape, rmap, Cm, K, inv_i, fac))).all() and np.isfinite(J).all()
    # -j alone: the forward map on the fixed grid; -j -r without a field: the constant of the inverse transform
    Cf, Kf = built.field_warp_terms(fv, mv)
    J, jh = built.read_nifti(str(tmp_path / "fwd_j.nii.jac.nii"))
    assert jh["dims"][:3] == V.shape[::-1] and (bits(J) == bits(io.jacobian(V.shape, A, Cf, Kf, field_u, built.jacobian_factor(fv, mv)))).all()
    assert _voxels(built, tmp_path / "fwd_j.nii").tobytes() == _voxels(built, tmp_path / "out_u.nii").tobytes()
    J = _voxels(built, tmp_path / "rev_j.nii.jac.nii")
    assert (bits(J) == bits(io.jacobian(M.shape, rmap, Cm, K, None, fac))).all()
    assert np.abs(J / np.linalg.det(T4[:3, :3].astype(np.float64)) - 1).max() < 2e-4
    assert _voxels(built, tmp_path / "rev_j.nii").tobytes() == out.tobytes()
    # the swapped command on the written pair
    assert _voxels(built, tmp_path / "swapped.nii").tobytes() == _voxels(built, tmp_path / "rev_u.nii").tobytes()
