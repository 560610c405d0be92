"""GPU suite: the composition of two alignments of DESIGN.md section 7i -- field_compose_kernel and compose_residual_kernel against
the CPU oracle tests/compose_oracle.c bit for bit, sift3d_compose_field against the stage restated in tests/compose_cases.py,
featCompose end to end on a synthetic triple of images, and featResample -u / -r next to the unchanged entry points."""
import ctypes as C

import numpy as np
import pytest

from _helpers import run as _run
from blockmatch_cases import same_field
from compose_cases import (OUTSIDE1, OUTSIDE2, ZEROED, ComposeOracle, cpu_compose_field, cpu_one_and_two_step, rms_error, same_compose_report, triple,
                           written)
from invert_cases import box_grid, forward_field, oblique

pytestmark = pytest.mark.gpu

M1 = oblique(scale=1.07, deg=20.0, axis=(0.3, -0.5, 0.8), trans=(3.0, -2.0, 1.5))
M2 = oblique(scale=0.96, deg=-14.0, axis=(-0.7, 0.2, 0.4), trans=(-4.0, 2.5, 6.0))


@pytest.fixture(scope="module")
def co(tmp_path_factory):
    return ComposeOracle(tmp_path_factory.mktemp("compose_oracle"))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def check_compose(built, co, m1, m2, mr, f1, f2, grid):
    """both kernels against the oracle: node bits, status words, cell bits (a NaN cell is NaN on both sides; which NaN an invalid
    operation makes is the processor's choice, not IEEE's); and the node kernel alone gives the same nodes"""
    w, st, r2 = co.compose(m1, m2, mr, f1, f2, grid)
    gw, gst, gr2 = built.compose_nodes(m1, m2, mr, f1, f2, grid)
    assert gst.shape == st.shape and (gst == st).all(), np.argwhere(gst != st)[:5]
    assert (bits(gw) == bits(w)).all(), np.argwhere(bits(gw) != bits(w))[:5]
    same = (bits(gr2) == bits(r2)) | (np.isnan(gr2) & np.isnan(r2))
    assert gr2.shape == r2.shape and same.all(), np.argwhere(~same)[:5]
    aw, ast, none = built.compose_nodes(m1, m2, mr, f1, f2, grid, residual=False)
    assert none is None and (bits(aw) == bits(w)).all() and (ast == st).all()
    return w, st, r2


def setup(built, tmp, h):
    """test_compose_cpu.setup: the composite grid over the A box 0 .. 40, grid 1 over the same box, grid 2 over its image"""
    mr = written(built, built.compose_matrix(M1, M2), tmp)
    g = box_grid(built, (0, 0, 0), (40, 40, 40), h, radius=5.0)
    g1 = box_grid(built, (0, 0, 0), (40, 40, 40), h, radius=12.0)
    c = np.array([[x, y, z] for x in (0, 40) for y in (0, 40) for z in (0, 40)], np.float64)
    Q = np.linalg.inv(np.asarray(M1, np.float64))
    img = c @ Q[:3, :3].T + Q[:3, 3]
    return mr, g, g1, box_grid(built, img.min(0), img.max(0), h, radius=12.0)


# ---- the kernels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fields", ["both", "first", "second", "none"])
@pytest.mark.parametrize("h", [1.0, 4.0, 7.5])
def test_compose_kernels_cpu_cases(built, co, tmp_path, fields, h):
    mr, g, g1, g2 = setup(built, tmp_path, h)
    f1 = forward_field("smooth", g1, seed=3, amp=2.0, wave=30.0) if fields in ("both", "first") else None
    f2 = forward_field("sine", g2, seed=4, amp=2.0, wave=30.0) if fields in ("both", "second") else None
    w, st, _ = check_compose(built, co, M1, M2, mr, f1, f2, g)
    assert not (st & ZEROED).any() and (f1 is None or np.abs(w).max() > 0.5)


@pytest.mark.parametrize("n", [(2, 2, 2), (9, 7, 5), (17, 8, 4)])
def test_compose_kernels_small_grids(built, co, tmp_path, n):
    """one lane of work per axis, a brick cut on every axis, and two bricks along x with whole bricks along y and z"""
    mr, _, g1, g2 = setup(built, tmp_path, 4.0)
    f1, f2 = forward_field("random", g1, seed=1, amp=1.0), forward_field("random", g2, seed=2, amp=1.0)
    grid = {"n": n, "origin": np.array([3.25, 1.5, 7.0], np.float32), "spacing": np.float32(2.5)}
    w, st, r2 = check_compose(built, co, M1, M2, mr, f1, f2, grid)
    assert (w != 0).all() and r2.shape == tuple(x - 1 for x in n[::-1]) and (r2 > 0).all()


def test_compose_kernels_139_cubed(built, co, tmp_path):
    """139^3 nodes: no multiple of the 8 x 8 x 4 brick on any axis, 2.7 million nodes, 138^3 cells"""
    m1, m2 = oblique(scale=0.96, deg=12.0), M2
    mr = written(built, built.compose_matrix(m1, m2), tmp_path)
    g1 = box_grid(built, (-20, -20, -20), (160, 160, 160), 4.0, radius=8.0)
    g2 = box_grid(built, (-40, -40, -40), (190, 190, 190), 4.0, radius=8.0)
    f1, f2 = forward_field("sine", g1, amp=3.0, wave=80.0), forward_field("sine", g2, amp=2.0, wave=60.0)
    grid = {"n": (139, 139, 139), "origin": np.array([-3.25, 1.5, -2.0], np.float32), "spacing": np.float32(1.0)}
    w, st, r2 = check_compose(built, co, m1, m2, mr, f1, f2, grid)
    assert (st == 0).all() and np.abs(w).max() > 3.0 and r2.max() > 0


def test_compose_kernels_partial_overlap_nan_and_oversized(built, co, tmp_path):
    """a composite grid of which only a part lies in grid 1 and whose intermediate positions leave grid 2; then NaN nodes in both
    fields and a field 1 a hundred times too large"""
    mr, _, g1, _ = setup(built, tmp_path, 4.0)
    g2 = box_grid(built, (5, 5, 5), (30, 30, 30), 4.0, radius=2.0)
    f1, f2 = forward_field("random", g1, seed=6, amp=1.0), forward_field("random", g2, seed=7, amp=1.0)
    grid = {"n": (37, 21, 50), "origin": np.array([20.0, 25.0, 15.0], np.float32), "spacing": np.float32(2.5)}
    w, st, _ = check_compose(built, co, M1, M2, mr, f1, f2, grid)
    for bit in (OUTSIDE1, OUTSIDE2):
        assert 0 < ((st & bit) != 0).sum() < st.size, bit
    assert ((st & OUTSIDE1 == 0) & (st & OUTSIDE2 == 0)).any()
    mr, g, g1, g2 = setup(built, tmp_path, 4.0)
    c1, c2 = forward_field("sine", g1, amp=2.0, wave=40.0), forward_field("sine", g2, amp=2.0, wave=40.0)
    s1, s2 = dict(c1, disp=c1["disp"].copy()), dict(c2, disp=c2["disp"].copy())
    rng = np.random.default_rng(1)
    for f in (s1, s2):
        for c in range(3):
            f["disp"][c][tuple(rng.integers(1, n - 1, 5) for n in f["n"][::-1])] = np.nan
    w, st, r2 = check_compose(built, co, M1, M2, mr, s1, s2, g)
    z = (st & ZEROED) != 0
    assert 0 < z.sum() < z.size / 4 and (w[:, z] == 0).all() and np.isfinite(w).all()
    big = dict(c1, disp=(c1["disp"] * 100.0).astype(np.float32))
    w, st, _ = check_compose(built, co, M1, M2, mr, big, c2, g)
    z = (st & ZEROED) != 0
    assert 0 < z.sum() < z.size and (w[:, z] == 0).all() and np.abs(w).max() <= 128.0


# ---- the stage ----------------------------------------------------------------------------------------------------------------------
def test_stage_equals_cpu(built, co, tmp_path):
    """sift3d_compose_field against the restatement, node bits and report: the end-to-end triple at the defaults, the CPU cases'
    grid with a margin and a radius of its own, one field and none, NaN nodes (zeroed nodes leave their cells out)"""
    s = triple(built)
    mr = written(built, built.compose_matrix(s["m1"], s["m2"]), tmp_path)
    grid = built.compose_grid(s["shape"]["A"], s["vk"], s["f1"], s["f2"])
    got, grep = built.compose_field(s["m1"], s["m2"], mr, s["f1"], s["f2"], grid)
    want, wrep = cpu_compose_field(built, co, s["m1"], s["m2"], mr, s["f1"], s["f2"], grid)
    same_field(got, want)
    same_compose_report(grep, wrep)
    assert grep["kernel_ms"][0] > 0 and grep["kernel_ms"][1] > 0 and grep["residual_cells"] > 0 and grep["zeroed"] == 0
    mr, g, g1, g2 = setup(built, tmp_path, 4.0)
    c1, c2 = forward_field("sine", g1, amp=2.0, wave=40.0), forward_field("sine", g2, amp=2.0, wave=40.0)
    spoiled = dict(c1, disp=c1["disp"].copy())
    spoiled["disp"][1, 7, 8, 9] = np.nan
    for f1, f2, kw in ((c1, c2, dict(margin=0)), (c1, c2, dict(radius=5.0)), (c1, None, dict(margin=2)), (None, c2, {}), (None, None, dict(margin=1)),
                       (spoiled, c2, dict(margin=0))):
        got, grep = built.compose_field(M1, M2, mr, f1, f2, g, **kw)
        want, wrep = cpu_compose_field(built, co, M1, M2, mr, f1, f2, g, **kw)
        same_field(got, want)
        same_compose_report(grep, wrep)
    assert grep["zeroed"] > 0 and grep["residual_cells"] < int(np.prod(np.array(g["n"]) - 1))


def test_compose_refusals(built):
    g = {"n": (8, 8, 8), "origin": np.zeros(3, np.float32), "spacing": np.float32(4.0)}
    sing = M1.copy()
    sing[:3, :3] = 0
    bad_row = M1.copy()
    bad_row[3, 0] = 1
    short = dict(g, n=(1, 8, 8), disp=np.zeros((3, 8, 8, 1), np.float32))
    for fn in (built.compose_nodes, built.compose_field):
        for a, b, c in ((sing, M2, M1), (M1, sing, M1), (M1, M2, sing), (bad_row, M2, M1), (M1, M2, bad_row)):
            with pytest.raises(built.Sift3DError):
                fn(a, b, c, None, None, g)
        for kw in (dict(max_nodes=100), dict(max_nodes=0)):
            with pytest.raises(built.Sift3DError):
                fn(M1, M2, M1, None, None, g, **kw)
        for f1, f2 in ((short, None), (None, short)):
            with pytest.raises(built.Sift3DError):
                fn(M1, M2, M1, f1, f2, g)
        for grid in (dict(g, spacing=np.float32(0.0)), dict(g, n=(8, 0, 8))):
            with pytest.raises(built.Sift3DError):
                fn(M1, M2, M1, None, None, grid, max_nodes=1 << 40)
    with pytest.raises(built.Sift3DError):
        built.compose_field(M1, M2, M1, None, None, dict(g, n=(1, 8, 8)))
    with pytest.raises(built.Sift3DError):
        built.compose_nodes(M1, M2, M1, None, None, dict(g, n=(1, 8, 8)))   # the residual needs cells
    w, st, none = built.compose_nodes(M1, M2, M1, None, None, dict(g, n=(1, 8, 8)), residual=False)
    assert w.shape == (3, 8, 8, 1) and none is None
    for kw in (dict(margin=-2), dict(radius=-1.0), dict(radius=float("nan"))):
        with pytest.raises(built.Sift3DError):
            built.compose_field(M1, M2, M1, None, None, g, **kw)
    # too little room: SIFT3D_ERR_CAPACITY, and the grid stays as the caller set it
    out = built._grid_struct(g)
    err = C.create_string_buffer(256)
    m = [np.ascontiguousarray(x, np.float32) for x in (M1, M2, M1)]
    rc = built.hip_lib().sift3d_compose_field(0, m[0].ctypes.data, m[1].ctypes.data, m[2].ctypes.data, None, None, None, C.byref(out), None, err, len(err))
    assert rc == -4 and tuple(out.n) == (8, 8, 8) and out.spacing == 4.0 and b"1536 floats" in err.value


# ---- the command line -------------------------------------------------------------------------------------------------------------
def write_triple(built, s, tmp):
    for name in "AB":
        built.write_nifti(str(tmp / (name + ".nii")), np.zeros(s["shape"][name], np.float32))
    built.write_nifti(str(tmp / "C.nii"), s["C"])
    for k in "12":
        built.write_matrix(str(tmp / (k + ".trans.txt")), s["m" + k])
        assert np.array_equal(built.read_similarity(str(tmp / (k + ".trans.txt"))), s["m" + k])
        built.write_field(str(tmp / (k + ".field.nii")), s["f" + k])


def test_feat_compose_end_to_end(built, co, tmp_path):
    """featCompose on the synthetic triple: the files it writes are the Python path's and the CPU restatement's, bit for bit;
    featResample -u runs on the composite pair; and C resampled onto A in one step through it is closer to the closed-form truth
    than C resampled onto B and then onto A (test_compose_cpu.test_one_interpolation_beats_two holds the ratio at 0.8 on the CPU
    restatement, whose bits these images have)."""
    from field_cases import FieldOracle
    s = triple(built)
    write_triple(built, s, tmp_path)
    r = _run([built.FEATCOMPOSE, "-d0", "-u1", "1.field.nii", "-u2", "2.field.nii", "A.nii", "1.trans.txt", "2.trans.txt", "out"], tmp_path)
    cpu = cpu_one_and_two_step(built, co, FieldOracle(tmp_path), s, tmp_path)
    built.write_matrix(str(tmp_path / "python.trans.txt"), built.compose_matrix(s["m1"], s["m2"]))
    assert (tmp_path / "out.trans.txt").read_bytes() == (tmp_path / "python.trans.txt").read_bytes()
    mr = built.read_similarity(str(tmp_path / "out.trans.txt"))
    assert np.array_equal(mr, cpu["mr"])
    field = built.read_field(str(tmp_path / "out.field.nii"))
    got, grep = built.compose_field(s["m1"], s["m2"], mr, s["f1"], s["f2"], built.compose_grid(s["shape"]["A"], s["vk"], s["f1"], s["f2"]))
    same_field(field, got)
    same_field(field, cpu["field"])
    same_compose_report(grep, cpu["rep"])
    built.write_field(str(tmp_path / "python.field.nii"), got)
    assert (tmp_path / "out.field.nii").read_bytes() == (tmp_path / "python.field.nii").read_bytes()
    text = (tmp_path / "out.field.txt").read_text().splitlines()
    last = text[-1].split("\t")
    wrep = cpu["rep"]
    assert text[0].startswith("# nodes %d %d %d spacing 4.000000" % field["n"]) and text[0].endswith("radius 20.000000 margin -1")
    assert last[:4] == [str(wrep[k]) for k in ("nodes", "outside1", "outside2", "zeroed")]
    assert last[4] == "%f" % wrep["max_disp"] and last[5:7] == [str(wrep["folds"]), str(wrep["residual_cells"])]
    assert last[7:] == ["%g" % wrep["rms_residual"], "%g" % wrep["max_residual"]]
    assert "Warning" not in r.stdout and wrep["zeroed"] == 0 and wrep["max_residual"] < 0.5
    R = [built.FEATRESAMPLE, "-d0"]
    _run(R + ["-u", "out.field.nii", "A.nii", "C.nii", "out.trans.txt", "one.nii"], tmp_path)
    _run(R + ["-u", "2.field.nii", "B.nii", "C.nii", "2.trans.txt", "c_on_b.nii"], tmp_path)
    _run(R + ["-u", "1.field.nii", "A.nii", "c_on_b.nii", "1.trans.txt", "two.nii"], tmp_path)
    one, two = (built.read_nifti(str(tmp_path / name))[0] for name in ("one.nii", "two.nii"))
    assert one.tobytes() == cpu["one"].tobytes() and two.tobytes() == cpu["two"].tobytes()
    e1, e2 = rms_error(one, s), rms_error(two, s)
    print("featCompose: one step %.4f, two steps %.4f, ratio %.3f" % (e1, e2, e1 / e2))
    assert e1 < e2
    # a coarse grid: at h = 12 the sines of the two fields (amplitude 1.5, wavelengths 45 and 50) are off their trilinear interpolants
    # by up to a (1 - cos(pi h / wavelength)) = 0.50 and 0.41 at a cell centre, so the residual maximum is above half a key unit: the
    # restatement says how far (1.42 over 36 cells), featCompose prints the line with those figures, and the exit status is 0
    coarse = "Warning: the composite field's grid is too coarse: interpolation residual up to %g key units (rms %g over %d cells)"
    r = _run([built.FEATCOMPOSE, "-d0", "-h12", "-u1", "1.field.nii", "-u2", "2.field.nii", "A.nii", "1.trans.txt", "2.trans.txt", "coarse"], tmp_path)
    grid = built.compose_grid(s["shape"]["A"], s["vk"], s["f1"], s["f2"], spacing=12.0)
    want, wrep = cpu_compose_field(built, co, s["m1"], s["m2"], mr, s["f1"], s["f2"], grid)
    same_field(built.read_field(str(tmp_path / "coarse.field.nii")), want)
    assert wrep["max_residual"] > 0.5 and wrep["residual_cells"] > 0 and wrep["zeroed"] == 0
    assert coarse % (wrep["max_residual"], wrep["rms_residual"], wrep["residual_cells"]) in r.stdout and "out of range" not in r.stdout
    # and a field 1 a hundred times too large on it: both warning lines, exit status 0 all the same
    big = dict(s["f1"], disp=(s["f1"]["disp"] * 100.0).astype(np.float32))
    built.write_field(str(tmp_path / "big.field.nii"), big)
    r = _run([built.FEATCOMPOSE, "-d0", "-h12", "-u1", "big.field.nii", "-u2", "2.field.nii", "A.nii", "1.trans.txt", "2.trans.txt", "far"], tmp_path)
    want, wrep = cpu_compose_field(built, co, s["m1"], s["m2"], mr, big, s["f2"], grid)
    same_field(built.read_field(str(tmp_path / "far.field.nii")), want)
    assert wrep["zeroed"] > 0 and "Warning: the composite field is out of range at %d of %d nodes" % (wrep["zeroed"], wrep["nodes"]) in r.stdout
    assert wrep["max_residual"] > 0.5 and wrep["residual_cells"] > 0
    assert coarse % (wrep["max_residual"], wrep["rms_residual"], wrep["residual_cells"]) in r.stdout
    # no fields: the transform alone, and a field that holds the %f residue
    _run([built.FEATCOMPOSE, "-d0", "A.nii", "1.trans.txt", "2.trans.txt", "plain"], tmp_path)
    grid = built.compose_grid(s["shape"]["A"], s["vk"])
    same_field(built.read_field(str(tmp_path / "plain.field.nii")), cpu_compose_field(built, co, s["m1"], s["m2"], mr, None, None, grid)[0])
    assert (tmp_path / "plain.trans.txt").read_bytes() == (tmp_path / "out.trans.txt").read_bytes()


def test_feat_resample_is_unchanged(built, tmp_path):
    """the regression guard: featResample -u and -r -u on a pair of the triple write the bytes the unchanged entry points give, in
    the same run"""
    s = triple(built)
    write_triple(built, s, tmp_path)
    built.write_nifti(str(tmp_path / "B.nii"), s["C"][4:60, 4:60, 4:60])   # -r resamples the fixed image's voxels
    B, Cv, vk = s["C"][4:60, 4:60, 4:60], s["C"], s["vk"]
    R = [built.FEATRESAMPLE, "-d0"]
    _run(R + ["-u", "2.field.nii", "B.nii", "C.nii", "2.trans.txt", "fwd.nii"], tmp_path)
    _run(R + ["-r", "-u", "2.field.nii", "B.nii", "C.nii", "2.trans.txt", "rev.nii"], tmp_path)
    A = built.resample_map(s["m2"], vk, vk)
    assert built.read_nifti(str(tmp_path / "fwd.nii"))[0].tobytes() == built.resample_field(Cv, B.shape, A, s["f2"], vk, vk).tobytes()
    m_inv = built.read_similarity(str(tmp_path / "rev.nii.inv.trans.txt"))
    built.write_matrix(str(tmp_path / "python.inv.trans.txt"), built.affine_invert(s["m2"]))
    assert (tmp_path / "rev.nii.inv.trans.txt").read_bytes() == (tmp_path / "python.inv.trans.txt").read_bytes()
    inv, _ = built.invert_field(s["m2"], m_inv, s["f2"], built.invert_grid(Cv.shape, vk, spacing=float(s["f2"]["spacing"])))
    same_field(built.read_field(str(tmp_path / "rev.nii.inv.field.nii")), inv)
    rmap = built.resample_map(m_inv, vk, vk)
    assert built.read_nifti(str(tmp_path / "rev.nii"))[0].tobytes() == built.resample_field(B, Cv.shape, rmap, inv, vk, vk).tobytes()
