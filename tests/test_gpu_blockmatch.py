"""GPU suite: the intensity refinement of DESIGN.md section 7f -- block_match_kernel against the CPU oracle
tests/blockmatch_oracle.c bit for bit, sift3d_refine_field_intensity against the stage restated in tests/blockmatch_cases.py,
featResample -i, and the nonrigid scenario end to end.  The serial oracle is what takes the time here: about 5 s for the 128^3
volume at the defaults and for the 256^3 volume at stride 8 (30 000 nodes each), and about 15 s for the restated stage on the
256^3 pair (two rounds of warp, search and two brute-force fits); the two end-to-end cases take 15 - 20 s each."""
import numpy as np
import pytest

from _helpers import run as _run
from blockmatch_cases import (BlockOracle, cpu_refine_intensity, lattice_numpy, same_field, same_report, scenario_score, scenario_setup,
                              shifts, volume, zero_field)
from field_cases import FieldOracle, nonrigid_volumes
from refine_cases import scenario_map

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bo(tmp_path_factory):
    return BlockOracle(tmp_path_factory.mktemp("blockmatch_oracle"))


@pytest.fixture(scope="module")
def fo(tmp_path_factory):
    return FieldOracle(tmp_path_factory.mktemp("field_oracle"))


def pair(kind, shape, seed, spoil=0):
    """F and a W that is F moved by up to 2 voxels per axis in three slabs plus noise (constant: W = F); spoil: that many NaN /
    +inf / -inf voxels in each"""
    rng = np.random.default_rng(seed)
    F = volume(kind, shape, seed)
    W = F.copy()
    if kind != "constant":
        nz = shape[0]
        for i, s in enumerate(((1, 0, -1), (0, 2, 1), (-2, -1, 0))):
            sl = slice(i * nz // 3, (i + 1) * nz // 3)
            W[sl] = np.roll(F, s, (0, 1, 2))[sl]
        W += rng.normal(0, 0.02 * float(F.std()), shape).astype(np.float32)
    for vol in (F, W):
        for bad in (np.nan, np.inf, -np.inf)[:3 if spoil else 0]:
            idx = tuple(rng.integers(0, n, spoil) for n in shape)
            vol[idx] = bad
    return F, W


def check(built, bo, F, W, first, stride, count, b, r, both=False):
    want = bo.match(F, W, first, stride, count, b, r)
    got = built.block_match(F, W, first, stride, count, b, r)
    assert got.shape == want.shape
    assert got.tobytes() == want.tobytes(), (np.argwhere((got != want).any(-1))[:5], first, stride, count, b, r)
    if both:   # the kernel's form for any b, r, and the specialised form without packed arithmetic
        for form in (1, 2):
            assert built.block_match(F, W, first, stride, count, b, r, generic=form).tobytes() == want.tobytes(), form
    return want


@pytest.mark.parametrize("b", [1, 4, 6])
@pytest.mark.parametrize("r", [1, 3, 4])
def test_kernel_16_cubed_every_voxel_a_node(built, bo, b, r):
    """16^3, stride 1, a node on every voxel: most nodes' windows leave the volume and are flagged"""
    F, W = pair("random", (16, 16, 16), 10 * b + r)
    w = check(built, bo, F, W, (0, 0, 0), 1, (16, 16, 16), b, r, both=True)
    assert (w[..., 3] == 0).sum() == max(16 - 2 * (b + r), 0) ** 3


@pytest.mark.parametrize("kind", ["random", "smooth", "constant"])
@pytest.mark.parametrize("b,r,stride", [(1, 1, 1), (1, 3, 1), (4, 1, 4), (4, 3, 4), (6, 4, 7), (4, 4, 5), (6, 3, 4)])
def test_kernel_non_cubic(built, bo, kind, b, r, stride):
    """37 x 21 x 50: counts that are no multiple of the workgroup's brick; with b + r = 10 the window fills y exactly"""
    shape = (50, 21, 37)
    F, W = pair(kind, shape, 3)
    first, count = lattice_numpy(shape, stride, b, r)
    w = check(built, bo, F, W, first, stride, count, b, r, both=True)
    assert (w[..., 3] == 0).all()
    if kind == "constant":
        assert (shifts(w) == 0).all() and (w[..., 4] == 0).all()


@pytest.mark.parametrize("b,r,stride,first", [(4, 3, 4, None), (4, 3, 4, (-2, 3, 1)), (6, 1, 7, None), (1, 1, 1, None), (4, 4, 4, (5, 8, 8))])
def test_kernel_130_67_33_non_finite(built, bo, b, r, stride, first):
    """130 x 67 x 33 with NaN, +inf and -inf voxels in F and in W, and lattices that start outside the volume"""
    shape = (33, 67, 130)
    F, W = pair("smooth", shape, 5, spoil=6)
    f0, count = lattice_numpy(shape, stride, b, r)
    w = check(built, bo, F, W, first or f0, stride, count, b, r)
    assert 0 < (w[..., 3] != 0).sum() < w[..., 3].size


@pytest.mark.parametrize("b,r", [(4, 3), (4, 4)])
def test_kernel_128_cubed_defaults(built, bo, b, r):
    F, W = pair("smooth", (128, 128, 128), 7, spoil=3)
    first, count = lattice_numpy(F.shape, 4, b, r)
    w = check(built, bo, F, W, first, 4, count, b, r, both=True)
    ok = w[..., 3] == 0
    planted = np.array(((-1, 0, 1), (1, 2, 0), (0, -1, -2)), np.int32)   # (x, y, z) per third of z; W(x + s) = F(x)
    assert ok.mean() > 0.9 and np.mean([(shifts(w)[ok] == p).all(-1).mean() for p in planted]) > 0.2


def test_kernel_256_cubed(built, bo):
    """256^3 at stride 8: 29 791 nodes, about 5 s of serial oracle"""
    F, W = pair("smooth", (256, 256, 256), 9)
    first, count = lattice_numpy(F.shape, 8, 4, 3)
    check(built, bo, F, W, first, 8, count, 4, 3)


@pytest.mark.parametrize("b,r", [(6, 6), (1, 6), (2, 5)])
def test_kernel_widest_search(built, bo, b, r):
    """29 x 27 x 26 at stride 1 with the widest search the API admits: the key's nibbles reach s + r = 12 and its |s|^2 field 108.
    At (6, 6) the lattice is 5 x 3 x 2 nodes, run once more from (10, 12, 12) so that some windows leave the volume.  One NaN,
    +inf and -inf voxel in F and in W, not two: the 25^3 window covers nearly the whole volume, and with two of each the oracle
    flags every node at (6, 6) for each of the seeds 1 .. 79."""
    shape = (26, 27, 29)
    F, W = pair("smooth", shape, 57, spoil=1)
    first, count = lattice_numpy(shape, 1, b, r)
    w = check(built, bo, F, W, first, 1, count, b, r, both=True)
    assert (w[..., 3] == 0).any()
    if (b, r) == (6, 6):
        w = check(built, bo, F, W, (10, 12, 12), 1, count, b, r, both=True)
        assert (w[..., 3] == 0).any() and (w[..., 3] != 0).any()


def test_kernel_refusals(built):
    F = volume("smooth", (16, 16, 16), 1)
    for kw in (dict(block=0), dict(block=7), dict(search=0), dict(search=7), dict(stride=0), dict(count=(0, 1, 1))):
        a = dict(first=(7, 7, 7), stride=4, count=(1, 1, 1), block=4, search=3)
        a.update(kw)
        with pytest.raises(built.Sift3DError):
            built.block_match(F, F, **a)
    with pytest.raises(built.Sift3DError):
        built.block_match(np.full_like(F, 2.0), F, (7, 7, 7), 4, (1, 1, 1), 4, 3)
    with pytest.raises(built.Sift3DError):
        built.block_match(np.full_like(F, np.nan), F, (7, 7, 7), 4, (1, 1, 1), 4, 3)


# ---- the stage -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenario(built, tmp_path_factory):
    return scenario_setup(built, tmp_path_factory.mktemp("scenario"), False)


def _stage(built, bo, fo, V, M, t, field, fv, mv, **params):
    got, rep = built.refine_field_intensity(V, M, t, field, fv, mv, **params)
    want, wrep = cpu_refine_intensity(built, bo, fo, V, M, t, field, fv, mv, **params)
    same_report(rep, wrep)
    same_field(got, want)
    return got, rep


def test_stage_equals_cpu_on_the_scenario(built, bo, fo, scenario):
    s = scenario
    field = s["parent"]["field_dict"]
    got, rep = _stage(built, bo, fo, s["V"], s["M"], s["T4"], field, s["fv"], s["mv"])
    assert rep["rounds"] == 2 and rep["round"][1]["kept"] > 10000 and rep["round"][0]["match_ms"] > 0 and rep["round"][1]["fit_ms"][1] > 0
    # without an input field; other parameters
    _stage(built, bo, fo, s["V"], s["M"], s["T4"], None, s["fv"], s["mv"], rounds=1)
    _stage(built, bo, fo, s["V"], s["M"], s["T4"], field, s["fv"], s["mv"], rounds=1, stride=5, block=6, search=4, radius=12.0, lam=0.0,
           variance_quantile=0.5, cost_fraction=0.5, spacing=7.5, min_tol=0.5)


def test_stage_returns_the_input_field(built, scenario):
    s = scenario
    field = s["parent"]["field_dict"]
    got, rep = built.refine_field_intensity(s["V"], s["M"], s["T4"], field, s["fv"], s["mv"], rounds=0)
    same_field(got, field)
    assert rep["rounds"] == 0 and not rep["empty_range"]
    for flat in (np.full_like(s["V"], 7.0), np.full_like(s["V"], np.nan)):
        got, rep = built.refine_field_intensity(flat, s["M"], s["T4"], field, s["fv"], s["mv"])
        same_field(got, field)
        assert rep["rounds"] == 0 and rep["empty_range"] == 1
    got, rep = built.refine_field_intensity(np.full_like(s["V"], 7.0), s["M"], s["T4"], None, s["fv"], s["mv"])
    same_field(got, zero_field(built.blockmatch_grid(s["V"].shape, s["fv"])))


def test_stage_refusals(built, scenario):
    s = scenario
    small = s["V"][:12, :40, :40]
    for kw in (dict(block=0), dict(search=9), dict(rounds=9), dict(stride=0), dict(max_nodes=100), dict(variance_quantile=1.0)):
        with pytest.raises(built.Sift3DError):
            built.refine_field_intensity(s["V"], s["M"], s["T4"], None, **kw)
    with pytest.raises(built.Sift3DError) as e:
        built.refine_field_intensity(small, s["M"], s["T4"], None)
    assert "wider than the volume" in str(e.value)
    sing = np.array(s["T4"], np.float32).copy()
    sing[:3, :3] = 0
    with pytest.raises(built.Sift3DError):
        built.refine_field_intensity(s["V"], s["M"], sing, None)


def test_stage_equals_cpu_on_a_256_pair(built, bo, fo):
    """256^3: blobs, and the same blobs through a similarity and the scenario's kind of sinusoidal warp (by the product's
    resampler: only an input here); T is the similarity alone, so the warp is what the stage has to find.  Stride 8."""
    from resample_cases import about_centre, rot
    V = built.synth_blobs(256, 256, 256, seed=77)
    A = about_centre(1.03 * rot((0.2, -0.5, 0.8), 6.0), V.shape, V.shape, (2.0, -1.5, 1.0))
    g = built.field_size(np.array([[0, 0, 0], [255, 255, 255]], np.float32), spacing=16.0, radius=16.0)
    n = g["n"]
    c, bb, a = np.meshgrid(np.arange(n[2]), np.arange(n[1]), np.arange(n[0]), indexing="ij")
    wave = 2.5 * np.stack([np.sin(0.3 * bb), np.sin(0.3 * c), np.sin(0.3 * a)]).astype(np.float32)
    M = built.resample_field(V, V.shape, A, dict(g, disp=wave))
    T4 = np.vstack([A, [0, 0, 0, 1]]).astype(np.float32)   # M(x) = V(A x): moving voxel x sits at fixed voxel A x; vox2key is the identity here
    got, rep = _stage(built, bo, fo, V, M, T4, None, None, None, stride=8)
    assert rep["rounds"] == 2 and rep["round"][1]["kept"] > 5000


# ---- the command line and the scenario end to end --------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [False, True])
def test_end_to_end_intensity(built, bo, fo, tmp_path, world):
    """featExtract, featMatchMultiple -a -e -u, featResample -i -u: the files, the output equal to sift3d_resample_field through
    the field that was written, the output without -i equal to the parent's path, and the in-memory figures equal to the CPU
    prediction (tests/blockmatch_cases.cpu_refine_intensity over field_cases.nonrigid_cpu)."""
    fixed, moving, V, M, A_true, vox_v, vox_m, hv, hm = nonrigid_volumes(built, tmp_path, world)
    opt = ["-w"] if world else []
    _run([built.FEATEXTRACT, "-d0"] + opt + [fixed, "fixed.key"], tmp_path)
    _run([built.FEATEXTRACT, "-d0"] + opt + [moving, "moving.key"], tmp_path)
    _run([built.FEATMATCH, "-a", "-e", "-u", "fixed.key", "moving.key"], tmp_path)
    trans, fpath = str(tmp_path / "moving.key.trans.txt"), str(tmp_path / "moving.key.field.nii")
    _run([built.FEATRESAMPLE, "-d0"] + opt + ["-i", "-u", fpath, fixed, moving, trans, "out_i.nii"], tmp_path)
    _run([built.FEATRESAMPLE, "-d0"] + opt + ["-i1", fixed, moving, trans, "out_i1.nii"], tmp_path)
    _run([built.FEATRESAMPLE, "-d0"] + opt + ["-u", fpath, fixed, moving, trans, "out_u.nii"], tmp_path)
    _run([built.FEATRESAMPLE, "-d0"] + opt + [fixed, moving, trans, "out_e.nii"], tmp_path)
    T4 = built.read_similarity(trans)
    A = scenario_map(built, T4, world, vox_v, vox_m, hv, hm)
    fv = built.key_vox2key(vox_v, hv["qto_xyz"] if world else None)
    mv = built.key_vox2key(vox_m, hm["qto_xyz"] if world else None)
    field_u = built.read_field(fpath)
    # without -i: the parent's bytes
    assert built.read_nifti(str(tmp_path / "out_u.nii"))[0].tobytes() == built.resample_field(M, V.shape, A, field_u, fv, mv).tobytes()
    assert built.read_nifti(str(tmp_path / "out_e.nii"))[0].tobytes() == built.resample_affine(M, V.shape, A).tobytes()
    # with -i: the files, and the output through the field that was written
    for name, start, rounds in (("out_i.nii", field_u, 2), ("out_i1.nii", None, 1)):
        field_i = built.read_field(str(tmp_path / (name + ".field.nii")))
        out_i, hdr = built.read_nifti(str(tmp_path / name))
        assert hdr["dims"] == hv["dims"]
        assert out_i.tobytes() == built.resample_field(M, V.shape, A, field_i, fv, mv).tobytes()
        want, rep = built.refine_field_intensity(V, M, T4, start, fv, mv, rounds=rounds)
        same_field(field_i, want)
        lines = (tmp_path / (name + ".field.txt")).read_text().splitlines()
        last = rep["round"][rounds - 1]
        assert lines[-1].split("\t")[:4] == [str(rounds), str(last["nodes"]), str(last["samples"]), str(last["kept"])]
    # in memory, equal to the CPU prediction
    (tmp_path / "cpu").mkdir()
    s = scenario_setup(built, tmp_path / "cpu", world)
    F, Mk = (built.match_filter(built.read_key(str(tmp_path / n))) for n in ("fixed.key", "moving.key"))
    t = built.refine_similarity(F, Mk, built.match_keys(F, Mk))[0]
    start = built.refine_field(F, Mk, t)[0]
    same_field(start, s["parent"]["field_dict"])
    got, rep = built.refine_field_intensity(V, M, t, start, fv, mv)
    want, wrep = cpu_refine_intensity(built, bo, fo, s["V"], s["M"], s["T4"], s["parent"]["field_dict"], s["fv"], s["mv"])
    same_report(rep, wrep)
    same_field(got, want)
    parent, mine = s["parent"]["field"], scenario_score(built, fo, s, got)
    print("intensity end to end%s: -u corr %.4f rms %.3f max %.3f; -i corr %.4f rms %.3f max %.3f" % ((" -w" if world else "",) + parent + mine))
    assert mine[1] < 0.7 * parent[1] and mine[2] < parent[2] and mine[0] > parent[0], (parent, mine)
