"""GPU suite: the correlation cost of the block search -- block_match_ncc_kernel against the CPU oracle
tests/blockmatch_ncc_oracle.c bit for bit on the families of cases of test_gpu_blockmatch.py, W on an intensity scale of its
own; sift3d_refine_field_intensity_metric against the stage restated in tests/blockmatch_ncc_cases.py on the scenario pair with
a remapped moving volume; metric 0 against sift3d_refine_field_intensity; the refusals; and featResample -i -c end to end.  The
serial oracle takes about twice the SSD one's time (three sums per voxel): about 10 s for the 128^3 and the 256^3 volume."""
import subprocess

import numpy as np
import pytest

from _helpers import run as _run
from blockmatch_cases import cpu_refine_intensity, lattice_numpy, same_field, same_report, scenario_score, scenario_setup, shifts, volume, zero_field
from blockmatch_ncc_cases import FLAT, NccOracle, cpu_refine_intensity_metric, remap, same_report_ncc
from field_cases import FieldOracle, hm_q, nonrigid_volumes
from refine_cases import scenario_map
from test_gpu_blockmatch import pair as ssd_pair

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def no(tmp_path_factory):
    return NccOracle(tmp_path_factory.mktemp("blockmatch_ncc_oracle"))


@pytest.fixture(scope="module")
def fo(tmp_path_factory):
    return FieldOracle(tmp_path_factory.mktemp("field_oracle"))


def pair(kind, shape, seed, spoil=0):
    """test_gpu_blockmatch.pair with W's finite intensities on another scale: 0.37 W - 55 and a ramp of 20 % along x"""
    F, W = ssd_pair(kind, shape, seed, spoil)
    ramp = (1.0 + 0.2 * np.arange(shape[2], dtype=np.float64) / shape[2])[None, None, :]
    with np.errstate(invalid="ignore"):
        W = np.where(np.isfinite(W), (0.37 * W.astype(np.float64) - 55.0) * ramp, W).astype(np.float32)
    return F, W


def check(built, no, F, W, first, stride, count, b, r, both=False):
    want = no.match(F, W, first, stride, count, b, r)
    got = built.block_match_ncc(F, W, first, stride, count, b, r)
    assert got.shape == want.shape
    assert got.tobytes() == want.tobytes(), (np.argwhere((got != want).any(-1))[:5], first, stride, count, b, r)
    if both:   # the kernel's form for any b, r
        assert built.block_match_ncc(F, W, first, stride, count, b, r, generic=1).tobytes() == want.tobytes()
    return want


@pytest.mark.parametrize("b", [1, 4, 6])
@pytest.mark.parametrize("r", [1, 3, 4])
def test_kernel_16_cubed_every_voxel_a_node(built, no, b, r):
    """16^3, stride 1, a node on every voxel: most nodes' windows leave the volume and are flagged"""
    F, W = pair("random", (16, 16, 16), 10 * b + r)
    w = check(built, no, F, W, (0, 0, 0), 1, (16, 16, 16), b, r, both=True)
    assert (w[..., 3] == 0).sum() == max(16 - 2 * (b + r), 0) ** 3


@pytest.mark.parametrize("kind", ["random", "smooth", "constant"])
@pytest.mark.parametrize("b,r,stride", [(1, 1, 1), (1, 3, 1), (4, 1, 4), (4, 3, 4), (6, 4, 7), (4, 4, 5), (6, 3, 4)])
def test_kernel_non_cubic(built, no, kind, b, r, stride):
    """37 x 21 x 50: counts that are no multiple of the workgroup's brick; with b + r = 10 the window fills y exactly"""
    shape = (50, 21, 37)
    F, W = pair(kind, shape, 3)
    first, count = lattice_numpy(shape, stride, b, r)
    w = check(built, no, F, W, first, stride, count, b, r, both=True)
    assert (w[..., 3] == 0).all()
    if kind == "constant":   # flat blocks: 2^31 at every shift, and the zero shift wins the ties
        assert (shifts(w) == 0).all() and (w[..., 4:12] == FLAT).all()


@pytest.mark.parametrize("b,r,stride,first", [(4, 3, 4, None), (4, 3, 4, (-2, 3, 1)), (6, 1, 7, None), (1, 1, 1, None), (4, 4, 4, (5, 8, 8))])
def test_kernel_130_67_33_non_finite(built, no, b, r, stride, first):
    """130 x 67 x 33 with NaN, +inf and -inf voxels in F and in W, and lattices that start outside the volume"""
    shape = (33, 67, 130)
    F, W = pair("smooth", shape, 5, spoil=6)
    f0, count = lattice_numpy(shape, stride, b, r)
    w = check(built, no, F, W, first or f0, stride, count, b, r)
    assert 0 < (w[..., 3] != 0).sum() < w[..., 3].size
    assert (w[..., 3] == no.ssd.match(F, W, first or f0, stride, count, b, r)[..., 3]).all()   # the flags are the SSD search's


@pytest.mark.parametrize("b,r", [(4, 3), (4, 4)])
def test_kernel_128_cubed_defaults(built, no, b, r):
    F, W = pair("smooth", (128, 128, 128), 7, spoil=3)
    first, count = lattice_numpy(F.shape, 4, b, r)
    w = check(built, no, F, W, first, 4, count, b, r, both=True)
    ok = w[..., 3] == 0
    planted = np.array(((-1, 0, 1), (1, 2, 0), (0, -1, -2)), np.int32)   # (x, y, z) per third of z; W(x + s) = F(x)
    assert ok.mean() > 0.9 and np.mean([(shifts(w)[ok] == p).all(-1).mean() for p in planted]) > 0.2


def test_kernel_256_cubed(built, no):
    """256^3 at stride 8: 29 791 nodes"""
    F, W = pair("smooth", (256, 256, 256), 9)
    first, count = lattice_numpy(F.shape, 8, 4, 3)
    check(built, no, F, W, first, 8, count, 4, 3)


@pytest.mark.parametrize("b,r", [(6, 6), (1, 6), (2, 5)])
def test_kernel_widest_search(built, no, b, r):
    """29 x 27 x 26 at stride 1 with the widest search the API admits: the key's nibbles reach s + r = 12 and its |s|^2 field 108.
    At (6, 6) the lattice is 5 x 3 x 2 nodes, run once more from (10, 12, 12) so that some windows leave the volume.  One NaN,
    +inf and -inf voxel in F and in W, not two: the 25^3 window covers nearly the whole volume, and with two of each the oracle
    flags every node at (6, 6) for each of the seeds 1 .. 79."""
    shape = (26, 27, 29)
    F, W = pair("smooth", shape, 57, spoil=1)
    first, count = lattice_numpy(shape, 1, b, r)
    w = check(built, no, F, W, first, 1, count, b, r, both=True)
    assert (w[..., 3] == 0).any()
    if (b, r) == (6, 6):
        w = check(built, no, F, W, (10, 12, 12), 1, count, b, r, both=True)
        assert (w[..., 3] == 0).any() and (w[..., 3] != 0).any()


def test_kernel_refusals(built):
    F = volume("smooth", (16, 16, 16), 1)
    for kw in (dict(block=0), dict(block=7), dict(search=0), dict(search=7), dict(stride=0), dict(count=(0, 1, 1))):
        a = dict(first=(7, 7, 7), stride=4, count=(1, 1, 1), block=4, search=3)
        a.update(kw)
        with pytest.raises(built.Sift3DError):
            built.block_match_ncc(F, F, **a)
    for flat in (np.full_like(F, 2.0), np.full_like(F, np.nan)):   # either volume without a range
        with pytest.raises(built.Sift3DError):
            built.block_match_ncc(flat, F, (7, 7, 7), 4, (1, 1, 1), 4, 3)
        with pytest.raises(built.Sift3DError) as e:
            built.block_match_ncc(F, flat, (7, 7, 7), 4, (1, 1, 1), 4, 3)
        assert "warped volume" in str(e.value)


# ---- the stage -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenario(built, tmp_path_factory):
    return scenario_setup(built, tmp_path_factory.mktemp("scenario"), False)


def _stage(built, no, fo, V, M, t, field, fv, mv, **params):
    got, rep = built.refine_field_intensity(V, M, t, field, fv, mv, metric="ncc", **params)
    want, wrep = cpu_refine_intensity_metric(built, no, fo, V, M, t, field, fv, mv, metric="ncc", **params)
    same_report_ncc(rep, wrep)
    same_field(got, want)
    return got, rep


@pytest.mark.parametrize("kind", ["affine", "smooth_bias"])
def test_stage_equals_cpu_on_the_remapped_scenario(built, no, fo, scenario, kind):
    s = scenario
    field = s["parent"]["field_dict"]
    M2 = remap(s["M"], kind)
    got, rep = _stage(built, no, fo, s["V"], M2, s["T4"], field, s["fv"], s["mv"])
    assert rep["rounds"] == 2 and rep["round"][1]["kept"] > 10000 and rep["round"][0]["match_ms"] > 0 and rep["round"][1]["fit_ms"][1] > 0
    assert (rep["moving_lo"], rep["moving_hi"]) == built.blockmatch_range(M2) and (rep["lo"], rep["hi"]) == built.blockmatch_range(s["V"])
    # without an input field; other parameters (the any-(b, r) form of the kernel is what b = 6 takes)
    _stage(built, no, fo, s["V"], M2, s["T4"], None, s["fv"], s["mv"], rounds=1)
    if kind == "affine":
        _stage(built, no, fo, s["V"], M2, s["T4"], field, s["fv"], s["mv"], rounds=1, stride=5, block=6, search=4, radius=12.0, lam=0.0,
               variance_quantile=0.5, cost_fraction=0.5, spacing=7.5, min_tol=0.5)


def test_metric_0_is_the_ssd_stage(built, scenario):
    s = scenario
    field = s["parent"]["field_dict"]
    M2 = remap(s["M"], "affine")
    for M, start in ((s["M"], field), (M2, None)):
        want, wrep = built.refine_field_intensity(s["V"], M, s["T4"], start, s["fv"], s["mv"])
        got, rep = built.refine_field_intensity(s["V"], M, s["T4"], start, s["fv"], s["mv"], metric=0)
        same_field(got, want)
        same_report(rep, dict(wrep, round=[{k: v for k, v in r.items() if not k.endswith("_ms")} for r in wrep["round"][:wrep["rounds"]]]))
        assert rep["rounds"] == 2 and rep["moving_lo"] == 0 and rep["moving_hi"] == 0


def test_stage_returns_the_input_field(built, scenario):
    s = scenario
    field = s["parent"]["field_dict"]
    got, rep = built.refine_field_intensity(s["V"], s["M"], s["T4"], field, s["fv"], s["mv"], metric="ncc", rounds=0)
    same_field(got, field)
    assert rep["rounds"] == 0 and not rep["empty_range"]
    # an empty range of either volume: no round, the input field back
    for flat in (np.full_like(s["V"], 7.0), np.full_like(s["V"], np.nan)):
        for V, M in ((flat, s["M"]), (s["V"], flat)):
            got, rep = built.refine_field_intensity(V, M, s["T4"], field, s["fv"], s["mv"], metric="ncc")
            same_field(got, field)
            assert rep["rounds"] == 0 and rep["empty_range"] == 1
    got, rep = built.refine_field_intensity(s["V"], np.full_like(s["M"], 7.0), s["T4"], None, s["fv"], s["mv"], metric="ncc")
    same_field(got, zero_field(built.blockmatch_grid(s["V"].shape, s["fv"])))
    # the SSD stage does not look at the moving volume's range
    assert built.refine_field_intensity(s["V"], np.full_like(s["M"], 7.0), s["T4"], None, s["fv"], s["mv"], rounds=1)[1]["empty_range"] == 0


def test_stage_refusals(built, scenario):
    s = scenario
    for metric in (2, -1, 7):
        with pytest.raises(built.Sift3DError) as e:
            built.refine_field_intensity(s["V"], s["M"], s["T4"], None, metric=metric)
        assert "unknown metric" in str(e.value) and e.value.code == -1   # SIFT3D_ERR_ARG
    with pytest.raises(ValueError):
        built.refine_field_intensity(s["V"], s["M"], s["T4"], None, metric="mi")
    for kw in (dict(block=0), dict(search=9), dict(rounds=9), dict(stride=0), dict(max_nodes=100), dict(variance_quantile=1.0)):
        with pytest.raises(built.Sift3DError):
            built.refine_field_intensity(s["V"], s["M"], s["T4"], None, metric="ncc", **kw)
    with pytest.raises(built.Sift3DError) as e:
        built.refine_field_intensity(s["V"][:12, :40, :40], s["M"], s["T4"], None, metric="ncc")
    assert "wider than the volume" in str(e.value)


# ---- the command line ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [False, True])
def test_end_to_end_correlation(built, no, fo, tmp_path, world):
    """featExtract, featMatchMultiple -a -e -u on the scenario's images, then featResample -i -c -u on the moving image with its
    intensities remapped (0.45 M + 310): the field written equals sift3d_refine_field_intensity_metric's and the CPU
    prediction's, the output is the remapped image through that field, the report names the metric and both ranges, and the
    registration meets section 7f's bar.  -i without -c writes what it wrote before this cost existed: the SSD stage's field (the
    CPU prediction of test_gpu_blockmatch.py) and a report without the new line.  -c without -i is refused."""
    fixed, moving, V, M, A_true, vox_v, vox_m, hv, hm = nonrigid_volumes(built, tmp_path, world)
    opt = ["-w"] if world else []
    _run([built.FEATEXTRACT, "-d0"] + opt + [fixed, "fixed.key"], tmp_path)
    _run([built.FEATEXTRACT, "-d0"] + opt + [moving, "moving.key"], tmp_path)
    _run([built.FEATMATCH, "-a", "-e", "-u", "fixed.key", "moving.key"], tmp_path)
    trans, fpath = str(tmp_path / "moving.key.trans.txt"), str(tmp_path / "moving.key.field.nii")
    M2 = remap(M, "affine")
    moving2 = str(tmp_path / "moving_remapped.nii")
    built.write_nifti(moving2, M2, voxel=vox_m, qform=hm_q(world))
    _run([built.FEATRESAMPLE, "-d0"] + opt + ["-i", "-c", "-u", fpath, fixed, moving2, trans, "out_c.nii"], tmp_path)
    _run([built.FEATRESAMPLE, "-d0"] + opt + ["-c", "-i1", fixed, moving2, trans, "out_c1.nii"], tmp_path)
    _run([built.FEATRESAMPLE, "-d0"] + opt + ["-i", "-u", fpath, fixed, moving, trans, "out_i.nii"], tmp_path)
    r = subprocess.run([built.FEATRESAMPLE, "-d0", "-c", fixed, moving2, trans, "out_x.nii"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode != 0 and "-c needs -i" in r.stdout and "Usage" in r.stdout and not (tmp_path / "out_x.nii").exists()
    T4 = built.read_similarity(trans)
    A = scenario_map(built, T4, world, vox_v, vox_m, hv, hm)
    fv = built.key_vox2key(vox_v, hv["qto_xyz"] if world else None)
    mv = built.key_vox2key(vox_m, hm["qto_xyz"] if world else None)
    field_u = built.read_field(fpath)
    (tmp_path / "cpu").mkdir()
    s = scenario_setup(built, tmp_path / "cpu", world)
    same_field(field_u, s["parent"]["field_dict"])
    # with -c: the files, the output through the field that was written, the library call, the CPU prediction
    for name, start, rounds in (("out_c.nii", field_u, 2), ("out_c1.nii", None, 1)):
        field_c = built.read_field(str(tmp_path / (name + ".field.nii")))
        out_c, hdr = built.read_nifti(str(tmp_path / name))
        assert hdr["dims"] == hv["dims"]
        assert out_c.tobytes() == built.resample_field(M2, V.shape, A, field_c, fv, mv).tobytes()
        want, rep = built.refine_field_intensity(V, M2, T4, start, fv, mv, metric="ncc", rounds=rounds)
        same_field(field_c, want)
        lines = (tmp_path / (name + ".field.txt")).read_text().splitlines()
        last = rep["round"][rounds - 1]
        assert lines[-1].split("\t")[:4] == [str(rounds), str(last["nodes"]), str(last["samples"]), str(last["kept"])]
        assert [ln.split()[1] for ln in lines if ln.startswith("#")] == ["nodes", "stride", "metric", "round"]
        assert lines[2] == "# metric ncc fixed quantised over %g .. %g moving quantised over %g .. %g" % (rep["lo"], rep["hi"], rep["moving_lo"],
                                                                                                         rep["moving_hi"])
        cpu, crep = cpu_refine_intensity_metric(built, no, fo, V, M2, T4, start, fv, mv, metric="ncc", rounds=rounds)
        same_report_ncc(rep, crep)
        same_field(field_c, cpu)
        if rounds == 2:
            parent, mine = s["parent"]["field"], scenario_score(built, fo, s, field_c)
            print("correlation end to end%s: -u corr %.4f rms %.3f max %.3f; -i -c corr %.4f rms %.3f max %.3f" % ((" -w" if world else "",) + parent + mine))
            assert mine[1] < 0.6 * parent[1] and mine[2] < parent[2] and mine[0] > parent[0], (parent, mine)
    # without -c: the SSD stage's field and report, as before
    field_i = built.read_field(str(tmp_path / "out_i.nii.field.nii"))
    cpu, crep = cpu_refine_intensity(built, no.ssd, fo, V, M, T4, field_u, fv, mv)
    same_field(field_i, cpu)
    lines = (tmp_path / "out_i.nii.field.txt").read_text().splitlines()
    assert [ln.split()[1] for ln in lines if ln.startswith("#")] == ["nodes", "stride", "round"] and len(lines) == 3 + 2
    last = crep["round"][1]
    assert lines[-1].split("\t")[:4] == ["2", str(last["nodes"]), str(last["samples"]), str(last["kept"])]
    assert "metric" not in "\n".join(lines)
