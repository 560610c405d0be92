"""GPU suite: the displacement field of DESIGN.md section 7e -- field_fit_kernel and field_warp_kernel against the CPU oracle
tests/field_oracle.c bit for bit, sift3d_refine_field against the stage restated in tests/field_cases.py, the command lines, and
the nonrigid scenario end to end."""
import subprocess

import numpy as np
import pytest

from _helpers import extract, run as _run
from field_cases import FieldOracle, cpu_field, nonrigid_cpu, nonrigid_score, nonrigid_volumes, sample_set
from refine_cases import RefineOracle, interval, scenario_map
from resample_cases import ResampleOracle, about_centre, rot, special_volume

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fo(tmp_path_factory):
    return FieldOracle(tmp_path_factory.mktemp("field_oracle"))


def _check_fit(built, fo, y, v, h, R, lam=0.1):
    got = built.fit_field(y, v, spacing=h, radius=R, lam=lam)
    want = fo.fit(y, v, got, R, lam)
    assert got["n"] == want["n"]
    assert got["disp"].tobytes() == want["disp"].tobytes()
    return got


@pytest.mark.parametrize("kind", ["random", "clustered", "lattice"])
@pytest.mark.parametrize("h", [1.0, 4.0, 7.5])
@pytest.mark.parametrize("Rk", ["h", 20.0, 64.0])
@pytest.mark.parametrize("n", [0, 1, 3, 2000])
def test_fit_kernel_equals_oracle(built, fo, kind, h, Rk, n):
    R = h if Rk == "h" else Rk
    if h == 1.0 and R == 64.0 and n > 50:   # 2.7 M nodes: the brute-force oracle is kept to a small set there
        n = 50
    y, v = sample_set(kind, 17 + n, n, box=30.0 if h == 1.0 else 60.0)
    _check_fit(built, fo, y, v, h, R)


@pytest.mark.parametrize("kind", ["random", "clustered", "lattice"])
@pytest.mark.parametrize("h,R", [(4.0, 20.0), (7.5, 7.5)])
def test_fit_kernel_50000_samples(built, fo, kind, h, R):
    y, v = sample_set(kind, 5, 50000, box=100.0)
    f = _check_fit(built, fo, y, v, h, R)
    # shuffled: the same bits
    p = np.random.default_rng(3).permutation(len(y))
    assert built.fit_field(y[p], v[p], spacing=h, radius=R)["disp"].tobytes() == f["disp"].tobytes()


def test_fit_kernel_non_finite_and_refusals(built, fo):
    y, v = sample_set("clustered", 8, 500)
    y[3, 0], y[4, 1], v[5, 2], v[6, 0] = np.nan, np.inf, np.nan, -np.inf
    _check_fit(built, fo, y, v, 4.0, 20.0)
    _check_fit(built, fo, y, v, 4.0, 20.0, lam=0.0)
    v[7, 1] = 200.0   # beyond SIFT3D_FIELD_MAX_DISP
    with pytest.raises(built.Sift3DError):
        built.fit_field(y, v)


def test_fit_kernel_grid_above_2_24_nodes(built, fo):
    y = np.array([[0, 0, 0], [255, 3, 7], [100, 255, 50], [40, 60, 255], [128, 128, 128]], np.float32)
    v = np.array([[1, 2, 3], [-1, 0.5, 2], [0, 0, -3], [2, 2, 2], [-0.25, 1, 0]], np.float32)
    f = _check_fit(built, fo, y, v, 1.0, 3.0)
    assert np.prod(f["n"]) > 2 ** 24, f["n"]
    assert f["disp"][0, 131, 131, 131] < 0 and f["disp"][2, 3, 3, 3] > 0   # the nodes at (128, 128, 128) and (0, 0, 0)


def _random_field(rng, shape_key, nan=False):
    d = rng.uniform(-3, 3, (3,) + shape_key).astype(np.float32)
    if nan:
        d.reshape(-1)[rng.choice(d.size, d.size // 30, replace=False)] = np.nan
    return d


@pytest.mark.parametrize("shape", [(1, 1, 1), (37, 5, 129), (130, 67, 33), (256, 256, 256)])
@pytest.mark.parametrize("interp", ["linear", "nearest"])
def test_warp_kernel_equals_oracle(built, fo, shape, interp):
    rng = np.random.default_rng(sum(shape))
    vol = special_volume(shape, 1) if max(shape) < 256 else built.synth_blobs(*shape[::-1], seed=3)
    out_shape = tuple(max(1, s - 3) for s in shape)
    A = about_centre(rot((1, 2, 3), 17.0), shape, out_shape, shift=(0.5, -0.75, 1.0))
    fv = built.key_vox2key((1.0, 1.0, 1.0))
    n = tuple(int(x) for x in (np.array(out_shape[::-1]) // 4 + 4))
    field = {"n": n, "origin": np.array([-6.0, -5.5, -7.25], np.float32), "spacing": np.float32(4.0),
             "disp": _random_field(rng, n[::-1], nan=max(shape) < 256)}
    Cm, K = built.field_warp_terms(fv, fv)
    for fill in (0.0, np.nan, -7.0):
        got = built.resample_field(vol, out_shape, A, field, fv, fv, interp, fill)
        want = fo.warp(vol, out_shape, A, Cm, K, field, interp, fill)
        assert np.array_equal(got, want, equal_nan=True), fill
        if max(shape) == 256:
            break
    # a zero field: the bytes of sift3d_resample_affine
    zero = dict(field, disp=np.zeros_like(field["disp"]))
    got = built.resample_field(vol, out_shape, A, zero, fv, fv, interp)
    want = built.resample_affine(vol, out_shape, A, interp)
    assert got.tobytes() == want.tobytes()


def test_warp_kernel_world_geometry(built, fo):
    rng = np.random.default_rng(4)
    vol = special_volume((40, 50, 60), 2)
    q_v, q_m = (0.1, 0.2, 0.3, -30.0, 20.0, 5.0, -1.0), (-0.2, 0.05, 0.1, 10.0, -40.0, 25.0, -1.0)
    import os
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        built.write_nifti(os.path.join(d, "f.nii"), np.zeros((1, 1, 1), np.float32), voxel=(1.0, 1.25, 1.5), qform=q_v)
        built.write_nifti(os.path.join(d, "m.nii"), np.zeros((1, 1, 1), np.float32), voxel=(1.0, 1.0, 1.0), qform=q_m)
        _, hv = built.read_nifti(os.path.join(d, "f.nii"))
        _, hm = built.read_nifti(os.path.join(d, "m.nii"))
    fv = built.key_vox2key((1.0, 1.25, 1.5), hv["qto_xyz"])
    mv = built.key_vox2key((1.0, 1.0, 1.0), hm["qto_xyz"])
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = rot((0, 0, 1), 10.0)
    cm = (mv.astype(np.float64) @ np.array([29.5, 24.5, 19.5, 1.0]))[:3]   # the moving image's centre onto the output's
    cf = (fv.astype(np.float64) @ np.array([17.5, 14.5, 13.5, 1.0]))[:3]
    T[:3, 3] = cf - T[:3, :3].astype(np.float64) @ cm + (1.0, -0.5, 0.5)
    A = built.resample_map(T, fv, mv)
    # the grid over the fixed key box of a 36 x 30 x 28 output
    corners = np.array([[i, j, k, 1] for i in (0, 35) for j in (0, 29) for k in (0, 27)], np.float64) @ fv.astype(np.float64).T
    lo = corners[:, :3].min(0) - 8
    n = tuple(int(x) for x in np.ceil((corners[:, :3].max(0) + 8 - lo) / 3.0) + 1)
    field = {"n": n, "origin": lo.astype(np.float32), "spacing": np.float32(3.0), "disp": _random_field(rng, n[::-1])}
    Cm, K = built.field_warp_terms(fv, mv)
    for interp in ("linear", "nearest"):
        got = built.resample_field(vol, (28, 30, 36), A, field, fv, mv, interp, np.nan)
        want = fo.warp(vol, (28, 30, 36), A, Cm, K, field, interp, np.nan)
        assert np.array_equal(got, want, equal_nan=True)
        assert np.isfinite(got).mean() > 0.3


@pytest.fixture(scope="module")
def extractions_256(built):
    v = built.synth_blobs(256, 256, 256, seed=12345)
    w = np.ascontiguousarray(np.roll(v, (3, -5, 7), axis=(0, 1, 2)))
    return extract(built, v), extract(built, w)


def _same_field(built, fo, f, m, t, got, rep, **params):
    ro = RefineOracle(fo_dir(fo))
    lo, hi = interval()
    want, wrep, _ = cpu_field(built, fo, f, m, t, lambda tt, r: ro.search(f, m, tt, r, lo, hi), **params)
    for k in ("accepted", "kept", "rms_before", "rms_after", "folds", "max_disp"):
        assert rep[k] == wrep[k], (k, rep[k], wrep[k])
    assert got["n"] == want["n"] and got["origin"].tobytes() == want["origin"].tobytes()
    assert got["disp"].tobytes() == want["disp"].tobytes()
    return wrep


def fo_dir(fo):
    import os
    return os.path.dirname(fo.L._name)


def test_refine_field_equals_cpu_on_256_extractions(built, fo, extractions_256):
    f, m = extractions_256
    assert len(f) > 15000 and len(m) > 15000
    t = built.refine_similarity(f, m, built.match_keys(f, m))[0]
    got, rep = built.refine_field(f, m, t)
    wrep = _same_field(built, fo, f, m, t, got, rep)
    assert wrep["accepted"] > 5000 and rep["fit_ms"][0] > 0 and rep["fit_ms"][1] > 0
    # other parameters, the sorted-key search index
    got, rep = built.refine_field(f, m, t, spacing=7.5, radius=12.0, lam=0.0, search_radius=4.0, index_cells_max=1)
    _same_field(built, fo, f, m, t, got, rep, spacing=7.5, radius=12.0, lam=0.0, search_radius=4.0)


@pytest.fixture(scope="module")
def nonrigid_keys(built, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("nonrigid")
    vols = nonrigid_volumes(built, tmp, False)
    _run([built.FEATEXTRACT, "-d0", vols[0], "fixed.key"], tmp)
    _run([built.FEATEXTRACT, "-d0", vols[1], "moving.key"], tmp)
    return tmp, vols


def test_featmatchmultiple_field_files(built, nonrigid_keys, tmp_path):
    src, _ = nonrigid_keys
    names = ["fixed.key", "moving.key"]
    ref = tmp_path / "ref"
    ref.mkdir()
    for d in (tmp_path, ref):
        for n in names:
            (d / n).write_bytes((src / n).read_bytes())
    _run([built.FEATMATCH, "-a", "-e"] + names, ref)
    _run([built.FEATMATCH, "-a", "-e", "-u"] + names, tmp_path)
    made = sorted(p.name for p in tmp_path.iterdir() if p.is_file())
    assert "moving.key.field.nii" in made and "moving.key.field.txt" in made
    for name in made:
        if name.startswith("moving.key.field") or name == "_command.txt":
            continue
        assert (tmp_path / name).read_bytes() == (ref / name).read_bytes(), name
    F, M = (built.match_filter(built.read_key(str(tmp_path / n)), 1, 4) for n in names)
    t = built.refine_similarity(F, M, built.match_keys(F, M))[0]
    want, rep = built.refine_field(F, M, t)
    got = built.read_field(str(tmp_path / "moving.key.field.nii"))
    assert got["n"] == want["n"] and got["disp"].tobytes() == want["disp"].tobytes()
    lines = (tmp_path / "moving.key.field.txt").read_text().splitlines()
    assert lines[-1].split("\t")[:2] == [str(rep["accepted"]), str(rep["kept"])]
    # -u7.5: another spacing
    _run([built.FEATMATCH, "-a", "-e", "-u7.5"] + names, tmp_path)
    assert built.read_field(str(tmp_path / "moving.key.field.nii"))["spacing"] == np.float32(7.5)
    # -u without -e fails; -s2 runs
    for bad in (["-a", "-u"], ["-u"]):
        r = subprocess.run([built.FEATMATCH] + bad + names, cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0
    _run([built.FEATMATCH, "-a", "-s2", "-e", "-u"] + names, tmp_path)


@pytest.mark.parametrize("world", [False, True])
def test_end_to_end_nonrigid(built, tmp_path, world):
    """The nonrigid scenario on the GPU: featExtract, featMatchMultiple -a -e [-u], featResample [-u].  The outputs equal the
    Python path on the same files, and the in-memory figures equal the CPU prediction (tests/field_cases.nonrigid_cpu).  The
    targets set beforehand are not met with the defaults; the field must improve on -a -e."""
    fixed, moving, V, M, A_true, vox_v, vox_m, hv, hm = nonrigid_volumes(built, tmp_path, world)
    opt = ["-w"] if world else []
    _run([built.FEATEXTRACT, "-d0"] + opt + [fixed, "fixed.key"], tmp_path)
    _run([built.FEATEXTRACT, "-d0"] + opt + [moving, "moving.key"], tmp_path)
    _run([built.FEATMATCH, "-a", "-e", "-u", "fixed.key", "moving.key"], tmp_path)
    trans, fpath = str(tmp_path / "moving.key.trans.txt"), str(tmp_path / "moving.key.field.nii")
    _run([built.FEATRESAMPLE, "-d0"] + opt + ["-u", fpath, fixed, moving, trans, "out_u.nii"], tmp_path)
    _run([built.FEATRESAMPLE, "-d0"] + opt + [fixed, moving, trans, "out_e.nii"], tmp_path)
    out_u, hdr = built.read_nifti(str(tmp_path / "out_u.nii"))
    out_e, _ = built.read_nifti(str(tmp_path / "out_e.nii"))
    for k in ("dims", "voxel", "qform_code", "sform_code"):
        assert hdr[k] == hv[k], k
    assert np.array_equal(hdr["qto_xyz"], hv["qto_xyz"])
    A = scenario_map(built, built.read_similarity(trans), world, vox_v, vox_m, hv, hm)
    fv = built.key_vox2key(vox_v, hv["qto_xyz"] if world else None)
    mv = built.key_vox2key(vox_m, hm["qto_xyz"] if world else None)
    field = built.read_field(fpath)
    assert out_u.tobytes() == built.resample_field(M, V.shape, A, field, fv, mv).tobytes()
    se = nonrigid_score(built, V, out_e, A, A_true)
    su = nonrigid_score(built, V, out_u, A, A_true, field, fv, mv)
    print("nonrigid end to end%s: -a -e corr %.4f rms %.3f max %.3f; -u corr %.4f rms %.3f max %.3f" % ((" -w" if world else "",) + se + su))
    assert su[1] < (0.7 if world else 0.6) * se[1] and su[0] > se[0], (se, su)
    # in memory, equal to the CPU prediction
    F, Mk = (built.match_filter(built.read_key(str(tmp_path / n))) for n in ("fixed.key", "moving.key"))
    t = built.refine_similarity(F, Mk, built.match_keys(F, Mk))[0]
    got, rep = built.refine_field(F, Mk, t)
    (tmp_path / "cpu").mkdir()
    want = nonrigid_cpu(built, tmp_path / "cpu", world)
    assert got["disp"].tobytes() == want["field_dict"]["disp"].tobytes()
    for k in ("accepted", "kept", "rms_before", "rms_after", "folds"):
        assert rep[k] == want["report"][k], k
    Am = scenario_map(built, built.similarity_matrix(t), world, vox_v, vox_m, hv, hm)
    assert nonrigid_score(built, V, built.resample_field(M, V.shape, Am, got, fv, mv), Am, A_true, got, fv, mv) == want["field"]
