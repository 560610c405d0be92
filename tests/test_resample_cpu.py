"""featResample's host side without a GPU: the voxel-to-voxel map against a float64 composition, the
.trans.txt reader, the key-coordinate convention of featExtract pinned on the oracle's extraction, and the CPU oracle's
inside and NaN rules on hand cases."""
import subprocess

import numpy as np
import pytest

import _oracle
from resample_cases import ResampleOracle, affine, rot


@pytest.fixture(scope="module")
def rorc(tmp_path_factory):
    return ResampleOracle(tmp_path_factory.mktemp("resample_oracle"))


def _want_map(T, F, M):
    """inv(M) . (inv(T) . F) in float64, rounded to float32 once"""
    F = np.eye(4) if F is None else np.asarray(F, np.float32).astype(np.float64)
    M = np.eye(4) if M is None else np.asarray(M, np.float32).astype(np.float64)
    T = np.asarray(T, np.float32).astype(np.float64)
    return (np.linalg.inv(M) @ (np.linalg.inv(T) @ F))[:3].astype(np.float32)


def _random_vox2key(rng):
    """a qform-like matrix: rotation, voxel sizes, qfac, offsets"""
    R = rot(rng.normal(size=3), rng.uniform(0, 180))
    S = np.diag(rng.uniform(0.5, 2.0, 3) * np.array([1, 1, rng.choice([-1, 1])]))
    return affine(R @ S, rng.uniform(-100, 100, 3)).astype(np.float32)


@pytest.mark.parametrize("case", ["identity", "shift", "quarter", "half", "double", "oblique"])
def test_resample_map_matches_float64_composition(built, case):
    rng = np.random.default_rng(["identity", "shift", "quarter", "half", "double", "oblique"].index(case) + 17)
    F = M = None
    if case == "identity":
        T = np.eye(4)
    elif case == "shift":
        T = affine(np.eye(3), (3.0, -7.5, 12.25))
    elif case == "quarter":
        T = affine(np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]]), (64, 0, 0))
    elif case == "half":
        T = affine(np.eye(3), (1, 2, 3), 0.5)
    elif case == "double":
        T = affine(np.eye(3), (-4, 0, 8), 2.0)
    else:
        T = affine(rot(rng.normal(size=3), 23.7), rng.uniform(-20, 20, 3), 1.13)
        F, M = _random_vox2key(rng), _random_vox2key(rng)
    T = T.astype(np.float32)
    got = built.resample_map(T, F, M)
    want = _want_map(T, F, M)
    assert got.dtype == np.float32 and got.shape == (3, 4)
    assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist()
    if case == "identity":
        assert (got == np.eye(4, dtype=np.float32)[:3]).all()


def test_resample_map_rejects_singular_and_non_affine(built):
    S = np.eye(4, dtype=np.float32)
    S[2, 2] = 0
    for args in ((S, None, None), (np.eye(4), S, None), (np.eye(4), None, S)):
        with pytest.raises(built.Sift3DError):
            built.resample_map(*args)
    P = np.eye(4, dtype=np.float32)
    P[3, 0] = 0.5   # a projective last row
    with pytest.raises(built.Sift3DError):
        built.resample_map(P)


def test_read_similarity_round_trips_write_matrix(built, tmp_path):
    rng = np.random.default_rng(5)
    R = rot(rng.normal(size=3), 31.0).astype(np.float32)
    d = {"scale": np.float32(0.913), "rot": R, "trans": np.array([12.345678, -3.25, 100.0625], np.float32)}
    p = tmp_path / "m.trans.txt"
    built.write_similarity(str(p), d)
    text = p.read_bytes()
    m = built.read_similarity(str(p))
    # the numbers of the file, parsed as doubles and rounded to float once
    want = np.array([float(t) for t in text.split()], np.float64).astype(np.float32).reshape(4, 4)
    assert m.view(np.uint32).tolist() == want.view(np.uint32).tolist()
    # written again with WriteMatrix's formats, the same bytes
    again = "".join("%f\t%f\t%f\t%f\n" % tuple(float(v) for v in m[r]) for r in range(3)) + "0.0\t0.0\t0.0\t1.0\n"
    assert again.encode() == text
    # and the unrounded matrix is within the %f rounding of it
    full = built.similarity_matrix(d)
    assert (full[3] == [0, 0, 0, 1]).all()
    assert np.abs(full[:3, :3] - np.float32(0.913) * R).max() == 0
    assert (np.abs(full - m) <= 5e-7 + np.spacing(np.abs(full))).all()


def test_read_similarity_rejects_bad_files(built, tmp_path):
    cases = {"short": "1 0 0 0\n0 1 0 0\n0 0 1 0\n",
             "last_row": "1 0 0 0\n0 1 0 0\n0 0 1 0\n0 0 0.5 1\n",
             "trailing": "1 0 0 0\n0 1 0 0\n0 0 1 0\n0 0 0 1\n7\n",
             "text": "1 0 0 0\n0 one 0 0\n0 0 1 0\n0 0 0 1\n"}
    for name, body in cases.items():
        p = tmp_path / (name + ".txt")
        p.write_text(body)
        with pytest.raises(built.Sift3DError):
            built.read_similarity(str(p))
    with pytest.raises(built.Sift3DError):
        built.read_similarity(str(tmp_path / "missing.txt"))
    ok = tmp_path / "ok.txt"
    ok.write_text("2.0\t0.0\t0.0\t1.5\n0.0\t2.0\t0.0\t0.0\n0.0\t0.0\t2.0\t0.0\n0.0\t0.0\t0.0\t1.0\n")
    assert (built.read_similarity(str(ok)) == np.array([[2, 0, 0, 1.5], [0, 2, 0, 0], [0, 0, 2, 0], [0, 0, 0, 1]], np.float32)).all()


# ---- the key-coordinate convention of featExtract, on the oracle's extraction ------------------------------------------------
def _blob(shape, voxel, c, sigma):
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    d2 = ((x - c[0]) * voxel[0]) ** 2 + ((y - c[1]) * voxel[1]) ** 2 + ((z - c[2]) * voxel[2]) ** 2
    return (1000 * np.exp(-d2 / (2 * sigma * sigma))).astype(np.float32)


QFORM = (0.1, 0.2, 0.3, -30.0, 20.0, 5.0, -1.0)


@pytest.mark.parametrize("shape,voxel,centre,sigma,world", [
    ((40, 40, 40), (1.0, 1.0, 1.0), (21.3, 17.6, 14.2), 3.0, False),
    ((32, 40, 48), (1.0, 1.25, 1.5), (23.0, 18.0, 14.0), 4.0, True),
    ((32, 40, 48), (2.0, 1.0, 1.0), (14.0, 18.0, 14.0), 3.0, True),
])
def test_key_convention_of_featextract(built, tmp_path, shape, voxel, centre, sigma, world):
    """An isolated blob centred on voxel c: the record at its centre is key_vox2key . c, i.e. c + 0.5 in voxel units and
    qto . (c + 0.5 f) under -w -- not c, and not qto . c."""
    _oracle.build()
    nii, key = str(tmp_path / "b.nii"), str(tmp_path / "b.key")
    built.write_nifti(nii, _blob(shape, voxel, centre, sigma), voxel=voxel, qform=QFORM)
    subprocess.run([_oracle.CLI] + (["-w"] if world else []) + [nii, key], check=True, capture_output=True)
    recs = built.read_key(key)
    _, hdr = built.read_nifti(nii)
    W = hdr["qto_xyz"] if world else None
    V2K = built.key_vox2key(voxel, W).astype(np.float64)
    pts = np.stack([recs["x"], recs["y"], recs["z"]], 1).astype(np.float64)
    c1 = np.array(list(centre) + [1.0])
    want = (V2K @ c1)[:3]
    err = np.linalg.norm(pts - want, axis=1)
    best = int(np.argmin(err))
    Winv = np.linalg.inv(np.eye(4) if W is None else W.astype(np.float64))
    vox_err = (Winv @ np.append(pts[best], 1.0))[:3] - (Winv @ np.append(want, 1.0))[:3]
    assert np.abs(vox_err).max() < 0.02, vox_err                     # the record sits where key_vox2key puts it
    naive = ((np.eye(4) if W is None else W.astype(np.float64)) @ c1)[:3]
    naive_vox = (Winv @ np.append(naive, 1.0))[:3] - (Winv @ np.append(pts[best], 1.0))[:3]
    assert np.abs(naive_vox).max() > 0.3                              # and not at world . c


# ---- the oracle's inside and NaN rules -------------------------------------------------------------------------------------
def _const_map(q):
    """a map whose every output voxel has source position q (zero linear part)"""
    A = np.zeros((3, 4), np.float32)
    A[:, 3] = q
    return A


def test_oracle_inside_rule_and_nan(rorc):
    n = (5, 4, 3)   # nx, ny, nz
    vol = np.arange(60, dtype=np.float32).reshape(3, 4, 5) + 1
    top = np.array([n[0] - 1, n[1] - 1, n[2] - 1], np.float32)
    fill = -7.0
    one = lambda A, mode="linear": rorc.resample(vol, (1, 1, 1), A, mode, fill)[0, 0, 0]
    # q = n - 1 exactly: inside, the last voxel (i1 clamps to n - 1)
    assert one(_const_map(top)) == vol[2, 3, 4]
    assert one(_const_map(top), "nearest") == vol[2, 3, 4]
    # q = nextafter(n - 1, inf) on one axis: outside
    for ax in range(3):
        q = top.copy()
        q[ax] = np.nextafter(q[ax], np.float32(np.inf))
        assert one(_const_map(q)) == fill and one(_const_map(q), "nearest") == fill
        q = np.zeros(3, np.float32)
        q[ax] = np.nextafter(np.float32(0), np.float32(-1))
        assert one(_const_map(q)) == fill
    # q = -0.0 on every axis: inside (-0 >= 0), voxel 0; made by a map row (-1, -1, -1, -0) at output voxel (0, 0, 0)
    A = np.zeros((3, 4), np.float32)
    A[:, :3] = -1
    A[:, 3] = np.float32(-0.0)
    got = rorc.resample(vol, (1, 1, 2), A, "linear", fill)
    assert got[0, 0, 0] == vol[0, 0, 0] and got[0, 0, 1] == fill      # voxel (1, 0, 0) maps to -1: outside
    # a NaN position on any axis: fill, in both modes; a NaN map too
    for ax in range(3):
        q = np.ones(3, np.float32)
        q[ax] = np.nan
        assert one(_const_map(q)) == fill and one(_const_map(q), "nearest") == fill
    assert np.isnan(rorc.resample(vol, (1, 1, 1), _const_map([np.nan] * 3), "linear", np.nan)[0, 0, 0])
    # inside, off the grid: x first, then y, then z, each (1 - w) a + w b
    q = np.array([1.25, 2.5, 0.75], np.float32)
    f = lambda x, y, z: np.float32(vol[z, y, x])
    lerp = lambda a, b, w: (np.float32(1) - w) * a + w * b
    wx, wy, wz = np.float32(0.25), np.float32(0.5), np.float32(0.75)
    e = [lerp(f(1, y, z), f(2, y, z), wx) for z in (0, 1) for y in (2, 3)]
    want = lerp(lerp(e[0], e[1], wy), lerp(e[2], e[3], wy), wz)
    assert one(_const_map(q)) == want
    assert one(_const_map(q), "nearest") == vol[1, 3, 1]   # floor(q + 0.5) = (1, 3, 1)


def test_oracle_nan_voxel_of_weight_zero(rorc):
    vol = np.ones((2, 2, 2), np.float32)
    vol[0, 0, 1] = np.nan         # voxel x = 1 of the first line
    # q = (0, 0, 0): the NaN corner has weight wx = 0 and still gives NaN (0 * NaN)
    assert np.isnan(rorc.resample(vol, (1, 1, 1), _const_map([0, 0, 0]))[0, 0, 0])
    # nearest reads one voxel only
    assert rorc.resample(vol, (1, 1, 1), _const_map([0, 0, 0]), "nearest")[0, 0, 0] == 1
    # at q = n - 1 on x the upper corner IS the lower one: the NaN is read with weight 1 - 0
    vol2 = np.ones((2, 2, 2), np.float32)
    vol2[0, 0, 0] = np.nan
    assert rorc.resample(vol2, (1, 1, 1), _const_map([1, 0, 0]))[0, 0, 0] == 1   # corners x = 1 only: no NaN
    vol3 = np.full((2, 2, 2), np.inf, np.float32)
    vol3[:, :, 0] = 1
    assert np.isnan(rorc.resample(vol3, (1, 1, 1), _const_map([0, 0, 0]))[0, 0, 0])   # 0 * inf


def test_oracle_plane_range_matches_whole(rorc):
    rng = np.random.default_rng(3)
    vol = rng.normal(size=(9, 7, 11)).astype(np.float32)
    A = np.array([[0.9, 0.1, 0, 0.3], [-0.1, 0.9, 0.05, 0.2], [0, -0.05, 1.1, -0.4]], np.float32)
    whole = rorc.resample(vol, (10, 8, 12), A)
    part = rorc.resample(vol, (10, 8, 12), A, z0=3, z1=7)
    assert part.tobytes() == whole[3:7].tobytes()
