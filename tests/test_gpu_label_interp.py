"""GPU suite: label-aware linear interpolation against the CPU oracle tests/label_interp_oracle.c -- equal bits
where the result is a number, NaN where it is NaN -- always through the C-ABI: sift3d_resample_affine, sift3d_resample_field and
sift3d_resample_affine_dev with SIFT3D_INTERP_LABEL, under the allocator's fill and past one grid of workgroups, the fusion stage
with label_interp, and featResample -l and featFuse -l end to end."""
import os
import subprocess

import numpy as np
import pytest

import grid_loop_cases as gl
from _helpers import caller_stream, run
from field_cases import FieldOracle
from fuse_cases import cpu_fuse, fused_labels, leg, same_report, scenario
from fuse_search_cases import FuseSearchOracle, cpu_fuse_search, same_search_report
from label_interp_cases import TIE_MAPS, LabelForNearest, LabelOracle, a_map, same, source, tie_case
from resample_cases import ResampleOracle, about_centre, rot
from test_gpu_caller_stream import bits
from test_gpu_fuse import report_text

pytestmark = pytest.mark.gpu

LABEL = 2   # SIFT3D_INTERP_LABEL


@pytest.fixture(scope="module")
def lo(tmp_path_factory):
    return LabelOracle(tmp_path_factory.mktemp("label_interp_oracle"))


@pytest.fixture(scope="module")
def ro(tmp_path_factory):
    return ResampleOracle(tmp_path_factory.mktemp("resample_oracle"))


@pytest.fixture(scope="module")
def fo(tmp_path_factory):
    return FieldOracle(tmp_path_factory.mktemp("field_oracle"))


@pytest.fixture(scope="module")
def fs(tmp_path_factory):
    return FuseSearchOracle(tmp_path_factory.mktemp("fuse_search_oracle"))


@pytest.fixture(scope="module")
def scen(built, ro, tmp_path_factory):
    return scenario(built, ro, tmp_path_factory.mktemp("fuse_scenario"))


@pytest.fixture(scope="module")
def wanted(built, fs, lo, ro, fo, scen):
    """the fusion scenario (SSD, power 2) through the restatement with M_k from the label oracle, once per search radius"""
    memo = {}

    def get(search):
        if search not in memo:
            lr, lf = LabelForNearest(lo, ro), LabelForNearest(lo, fo)
            args = (built, fs, lr, lf, scen["target"], leg(scen, "ssd"), scen["vox2key"])
            memo[search] = cpu_fuse(*args, metric="ssd", power=2) if search == 0 else cpu_fuse_search(*args, metric="ssd", power=2, search=search)
        return memo[search]
    return get


# ---- 1: sift3d_resample_affine -------------------------------------------------------------------------------------------------------
# (source shape zyx, output shape zyx, map, source kind, fill): 1^3, 5 x 4 x 3, 37 x 5 x 129 and 130 x 67 x 33 as nx x ny x nz; outputs
# larger and smaller than the source; rows of 1, 5, 8, 22, 33, 37, 40, 61, 67, 70, 130, 140 and 171 voxels
NAN = float("nan")
CASES = [((1, 1, 1), (1, 1, 1), "identity", "iid", 0.0),
         ((1, 1, 1), (3, 2, 5), "half_x", "blobby", -7.0),
         ((3, 4, 5), (3, 4, 5), "identity", "blobby", 0.0),
         ((3, 4, 5), (5, 7, 8), "half_xyz", "iid", NAN),
         ((3, 4, 5), (2, 3, 4), "oblique", "special", -7.0),
         ((129, 5, 37), (129, 5, 37), "identity", "blobby", -7.0),
         ((129, 5, 37), (131, 7, 40), "half_xyz", "blobby", NAN),
         ((129, 5, 37), (64, 9, 70), "oblique", "special", -7.0),
         ((33, 67, 130), (33, 67, 130), "identity", "special", 0.0),
         ((33, 67, 130), (33, 67, 130), "half_x", "blobby", -7.0),
         ((33, 67, 130), (33, 67, 130), "qz", "blobby", -7.0),
         ((33, 67, 130), (130, 33, 67), "qx", "iid", 0.0),
         ((33, 67, 130), (67, 130, 33), "qy", "special", NAN),
         ((33, 67, 130), (50, 90, 171), "scale_half", "blobby", 0.0),
         ((33, 67, 130), (17, 30, 61), "scale_2", "iid", -7.0),
         ((33, 67, 130), (40, 70, 140), "oblique2", "blobby", -7.0),
         ((33, 67, 130), (40, 70, 140), "oblique", "iid", NAN),
         ((33, 67, 130), (20, 21, 22), "outside", "iid", NAN)]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_resample_label_bit_equal_to_oracle(built, lo, case):
    src_shape, out_shape, kind, skind, fill = CASES[case]
    vol = source(skind, src_shape, case + 1)
    A = a_map(kind, src_shape, out_shape)
    got = built.resample_affine(vol, out_shape, A, "label", fill)
    same(got, lo.resample(vol, out_shape, A, fill))
    if kind == "outside":
        assert np.isnan(got).all() if fill != fill else (got == np.float32(fill)).all()
    if kind == "identity":       # finite voxels: the source's bytes; the others: the unlabelled class alone, NaN
        fin = np.isfinite(vol)
        assert (got.view(np.uint32)[fin] == vol.view(np.uint32)[fin]).all() and np.isnan(got[~fin]).all()
    else:                        # never a blend: every number in the output is the fill or a value the source holds
        assert np.isin(got[np.isfinite(got)], np.append(vol[np.isfinite(vol)], np.float32(fill))).all()


@pytest.mark.parametrize("fill", [0.0, NAN])
@pytest.mark.parametrize("kind", TIE_MAPS)
def test_tie_cases_bit_equal_to_oracle(built, lo, kind, fill):
    """the two cases test_label_interp_cpu.py holds to a quarter and more of exact ties"""
    vol, out_shape, A = tie_case(kind)
    same(built.resample_affine(vol, out_shape, A, "label", fill), lo.resample(vol, out_shape, A, fill))


def test_hand_cases_on_the_device(built, lo):
    """the inside, NaN, tie and -0 rules of test_label_interp_cpu.py's hand cases, through the kernel"""
    vol = np.arange(60, dtype=np.float32).reshape(3, 4, 5) % 3 + 1
    vol[0, 0, 1], vol[0, 0, 2], vol[1, 1, 1], vol[1, 1, 2], vol[2, 3, 4] = np.nan, 2.0, -0.0, 0.0, 5.0
    top = np.array([4, 3, 2], np.float32)
    qs = [top, np.float32([0, 0, 0]), np.float32([1.5, 0, 0]), np.float32([1.5, 1, 1]), np.float32([1.0, 0, 0]), np.float32([1.25, 2.5, 0.75]),
          np.float32([1.5, 1.5, 0.25]), np.float32([np.nan, 1, 1])]
    for ax in range(3):
        q = top.copy()
        q[ax] = np.nextafter(q[ax], np.float32(np.inf))
        qs.append(q)
    for q in qs:
        A = np.zeros((3, 4), np.float32)
        A[:, 3] = q
        same(built.resample_affine(vol, (2, 3, 4), A, "label", -7.0), lo.resample(vol, (2, 3, 4), A, -7.0))
    # at (0, 0, 0) the NaN voxel (1, 0, 0) is a corner of weight 0: label mode does not see it, linear mode does
    A = np.zeros((3, 4), np.float32)
    assert built.resample_affine(vol, (1, 1, 1), A, "label", -7.0)[0, 0, 0] == vol[0, 0, 0] == 1.0
    assert np.isnan(built.resample_affine(vol, (1, 1, 1), A, "linear", -7.0)).all()
    # -0 and 0 at (1.5, 1, 1) are one class: the bits of its lower corner
    A[:, 3] = (1.5, 1, 1)
    assert built.resample_affine(vol, (1, 1, 1), A, "label", -7.0).view(np.uint32)[0, 0, 0] == np.float32(-0.0).view(np.uint32)


def test_an_unknown_mode_is_refused_with_the_three_names(built, monkeypatch):
    monkeypatch.setitem(built.INTERP, "unknown", 3)
    vol, A = np.zeros((4, 4, 4), np.float32), np.zeros((3, 4), np.float32)
    fv = built.key_vox2key()
    field = {"n": (2, 2, 2), "origin": np.zeros(3, np.float32), "spacing": np.float32(4.0), "disp": np.zeros((3, 2, 2, 2), np.float32)}
    for call in (lambda: built.resample_affine(vol, (4, 4, 4), A, "unknown"), lambda: built.resample_field(vol, (4, 4, 4), A, field, fv, fv, "unknown")):
        with pytest.raises(built.Sift3DError, match="SIFT3D_INTERP_LINEAR, SIFT3D_INTERP_NEAREST or SIFT3D_INTERP_LABEL"):
            call()
    with pytest.raises(KeyError):
        built.resample_affine(vol, (4, 4, 4), A, "cubic")


# ---- 2: sift3d_resample_field --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (37, 5, 129), (130, 67, 33)])
def test_field_warp_label_equals_oracle(built, lo, shape):
    """test_gpu_field.py's kind of field (random nodes, some NaN) under label mode; a zero field gives the bytes of the affine form"""
    rng = np.random.default_rng(sum(shape))
    vol = source("blobby", shape, 1)
    out_shape = tuple(max(1, s - 3) for s in shape)
    A = about_centre(rot((1, 2, 3), 17.0), shape, out_shape, shift=(0.5, -0.75, 1.0))
    fv = built.key_vox2key((1.0, 1.0, 1.0))
    n = tuple(int(x) for x in (np.array(out_shape[::-1]) // 4 + 4))
    disp = rng.uniform(-3, 3, (3,) + n[::-1]).astype(np.float32)
    disp.reshape(-1)[rng.choice(disp.size, disp.size // 30, replace=False)] = np.nan
    field = {"n": n, "origin": np.array([-6.0, -5.5, -7.25], np.float32), "spacing": np.float32(4.0), "disp": disp}
    Cm, K = built.field_warp_terms(fv, fv)
    for fill in (0.0, np.nan, -7.0):
        same(built.resample_field(vol, out_shape, A, field, fv, fv, "label", fill), lo.warp(vol, out_shape, A, Cm, K, field, fill))
    zero = dict(field, disp=np.zeros_like(field["disp"]))
    assert built.resample_field(vol, out_shape, A, zero, fv, fv, "label").tobytes() == built.resample_affine(vol, out_shape, A, "label").tobytes()


# ---- 3: sift3d_resample_affine_dev ----------------------------------------------------------------------------------------------------
DEV_SRC, DEV_OUT = (33, 67, 130), (40, 70, 141)


def test_dev_entry_point_equals_host_form(built):
    import torch
    vol = source("blobby", DEV_SRC, 9)
    A = a_map("oblique2", DEV_SRC, DEV_OUT)
    want = built.resample_affine(vol, DEV_OUT, A, "label", -7.0)
    d_src = torch.from_numpy(vol).cuda()
    d_dst = torch.full(DEV_OUT, 3.0, dtype=torch.float32, device="cuda")
    with built.Context(64, 64, 64) as ctx:
        ctx.resample_affine_dev(d_src.data_ptr(), vol.shape, d_dst.data_ptr(), d_dst.shape, A, "label", -7.0)
        torch.cuda.synchronize()
    same(d_dst.cpu().numpy(), want)


def test_dev_entry_point_on_the_callers_stream(built, lo):
    """test_gpu_caller_stream.py's pattern: after sift3d_set_stream(S) the producer, the call and the consumer are all queued on the
    non-blocking stream S with no synchronisation anywhere; three inputs, every output the oracle's bits"""
    import torch
    A = a_map("oblique2", DEV_SRC, DEV_OUT)
    base = source("iid", DEV_SRC, 5)
    want = [lo.resample((base + np.float32(k)).astype(np.float32), DEV_OUT, A, -7.0) for k in range(3)]
    with caller_stream(1) as S, built.Context(64, 64, 64) as ctx:
        d_base = torch.from_numpy(base).cuda()
        d_in = torch.empty_like(d_base)
        d_out = torch.empty(DEV_OUT, dtype=torch.float32, device="cuda")
        junk = torch.empty((16, 1024, 1024), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()                   # the set-up above ran on the default stream: done before S starts
        ctx.set_stream(S.handle)
        for k in range(3):
            with torch.cuda.stream(S.torch):
                d_out.fill_(float("nan"))
                junk.normal_()                     # S is busy ahead of the producer
                d_in.copy_(d_base + float(k))      # producer: queued, not finished
                ctx.resample_affine_dev(d_in.data_ptr(), DEV_SRC, d_out.data_ptr(), DEV_OUT, A, "label", -7.0)
                got = d_out.clone()                # consumer on S, no ctx.sync()
                d_in.fill_(-1.0)                   # and the input is overwritten straight away
                got = got.cpu().numpy()
            assert (bits(got) == bits(want[k])).all(), k
        torch.cuda.synchronize()


# ---- 4: under the allocator's fill ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", [0xFF, 0x00], ids=["ff", "00"])
def test_label_resampling_under_the_fill(built, lo, byte):
    shape, out_shape = (37, 5, 129), (34, 9, 126)
    vol = source("blobby", shape, 2)
    A = a_map("oblique", shape, out_shape)
    want = lo.resample(vol, out_shape, A, -7.0)
    with built.alloc_fill(byte) as stats:
        got = built.resample_affine(vol, out_shape, A, "label", -7.0)
        blocks, nbytes = stats()
    assert blocks > 0 and nbytes > 0, "nothing was allocated under the fill: the case checks nothing"
    same(got, want)
    assert np.isfinite(want).any() and (want == np.float32(-7.0)).any()


# ---- 5: past one grid of workgroups ---------------------------------------------------------------------------------------------------
def test_label_resample_kernel_past_the_cap(built, lo):
    """grid_loop_cases' "y" shape: 2^22 + 32 bricks along y, so 32 workgroups go round the loop a second time; the whole output is
    compared, the second-round bricks (the module's last band) are inside the source, and the output's first third is fill"""
    K = gl.header_constants()
    shape = gl.RESAMPLE_SHAPES["y"]
    vol = gl.thin_source(shape)
    A = gl.thin_map(vol.shape, shape)
    launch = gl.brick_launch_of(shape, K)
    assert launch["nbricks"] == launch["grid"] + gl.EXCESS
    want = lo.resample(vol, shape, A, -7.0)
    filled = float((want == np.float32(-7.0)).mean())
    last = want[gl.second_round_mask(shape, launch, K)]
    assert 0.1 < filled < 0.9 and last.size == gl.EXCESS * K["BRICK_BY"] and (last == np.float32(-7.0)).mean() < 0.7 and np.isnan(want).any()
    got = built.resample_affine(vol, shape, A, "label", -7.0)
    differ = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    assert not differ.any(), "%d voxels differ, %d of them in second-round bricks" % (differ.sum(), (differ & gl.second_round_mask(shape, launch, K)).sum())


# ---- 6: the fusion stage --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("search", [0, 1])
def test_stage_with_label_interp_equals_its_restatement(built, scen, wanted, search):
    words, rep = built.fuse_labels(scen["target"], leg(scen, "ssd"), scen["vox2key"], metric="ssd", power=2, search=search, label_interp=LABEL)
    want, want_rep = wanted(search)
    assert np.array_equal(words, want)
    same_report(rep, want_rep)
    if search:
        same_search_report(rep, want_rep)
    by_name = built.fuse_labels(scen["target"], leg(scen, "ssd"), scen["vox2key"], metric="ssd", power=2, search=search, label_interp="label")[0]
    assert np.array_equal(by_name, words)


def test_stage_refuses_linear_labels_and_defaults_to_nearest(built, fs, ro, fo, scen):
    atlases = leg(scen, "ssd")[:2]
    for bad in (0, 3, -1):
        with pytest.raises(built.Sift3DError, match="label_interp must be SIFT3D_INTERP_NEAREST"):
            built.fuse_labels(scen["target"], atlases, scen["vox2key"], label_interp=bad)
        with pytest.raises(built.Sift3DError, match="label_interp must be SIFT3D_INTERP_NEAREST"):
            built.fuse_labels(scen["target"], atlases, scen["vox2key"], search=1, label_interp=bad)
    assert built.fuse_params().label_interp == built.INTERP["nearest"]
    want, want_rep = cpu_fuse(built, fs, ro, fo, scen["target"], atlases, scen["vox2key"], metric="ssd", power=2)
    for kw in ({}, {"label_interp": 1}, {"label_interp": "nearest"}):
        words, rep = built.fuse_labels(scen["target"], atlases, scen["vox2key"], **kw)
        assert np.array_equal(words, want)
        same_report(rep, want_rep)


# ---- 7: the command lines -------------------------------------------------------------------------------------------------------------
def write_scenario(built, scen, tmp_path):
    """the scenario's files; returns featFuse's four arguments per atlas"""
    built.write_nifti(str(tmp_path / "target.nii"), scen["target"])
    built.write_nifti(str(tmp_path / "truth.nii"), scen["truth"])
    groups = []
    for k, a in enumerate(leg(scen, "ssd")):
        built.write_nifti(str(tmp_path / ("atlas%d.nii" % k)), a["image"])
        built.write_nifti(str(tmp_path / ("labels%d.nii" % k)), a["labels"])
        built.write_matrix(str(tmp_path / ("atlas%d.trans.txt" % k)), a["t"])
        built.write_field(str(tmp_path / ("atlas%d.field.nii" % k)), a["field"])
        groups += ["atlas%d.nii" % k, "labels%d.nii" % k, "atlas%d.trans.txt" % k, "atlas%d.field.nii" % k]
    return groups


def test_featresample_label_end_to_end(built, scen, tmp_path):
    """featResample -l, with and without -u, equals the Python path driven by the same .trans.txt (and field file); -l -n is a
    usage error"""
    write_scenario(built, scen, tmp_path)
    a = leg(scen, "ssd")[1]
    vk = built.key_vox2key()
    A = built.resample_map(built.read_similarity(str(tmp_path / "atlas1.trans.txt")), vk, vk)
    field = built.read_field(str(tmp_path / "atlas1.field.nii"))
    shape = scen["target"].shape
    for options, want in ((["-l"], built.resample_affine(a["labels"], shape, A, "label")),
                          (["-l", "-u", "atlas1.field.nii"], built.resample_field(a["labels"], shape, A, field, vk, vk, "label")),
                          (["-l", "-fnan"], built.resample_affine(a["labels"], shape, A, "label", np.nan))):
        run(["timeout", "-k", "10", "120", built.FEATRESAMPLE, "-d0"] + options + ["target.nii", "labels1.nii", "atlas1.trans.txt", "out.nii"], tmp_path)
        got, hdr = built.read_nifti(str(tmp_path / "out.nii"))
        assert hdr["dims"] == (40, 40, 40, 1) and got.tobytes() == want.tobytes(), options
    assert not np.array_equal(want, built.resample_affine(a["labels"], shape, A, "nearest", np.nan), equal_nan=True)   # -l is not -n
    for argv in (["-l", "-n"], ["-n", "-l"], ["-lx"]):
        r = subprocess.run(["timeout", "-k", "10", "60", built.FEATRESAMPLE] + argv + ["target.nii", "labels1.nii", "atlas1.trans.txt", "bad.nii"],
                           cwd=tmp_path, capture_output=True, text=True)
        assert r.returncode == 255 and "Usage: featResample" in r.stdout and "  -l  " in r.stdout, (argv, r.returncode, r.stdout[-500:])
        assert ("-n and -l" in r.stdout) == (argv != ["-lx"]) and not os.path.exists(str(tmp_path / "bad.nii"))


def fuse_outputs(built, tmp_path, options, groups):
    run(["timeout", "-k", "10", "120", built.FEATFUSE, "-d0"] + options + ["target.nii", "out.nii"] + groups, tmp_path)
    return [open(str(tmp_path / name), "rb").read() for name in ("out.nii", "out.nii.conf.nii", "out.nii.fuse.txt")]


def test_featfuse_label_end_to_end(built, fs, ro, fo, scen, wanted, tmp_path):
    """featFuse -l writes the three outputs the stage with label_interp = 2 implies, the report with its extra second line; without
    -l it writes the bytes of fuse_labels with the defaults"""
    groups = write_scenario(built, scen, tmp_path)
    for options, (want, rep), extra in ((["-l", "-t", "truth.nii"], wanted(0), "# label_interp label\n"),
                                        (["-t", "truth.nii"], built.fuse_labels(scen["target"], leg(scen, "ssd"), scen["vox2key"]), "")):
        got = fuse_outputs(built, tmp_path, options, groups)
        labels = fused_labels(want, 0.0)
        conf = (want[..., 1].astype(np.float32) / np.float32(65535.0)).astype(np.float32)
        assert got[0][-labels.nbytes:] == labels.tobytes() and got[1][-conf.nbytes:] == conf.tobytes(), options
        text = report_text(5, 2, "ssd", 2, 0.0, rep, fused_labels(want), scen["truth"], built)
        cut = text.index("\n") + 1
        assert got[2].decode() == text[:cut] + extra + text[cut:], options
        assert (b"label_interp" in got[2]) == bool(extra)
    r = subprocess.run(["timeout", "-k", "10", "60", built.FEATFUSE, "-lx", "t.nii", "o.nii", "a", "b", "c", "-"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 255 and "Usage: featFuse" in r.stdout and "  -l  " in r.stdout
