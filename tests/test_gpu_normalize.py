"""GPU suite: the intensity matching against the CPU oracle tests/normalize_oracle.c, always through the C-ABI:
sift3d_overlap_histograms, sift3d_apply_transfer and the stage sift3d_normalize_intensity on every shape, map kind, field, mask and
vox2key, past both launch caps, with non-finite voxels and a NaN field node, on one-bin volumes, at every knot count either side of
the bisection's step counts, under poisoned allocations, call after call, their refusals; and featNormalize end to end.  Every
comparison is equality: of every histogram word, sum and count, of every double of the table, of every output word."""
import os
import re

import numpy as np
import pytest

from _helpers import run
from normalize_cases import (BIG_IMAGE, BIG_REF, FV, KNOTS, MAP_KINDS, MODES, SHAPES, NormalizeOracle, Refused, bits32, matrix_of_map, one_bin_pair, pair, same_stage,
                             same_tables, same_words, scenario)
from blockmatch_cases import volume
from invert_cases import forward_field
from register_cases import map_of
from resample_cases import ResampleOracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def no(tmp_path_factory):
    return NormalizeOracle(tmp_path_factory.mktemp("normalize_oracle"))


def against_oracle(built, no, R, a, M=None, rv=None, modes=MODES, knots=64):
    """the first kernel alone, then the stage in every mode, against the oracle; returns the counted voxels"""
    ar, br = no.range(R), no.range(a["image"])
    if ar is None or br is None:            # a single voxel: the kernel with ranges given, and the stage's refusal
        ar, br = (np.float32(-900.0), np.float32(1100.0)), (np.float32(-500.0), np.float32(400.0))
        same_words(built.overlap_histograms(R, a, ar, br, rv, M), no.overlap(built, R, a, ar, br, rv, M))
        with pytest.raises(built.Sift3DError, match="no two distinct finite values") as e:
            built.normalize_intensity(R, a, rv, M)
        assert e.value.code == -1
        return 0
    want = no.overlap(built, R, a, ar, br, rv, M)
    same_words(built.overlap_histograms(R, a, ar, br, rv, M), want)
    for mode in modes:
        try:
            expect = no.stage(built, R, a, rv, M, mode=mode, knots=knots)
        except Refused as r:
            with pytest.raises(built.Sift3DError, match=r.text) as e:
                built.normalize_intensity(R, a, rv, M, mode=mode, knots=knots)
            assert e.value.code == -1 and e.value.report["sums"] == want[2] and e.value.report["counts"] == want[3]
            continue
        same_stage(built.normalize_intensity(R, a, rv, M, mode=mode, knots=knots), expect)
    return want[2][0]


# ---- shapes, map kinds, fields, masks, keys --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s[::-1])))
def test_every_map_kind_field_and_mask_equals_the_oracle(built, no, shape):
    """1 voxel, 4 x 3 x 2, a brick plus one voxel per axis and 70 x 19 x 11, the image's shape a few voxels off per axis; the identity, an
    integer shift, a half-voxel shift, a 20 degree rotation and everything outside (the n < 2 refusal); with and without a field, with
    and without a mask; NaN and +-inf voxels in both volumes"""
    seen = 0
    for n, kind in enumerate(MAP_KINDS):
        for field, masked in ((False, False), (True, False), (False, True), (True, True)):
            R, a, M = pair(built, shape, kind, field=field, seed=10 + n, masked=masked, k=1 + n % 4)
            seen += against_oracle(built, no, R, a, M)
    assert seen > 0 or shape == SHAPES[0]


def test_under_an_anisotropic_permuting_vox2key(built, no):
    """both images under FV: the identity, a translation in key units and a slight anisotropic scale with it"""
    moves = [None, np.eye(4, dtype=np.float32), np.diag([1.02, 0.98, 1.0, 1.0]).astype(np.float32)]
    moves[1][:3, 3] = [0.7, -1.3, 0.9]
    moves[2][:3, 3] = [-0.4, 0.6, 1.2]
    for shape in SHAPES[2:]:
        seen = 0
        for n, t in enumerate(moves):
            R, a, M = pair(built, shape, "identity", field=bool(n % 2), ref_vox2key=FV, seed=20 + n, masked=n == 2)
            a["vox2key"], a["t"] = FV, t
            seen += against_oracle(built, no, R, a, M, FV)
        assert seen > R.size


def test_non_finite_voxels_and_a_nan_field_node(built, no):
    """a NaN or infinite image voxel reaches the samples that read it with weight 0 and they are excluded; a NaN node of the field makes the
    positions around it NaN, and they are outside"""
    v = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    for bad in (np.nan, np.inf, -np.inf):
        w = (2 * v + 1).astype(np.float32)
        w[0, 0, 1] = bad
        got = built.overlap_histograms(v, {"image": w}, no.range(v), no.range(w))
        same_words(got, no.overlap(built, v, {"image": w}, no.range(v), no.range(w)))
        assert got[3] == {"masked": 0, "outside": 0, "excluded": 2} and got[2][0] == 22
    shape = SHAPES[3]
    R, a, _ = pair(built, shape, "half", field=True, seed=31, k=0)
    whole = no.overlap(built, R, a, no.range(R), no.range(a["image"]))
    a["field"] = dict(a["field"], disp=a["field"]["disp"].copy())
    n = a["field"]["n"]
    a["field"]["disp"][1, n[2] // 2, n[1] // 2, n[0] // 2] = np.nan
    counted = against_oracle(built, no, R, a)
    want = no.overlap(built, R, a, no.range(R), no.range(a["image"]))
    assert 0 < counted < whole[2][0] and want[3]["outside"] > whole[3]["outside"]


@pytest.mark.parametrize("top", [False, True], ids=["bin0", "bin1023"])
def test_every_counted_voxel_in_one_bin(built, no, top):
    """the contended path (every lane of every wave holds one bin) and the upper end of the sums: linear refuses, hist has its table"""
    for shape in (SHAPES[3], (9, 40, 130)):
        R, a, M = one_bin_pair(shape, top)
        n = against_oracle(built, no, R, a, M)
        assert n == R.size - 1
        ha, hb, sums, counts = built.overlap_histograms(R, a, no.range(R), no.range(a["image"]), None, M)
        q = 1023 if top else 0
        assert ha[q] == hb[q] == n and sums == [n, n * q, n * q, n * q * q, n * q * q, n * q * q]


def test_background_beside_texture(built, no):
    """a constant background over most of the volume, texture in the rest: waves that hold one bin beside waves that do not, in one launch"""
    shape = (12, 33, 100)
    R, B = volume("smooth", shape, 41), (np.float32(0.5) * volume("smooth", shape, 42) + np.float32(20.0)).astype(np.float32)
    R[:, :, :61], B[:, :20, :] = -1500.0, -900.0
    against_oracle(built, no, R, {"image": B, "t": matrix_of_map(map_of("shift", shape, shape))})


# ---- the scenario ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma", [False, True], ids=["gain_offset", "gamma"])
def test_scenario_equals_the_oracle(built, no, tmp_path_factory, tmp_path, gamma):
    """section 7s's scenario (test_normalize_cpu.py has its figures): each of the five remapped atlases normalised to the target through its
    own transform and field under the grid's vox2key, in both modes, on both legs: every word the oracle's"""
    ro = ResampleOracle(tmp_path_factory.mktemp("resample_oracle"))
    target, gv, clean, remapped = scenario(built, ro, tmp_path, gamma)
    for a in remapped:
        for mode in MODES:
            got = built.normalize_intensity(target, a, gv, None, mode=mode, knots=64)
            same_stage(got, no.stage(built, target, a, gv, None, mode=mode, knots=64))
            assert got[1]["sums"][0] > 0.5 * target.size


# ---- past the launch caps ----------------------------------------------------------------------------------------------------------------
def test_past_both_launch_caps(built, no):
    """BIG_REF has more bricks than two trips of the histogram launch's workgroups, BIG_IMAGE more voxels than two trips of the apply launch's
    (test_normalize_cpu.py holds both to the kernel's #defines): a change in the reference's last row changes the sums, and the image's last
    voxels are mapped"""
    R = volume("smooth", BIG_REF, 5)
    B = (np.float32(0.5) * volume("smooth", BIG_IMAGE, 6) + np.float32(7.0)).astype(np.float32)
    B[-1, -1, -40:-20] = np.nan
    a = {"image": B, "t": matrix_of_map(map_of("half", BIG_REF, BIG_IMAGE))}
    want = no.stage(built, R, a, mode="hist", knots=64)
    got = built.normalize_intensity(R, a, mode="hist", knots=64)
    same_stage(got, want)
    assert np.isfinite(got[0][-1, -1, -19:]).all() and np.isnan(got[0][-1, -1, -40:-20]).all()
    R2 = R.copy()
    R2[-1, -1, -100:-50] += 300.0
    ar, br = no.range(R2), no.range(B)
    got2 = built.overlap_histograms(R2, a, ar, br)
    same_words(got2, no.overlap(built, R2, a, ar, br))
    assert got2[2][0] == got[1]["sums"][0] and got2[2][1] != got[1]["sums"][1]
    last = no.overlap(built, R[-1:], dict(a, t=matrix_of_map(map_of("half", BIG_REF, BIG_IMAGE) + np.array([[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, BIG_REF[0] - 1.0]]))), no.range(R), no.range(B))
    assert last[2][0] > 0           # the reference's last plane is counted


# ---- the apply kernel alone ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", KNOTS)
def test_apply_at_every_knot_count(built, no, Q):
    """Q = 2, 3, 64, 65, 255, 256: m = Q + 1 knots, either side of the powers of two at which the bisection takes another step; voxels below,
    at, between and above the knots, beyond the image's range, non-finite ones with their bits; a length that is no multiple of four"""
    rng = np.random.default_rng(Q)
    a, b = rng.integers(0, 1024, 30000), rng.integers(0, 1024, 30000)
    la, lb = [int(x) for x in a], [int(x) for x in b]
    sums = [len(la), sum(la), sum(lb), sum(x * x for x in la), sum(x * x for x in lb), sum(x * y for x, y in zip(la, lb))]
    ar, br = (np.float32(-100.0), np.float32(923.5)), (np.float32(0.5), np.float32(2.25))
    for mode in MODES:
        t = built.normalize_transfer(mode, np.bincount(a, minlength=1024), np.bincount(b, minlength=1024), sums, ar, br, Q)
        same_tables(t, no.transfer(mode, np.bincount(a, minlength=1024), np.bincount(b, minlength=1024), sums, ar, br, Q))
        assert t["m"] == (Q + 1 if mode == "hist" else 2)
        lo, hi = float(br[0]), float(br[1])
        at_knots = (lo + (hi - lo) * t["xb"] / 1023.0).astype(np.float32)
        v = np.concatenate([rng.uniform(lo, hi, 5001), rng.uniform(lo - 3, hi + 3, 500), at_knots, np.nextafter(at_knots, np.float32(-np.inf)), np.nextafter(at_knots, np.float32(np.inf)),
                            [lo, hi, np.nan, np.inf, -np.inf, 0.0, -0.0, 1e30, -1e30]]).astype(np.float32)
        raw = bits32(v[1:] if v.size % 4 == 0 else v).copy()      # the scalar tail after the last whole float4
        raw[:3] = [0x7FC12345, 0xFFC00001, 0x7F800001]
        v = raw.view(np.float32)
        assert v.size % 4 != 0
        got, want = built.apply_transfer(v, t), no.apply(v, t)
        assert np.array_equal(bits32(got), bits32(want)), int((bits32(got) != bits32(want)).sum())
        assert np.array_equal(bits32(got)[:3], raw[:3])
        for n in (1, 2, 3, 4, 5):
            assert np.array_equal(bits32(built.apply_transfer(v[3:3 + n], t)), bits32(want[3:3 + n]))


# ---- poisoned allocations, state between calls ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", [0xA7, 0x00])
def test_under_poisoned_allocations(built, no, byte):
    """every device block of the call holds the byte before the call uses it: a histogram word or an output word that the call does not
    write itself would show.  The blocks of the stage: the reference, the mask, the image, the nodes, the result words, the output, the knots"""
    shape = SHAPES[3]
    R, a, M = pair(built, shape, "rotation", field=True, seed=51, masked=True)
    ar, br = no.range(R), no.range(a["image"])
    with built.alloc_fill(byte) as stats:
        same_words(built.overlap_histograms(R, a, ar, br, None, M), no.overlap(built, R, a, ar, br, None, M))
        assert stats()[0] == 5
        for mode in MODES:
            got = built.normalize_intensity(R, a, None, M, mode=mode, knots=33)
            same_stage(got, no.stage(built, R, a, None, M, mode=mode, knots=33))
        n_blocks, nbytes = stats()
        assert n_blocks == 2 * 7 and nbytes >= 2 * (8 * R.size + 8 * a["image"].size)        # since stats was last read
        plain = dict(a, field=None)
        same_stage(built.normalize_intensity(R, plain, mode="hist"), no.stage(built, R, plain, mode="hist"))
        assert stats()[0] == 5
        t = got[1]["table"]
        assert np.array_equal(bits32(built.apply_transfer(a["image"], t)), bits32(no.apply(a["image"], t))) and stats()[0] == 3


def test_call_after_call(built, no):
    """calls in one process with other shapes, modes, fields and masks: nothing of one is left in the next"""
    for n, (shape, kind, field, masked, Q) in enumerate(((SHAPES[3], "rotation", True, True, 256), (SHAPES[2], "identity", False, False, 2), (SHAPES[1], "half", True, False, 64),
                                                         (SHAPES[3], "shift", False, True, 65), (SHAPES[3], "rotation", True, True, 256))):
        R, a, M = pair(built, shape, kind, field=field, seed=60 + n % 4, masked=masked)
        against_oracle(built, no, R, a, M, knots=Q)


# ---- the report ---------------------------------------------------------------------------------------------------------------------------------
def test_report(built, no):
    R, a, M = pair(built, SHAPES[3], "half", seed=70, masked=True)
    out, rep = built.normalize_intensity(R, a, None, M, mode="hist", knots=16)
    want = no.stage(built, R, a, None, M, mode="hist", knots=16)[1]
    assert (rep["mode"], rep["knots"], rep["reference_voxels"], rep["image_voxels"]) == (1, 16, R.size, a["image"].size)
    assert rep["hist_ms"] > 0 and rep["apply_ms"] > 0 and rep["wall_ms"] >= rep["hist_ms"] + rep["apply_ms"]
    text = built.normalize_report_text(rep).split("\n")
    assert text[0] == "# mode hist knots 16 kept %d" % want["table"]["m"]
    assert text[3] == "# reference_voxels %d counted %d masked %d outside %d excluded %d" % (R.size, want["sums"][0], want["counts"]["masked"], want["counts"]["outside"], want["counts"]["excluded"])


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals(built):
    """all on the host, before anything is allocated: the extents below are never backed by memory"""
    import ctypes as C
    L = built.hip_lib()
    tiny = np.arange(8, dtype=np.float32)
    out = np.zeros(8, np.float32)
    h = np.zeros(2048 + 9, np.int64)
    singular = np.zeros(16, np.float32)
    singular[15] = 1
    disp = np.zeros(24, np.float32)

    def field(n=(2, 2, 2), spacing=4.0, capacity=24):
        f = built.Field()
        f.n[:] = n
        f.spacing, f.capacity, f.disp = spacing, capacity, disp.ctypes.data
        return f

    def call(stage=True, ref=(2, 2, 2), src=(2, 2, 2), reference=True, image=True, t=None, rv=None, fld=None, ar=(0.0, 1.0), br=(0.0, 1.0), dst=True, **params):
        a = built.AverageImage()
        a.image, (a.nx, a.ny, a.nz) = (tiny.ctypes.data if image else None), src
        a.moving_to_fixed = None if t is None else t.ctypes.data
        a.field = None if fld is None else C.addressof(fld)
        err = C.create_string_buffer(512)
        r = tiny.ctypes.data if reference else None
        if stage:
            p = built.normalize_params(**params)
            rc = L.sift3d_normalize_intensity(r, *ref, None if rv is None else rv.ctypes.data, None, C.addressof(a), C.byref(p), out.ctypes.data if dst else None, None, err, len(err))
        else:
            rc = L.sift3d_overlap_histograms(0, r, *ref, None if rv is None else rv.ctypes.data, None, C.addressof(a), (C.c_float * 2)(*ar), (C.c_float * 2)(*br),
                                             h.ctypes.data if dst else None, h[1024:].ctypes.data, h[2048:].ctypes.data, h[2054:].ctypes.data, None, err, len(err))
        return rc, err.value.decode()

    with built.alloc_fill(0x5A) as stats:
        for stage in (True, False):
            for kw, text in (({"reference": False}, "null pointer"), ({"image": False}, "null pointer"), ({"dst": False}, "null pointer"),
                             ({"ref": (0, 2, 2)}, "reference: nx ny nz = 0 2 2: extents 1 .. 4096, at most 2^30 voxels"), ({"ref": (4097, 2, 2)}, "reference: nx ny nz = 4097 2 2"),
                             ({"ref": (4096, 4096, 65)}, "reference: nx ny nz = 4096 4096 65"), ({"src": (2, 0, 2)}, "image: nx ny nz = 2 0 2: extents 1 .. 4096, at most 2^30 voxels"),
                             ({"src": (2, 2, 4097)}, "image: nx ny nz = 2 2 4097"), ({"src": (4096, 4096, 65)}, "image: nx ny nz = 4096 4096 65"),
                             ({"t": singular}, "image: a matrix's last row is not 0 0 0 1, or a matrix is singular"), ({"rv": singular}, "image: a matrix's last row"),
                             ({"fld": field(n=(1, 2, 2))}, "image: the field needs 2 .. 2^24 nodes per axis"), ({"fld": field(spacing=0.0)}, "image: the field's spacing must be positive and finite"),
                             ({"fld": field(capacity=23)}, "image: the field's disp holds fewer than 3 n0 n1 n2 floats")):
                rc, err = call(stage, **kw)
                assert rc == -1 and text in err, (stage, kw, rc, err)
        for kw, text in (({"mode": 2}, "mode = 2: 0 (linear) or 1 (hist)"), ({"mode": "hist", "knots": 1}, "knots = 1: 2 .. 256"), ({"mode": "hist", "knots": 257}, "knots = 257: 2 .. 256")):
            rc, err = call(True, **kw)
            assert rc == -1 and text in err, (kw, rc, err)
        for kw, text in (({"ar": (1.0, 1.0)}, "ref_range = 1 1: finite, hi > lo"), ({"br": (0.0, np.nan)}, "image_range = 0 nan: finite, hi > lo"), ({"br": (-np.inf, 0.0)}, "image_range = -inf 0")):
            rc, err = call(False, **kw)
            assert rc == -1 and text in err, (kw, rc, err)
        flat = np.full((2, 2, 2), 3.0, np.float32)
        vol = tiny.reshape(2, 2, 2)
        for R, B, text in ((flat, vol, "reference: no two distinct finite values"), (vol, flat, "image: no two distinct finite values"),
                           (vol, np.full((2, 2, 2), np.nan, np.float32), "image: no two distinct finite values")):
            with pytest.raises(built.Sift3DError, match=re.escape(text)) as e:
                built.normalize_intensity(R, {"image": B})
            assert e.value.code == -1
        table = built.normalize_transfer("linear", np.bincount([1, 5], minlength=1024), np.bincount([2, 9], minlength=1024), [2, 6, 11, 26, 85, 47], (0.0, 1.0), (0.0, 1.0))
        bad = dict(table, struct=None, xb=np.array([3.0, 3.0]))
        for args, text in (((vol, bad), "table: xb[1] is not above xb[0]"), ((vol, dict(table, struct=None, xb=table["xb"][:1], xa=table["xa"][:1])), "table: m = 1 knots: 2 .. 257")):
            with pytest.raises(built.Sift3DError, match=re.escape(text)):
                built.apply_transfer(*args)
        err = C.create_string_buffer(512)
        assert L.sift3d_apply_transfer(0, tiny.ctypes.data, 0, C.byref(table["struct"]), out.ctypes.data, None, err, len(err)) == -1 and b"n = 0 voxels: 1 .. 2^30" in err.value
        assert L.sift3d_apply_transfer(0, None, 8, C.byref(table["struct"]), out.ctypes.data, None, err, len(err)) == -1 and b"null pointer" in err.value
        assert stats()[0] == 0          # nothing was allocated by any of them
        rc, err = call(True)
        assert rc == 0 and err == "" and stats()[0] == 5


# ---- featNormalize --------------------------------------------------------------------------------------------------------------------------------
def test_featnormalize_end_to_end(built, no, tmp_path):
    """on NIfTI files the test writes: <out> and <out>.normalize.txt are the bytes the stage implies, in both modes, with a transform and a
    field, with "-" for both, and with -k"""
    assert os.path.exists(built.FEATNORMALIZE)
    shape, key = SHAPES[3], built.key_vox2key()
    R, a, M = pair(built, shape, "identity", seed=81, masked=True, k=2)
    B = a["image"]
    built.write_nifti(str(tmp_path / "r.nii"), R)
    built.write_nifti(str(tmp_path / "b.nii"), B)
    built.write_nifti(str(tmp_path / "m.nii"), M)
    t = np.eye(4, dtype=np.float32)
    t[:3, 3] = [0.5, -1.0, 0.25]
    assert built.host_lib().sift3d_write_matrix(os.fsencode(str(tmp_path / "b.trans.txt")), t.ctypes.data) == 0
    t = built.read_similarity(str(tmp_path / "b.trans.txt"))
    built.write_field(str(tmp_path / "b.field.nii"), forward_field("smooth", built.blockmatch_grid(shape, key, spacing=4.0), seed=82, amp=1.0, wave=25.0))
    field = built.read_field(str(tmp_path / "b.field.nii"))

    def check(stem, image, mask, **params):
        out, rep = built.normalize_intensity(R, image, key, mask, **params)
        same_stage((out, rep), no.stage(built, R, image, key, mask, **params))
        got = built.read_nifti(str(tmp_path / stem))
        got = got[0] if isinstance(got, tuple) else got
        assert got.shape == B.shape and np.array_equal(bits32(np.asarray(got, np.float32)), bits32(out)), stem
        strip = lambda text: [l for l in text.split("\n") if not re.match(r"^\d+\.\d{3} \d+\.\d{3} \d+\.\d{3}$", l)]
        report = open(str(tmp_path / (stem + ".normalize.txt"))).read()
        assert report.startswith("# featNormalize v1.0\n# mode %s knots %d kept " % (params["mode"], params["knots"]))
        assert strip(report)[1:] == strip(built.normalize_report_text(rep))

    run(["timeout", "-k", "10", "120", built.FEATNORMALIZE, "-d0", "-mhist", "-q32", "r.nii", "b.nii", "b.trans.txt", "b.field.nii", "hist.nii"], tmp_path)
    check("hist.nii", {"image": B, "t": t, "vox2key": key, "field": field}, None, mode="hist", knots=32)
    run(["timeout", "-k", "10", "120", built.FEATNORMALIZE, "-k", "m.nii", "r.nii", "b.nii", "-", "-", "lin.nii"], tmp_path)
    check("lin.nii", {"image": B, "vox2key": key}, M, mode="linear", knots=64)
    r = run(["timeout", "-k", "10", "120", built.FEATNORMALIZE, "-mhist", "-k", "m.nii", "r.nii", "b.nii", "b.trans.txt", "-", "both.nii"], tmp_path)
    check("both.nii", {"image": B, "t": t, "vox2key": key}, M, mode="hist", knots=64)
    assert "Done." in r.stdout
    # a mask that leaves nothing: the refusal's text, status 255, no file left behind
    built.write_nifti(str(tmp_path / "z.nii"), np.zeros(shape, np.float32))
    before = sorted(os.listdir(tmp_path))
    import subprocess
    r = subprocess.run([built.FEATNORMALIZE, "-k", "z.nii", "r.nii", "b.nii", "-", "-", "none.nii"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 255 and "Error: could not normalize: 0 voxels are counted: at least 2 are needed" in r.stdout and sorted(os.listdir(tmp_path)) == before
