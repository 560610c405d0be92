"""GPU suite: the template from warped images against the CPU oracle tests/average_oracle.c, always through the
C-ABI: sift3d_average_warped on every shape, image count, trim, field mix and map kind, past the workgroup cap, with non-finite
voxels, under poisoned allocations, call after call, its refusals and its report; and featAverage end to end.  Every comparison is
equality of every word of avg, var and mask with the oracle's."""
import os
import re

import numpy as np
import pytest

from _helpers import run
from average_cases import (BIG, COUNTS, FV, GROUP_EDGES, MAP_KINDS, SHAPES, TRIMS, AverageOracle, bits32, cpu_average, group, matrix_of_map, same_planes, warped_planes)
from blockmatch_cases import volume
from invert_cases import forward_field
from register_cases import holes, map_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ao(tmp_path_factory):
    return AverageOracle(tmp_path_factory.mktemp("average_oracle"))


def against_oracle(built, ao, shape, images, grid_vox2key=None, trims=TRIMS, min_counts=(1,), fill=np.nan):
    """the product against the oracle for every trim and minimum count; returns the last mask.  The oracle warps every image once."""
    planes = warped_planes(built, ao, shape, images, grid_vox2key)
    for trim in trims:
        for min_count in min_counts:
            got = built.average_warped(shape, images, grid_vox2key, trim=trim, min_count=min_count, fill=fill)
            same_planes(got, ao.average(planes, trim, min_count, fill))
    return got[2]


# ---- shapes, counts, trims, fields ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s[::-1])))
def test_every_count_and_trim_equals_the_oracle(built, ao, shape):
    """1 voxel, 4 x 3 x 2, a brick plus one voxel per axis and 70 x 19 x 11; K = 1, 2, 5, 32; trim 0, 1, 15; sources of differing shapes
    with NaN and +-inf voxels; fields of two spacings beside images without one; the map kinds in turn"""
    seen = 0
    for K in COUNTS:
        mask = against_oracle(built, ao, shape, group(built, shape, K, "mixed", seed=3), min_counts=(1, min(K, 3)), fill=-7.0)
        seen += int((mask != 0).sum())
    assert seen > 0


@pytest.mark.parametrize("K", GROUP_EDGES)
def test_counts_at_the_grouping_thresholds(built, ao, K):
    """K = 8, 9, 16, 17: the last count of the kernel's four-voxel and two-voxel instantiations and the first of the next (COUNTS has both ends)"""
    for shape in SHAPES[2:]:
        mask = against_oracle(built, ao, shape, group(built, shape, K, "mixed", seed=K), min_counts=(1, 4), fill=0.0)
    assert (mask != 0).any()


@pytest.mark.parametrize("fields", ["none", "all", "mixed"])
def test_field_mixes_equal_the_oracle(built, ao, fields):
    """no field, every image with one, and mixed, in voxel keys and under an anisotropic, permuting grid vox2key"""
    for shape in SHAPES[2:]:
        against_oracle(built, ao, shape, group(built, shape, 5, fields, seed=5))
        mask = against_oracle(built, ao, shape, group(built, shape, 5, fields, seed=6, grid_vox2key=FV), FV, trims=(1,))
    assert (mask != 0).any()


def test_every_image_contributing(built, ao):
    """maps that keep nearly every image on the grid: n reaches K = 32, and the sort runs over a full column"""
    shape, rng = SHAPES[3], np.random.default_rng(8)
    images = []
    for k in range(32):
        v = (volume("smooth", tuple(n + 8 for n in shape), 80 + k) + np.float32(5.0 * k)).astype(np.float32)
        A = np.hstack([np.eye(3) + rng.normal(0, 0.003, (3, 3)), np.full((3, 1), 4.5 if k % 2 else 4.0)])
        a = {"image": v, "t": matrix_of_map(A)}
        if k % 3 == 0:
            a["field"] = forward_field("smooth", built.blockmatch_grid(shape, None, spacing=4.0 if k % 2 else 6.0), seed=k, amp=1.0, wave=25.0)
        images.append(a)
    mask = against_oracle(built, ao, shape, images, min_counts=(1, 32))
    assert (mask == 0xffffffff).sum() > mask.size // 2


@pytest.mark.parametrize("kind", MAP_KINDS)
def test_map_kinds_equal_the_oracle(built, ao, kind):
    """the identity, an integer shift, a half-voxel shift, a 20 degree rotation and everything outside, each alone (K = 1) and beside an
    identity image (K = 2).  A map with a NaN entry cannot be given: sift3d_resample_map refuses its matrix (test_refusals)"""
    shape = SHAPES[3]
    v = holes(volume("smooth", shape, 2), 12)
    one = {"image": v, "t": matrix_of_map(map_of(kind, shape, shape))}
    mask = against_oracle(built, ao, shape, [one])
    assert (mask != 0).any() == (kind != "outside")
    mask = against_oracle(built, ao, shape, [{"image": volume("smooth", shape, 4)}, one])
    assert (mask & 1).all() and ((mask & 2) != 0).any() == (kind != "outside")


def test_non_finite_voxels_and_nodes(built, ao):
    """a NaN or infinite source voxel reaches the samples that read it with weight 0 and they do not contribute; a NaN node of a field makes
    the positions around it NaN"""
    v = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    for bad in (np.nan, np.inf, -np.inf):
        w = v.copy()
        w[0, 0, 1] = bad
        got = built.average_warped(v.shape, [{"image": v}, {"image": w}])
        same_planes(got, cpu_average(built, ao, v.shape, [{"image": v}, {"image": w}]))
        assert int((got[2] == 1).sum()) == 2 and int((got[2] == 3).sum()) == 22
    shape = SHAPES[3]
    grid = built.blockmatch_grid(shape, None, spacing=4.0)
    field = forward_field("smooth", grid, seed=1, amp=1.0, wave=25.0)
    field["disp"] = field["disp"].copy()
    field["disp"][1, grid["n"][2] // 2, grid["n"][1] // 2, grid["n"][0] // 2] = np.nan
    images = [{"image": volume("smooth", shape, 1)}, {"image": volume("smooth", shape, 2), "field": field}]
    mask = against_oracle(built, ao, shape, images)
    assert 0 < int((mask == 1).sum()) < mask.size // 2


def test_past_the_workgroup_cap(built, ao):
    """BIG has more bricks than two trips of the launch's workgroups (test_average_cpu.py holds it to the kernel's #defines): the last
    plane is reached by the third trip only, and a change there changes the result"""
    a = volume("smooth", BIG, 5)
    b = (np.float32(0.5) * np.roll(a, 2, 1) + np.float32(7.0)).astype(np.float32)
    b[-1, -1, -40:] = np.nan
    images = [{"image": a}, {"image": b, "t": matrix_of_map(map_of("half", BIG, BIG))}]
    planes = warped_planes(built, ao, BIG, images)
    got = built.average_warped(BIG, images, trim=1)
    same_planes(got, ao.average(planes, 1))
    a2 = a.copy()
    a2[-1, -1, -100:-50] += 300.0
    images[0] = {"image": a2}
    planes[0] = a2                        # the identity map returns the image
    got2 = built.average_warped(BIG, images, trim=0)
    same_planes(got2, ao.average(planes, 0))
    assert not np.array_equal(got[0][-1, -1], got2[0][-1, -1])


# ---- poisoned allocations, state between calls ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("byte", [0xA7, 0x00])
def test_under_poisoned_allocations(built, ao, byte):
    """every device block of the call holds the byte before the call uses it: an output word or a descriptor field that the call does not
    write itself would show.  The blocks: three planes, the descriptors, one per image and one per field"""
    shape = SHAPES[3]
    images = group(built, shape, 5, "mixed", seed=21)
    planes = warped_planes(built, ao, shape, images)
    n_fields = sum("field" in a for a in images)
    assert 0 < n_fields < 5
    with built.alloc_fill(byte) as stats:
        for trim, min_count in ((0, 1), (15, 2)):
            got = built.average_warped(shape, images, trim=trim, min_count=min_count, fill=3.0)
            n_blocks, nbytes = stats()
            assert n_blocks == 4 + 5 + n_fields and nbytes >= 12 * int(np.prod(shape)) + 4 * sum(a["image"].size for a in images), (n_blocks, nbytes)
            same_planes(got, ao.average(planes, trim, min_count, 3.0))


def test_second_call_equals_its_oracle(built, ao):
    """two calls in one process with other shapes, K and trims: nothing of the first is left in the second"""
    against_oracle(built, ao, SHAPES[3], group(built, SHAPES[3], 32, "mixed", seed=30), trims=(15,))
    against_oracle(built, ao, SHAPES[2], group(built, SHAPES[2], 2, "none", seed=31), trims=(0,))
    against_oracle(built, ao, SHAPES[1], group(built, SHAPES[1], 5, "all", seed=32), trims=(1,))


# ---- the report ---------------------------------------------------------------------------------------------------------------------------------
def test_report_equals_the_oracle(built, ao):
    shape = SHAPES[3]
    images = group(built, shape, 5, "mixed", seed=40)
    avg, var, mask, rep = built.average_warped(shape, images, trim=1, min_count=3)
    want = ao.counts(mask, 5, 3)
    assert (rep["images"], rep["trim"], rep["min_count"], rep["voxels"]) == (5, 1, 3, mask.size)
    assert (rep["none"], rep["below"], rep["count"]) == (want["none"], want["below"], want["count"]) and [i["contributing"] for i in rep["image"]] == want["contributing"]
    assert rep["kernel_ms"] > 0 and rep["wall_ms"] >= rep["kernel_ms"] and all(i["upload_ms"] > 0 for i in rep["image"])
    assert int(np.isnan(avg).sum()) == want["below"] > want["none"] > 0
    text = built.average_report_text(rep).split("\n")
    assert text[0] == "# images 5 trim 1 min_count 3" and text[1] == "# voxels %d none %d below %d" % (mask.size, want["none"], want["below"])


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals(built):
    """all on the host, before anything is allocated: the extents below are never backed by memory"""
    import ctypes as C
    L = built.hip_lib()
    tiny = np.arange(8, dtype=np.float32)
    out = np.zeros(8, np.float32), np.zeros(8, np.float32), np.zeros(8, np.uint32)
    singular = np.zeros(16, np.float32)
    singular[15] = 1
    nan_entry = np.eye(4, dtype=np.float32).reshape(16)
    nan_entry[6] = np.nan
    disp = np.zeros(24, np.float32)

    def field(n=(2, 2, 2), spacing=4.0, capacity=24):
        f = built.Field()
        f.n[:] = n
        f.spacing, f.capacity, f.disp = spacing, capacity, disp.ctypes.data
        return f

    def call(grid=(2, 2, 2), K=1, src=(2, 2, 2), image=True, t=None, vox2key=None, gv=None, fld=None, at=0, avg=True, **params):
        arr = (built.AverageImage * 33)()
        for k in range(min(max(K, 1), 33)):
            arr[k].image, (arr[k].nx, arr[k].ny, arr[k].nz) = tiny.ctypes.data, (2, 2, 2)
        a = arr[at]
        a.image, (a.nx, a.ny, a.nz) = (tiny.ctypes.data if image else None), src
        a.moving_to_fixed = None if t is None else t.ctypes.data
        a.vox2key = None if vox2key is None else vox2key.ctypes.data
        a.field = None if fld is None else C.addressof(fld)
        err, p = C.create_string_buffer(512), built.average_params(**params)
        rc = L.sift3d_average_warped(*grid, None if gv is None else gv.ctypes.data, K, arr, C.byref(p), out[0].ctypes.data if avg else None, out[1].ctypes.data,
                                     out[2].ctypes.data, None, err, len(err))
        return rc, err.value.decode()

    with built.alloc_fill(0x5A) as stats:
        for kw, text in (({"K": 0}, "K = 0 images: 1 .. 32"), ({"K": 33}, "K = 33 images: 1 .. 32"), ({"avg": False}, "null pointer"),
                         ({"grid": (0, 2, 2)}, "grid: nx ny nz = 0 2 2: extents must be 1 .. 2^24"), ({"grid": (2, 2, (1 << 24) + 1)}, "grid: nx ny nz = 2 2 16777217: extents must be 1 .. 2^24"),
                         ({"grid": (1 << 24, 1 << 24, 2)}, "grid: more than 2^40 voxels"), ({"trim": 16}, "trim = 16: 0 .. 15"), ({"trim": -1}, "trim = -1: 0 .. 15"),
                         ({"min_count": 0}, "min_count = 0: 1 .. K = 1"), ({"K": 3, "min_count": 4}, "min_count = 4: 1 .. K = 3"), ({"form": 1}, "form = 1: -1 or 0"),
                         ({"max_voxels": 0}, "max_voxels = 0: at least 1"), ({"K": 3, "at": 2, "image": False}, "image 2: null pointer"),
                         ({"K": 3, "at": 1, "src": (2, 0, 2)}, "image 1: source extents must be 1 .. 2^24"), ({"src": ((1 << 24) + 1, 2, 2)}, "image 0: source extents must be 1 .. 2^24"),
                         ({"src": (1 << 24, 1 << 24, 2)}, "image 0: volume larger than 2^38 voxels"), ({"K": 2, "at": 1, "t": singular}, "image 1: a matrix's last row is not 0 0 0 1, or a matrix is singular"),
                         ({"t": nan_entry}, "image 0: a matrix's last row is not 0 0 0 1, or a matrix is singular"), ({"vox2key": singular}, "image 0: a matrix's last row"),
                         ({"gv": singular}, "image 0: a matrix's last row"), ({"K": 2, "at": 1, "fld": field(n=(1, 2, 2))}, "image 1: the field needs 2 .. 2^24 nodes per axis"),
                         ({"fld": field(spacing=0.0)}, "image 0: the field's spacing must be positive and finite"), ({"fld": field(capacity=23)}, "image 0: the field's disp holds fewer than 3 n0 n1 n2 floats"),
                         ({"K": 3, "max_voxels": 20}, "image 2: the source voxels up to it, 24, exceed max_voxels = 20")):
            rc, err = call(**kw)
            assert rc == -1 and text in err, (kw, rc, err)
        with pytest.raises(built.Sift3DError, match=re.escape("min_count = 2: 1 .. K = 1")) as e:
            built.average_warped((2, 2, 2), [{"image": tiny.reshape(2, 2, 2)}], min_count=2)
        assert e.value.code == -1
        assert stats()[0] == 0          # nothing was allocated by any of them
        rc, err = call(K=3, max_voxels=24)
        assert rc == 0 and err == "" and stats()[0] == 7


# ---- featAverage --------------------------------------------------------------------------------------------------------------------------------
def test_feataverage_end_to_end(built, ao, tmp_path):
    """on NIfTI files the test writes: <out>, <out>.sd.nii, <out>.count.nii and <out>.average.txt are the bytes the stage implies, with
    -m median, -t1 and -k3, "-" for the transform and for the field, and -u with the mean field through the shared writer"""
    assert os.path.exists(built.FEATAVERAGE)
    shape, key = SHAPES[3], built.key_vox2key()
    grid = built.blockmatch_grid(shape, key, spacing=4.0)
    images, args_fields, args_plain = [], [], []
    for k in range(4):
        v = (volume("smooth", shape, 50 + k) + np.float32(20.0 * k)).astype(np.float32)
        built.write_nifti(str(tmp_path / ("i%d.nii" % k)), v)
        t = np.eye(4, dtype=np.float32)
        t[:3, 3] = [0.5 * k, -1.0 * k, 0.25 * k]
        assert built.host_lib().sift3d_write_matrix(os.fsencode(str(tmp_path / ("i%d.trans.txt" % k))), t.ctypes.data) == 0
        t = built.read_similarity(str(tmp_path / ("i%d.trans.txt" % k)))
        field = forward_field("smooth", grid, seed=60 + k, amp=1.0, wave=25.0)
        built.write_field(str(tmp_path / ("i%d.field.nii" % k)), field)
        field = built.read_field(str(tmp_path / ("i%d.field.nii" % k)))
        images.append({"image": v, "t": t, "vox2key": key, "field": field})
        args_fields += ["i%d.nii" % k, "i%d.trans.txt" % k, "i%d.field.nii" % k]
        args_plain += ["i%d.nii" % k, "i%d.trans.txt" % k if k % 2 else "-", "-" if k % 2 else "i%d.field.nii" % k]
    plain = [{"image": a["image"], "vox2key": key, "t": a["t"] if k % 2 else None, "field": None if k % 2 else a["field"]} for k, a in enumerate(images)]

    def check(stem, group_, trim, min_count, fill):
        avg, var, mask, rep = built.average_warped(shape, group_, key, trim=trim, min_count=min_count, fill=fill)
        same_planes((avg, var, mask), cpu_average(built, ao, shape, group_, key, trim, min_count, fill))
        count = np.array([bin(int(m)).count("1") for m in mask.reshape(-1)], np.float32).reshape(shape)
        with np.errstate(invalid="ignore"):
            sd = np.where(count < min_count, var, np.sqrt(var)).astype(np.float32)
        for name, want in ((stem, avg), (stem + ".sd.nii", sd), (stem + ".count.nii", count)):
            got = built.read_nifti(str(tmp_path / name))
            got = got[0] if isinstance(got, tuple) else got
            assert np.array_equal(bits32(np.asarray(got, np.float32)), bits32(want)), name
        strip = lambda text: [l for l in text.split("\n") if not re.match(r"^\d+\.\d{3} \d+\.\d{3}$", l) and not re.match(r"^\d+ \d+ \d+\.\d{3}$", l)]
        report = open(str(tmp_path / (stem + ".average.txt"))).read()
        assert report.startswith("# featAverage v1.0\n# images 4 trim %d min_count %d\n" % (trim, min_count))
        assert strip(report)[1:] == strip(built.average_report_text(rep))
        assert [l.split()[:2] for l in report.split("\n")[4:8]] == [[str(k + 1), str(i["contributing"])] for k, i in enumerate(rep["image"])]
        return mask

    run(["timeout", "-k", "10", "120", built.FEATAVERAGE, "-d0", "-mmedian", "-k3", "i0.nii", "med.nii"] + args_plain, tmp_path)
    mask = check("med.nii", plain, 15, 3, np.nan)
    assert 0 < int((mask == 15).sum()) < mask.size
    assert not os.path.exists(str(tmp_path / "med.nii.mean.field.nii"))
    run(["timeout", "-k", "10", "120", built.FEATAVERAGE, "-t1", "-f-5", "-u", "i0.nii", "trim.nii"] + args_fields, tmp_path)
    check("trim.nii", images, 1, 1, -5.0)
    mean = built.mean_field([a["field"] for a in images])
    got = built.read_field(str(tmp_path / "trim.nii.mean.field.nii"))
    assert got["n"] == mean["n"] and np.array_equal(bits32(got["disp"]), bits32(mean["disp"])) and np.array_equal(bits32(mean["disp"]), bits32(ao.mean_field([a["field"] for a in images])))
    head = open(str(tmp_path / "trim.nii.mean.field.txt")).read()
    assert head.startswith("# nodes %d %d %d spacing " % tuple(mean["n"])) and head.endswith(" mean of 4 fields\n")
    run(["timeout", "-k", "10", "120", built.FEATAVERAGE, "i0.nii", "mean.nii"] + args_plain[:3], tmp_path)
    check_one = built.average_warped(shape, plain[:1], key)
    got = built.read_nifti(str(tmp_path / "mean.nii"))
    got = got[0] if isinstance(got, tuple) else got
    assert np.array_equal(bits32(np.asarray(got, np.float32)), bits32(check_one[0]))
