"""GPU suite: the box walk of descriptor_kernel<true> (3d_sift_cuda_amd/csrc/desc_bins.h) against the oracle's o3_describe_level,
on planted levels built like those of tests/keypoint_cases.py whose images make the 64 bins go wrong if the walk is wrong:

  ramp      a linear ramp: every one of the 729 interior voxels of a patch has the same gradient, so ONE octant holds them all and
            each of its eight bins sums its whole 5^3 box (the other 56 lanes add 125 times +0)
  blocks    a checkerboard of 3-voxel cubes sampled at 0.4 voxels: plateaus of exactly zero gradient (octant 8, no contribution)
            between ramps, so most voxels of a box take no part
  planes    an image that is zero except on the voxel planes through the keypoints, sampled at one voxel or more: the patch
            varies across its centre planes x, y, z = 5 only -- the voxels whose weight is 0.5 for both spatial bins of an axis

and one level in descriptor modes 0..3, since the normalisation and the ranking behind the bins are shared with the BRIEF family.
Bar: that of tests/test_gpu_keypoint_stage.py (whose helpers run the stage) -- the records are the oracle's byte for byte.  The
eigenvalue test is switched off (threshold -1) where the image is degenerate by construction, so that the records exist.
"""
import numpy as np
import pytest

import keypoint_cases as kc
from test_gpu_keypoint_stage import compare_records, groups_of, run, want

pytestmark = pytest.mark.gpu
F = np.float32


def grid(shape):
    nx, ny, nz = shape
    return np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")


def plant_lattice(lv, margin, step):
    nx, ny, nz = lv.shape
    pts = [(x, y, z) for z in kc.lattice(margin, nz - 1 - margin, step) for y in kc.lattice(margin, ny - 1 - margin, step)
           for x in kc.lattice(margin, nx - 1 - margin, step)]
    for i, p in enumerate(pts):
        lv.plant(p, i % 2)
    return lv


def ramp_level(shape, seed):
    rng = np.random.default_rng(seed)
    z, y, x = grid(shape)
    s = rng.choice([-1.0, 1.0], 3)
    img = (s[0] * 1.0 * x + s[1] * 0.7 * y + s[2] * 0.45 * z).astype(F)
    return plant_lattice(kc.Level("bins_ramp_%dx%dx%d" % shape, shape, kc.sigmas(0.5), rng, img=img), 6, 5)


def blocks_level(shape, seed):
    rng = np.random.default_rng(seed)
    z, y, x = grid(shape)
    img = ((x // 3 + y // 3 + z // 3) % 2).astype(F)
    return plant_lattice(kc.Level("bins_blocks_%dx%dx%d" % shape, shape, kc.sigmas(0.5), rng, img=img), 6, 5)


def planes_level(shape, seed):
    """Scale 2 * 1.27 * 1.0268 = 2.6 (h == l puts the vertex midway), samples 1.04 voxels apart, offset 0: the un-reoriented patch
    of a keypoint reads the planes through it with its centre planes alone.  The planes of different keypoints are 13 voxels
    apart, beyond the 5.2 + 1 a patch reaches along an axis."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    xs, ys, zs = (9, 22, 35), (9, 22), (9, 22)
    assert xs[2] + 9 <= nx - 1 and ys[1] + 9 <= ny - 1 and zs[1] + 9 <= nz - 1
    img = np.zeros((nz, ny, nx), F)
    for v in xs:
        img[:, :, v] += F(1.0)
    for v in ys:
        img[:, v, :] += F(0.75)
    for v in zs:
        img[v, :, :] += F(0.5)
    lv = kc.Level("bins_planes_%dx%dx%d" % shape, shape, kc.sigmas(1.27), rng, img=img)
    for i, p in enumerate([(x, y, z) for z in zs for y in ys for x in xs]):
        lv.plant(p, i % 2, axes=[0.5] * 6, h=0.6, l=0.6)
    return lv


BUILDERS = {"ramp": ramp_level, "blocks": blocks_level, "planes": planes_level}
_LEVELS = {}


def level(kind, shape):
    if (kind, shape) not in _LEVELS:
        _LEVELS[(kind, shape)] = BUILDERS[kind](shape, 900 + 10 * sorted(BUILDERS).index(kind) + kc.SHAPES.index(shape))
    return _LEVELS[(kind, shape)]


@pytest.mark.parametrize("shape", kc.SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("kind", sorted(BUILDERS))
def test_bins_on_planted_images(built, oracle, kind, shape):
    lv = level(kind, shape)
    w, dg = want(oracle, lv, -1.0)
    assert len(w) >= (12 if kind == "planes" else 100) and (w["info"] & 0x20).any() and not (w["info"] & 0x20).all()
    _, recs, grp = run(built, [(lv, 1, 1.0, None)], eig=-1.0, candidates=False)
    compare_records(recs, w)
    assert (grp == groups_of(lv, dg, 1)).all()


def test_bins_in_every_descriptor_mode(built, oracle):
    lv = level("blocks", kc.SHAPES[1])
    for mode in (0, 1, 2, 3):
        w, dg = want(oracle, lv, -1.0, mode)
        _, recs, grp = run(built, [(lv, 0, 1.0, None)], mode=mode, eig=-1.0, candidates=False)
        compare_records(recs, w)
        assert (grp == groups_of(lv, dg, 0)).all()
