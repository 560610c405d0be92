"""GPU suite: every branch of the extrema launch plan (3d_sift_cuda_amd/csrc/extrema_plan.h) through sift3d_extrema, held to the
oracle with lists equal in order and in bits.

The shapes are the smallest that reach each branch; they were chosen by running tests/extrema_plan_check.cpp with the list
capacity sift3d_extrema offers (voxels / 64 + 64 * 1024), which names the same forms as listed here (nx x ny x nz):
  march            8 x 514 x 34    one x tile, 32 workgroups of 4 wavefronts in y (128 y tiles), four chunks of 8 planes
                   260 x 258 x 34  a second x tile that holds 4 columns
  plane per block  8 x 3 x 3       one plane, one row, six voxels
                   252 x 6 x 5     two 248-wide tiles, the second holding 2 output columns
                   12 x 10 x 70    68 z blocks on 64 segments: the hashed segment mapping
  strict           8 x 514 x 34 and 12 x 10 x 70 with one NaN and one +inf planted in d_cur (32 and 68 one-plane blocks)
  generic          7 x 5 x 3 (X < 8) and 9 x 9 x 9 (X % 4 != 0)
tests/test_extrema_plan.py holds the plan of each of them on the CPU (its ODD list).

Input: d_cur is seeded noise quantised to 8 levels, so that neighbours tie; d_prev and d_next are the same noise kept at one
voxel in fifty and zero elsewhere, so that the second phase refutes about one own-level extremum in eight and passes the
rest.  Six to twenty-one interior voxels rarely hold both a minimum and a maximum: for the three smallest shapes the seed
is the first for which the oracle finds one of each (searched once with the oracle, on the CPU); the others take seed 0.
"""
import functools

import numpy as np
import pytest

import _oracle

pytestmark = pytest.mark.gpu

# (nx, ny, nz) -> seed
MARCH = {(8, 514, 34): 0, (260, 258, 34): 0}
PLANE = {(8, 3, 3): 1642, (252, 6, 5): 0, (12, 10, 70): 0}
GENERIC = {(7, 5, 3): 2519, (9, 9, 9): 1}
STRICT = {(8, 514, 34): 0, (12, 10, 70): 0}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_lists(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for f in ("x", "y", "z"):
        assert (got[f] == want[f]).all()
    assert (bits(got["value"]) == bits(want["value"])).all()


@functools.lru_cache(maxsize=None)
def case(shape, seed, planted, with_next=True):
    """(d_prev, d_cur, d_next or None, the oracle's minima, maxima): made once, shared, left unchanged."""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    q = lambda: rng.integers(0, 8, (nz, ny, nx)).astype(np.float32)
    sparse = lambda: (q() - 3.5) * (rng.random((nz, ny, nx)) < 0.02).astype(np.float32)
    cur, prev, nxt = q() - 3.5, sparse(), sparse()
    if planted:
        cur[nz // 2, ny // 2, nx // 2] = np.nan
        cur[nz // 2, ny // 2 - 1, nx // 2 - 2] = np.inf
    orc = _oracle.load()
    with np.errstate(all="ignore"):
        omin, omax = orc.detect3(prev, cur, nxt) if with_next else orc.detect(prev, cur)
    for a in (prev, cur, nxt, omin, omax):
        a.setflags(write=False)
    return prev, cur, (nxt if with_next else None), omin, omax


def run(built, shape, seed, planted=False, with_next=True):
    prev, cur, nxt, omin, omax = case(shape, seed, planted, with_next)
    assert len(omin) > 0 and len(omax) > 0, (shape, len(omin), len(omax))
    nx, ny, nz = shape
    with built.Context(nx, ny, nz) as ctx:
        mins, maxs = ctx.extrema(prev, cur, nxt, capacity=cur.size)
    same_lists(mins, omin)
    same_lists(maxs, omax)
    return omin, omax


ids = lambda s: "%dx%dx%d" % s


@pytest.mark.parametrize("shape", sorted(MARCH), ids=ids)
def test_march(built, shape):
    run(built, shape, MARCH[shape])


@pytest.mark.parametrize("shape", sorted(PLANE), ids=ids)
def test_plane_per_block(built, shape):
    run(built, shape, PLANE[shape])


@pytest.mark.parametrize("shape", sorted(STRICT), ids=ids)
def test_strict_with_nan_and_inf(built, shape):
    omin, omax = run(built, shape, STRICT[shape], planted=True)
    nx, ny, nz = shape
    planted = (nx // 2 - 2, ny // 2 - 1, nz // 2)        # the +inf is a maximum; nothing beside the NaN is an extremum
    assert any((m["x"], m["y"], m["z"]) == planted for m in omax)
    for m in list(omin) + list(omax):
        assert max(abs(int(m["x"]) - nx // 2), abs(int(m["y"]) - ny // 2), abs(int(m["z"]) - nz // 2)) > 1


@pytest.mark.parametrize("shape", sorted(GENERIC), ids=ids)
def test_generic(built, shape):
    run(built, shape, GENERIC[shape])


def test_no_level_above(built):
    """d_next = None (the reference's own entry point: 26 + 27 comparisons) on the second march shape; the lists are longer than
    with a level above, so the second phase did refute something there."""
    shape = (260, 258, 34)
    omin, omax = run(built, shape, MARCH[shape], with_next=False)
    _, _, _, omin3, omax3 = case(shape, MARCH[shape], False, True)
    assert len(omin) > len(omin3) and len(omax) > len(omax3)
