"""CPU suite: the premise of test_gpu_grid_loops.py.  The caps and brick edges are read out of warp_device.h,
brick_launch_of, node_launch_of and brick_slot0 are restated (tests/grid_loop_cases.py), and every shape the GPU tests use is held
to exceed its cap by a few bricks: where a cap is raised or a brick changed these tests fail, they do not silently stop covering
the second trip of the loops.  The walk itself -- brick_slot0, then strides of the grid -- is held to visit every slot once."""
import numpy as np
import pytest

import grid_loop_cases as gl
from grid_loop_cases import BRICK_SHAPES, CELL_GRID, EXCESS, NODE_GRID, NODE_SHAPES, RESAMPLE_SHAPES, THIN_SHAPE


@pytest.fixture(scope="module")
def K():
    return gl.header_constants()


def test_header_constants_are_what_the_shapes_were_chosen_for(K):
    assert (K["BRICK_BX"], K["BRICK_BY"], K["BRICK_BZ"]) == (32, 8, 4) and K["BRICK_TX"] * K["BRICK_VX"] == K["BRICK_BX"]
    assert (K["NODE_BX"], K["NODE_BY"], K["NODE_BZ"]) == (8, 8, 4)
    assert K["BRICK_MAX_GRID"] == gl.BRICK_CAP and K["NODE_MAX_GRID"] == gl.NODE_CAP
    assert K["BRICK_MAX_GRID"] % 8 == 0   # brick_slot0 deals grid / 8 slots to each XCD


def test_the_parser_reads_an_edited_header(tmp_path, K):
    """a cap edited upward in a copy of the header is read as edited, and the shapes then no longer pass it"""
    text = open(gl.HEADER).read()
    for name, shapes, launch in (("BRICK_MAX_GRID", BRICK_SHAPES, gl.brick_launch_of), ("NODE_MAX_GRID", NODE_SHAPES, gl.node_launch_of)):
        old = "#define %s (1u << %d)" % (name, K[name].bit_length() - 1)
        assert text.count(old) == 1
        path = tmp_path / (name + ".h")
        path.write_text(text.replace(old, "#define %s (1u << %d)" % (name, K[name].bit_length())))
        K2 = gl.header_constants(str(path))
        assert K2[name] == 2 * K[name]
        for shape in shapes.values():
            b = launch(shape, K2)
            assert b["nbricks"] <= K2[name] and b["grid"] >= b["nbricks"]   # one trip: what the premise tests below refuse


@pytest.mark.parametrize("name", sorted(BRICK_SHAPES))
def test_brick_shapes_pass_the_cap(K, name):
    shape = BRICK_SHAPES[name]
    b = gl.brick_launch_of(shape, K)
    over = b["nbricks"] - K["BRICK_MAX_GRID"]
    print("%s %r: %d bricks, %d beyond BRICK_MAX_GRID" % (name, shape, b["nbricks"], over))
    assert b["grid"] == K["BRICK_MAX_GRID"] and over == EXCESS and 16 <= over <= 400
    assert np.prod([float(d) for d in shape]) * 4 <= 0.6 * 2 ** 30   # the output: no device allocation above about 0.6 GB
    assert max(shape) < 2 ** 31


def test_the_orientations_exercise_each_division(K):
    long_axis = {name: [a for a in "zyx" if gl.brick_launch_of(s, K)["nb" + a] > 1] for name, s in RESAMPLE_SHAPES.items()}
    assert long_axis == {"z, float4 rows": ["z"], "z, rows of three": ["z"], "y": ["y"], "x": ["x"]}
    assert RESAMPLE_SHAPES["z, float4 rows"][2] % K["BRICK_VX"] == 0 and RESAMPLE_SHAPES["z, rows of three"][2] % K["BRICK_VX"] != 0
    assert sum(max(s) > 2 ** 24 for s in RESAMPLE_SHAPES.values()) >= 2   # (float)index is inexact along these
    b = gl.brick_launch_of(THIN_SHAPE, K)
    assert (b["nbx"], b["nby"]) == (1, 2) and max(THIN_SHAPE) + 1 <= 2 ** 24   # the fusion's extents, the Jacobian's exact indices


def test_bands_hold_every_second_round_brick(K):
    b = gl.brick_launch_of(THIN_SHAPE, K)
    first, middle, last = gl.bands(THIN_SHAPE, b, K)
    assert first == (0, 64) and middle[1] - middle[0] == 64 and last[1] == THIN_SHAPE[0] and last[1] - last[0] >= 64
    planes = set()
    for L in gl.second_round(b):
        z = gl.brick_voxels(L, THIN_SHAPE, b, K)[0]
        planes.update(range(z.start, z.stop))
    assert planes and planes <= set(range(*last)) and len(gl.second_round(b)) == EXCESS
    (lo, hi), inner = gl.padded(last, 3, THIN_SHAPE[0])
    assert (lo, hi) == (last[0] - 3, THIN_SHAPE[0]) and inner == slice(3, 3 + last[1] - last[0])
    assert gl.padded(first, 3, THIN_SHAPE[0]) == ((0, 67), slice(0, 64))


@pytest.mark.parametrize("name", sorted(NODE_SHAPES))
def test_node_shapes_pass_the_cap(K, name):
    n = NODE_SHAPES[name]
    b = gl.node_launch_of(n, K)
    over = b["nbricks"] - K["NODE_MAX_GRID"]
    print("%s %r: %d bricks, %d beyond NODE_MAX_GRID" % (name, n, b["nbricks"], over))
    assert b["grid"] == K["NODE_MAX_GRID"] and over == EXCESS and 16 <= over <= 400
    assert max(n) <= 2 ** 24 and int(np.prod(n)) <= 2 ** 26   # the per-axis limit and the default max_nodes
    assert CELL_GRID == tuple(x - 1 for x in NODE_GRID)


def test_fit_samples_pass_the_cap_and_widen_the_sample_cells(K):
    y, v = gl.fit_samples()
    n = gl.fit_grid_rule(y)
    b = gl.node_launch_of(n, K)
    over = b["nbricks"] - K["NODE_MAX_GRID"]
    print("fit %r: %d bricks, %d beyond NODE_MAX_GRID" % (n, b["nbricks"], over))
    assert n[:2] == (3, 3) and b["grid"] == K["NODE_MAX_GRID"] and over == EXCESS
    assert max(n) <= 2 ** 24 and int(np.prod(n)) <= 2 ** 26 and 3 * 4 * int(np.prod(n)) <= 0.6 * 2 ** 30
    at_r, cells = gl.fit_cells_rule(y)
    assert at_r > 2 ** 20 and max(cells) <= 2 ** 20 + 1 and cells[:2] == (1, 1)   # the widened branch of fit_on_grid
    # the two close samples: within R of each other and of the node (1, 1, n2 - 6), in the last but one brick, a second-round one
    o = np.float32(y[:, 2].min() - np.float32(gl.FIT_RADIUS))
    node = np.array([0.25, 0.25, o + np.float32(n[2] - 6) * np.float32(gl.FIT_SPACING)], np.float64)
    assert np.linalg.norm(y[10] - y[11]) < gl.FIT_RADIUS and all(np.linalg.norm(y[k].astype(np.float64) - node) < gl.FIT_RADIUS for k in (10, 11))
    assert (n[2] - 6) // K["NODE_BZ"] == b["nbricks"] - 2 >= b["grid"]
    assert np.isfinite(v).all() and np.abs(v).max() < 128.0


# ---- the walk -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [8, 16, 24, 64, 1000])
def test_brick_walk_small_grids(grid):
    """one slot at a time: every slot 0 .. nbricks - 1 once, at brick counts below, at and beyond the grid"""
    firsts = [gl.brick_slot0(b, grid) for b in range(grid)]
    assert sorted(firsts) == list(range(grid))
    for nbricks in (grid - 7, grid - 1, grid, grid + 1, grid + 16, 3 * grid - 1, 8 * grid + 5):   # the grid is nbricks rounded up to 8, or less
        assert sorted(gl.visited(firsts, nbricks, grid)) == list(range(nbricks)), nbricks
        missed = sorted(set(range(nbricks)) - set(gl.visited(firsts, nbricks, grid, max_trips=1)))
        assert missed == list(range(min(grid, nbricks), nbricks))   # the loop that stops after one trip misses the second round alone


def _walk_arithmetically(firsts, nbricks, grid):
    """every slot 0 .. nbricks - 1 once, without walking: the first slots are 0 .. grid - 1 each once, so the visited slots
    first + t grid (t < trips) are distinct (their residues and quotients mod grid are), all below nbricks, nbricks in number"""
    firsts = np.asarray(firsts, np.int64)
    assert np.array_equal(np.sort(firsts), np.arange(grid))
    t = gl.trips(firsts, nbricks, grid)
    last = firsts + (t - 1) * grid
    assert int(t.sum()) == nbricks and int(last[t > 0].max()) == nbricks - 1 and (last[t > 0] < nbricks).all()
    return t


@pytest.mark.parametrize("excess", [16, EXCESS, 8 * (1 << 22) + 5])
def test_brick_walk_at_the_capped_grid(K, excess):
    grid = K["BRICK_MAX_GRID"]
    firsts = gl.brick_slot0(np.arange(grid, dtype=np.int64), grid)
    t = _walk_arithmetically(firsts, grid + excess, grid)
    assert t.min() == 1 + excess // grid and t.max() == 1 + (excess + grid - 1) // grid
    # who goes round again: the blocks whose first slot is below the excess (mod the grid); up to grid / 8 of them sit on one XCD
    again = np.flatnonzero(t == t.max())
    assert len(again) == (excess % grid or grid) and len(set(again & 7)) == (1 if excess % grid <= grid // 8 else 8)
    assert np.array_equal(np.sort(firsts[again]), np.arange(len(again)))


@pytest.mark.parametrize("excess", [16, EXCESS, 8 * (1 << 20) + 5])
def test_node_walk_at_the_capped_grid(K, excess):
    grid = K["NODE_MAX_GRID"]
    t = _walk_arithmetically(np.arange(grid, dtype=np.int64), grid + excess, grid)
    assert t.min() == 1 + excess // grid and (t == t.max()).sum() == (excess % grid or grid)
    for g in (1, 5, 64):
        for nbricks in (g, g + 1, 3 * g + 2):
            assert sorted(gl.visited(range(min(g, nbricks)), nbricks, g)) == list(range(nbricks))


# ---- the tests can fail -------------------------------------------------------------------------------------------------------------
def test_a_loop_of_one_trip_differs_in_the_second_round_bricks_alone(K, tmp_path):
    """The resampling oracle on the y-long shape, and the same output as a kernel would leave it whose loop stopped after its first
    trip (`L < min(nbricks, grid)`): the bricks no block reached keep the buffer's sentinel.  The comparison the GPU test makes
    differs in exactly the voxels of the second-round bricks."""
    from resample_cases import ResampleOracle
    shape = RESAMPLE_SHAPES["y"]
    b = gl.brick_launch_of(shape, K)
    vol = gl.thin_source(shape)
    A = gl.thin_map(vol.shape, shape)
    want = ResampleOracle(tmp_path).resample(vol, shape, A, "linear", -7.0)
    firsts = gl.brick_slot0(np.arange(b["grid"], dtype=np.int64), b["grid"])
    assert np.array_equal(np.sort(firsts), np.arange(b["grid"]))      # one trip reaches the slots 0 .. grid - 1 and no other
    got = np.full(shape, 12345.0, np.float32)
    reached = ~gl.second_round_mask(shape, b, K)
    got[reached] = want[reached]
    differ = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    assert differ.sum() == EXCESS * K["BRICK_BY"] and np.array_equal(differ, ~reached)
    assert not (want == 12345.0).any()
