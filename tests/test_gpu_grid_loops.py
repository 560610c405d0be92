"""GPU suite: every grid-capped kernel past one grid of workgroups.  The kernels of the warp family and of the
label fusion launch at most BRICK_MAX_GRID (2^22) or NODE_MAX_GRID (2^20) workgroups and walk the rest of their bricks in a loop,
`for (L = ...; L < nbricks; L += gridDim.x)`.  A brick counts whether or not it is full, so thin shapes (tests/grid_loop_cases.py;
test_grid_loops_cpu.py holds each of them to exceed its cap by 32 bricks) send 32 workgroups round the loop a second time at a
size the CPU oracles check whole, or on bands that hold every second-round brick.  Every comparison is bit for bit against the
kernel's own oracle, as in the kernel's own test file.  At the other end of the documented range: a source of 2^24 voxels along an
axis."""
import numpy as np
import pytest

import grid_loop_cases as gl
from compose_cases import OUTSIDE1, OUTSIDE2, ComposeOracle, written
from field_cases import FieldOracle
from fuse_search_cases import NO_SHIFT, FuseSearchOracle, block_labels
from grid_loop_cases import EXCESS, NODE_GRID, RESAMPLE_SHAPES, THIN_SHAPE
from invert_cases import CONVERGED, DIVERGED, NOT_CONVERGED, InvertOracle, box_grid, forward_field, oblique, state, written_inverse
from resample_cases import ResampleOracle
from test_gpu_compose import check_compose
from test_gpu_fuse_search import same_search
from test_gpu_invert import check_invert

pytestmark = pytest.mark.gpu

FILL = -7.0


@pytest.fixture(scope="module")
def K():
    return gl.header_constants()


@pytest.fixture(scope="module")
def rorc(tmp_path_factory):
    return ResampleOracle(tmp_path_factory.mktemp("resample_oracle"))


@pytest.fixture(scope="module")
def fo(tmp_path_factory):
    return FieldOracle(tmp_path_factory.mktemp("field_oracle"))


@pytest.fixture(scope="module")
def io(tmp_path_factory):
    return InvertOracle(tmp_path_factory.mktemp("invert_oracle"))


@pytest.fixture(scope="module")
def co(tmp_path_factory):
    return ComposeOracle(tmp_path_factory.mktemp("compose_oracle"))


@pytest.fixture(scope="module")
def fs(tmp_path_factory):
    return FuseSearchOracle(tmp_path_factory.mktemp("fuse_search_oracle"))


def same_bits(got, want, shape=None, K=None):
    """test_gpu_resample._same without its copies: equal bits wherever the result is a number, NaN where it is NaN.  With the whole
    volume's shape, a failure says how many of the differing voxels lie in second-round bricks."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    differ = got.view(np.uint32) != want.view(np.uint32)
    if differ.any():
        differ &= ~(np.isnan(got) & np.isnan(want))
    bad = np.flatnonzero(differ.reshape(-1))
    if bad.size:
        where = ""
        if shape is not None and tuple(shape) == got.shape:
            where = ", %d of them in second-round bricks" % int((differ & gl.second_round_mask(shape, gl.brick_launch_of(shape, K), K)).sum())
        raise AssertionError("%d voxels differ%s, first at %r: %r vs %r" % (bad.size, where, np.unravel_index(bad[:4], got.shape), got.reshape(-1)[bad[:4]],
                                                                         want.reshape(-1)[bad[:4]]))


def both_shares(want, fill=FILL):
    """a good share of the output inside the source, a good share the fill, and the last voxels (second-round bricks) not fill alone"""
    filled = float((want == np.float32(fill)).mean())
    at_end = float((want.reshape(-1)[-256:] == np.float32(fill)).mean())
    print("fill at %.1f %% of the output, at %.1f %% of its last 256 voxels" % (100 * filled, 100 * at_end))
    assert 0.1 < filled < 0.9 and at_end < 0.7, (filled, at_end)


# ---- resample_kernel ------------------------------------------------------------------------------------------------------------------
def resample_case(name):
    shape = RESAMPLE_SHAPES[name]
    vol = gl.thin_source(shape)
    return vol, shape, gl.thin_map(vol.shape, shape)


@pytest.mark.parametrize("mode", ["linear", "nearest"])
@pytest.mark.parametrize("name", sorted(RESAMPLE_SHAPES))
def test_resample_kernel_past_the_cap(built, rorc, K, name, mode):
    """2^22 + 32 bricks along z (vector and scalar stores), y and x in turn; a source with NaN and infinities; the output's first
    third takes the fill and its end, the second-round bricks, lies inside the source.  The long axes pass 2^24, where
    (float)index is inexact: the oracle makes the same conversion."""
    vol, shape, A = resample_case(name)
    want = rorc.resample(vol, shape, A, mode, FILL)
    both_shares(want)
    assert np.isnan(want).any() and np.isinf(want).any()
    same_bits(built.resample_affine(vol, shape, A, mode, FILL), want, shape, K)


def test_resample_dev_past_the_cap_leaves_no_sentinel(built, rorc, K):
    import torch
    vol, shape, A = resample_case("y")
    want = rorc.resample(vol, shape, A, "linear", FILL)
    d_src = torch.from_numpy(vol).cuda()
    d_dst = torch.full(shape, 12345.0, dtype=torch.float32, device="cuda")
    with built.Context(64, 64, 64) as ctx:
        ctx.resample_affine_dev(d_src.data_ptr(), vol.shape, d_dst.data_ptr(), shape, A, "linear", FILL)
        torch.cuda.synchronize()
    got = d_dst.cpu().numpy()
    del d_dst
    assert not (got == 12345.0).any()
    same_bits(got, want, shape, K)


# ---- field_warp_kernel and jacobian_map_kernel ----------------------------------------------------------------------------------------
def thin_warp_case(built):
    """the thin output (two bricks along y), a small source, and a field grid over the last planes' lower y alone: in the
    second-round bricks and before them part of the output takes the field's term and part does not"""
    vol = gl.thin_source(THIN_SHAPE)
    A = gl.thin_map(vol.shape, THIN_SHAPE)
    fv = built.key_vox2key((1.0, 1.0, 1.0))
    Cm, Km = built.field_warp_terms(fv, fv)
    oz = THIN_SHAPE[0]
    key_z = float(Cm[2, 2]) * oz + float(Cm[2, 3])           # the key z of the plane after the last
    n = (2, 2, 300)
    rng = np.random.default_rng(8)
    field = {"n": n, "origin": np.array([-1.0, 2.0, key_z - 700.0], np.float32), "spacing": np.float32(4.0),
             "disp": rng.uniform(-1, 1, (3,) + n[::-1]).astype(np.float32)}
    return vol, A, fv, Cm, Km, field


def inside_field(Cm, field, shape, z0, z1):
    """bool (z1 - z0, oy, ox): the output voxels whose key position lies inside the field's grid (float64: no voxel is near its border)"""
    k, j, i = np.meshgrid(np.arange(z0, z1), np.arange(shape[1]), np.arange(shape[2]), indexing="ij")
    p = np.stack([i, j, k, np.ones_like(i)], -1).astype(np.float64) @ np.asarray(Cm, np.float64).T
    lo = np.asarray(field["origin"], np.float64)
    hi = lo + float(field["spacing"]) * (np.array(field["n"]) - 1)
    return ((p >= lo) & (p <= hi)).all(-1)


@pytest.mark.parametrize("interp", ["linear", "nearest"])
def test_field_warp_kernel_past_the_cap(built, fo, rorc, K, interp):
    vol, A, fv, Cm, Km, field = thin_warp_case(built)
    want = fo.warp(vol, THIN_SHAPE, A, Cm, Km, field, interp, FILL)
    both_shares(want)
    assert np.isnan(want).any() and np.isinf(want).any()
    # the field's term in part of the second-round bricks and not in the rest of them
    last = gl.bands(THIN_SHAPE, gl.brick_launch_of(THIN_SHAPE, K), K)[-1]
    inside = inside_field(Cm, field, THIN_SHAPE, *last)
    plain = rorc.resample(vol, THIN_SHAPE, A, interp, FILL, *last)
    moved = want[last[0]:last[1]].view(np.uint32) != plain.view(np.uint32)
    assert 0.2 < inside.mean() < 0.8 and moved[inside].mean() > 0.2 and not moved[~inside].any()
    assert not inside_field(Cm, field, THIN_SHAPE, 0, 64).any()
    same_bits(built.resample_field(vol, THIN_SHAPE, A, field, fv, fv, interp, FILL), want, THIN_SHAPE, K)


@pytest.mark.parametrize("with_field", [False, True])
def test_jacobian_map_kernel_past_the_cap(built, io, K, with_field):
    """forms 0 and 1 on the thin output (every index below 2^24: the central differences stay differences): each against the oracle
    on the bands (the first 64 planes, 64 in the middle, every plane of the second-round bricks), and against each other whole"""
    vol, A, fv, Cm, Km, field = thin_warp_case(built)
    field = field if with_field else None
    factor = built.jacobian_factor(fv, fv)
    bands = gl.bands(THIN_SHAPE, gl.brick_launch_of(THIN_SHAPE, K), K)
    want = [io.jacobian(THIN_SHAPE, A, Cm, Km, field, factor, z0, z1) for z0, z1 in bands]
    assert all((w != 0).all() for w in want)
    if with_field:
        inside = inside_field(Cm, field, THIN_SHAPE, *bands[-1])
        none = io.jacobian(THIN_SHAPE, A, Cm, Km, None, factor, *bands[-1])
        assert (want[-1][inside] != none[inside]).mean() > 0.5 and (want[-1][~inside] == none[~inside]).mean() > 0.5
        assert len(np.unique(want[-1])) > 100
    got = {}
    for form in (0, 1):
        got[form] = built.jacobian_map(THIN_SHAPE, A, fv, fv, field, form=form)
        for (z0, z1), w in zip(bands, want):
            same_bits(np.ascontiguousarray(got[form][z0:z1]), w)
    same_bits(got[1], got[0], THIN_SHAPE, K)


# ---- fuse_weight_kernel and fuse_search_kernel ----------------------------------------------------------------------------------------
def _tiled(block, shape):
    """block (planes, ny, nx) repeated along z to shape"""
    return np.resize(block, shape)


@pytest.fixture(scope="module")
def thin_pair(fs):
    """T, W, labels and the two ranges on the thin shape, 75.5 M voxels each.  W is a noisy copy of T with another gain and offset (a
    few quantisation steps, so that neither similarity saturates), moved by (tx, ty, tz) = (0, -1, 1).  All are blocks of an odd
    number of planes repeated along z, so their content does not follow the bricks."""
    rng = np.random.default_rng(21)
    nz, ny, nx = THIN_SHAPE
    z, y = np.meshgrid(np.arange(65537), np.arange(ny), indexing="ij")
    base = (300.0 * np.sin(z * 0.05 + y * 0.05) + rng.normal(0, 4.0, z.shape))[..., None].astype(np.float32)
    T = _tiled(base, THIN_SHAPE)
    T += (np.arange(nz, dtype=np.float32) * np.float32(2e-5))[:, None, None]
    noise = rng.normal(0, 4.0, (40961, ny, nx)).astype(np.float32)
    W = np.roll(T, (1, -1), (0, 1))
    W *= np.float32(0.99)
    W += np.float32(4.0)
    W += _tiled(noise, THIN_SHAPE)
    labels = _tiled(block_labels((121, ny, nx), 2), THIN_SHAPE)
    return {"T": T, "W": W, "labels": labels, "rt": fs.range(T), "rw": fs.range(W)}


@pytest.fixture(scope="module")
def thin_quantised(fs, thin_pair):
    """(qT, qW) of the pair per metric, by the oracle's quantiser with the explicit range the kernel is given too"""
    memo = {}

    def get(metric):
        if metric not in memo:
            memo[metric] = fs.quantised(thin_pair["T"], thin_pair["W"], metric, w_range=w_range_of(thin_pair, metric))
        return memo[metric]
    return get


def w_range_of(p, metric):
    return p["rt"] if metric == "ssd" else p["rw"]


def thin_bands(K):
    return gl.bands(THIN_SHAPE, gl.brick_launch_of(THIN_SHAPE, K), K)


@pytest.mark.parametrize("metric", ["ssd", "ncc"])
def test_fuse_weight_kernel_past_the_cap_whole_volume(built, fs, K, thin_pair, thin_quantised, metric):
    """b = 1, the form for any b: the whole volume against the oracle.  And the premise of the banded tests below: a band's
    interior words are the whole volume's words."""
    p = thin_pair
    qt, qw = thin_quantised(metric)
    want = fs.weights_q(qt, qw, 1, metric)
    assert 0 < want.max() <= 32768 and len(np.unique(want[-64:])) > 10
    for band in thin_bands(K):
        (lo, hi), inner = gl.padded(band, 1, THIN_SHAPE[0])
        assert np.array_equal(fs.weights_q(qt[lo:hi], qw[lo:hi], 1, metric)[inner], want[band[0]:band[1]]), band
    got = built.fuse_weights(p["T"], p["W"], block=1, metric=metric, w_range=w_range_of(p, metric), generic=1)
    differ = got != want
    assert not differ.any(), "%d voxels differ, %d of them in second-round bricks" % (
        differ.sum(), (differ & gl.second_round_mask(THIN_SHAPE, gl.brick_launch_of(THIN_SHAPE, K), K)).sum())


@pytest.mark.parametrize("generic", [0, 1])
@pytest.mark.parametrize("metric", ["ssd", "ncc"])
def test_fuse_weight_kernel_past_the_cap_bands(built, fs, K, thin_pair, thin_quantised, metric, generic):
    """b = 2 in both forms, on the bands: the brute force on the quantised planes of a band widened by b"""
    p = thin_pair
    qt, qw = thin_quantised(metric)
    got = built.fuse_weights(p["T"], p["W"], block=2, metric=metric, w_range=w_range_of(p, metric), generic=generic)
    for band in thin_bands(K):
        (lo, hi), inner = gl.padded(band, 2, THIN_SHAPE[0])
        want = fs.weights_q(qt[lo:hi], qw[lo:hi], 2, metric)[inner]
        assert np.array_equal(got[band[0]:band[1]], want), (band, int((got[band[0]:band[1]] != want).sum()))
        assert 0 < want.max() <= 32768 and len(np.unique(want)) > 10


@pytest.mark.parametrize("generic", [0, 1])
@pytest.mark.parametrize("metric", ["ssd", "ncc"])
@pytest.mark.parametrize("b,r", [(1, 1), (2, 1)])
def test_fuse_search_kernel_past_the_cap_bands(built, fs, K, thin_pair, thin_quantised, b, r, metric, generic):
    """with labels, on the bands: the brute force on the planes of a band widened by b + r"""
    p = thin_pair
    qt, qw = thin_quantised(metric)
    got = built.fuse_search(p["T"], p["W"], p["labels"], block=b, radius=r, metric=metric, w_range=w_range_of(p, metric), generic=generic)
    unvoted = 0
    for band in thin_bands(K):
        (lo, hi), inner = gl.padded(band, b + r, THIN_SHAPE[0])
        want = tuple(a[inner] for a in fs.search_q(qt[lo:hi], qw[lo:hi], p["labels"][lo:hi], b, r, metric))
        same_search(tuple(np.ascontiguousarray(a[band[0]:band[1]]) for a in got), want)
        voted = want[1] != NO_SHIFT
        unvoted += int((~voted).sum())
        assert voted.any() and len(np.unique(want[1][voted])) > 1 and len(np.unique(want[0][voted])) > 10
    assert unvoted > 0   # voxels whose every candidate has a label that is not finite


# ---- the node kernels -----------------------------------------------------------------------------------------------------------------
SPACING = 1.0 / 64     # of the node grids: 2 x 2 x 4 194 432 nodes, a line of 65 538 key units
ORIGIN = np.array([-0.3, 0.2, -100.0], np.float32)
M1 = oblique(scale=1.03, deg=20.0, axis=(0.0, 0.0, 1.0), trans=(3.0, -2.0, 1.5))     # rotations about z: the line's image is a line along z
M2 = oblique(scale=0.97, deg=-14.0, axis=(0.0, 0.0, 1.0), trans=(-4.0, 2.5, 6.0))


def line_grid():
    return {"n": NODE_GRID, "origin": ORIGIN.copy(), "spacing": np.float32(SPACING)}


def line_image(built, T, f0, f1, spacing, radius=20.0):
    """a grid (box_grid) over the image under the 4 x 4 T of the part f0 .. f1 (fractions of its length) of the line, and `radius`
    beyond it: a sine field's values fall to 0 over the outermost 10 key units (forward_field)"""
    length = SPACING * (NODE_GRID[2] - 1)
    c = np.array([[ORIGIN[0] + x, ORIGIN[1] + y, ORIGIN[2] + f * length] for x in (0.0, SPACING) for y in (0.0, SPACING) for f in (f0, f1)], np.float64)
    T = np.asarray(T, np.float64)
    img = c @ T[:3, :3].T + T[:3, 3]
    return box_grid(built, img.min(0), img.max(0), spacing, radius=radius)


def sectioned_field(grid, sections, seed):
    """a field on grid made along z of sections (fraction of the nodes, kind): "sine" (smooth, amplitude 0.5), "zero", "rough"
    (white noise of standard deviation 6: no contraction) and "nan" """
    rng = np.random.default_rng(seed)
    n0, n1, n2 = grid["n"]
    d = forward_field("sine", grid, amp=0.5, wave=40.0)["disp"].copy()
    at = 0.0
    for frac, kind in sections:
        a, b = int(round(at * n2)), int(round((at + frac) * n2))
        at += frac
        if kind == "zero":
            d[:, a:b] = 0.0
        elif kind == "rough":
            d[:, a:b] = rng.normal(0, 6.0, d[:, a:b].shape)
        elif kind == "nan":
            d[:, a:b] = np.nan
    return dict(grid, disp=d)


def test_field_invert_kernel_past_the_cap(built, io, tmp_path):
    """2^20 + 32 bricks of nodes.  The forward field covers the last quarter of the line (the second-round bricks among it): smooth,
    then a rough stretch and a stretch of NaN, then smooth to the end: nodes end in all three states."""
    m_inv = written_inverse(built, M1, tmp_path)
    fwd = sectioned_field(line_image(built, M1, 0.75, 1.0, 2.0), [(0.3, "sine"), (0.02, "rough"), (0.01, "nan"), (0.67, "sine")], 5)
    u, st, r2 = check_invert(built, io, M1, m_inv, fwd, line_grid())
    s = state(st)
    counts = [int((s == k).sum()) for k in (CONVERGED, NOT_CONVERGED, DIVERGED)]
    print("converged %d, not converged %d, diverged %d" % tuple(counts))
    assert min(counts) > 0
    tail = slice(-4 * EXCESS, None)                       # the second-round bricks' nodes
    assert (s[tail] == CONVERGED).all() and np.abs(u[:, tail]).max() > 0.1 and np.abs(u[:, :64]).max() < 0.1


def test_field_invert_kernel_past_the_cap_without_a_field(built, io, tmp_path):
    m_inv = written_inverse(built, M1, tmp_path)
    u, st, r2 = check_invert(built, io, M1, m_inv, None, line_grid())
    assert (state(st) == CONVERGED).all() and (u[:, -4 * EXCESS:] != 0).any()


def test_compose_kernels_past_the_cap(built, co, tmp_path):
    """field_compose_kernel over 2^20 + 32 bricks of nodes and compose_residual_kernel over as many bricks of cells.  Field 1 covers
    the line from its half to nine tenths, field 2 the image of its last quarter: every combination of OUTSIDE1 and OUTSIDE2."""
    mr = written(built, built.compose_matrix(M1, M2), tmp_path)
    f1 = forward_field("sine", line_image(built, np.eye(4), 0.5, 0.9, 4.0), amp=1.0, wave=40.0)
    f2 = forward_field("sine", line_image(built, np.linalg.inv(M1.astype(np.float64)), 0.75, 1.0, 4.0), amp=1.0, wave=50.0)
    w, st, r2 = check_compose(built, co, M1, M2, mr, f1, f2, line_grid())
    seen = sorted(int(x) for x in np.unique(st))
    assert seen == [0, OUTSIDE1, OUTSIDE2, OUTSIDE1 | OUTSIDE2], seen
    assert r2.shape == tuple(n - 1 for n in NODE_GRID[::-1]) and (r2[-4 * EXCESS:] > 0).any() and (w[:, -4 * EXCESS:] != 0).any()


def test_field_fit_kernel_past_the_cap(built, fo, K):
    """3 x 3 x (2^22 + 127) nodes from twelve samples along z: 2^20 + 32 bricks, and more than 2^20 sample cells along z at the edge
    R (1 + 2^-10), so the fit widens its cells"""
    y, v = gl.fit_samples()
    h, R, lam = gl.FIT_SPACING, gl.FIT_RADIUS, 0.1
    got = built.fit_field(y, v, spacing=h, radius=R, lam=lam, max_nodes=1 << 26)
    n = gl.fit_grid_rule(y)
    b = gl.node_launch_of(n, K)
    assert got["n"] == n and b["nbricks"] == K["NODE_MAX_GRID"] + EXCESS
    at_r, cells = gl.fit_cells_rule(y)
    assert at_r > 2 ** 20 >= max(cells) - 1
    want = fo.fit(y, v, got, R, lam)
    assert got["n"] == want["n"]
    differ = got["disp"].view(np.uint32) != want["disp"].view(np.uint32)
    assert not differ.any(), "%d values differ, %d of them in second-round bricks" % (differ.sum(), differ[:, K["NODE_BZ"] * b["grid"]:].sum())
    second = want["disp"][:, K["NODE_BZ"] * b["grid"]:]
    assert (second != 0).any() and (want["disp"][:, :64] != 0).any() and not want["disp"][:, 1000:2000].any()


# ---- a source extent of 2^24 ----------------------------------------------------------------------------------------------------------
N24 = 1 << 24


def long_source(axis):
    """a source of 2^24 voxels along axis (0: z, 1: y, 2: x) and 2, 1 along the others"""
    shape = [2, 1]
    shape.insert(axis, N24)
    rng = np.random.default_rng(30 + axis)
    vol = rng.standard_normal(tuple(shape), np.float32)
    vol *= np.float32(100.0)
    ends = [slice(None)] * 3
    ends[axis] = slice(-3, None)
    vol[tuple(ends)] += np.arange(1, 7, dtype=np.float32).reshape(vol[tuple(ends)].shape) * np.float32(1000.0)   # the last voxels: unmistakable
    return vol


def end_positions():
    """the positions along the long axis: n - 1, the float below it, n - 1.5, the float above n - 1 (fill), 0 and -0"""
    top = np.float32(N24 - 1)
    return [top, np.nextafter(top, np.float32(0)), np.float32(N24 - 1.5), np.nextafter(top, np.float32(np.inf)), np.float32(0.0), np.float32(-0.0)]


def end_map(axis, q):
    """zero linear part: every output voxel at the position q along the source's long axis, 0.5 and 0 along the other two"""
    A = np.zeros((3, 4), np.float32)
    other = [a for a in range(3) if a != axis]
    A[2 - axis, 3] = q
    A[2 - other[0], 3] = 0.5
    return A


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_source_extent_2_24(built, rorc, fo, axis):
    vol = long_source(axis)
    assert vol.shape[axis] == N24 and vol.nbytes <= 128 * 2 ** 20
    fv = built.key_vox2key((1.0, 1.0, 1.0))
    Cm, Km = built.field_warp_terms(fv, fv)
    zero = {"n": (2, 2, 2), "origin": np.zeros(3, np.float32), "spacing": np.float32(20.0), "disp": np.zeros((3, 2, 2, 2), np.float32)}
    for q in end_positions():
        A = end_map(axis, q)
        for mode in ("linear", "nearest"):
            want = rorc.resample(vol, (2, 3, 4), A, mode, FILL)
            assert (want == np.float32(FILL)).all() == (q > np.float32(N24 - 1)), (q, mode)
            same_bits(built.resample_affine(vol, (2, 3, 4), A, mode, FILL), want)
            if axis == 2:
                same_bits(built.resample_field(vol, (2, 3, 4), A, zero, fv, fv, mode, FILL), fo.warp(vol, (2, 3, 4), A, Cm, Km, zero, mode, FILL))
    # the last voxel itself, where nothing is interpolated along the long axis
    A = end_map(axis, np.float32(N24 - 1))
    A[2 - [a for a in range(3) if a != axis][0], 3] = 0.0
    last = [0, 0, 0]
    last[axis] = N24 - 1
    assert (built.resample_affine(vol, (1, 1, 1), A, "nearest", FILL) == vol[tuple(last)]).all()


def test_source_extent_beyond_2_24_is_refused(built):
    vol = np.zeros((1, 1, N24 + 1), np.float32)
    A = np.zeros((3, 4), np.float32)
    for v in (vol, vol.reshape(1, N24 + 1, 1), vol.reshape(N24 + 1, 1, 1)):
        with pytest.raises(built.Sift3DError, match="source extents"):
            built.resample_affine(v, (2, 2, 2), A)
