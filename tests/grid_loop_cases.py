"""Shared pieces of the grid-loop tests (test_grid_loops_cpu.py, test_gpu_grid_loops.py): the caps and brick
edges read out of warp_device.h, the launch arithmetic of brick_launch_of, node_launch_of and brick_slot0 restated in Python, and
the thin shapes at which every capped kernel goes round its loop, `for (L = ...; L < nbricks; L += gridDim.x)`, a second time.

The shapes are literals.  They do not follow the header: where a cap is raised or a brick changed, test_grid_loops_cpu.py fails
rather than the GPU tests silently no longer passing the cap."""
import os
import re

import numpy as np

from resample_cases import special_volume

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3d_sift_cuda_amd", "csrc", "warp_device.h")
NAMES = ("BRICK_TX", "BRICK_VX", "BRICK_BX", "BRICK_BY", "BRICK_BZ", "BRICK_MAX_GRID", "NODE_BX", "NODE_BY", "NODE_BZ", "NODE_MAX_GRID")


def header_constants(path=None):
    """{name: int} of NAMES: each `#define NAME value` of the header, the value an integer, a shift or a product of earlier names"""
    path = HEADER if path is None else path
    text = open(path).read()
    out = {}
    for name in NAMES:
        m = re.findall(r"^#define[ \t]+%s[ \t]+(.+?)[ \t]*(?:/\*.*)?$" % name, text, re.M)
        assert len(m) == 1, "%s is defined %d times in %s" % (name, len(m), path)
        expr = re.sub(r"\b(\d+)[uU]?[lL]{0,2}\b", r"\1", m[0])
        expr = re.sub(r"\b[A-Z_]+\b", lambda w: str(out[w.group(0)]), expr)
        assert re.fullmatch(r"[\d\s()*+<]+", expr), (name, m[0])
        out[name] = int(eval(expr, {"__builtins__": {}}))
    return out


def _cdiv(a, b):
    return (a + b - 1) // b


def brick_launch_of(shape, K):
    """brick_launch_of restated for an output or volume of shape (oz, oy, ox): nbx, nby, nbz, nbricks, grid"""
    oz, oy, ox = (int(d) for d in shape)
    nbx, nby, nbz = _cdiv(ox, K["BRICK_BX"]), _cdiv(oy, K["BRICK_BY"]), _cdiv(oz, K["BRICK_BZ"])
    nbricks = nbx * nby * nbz
    return {"nbx": nbx, "nby": nby, "nbz": nbz, "nbricks": nbricks, "grid": min(_cdiv(nbricks, 8) * 8, K["BRICK_MAX_GRID"])}


def node_launch_of(n, K):
    """node_launch_of restated for a grid of n = (n0, n1, n2) nodes (or cells)"""
    nb0, nb1, nb2 = _cdiv(int(n[0]), K["NODE_BX"]), _cdiv(int(n[1]), K["NODE_BY"]), _cdiv(int(n[2]), K["NODE_BZ"])
    nbricks = nb0 * nb1 * nb2
    return {"nb0": nb0, "nb1": nb1, "nb2": nb2, "nbricks": nbricks, "grid": min(nbricks, K["NODE_MAX_GRID"])}


def brick_slot0(b, grid):
    """brick_slot0 restated: block b's first slot at a grid that is a multiple of 8 (b an integer or an integer array)"""
    return (b & 7) * (grid >> 3) + (b >> 3)


def trips(first, nbricks, grid):
    """how often a block whose first slot is `first` goes round `for (L = first; L < nbricks; L += grid)`"""
    return np.maximum((nbricks - np.asarray(first, np.int64) + grid - 1) // grid, 0)


def visited(firsts, nbricks, grid, max_trips=None):
    """the slots the blocks visit, in block order, one at a time: for small launches only.  max_trips = 1 is the loop that stops
    after its first trip, `L < min(nbricks, grid)`."""
    out = []
    for first in firsts:
        L, t = int(first), 0
        while L < nbricks and (max_trips is None or t < max_trips):
            out.append(L)
            L += grid
            t += 1
    return out


def second_round(launch):
    """the slots no block reaches on its first trip: grid .. nbricks - 1 (brick_slot0 is a permutation of 0 .. grid - 1)"""
    return range(launch["grid"], launch["nbricks"])


def brick_voxels(L, shape, launch, K):
    """the (z, y, x) slices of brick slot L inside a volume of shape (oz, oy, ox): brick_origin restated, x fastest, z slowest"""
    bx, t = L % launch["nbx"], L // launch["nbx"]
    by, bz = t % launch["nby"], t // launch["nby"]
    lo = (bz * K["BRICK_BZ"], by * K["BRICK_BY"], bx * K["BRICK_BX"])
    edge = (K["BRICK_BZ"], K["BRICK_BY"], K["BRICK_BX"])
    return tuple(slice(lo[a], min(lo[a] + edge[a], shape[a])) for a in range(3))


def second_round_mask(shape, launch, K):
    """bool array of shape: the voxels of the second-round bricks"""
    m = np.zeros(shape, bool)
    for L in second_round(launch):
        m[brick_voxels(L, shape, launch, K)] = True
    return m


# ---- the shapes ---------------------------------------------------------------------------------------------------------------------
EXCESS = 32                # bricks beyond the cap, in every shape: several workgroups go round a second time
BRICK_CAP, NODE_CAP = 1 << 22, 1 << 20   # what the shapes were chosen for; test_grid_loops_cpu.py holds the header to them

# (oz, oy, ox) of the resampler's outputs: the long axis along z (rows of one float4, and of three voxels: the scalar store), y and x
# exercise L / nby, L / nbx % nby and L % nbx in turn
RESAMPLE_SHAPES = {"z, float4 rows": (4 * (BRICK_CAP + EXCESS), 1, 4),
                   "z, rows of three": (4 * (BRICK_CAP + EXCESS), 1, 3),
                   "y": (1, 8 * (BRICK_CAP + EXCESS), 1),
                   "x": (1, 1, 32 * (BRICK_CAP + EXCESS))}
# long along z with two bricks along y: field_warp_kernel, jacobian_map_kernel (every index below 2^24: the central differences stay
# differences), and the fusion kernels, whose extents stop at 2^24
THIN_SHAPE = (4 * (BRICK_CAP // 2 + EXCESS // 2), 9, 1)
BRICK_SHAPES = dict(RESAMPLE_SHAPES, thin=THIN_SHAPE)

# (n0, n1, n2) nodes: field_invert_kernel and field_compose_kernel on 2 x 2 x n2; compose_residual_kernel on the n - 1 cells per axis
# of that grid; field_fit_kernel on the 3 x 3 x n2 grid its samples give (fit_samples)
NODE_GRID = (2, 2, 4 * (NODE_CAP + EXCESS))
CELL_GRID = tuple(n - 1 for n in NODE_GRID)
FIT_SPACING, FIT_RADIUS = 1.0, 0.75
FIT_Z = (-float(1 << 21), float((1 << 21) + 4 * (EXCESS - 1)))   # the first and the last sample's z: both exact in float32
NODE_SHAPES = {"nodes": NODE_GRID, "cells": CELL_GRID}   # the fit's grid is added by fit_grid_rule, from the samples


def fit_grid_rule(y, h=FIT_SPACING, R=FIT_RADIUS):
    """the grid rule restated: n = floor((max - min + 2R) / h) + 2 per axis"""
    y = np.asarray(y, np.float32).astype(np.float64).reshape(-1, 3)
    return tuple(int(np.floor((y[:, k].max() - y[:, k].min() + 2.0 * R) / h)) + 2 for k in range(3))


def fit_cells_rule(y, R=FIT_RADIUS):
    """(cells along the longest axis at the edge R (1 + 2^-10), the sample cells per axis the fit then takes): the rule of
    fit_on_grid restated: the edge is widened until an axis has at most 2^20 cells (and one more: floor(...) + 1) and the grid
    at most 2^24"""
    y = np.asarray(y, np.float32).astype(np.float64).reshape(-1, 3)
    ext = y.max(0) - y.min(0)
    edge0 = R * (1.0 + 1.0 / 1024.0)
    edge = max(edge0, ext.max() / float(1 << 20))
    while True:
        cn = [int(np.floor(e / edge)) + 1 for e in ext]
        if float(cn[0]) * cn[1] * cn[2] <= float(1 << 24):
            break
        edge *= 2
    return int(np.floor(ext.max() / edge0)) + 1, tuple(cn)


def fit_samples():
    """(y, v) float32, 12 x 3: ten samples strung along z from FIT_Z[0] to FIT_Z[1] at x = y = 0, so that the grid rule gives
    3 x 3 x n2 nodes with more than NODE_CAP bricks along z, and two more within R of each other and of the node (1, 1, n2 - 6),
    which lies in the last but one brick: the far end of the field is not all zeros"""
    z = np.linspace(FIT_Z[0], FIT_Z[1], 10).astype(np.float32)
    z[0], z[-1] = FIT_Z
    y = np.zeros((12, 3), np.float32)
    y[:10, 2] = z
    n2 = fit_grid_rule(y[:10])[2]
    node = np.float32(np.float32(FIT_Z[0] - FIT_RADIUS) + np.float32(n2 - 6) * np.float32(FIT_SPACING))   # origin + (float)c * h
    y[10] = (0.0, 0.0, node)
    y[11] = (0.0, 0.0, node + np.float32(0.25))
    v = np.random.default_rng(12).uniform(-4, 4, (12, 3)).astype(np.float32)
    return y, v



def thin_source(out_shape, seed=2):
    """a small source for a thin output: special_volume (NaN, infinities, denormals, -0) of 200 voxels along the output's long axes
    and 2 or 3 along the others, so that the line the output draws through it (thin_map) meets a good part of its voxels"""
    return special_volume(tuple(200 if o > 64 else (3 if o > 4 else 2) for o in out_shape), seed)


def thin_map(src_shape, out_shape, first=-0.5, last=0.98):
    """3 x 4 float32, output voxel -> source voxel.  A long axis of the output runs along a diagonal of the source: over its length
    its own source coordinate goes from `first` to `last` times the source's extent (so the output's first third takes the fill,
    and its last voxels -- the second-round bricks -- lie inside the source) and the two other coordinates span 0.8 and -0.6 of
    theirs about the centre; a short axis spans 0.8 of the source's extent about the centre."""
    src, out = src_shape[::-1], out_shape[::-1]   # x, y, z
    A = np.zeros((3, 4))
    A[:, 3] = [(n - 1) / 2.0 for n in src]
    for c in range(3):
        if out[c] > 64:
            for r in range(3):
                span = (last - first, 0.8, -0.6)[(r - c) % 3] * (src[r] - 1)
                A[r, c] = span / (out[c] - 1)
                A[r, 3] += (first * (src[r] - 1) - (src[r] - 1) / 2.0) if r == c else -span / 2.0
        elif out[c] > 1:
            A[c, c] = 0.8 * (src[c] - 1) / (out[c] - 1)
            A[c, 3] -= 0.4 * (src[c] - 1)
        else:
            A[c, c] = 0.4   # no output voxel sees it; the map's Jacobian determinant is not 0
    return A.astype(np.float32)


# ---- bands of a volume that is long along z ---------------------------------------------------------------------------------------
def bands(shape, launch, K, width=64):
    """[(z0, z1)] the planes a banded comparison must contain: the first `width`, `width` around the middle, and every plane of every
    second-round brick (the bricks are numbered z slowest, so these are the last ones), at least `width` of them"""
    nz = shape[0]
    last = _cdiv(launch["nbricks"] - launch["grid"], launch["nbx"] * launch["nby"]) * K["BRICK_BZ"]
    return [(0, width), (nz // 2 - width // 2, nz // 2 + width // 2), (nz - max(width, last), nz)]


def padded(band, pad, nz):
    """(the band widened by pad planes on the sides that are not the volume's own ends, the band's place inside it)"""
    z0, z1 = band
    lo, hi = max(z0 - pad, 0), min(z1 + pad, nz)
    return (lo, hi), slice(z0 - lo, z1 - lo)
