"""The oracle's pyramid level by level, and the volumes tests/test_gpu_pyramid_levels.py runs through the pipeline.

oracle_pyramid chains oracle.blur, oracle.octave_levels and oracle.subsample exactly as run_pyramid in oracle/sift3d_oracle.c
does; tests/test_pyramid_cpu.py ties it to oracle.candidates, which the rest of the suite trusts.  All volumes are
(nz, ny, nx) float32; shapes are given as (nx, ny, nz), as everywhere in the suite.
"""
import numpy as np

TINY_VOX = 4096   # SIFT3D_TINY_VOX: an octave of at most this many voxels is built by one workgroup


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def initial_sigma(init_scale):
    """run_pyramid's first blur, float32 arithmetic as there: sqrtf(1.6f * 1.6f - (0.5f / init_scale)^2)"""
    f = np.float32
    si = f(0.5)
    if init_scale > 0:
        si = f(si / f(init_scale))
    s = f(1.6)
    return float(np.sqrt(f(f(s * s) - f(si * si)), dtype=np.float32))


def octave_shapes(dims):
    """(nx, ny, nz) of every octave: halve while every dimension stays above 2"""
    x, y, z = dims
    out = []
    while x > 2 and y > 2 and z > 2:
        out.append((x, y, z))
        x, y, z = x // 2, y // 2, z // 2
    return out


def tiny_octaves(dims):
    """how many octaves of the shape hold at most TINY_VOX voxels"""
    return sum(1 for x, y, z in octave_shapes(dims) if x * y * z <= TINY_VOX)


def oracle_pyramid(oracle, vol, init_scale=1.0):
    """[(G, D)] per octave: G[0..5] the Gaussian levels, D[0..4] the DoG levels D_k = G_k - G_{k+1}."""
    vol = np.ascontiguousarray(vol, np.float32)
    g0 = oracle.blur(vol, initial_sigma(init_scale))
    out = []
    while min(g0.shape) > 2:
        G, D = oracle.octave_levels(g0)
        out.append((G, D))
        g0 = oracle.subsample(G[3])
    return out


def blobs_offset(pkg, dims, seed, offset=0.0):
    """pkg.synth_blobs plus a constant: with a large one, what a run leaves in pad columns and buffer tails is far from zero"""
    return pkg.synth_blobs(*dims, seed=seed) + np.float32(offset)


def signed_blobs(dims, seed, count=40):
    """Gaussian blobs of both signs with sigmas from 0.7 voxels to a third of the shortest side, on a small linear ramp: every
    octave down to the last has structure of its own scale, so a wrong tap, row or level shows in the coarse volumes."""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    x, y, z = (np.arange(n, dtype=np.float64) for n in dims)
    v = 0.0625 * z[:, None, None] - 0.125 * y[None, :, None] + 0.25 * x[None, None, :]
    smax = max(1.0, min(dims) / 3.0)
    for _ in range(count):
        c = rng.uniform(0.0, 1.0, 3) * (nx - 1, ny - 1, nz - 1)
        s = float(np.exp(rng.uniform(np.log(0.7), np.log(smax))))
        a = float(rng.choice((-1.0, 1.0)) * rng.uniform(50.0, 200.0))
        gx, gy, gz = (np.exp(-(t - ct) ** 2 / (2.0 * s * s)) for t, ct in ((x, c[0]), (y, c[1]), (z, c[2])))
        v = v + a * gz[:, None, None] * gy[None, :, None] * gx[None, None, :]
    return v.astype(np.float32)


def compare_levels(got, want, what=""):
    """got: Context.pyramid(); want: oracle_pyramid.  Returns (lines, missing): one line per stored level that differs from the
    oracle's in any bit (octave, kind, level, count and first position of the differing voxels), and the (octave, kind, level)
    the run did not store.  Every other voxel must have the oracle's bits; a NaN matches only where the oracle has a NaN too
    (sign and payload of a NaN are the one thing x86 and the GPU may encode differently)."""
    lines, missing = [], []
    if len(got) != len(want):
        lines.append("%s: %d octaves read back, the oracle has %d" % (what, len(got), len(want)))
    for o, (g, (G, D)) in enumerate(zip(got, want)):
        for kind, have, ref in (("L", g["L"], G), ("D", g["D"], D)):
            for j in range(5):
                if have[j] is None:
                    missing.append((o, kind, j))
                    continue
                if have[j].shape != ref[j].shape:
                    lines.append("%s octave %d %s_%d: shape %s, the oracle's %s" % (what, o, kind, j, have[j].shape, ref[j].shape))
                    continue
                bad = (bits(have[j]) != bits(ref[j])) & ~(np.isnan(have[j]) & np.isnan(ref[j]))
                if bad.any():
                    zyx = tuple(int(i) for i in np.argwhere(bad)[0])
                    lines.append("%s octave %d %s_%d: %d of %d voxels differ, first at (z, y, x) = %s: %r, the oracle's %r"
                                 % (what, o, kind, j, int(bad.sum()), bad.size, zyx, float(have[j][zyx]), float(ref[j][zyx])))
    return lines, missing
