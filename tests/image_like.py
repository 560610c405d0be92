"""Seeded volumes that look like the images the extractor is for, rather than like smooth blob fields.

Every generator takes the blob field it starts from (pkg.synth_blobs, bit-identical on every host) or only a shape and a
seed, and is plain numpy from there, so the same bytes come out everywhere.  All volumes are (nz, ny, nx) float32.

Classes:
  quantized      uint8 (0..255) and int16 with a -1024 background, stored as float32: plateaus, step edges, exact ties
  piecewise      nested constant ellipsoids (a Shepp-Logan-like phantom), axis-aligned and oblique step edges, slabs
  hdr            the blob field times 1e6 and times 1e-6, and times 1e-36 (DoG differences in the denormal range)
  nan            NaN outside a sphere or a box, isolated NaN voxels, a NaN slab touching one face
  inf            isolated +-inf voxels, values near FLT_MAX: operator- and candidate-level only (the reference has no defined
                 output past the detection for these: float-to-int conversions of non-finite coordinates)
"""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)


def _grid(shape):
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64),
                          indexing="ij")
    # centred, scaled to [-1, 1] along every axis
    return (2 * z / max(nz - 1, 1) - 1, 2 * y / max(ny - 1, 1) - 1, 2 * x / max(nx - 1, 1) - 1)


def _unit(blobs):
    b = blobs.astype(np.float64)
    lo, hi = b.min(), b.max()
    return (b - lo) / (hi - lo) if hi > lo else np.zeros_like(b)


def quantized_u8(blobs):
    return np.round(255.0 * _unit(blobs)).astype(np.uint8).astype(np.float32)


def quantized_i16(blobs):
    """CT-like: a -1024 background where the blob field is low, integer Hounsfield-like values elsewhere."""
    u = _unit(blobs)
    v = np.where(u < 0.35, -1024.0, np.round(-200.0 + 1400.0 * u))
    return v.astype(np.int16).astype(np.float32)


def phantom(shape, seed=0):
    """Nested constant-intensity ellipsoids (additive, as the Shepp-Logan phantom), rotated about z, on a zero background."""
    rng = np.random.default_rng(seed)
    z, y, x = _grid(shape)
    v = np.zeros(shape, np.float64)
    ell = [(0.0, 0.0, 0.0, 0.69, 0.92, 0.81, 0.0, 100.0), (0.0, -0.0184, 0.0, 0.6624, 0.874, 0.78, 0.0, -80.0),
           (0.22, 0.0, 0.0, 0.11, 0.31, 0.22, -18.0, -20.0), (-0.22, 0.0, 0.0, 0.16, 0.41, 0.28, 18.0, -20.0),
           (0.0, 0.35, -0.15, 0.21, 0.25, 0.41, 0.0, 10.0), (0.0, 0.1, 0.25, 0.046, 0.046, 0.05, 0.0, 10.0),
           (0.0, -0.1, 0.25, 0.046, 0.046, 0.05, 0.0, 10.0), (-0.08, -0.605, 0.0, 0.046, 0.023, 0.05, 0.0, 10.0)]
    for (cx, cy, cz, ax, ay, az, deg, val) in ell:
        t = np.deg2rad(deg)
        xr = (x - cx) * np.cos(t) + (y - cy) * np.sin(t)
        yr = -(x - cx) * np.sin(t) + (y - cy) * np.cos(t)
        v += np.where((xr / ax) ** 2 + (yr / ay) ** 2 + ((z - cz) / az) ** 2 <= 1.0, val, 0.0)
    # a few small random ellipsoids: more plateau corners at different scales
    for _ in range(6):
        c = rng.uniform(-0.6, 0.6, 3)
        a = rng.uniform(0.05, 0.2, 3)
        v += np.where(((z - c[0]) / a[0]) ** 2 + ((y - c[1]) / a[1]) ** 2 + ((x - c[2]) / a[2]) ** 2 <= 1.0,
                      float(rng.integers(-30, 31)), 0.0)
    return v.astype(np.float32)


def steps(shape, seed=0):
    """Axis-aligned and oblique step edges and constant slabs: large flat regions, ties everywhere."""
    rng = np.random.default_rng(seed)
    z, y, x = _grid(shape)
    v = np.where(x > -0.3, 40.0, 0.0) + np.where(y < 0.25, 25.0, 0.0)
    v += np.where(0.6 * x + 0.5 * y - 0.62 * z > 0.1, 30.0, 0.0)           # oblique plane
    v += np.where(np.abs(z - 0.3) < 0.12, 55.0, 0.0)                         # a slab
    v += np.where((np.abs(x + 0.5) < 0.15) & (np.abs(y) < 0.5), -35.0, 0.0)  # a bar
    v += np.floor(rng.uniform(0, 3)) * np.where(x + y + z > 0.8, 7.0, 0.0)
    return v.astype(np.float32)


def nan_outside_sphere(blobs, r=1.3):
    z, y, x = _grid(blobs.shape)
    v = blobs.astype(np.float32).copy()
    v[x * x + y * y + z * z > r * r] = np.nan
    return v


def nan_outside_box(blobs, frac=0.03):
    v = np.full(blobs.shape, np.nan, np.float32)
    nz, ny, nx = blobs.shape
    a = [max(1, int(round(frac * n))) for n in (nz, ny, nx)]
    sl = tuple(slice(a[i], n - a[i]) for i, n in enumerate((nz, ny, nx)))
    v[sl] = blobs[sl]
    return v


def nan_voxels(blobs, count=2, seed=0):
    """Isolated NaN voxels away from the faces: the blur grows each into a NaN cube."""
    rng = np.random.default_rng(seed)
    v = blobs.astype(np.float32).copy()
    nz, ny, nx = v.shape
    for _ in range(count):
        v[rng.integers(2, nz - 2), rng.integers(2, ny - 2), rng.integers(2, nx - 2)] = np.nan
    return v


def nan_slab(blobs, depth=3):
    """NaN planes at the y = 0 face."""
    v = blobs.astype(np.float32).copy()
    v[:, :depth, :] = np.nan
    return v


def inf_voxels(blobs, count=4, seed=0):
    rng = np.random.default_rng(seed)
    v = blobs.astype(np.float32).copy()
    nz, ny, nx = v.shape
    for i in range(count):
        v[rng.integers(2, nz - 2), rng.integers(2, ny - 2), rng.integers(2, nx - 2)] = np.inf if i % 2 == 0 else -np.inf
    return v


def near_flt_max(blobs):
    """Magnitudes up to ~3e38: a blur or a DoG of these overflows to an infinity."""
    u = _unit(blobs)
    return (3.0e38 * (2.0 * u - 1.0)).astype(np.float32)


# name -> (maker(blobs, shape, seed), has a defined reference output past the detection)
CLASSES = {
    "u8": (lambda b, s, k: quantized_u8(b), True),
    "i16": (lambda b, s, k: quantized_i16(b), True),
    "phantom": (lambda b, s, k: phantom(s, k), True),
    "steps": (lambda b, s, k: steps(s, k), True),
    "hdr_large": (lambda b, s, k: (b * np.float32(1e6)).astype(np.float32), True),
    "hdr_small": (lambda b, s, k: (b * np.float32(1e-6)).astype(np.float32), True),
    "hdr_denormal": (lambda b, s, k: (b * np.float32(1e-36)).astype(np.float32), False),
    "nan_sphere": (lambda b, s, k: nan_outside_sphere(b), True),
    "nan_box": (lambda b, s, k: nan_outside_box(b), True),
    "nan_voxels": (lambda b, s, k: nan_voxels(b, seed=k), True),
    "nan_slab": (lambda b, s, k: nan_slab(b), True),
    "inf_voxels": (lambda b, s, k: inf_voxels(b, seed=k), False),
    "near_max": (lambda b, s, k: near_flt_max(b), False),
}
RECORD_CLASSES = [k for k, (_, ok) in CLASSES.items() if ok]
NAN_CLASSES = ["nan_sphere", "nan_box", "nan_voxels", "nan_slab"]


def make(name, blobs, seed=0):
    """The class `name` built on `blobs` (pkg.synth_blobs of the wanted shape)."""
    return CLASSES[name][0](blobs, blobs.shape, seed)


def dog_triples(shape, seed=0):
    """Small DoG-level triples (prev, cur, next) that stress the extremum test: partial plateaus (ties with some of the 26),
    NaN and +-inf in each of the three levels, signed zeros.  name -> (prev, cur, next)."""
    rng = np.random.default_rng(seed)
    out = {}
    base = lambda: np.round(rng.normal(0, 2, shape)).astype(np.float32)  # small integers: many exact ties
    p, c, n = base(), base(), base()
    out["ties"] = (p, c, n)
    # plateau pieces: a peak whose 26 contain one equal value, and a valley tied with the level above
    p2, c2, n2 = p.copy(), c.copy(), n.copy()
    c2[3:6, 3:6, 3:6] = -5
    c2[4, 4, 4] = 9
    c2[4, 4, 5] = 9
    p2[4, 4, 4] = -9
    c2[8:11, 3:6, 3:6] = 5
    c2[9, 4, 4] = -9
    n2[9, 4, 4] = -9
    out["partial_plateau"] = (p2, c2, n2)
    zs = np.zeros(shape, np.float32)
    zs[::2] = -0.0
    out["signed_zero"] = (zs.copy(), zs.copy(), zs.copy())
    for lvl, name in enumerate(("prev", "cur", "next")):
        for tag, val in (("nan", np.nan), ("inf", np.inf), ("ninf", -np.inf)):
            t = [p.copy(), c.copy(), n.copy()]
            m = rng.random(shape) < 0.04
            t[lvl][m] = val
            out["%s_%s" % (tag, name)] = tuple(t)
    return out


def np_extrema(Dp, Dc, Dn):
    """A plain numpy restatement of the reference's extremum decision (MultiScale.cpp:2408-2524 then :1135-1318): a voxel
    of the interior is a maximum iff every one of its 26 neighbours in Dc and every one of the 27 in Dp and in Dn (when Dn
    is given) compares strictly below it -- a NaN anywhere compares false -- and a minimum likewise with "above".  Returns
    (minima, maxima) as sorted lists of (z, y, x)."""
    Dc = np.asarray(Dc, np.float32)
    nz, ny, nx = Dc.shape
    inner = (slice(1, nz - 1), slice(1, ny - 1), slice(1, nx - 1))
    c = Dc[inner]
    mx = np.ones(c.shape, bool)
    mn = np.ones(c.shape, bool)
    with np.errstate(invalid="ignore"):
        for lvl, own in ((Dp, False), (Dc, True), (Dn, False)):
            if lvl is None:
                continue
            lvl = np.asarray(lvl, np.float32)
            for dz in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        if own and dz == dy == dx == 0:
                            continue
                        v = lvl[1 + dz:nz - 1 + dz, 1 + dy:ny - 1 + dy, 1 + dx:nx - 1 + dx]
                        mx &= v < c
                        mn &= v > c
    f = lambda m: sorted((int(z) + 1, int(y) + 1, int(x) + 1) for z, y, x in zip(*np.nonzero(m)))
    return f(mn), f(mx)
