"""Planted inputs for the per-keypoint stage (keypoint_kernel + descriptor_kernel against o3_describe_level).

Plain numpy, seeded, nothing from the product.  A *level* is what the stage reads: the Gaussian image `img`, the three DoG volumes
`Dp, Dc, Dn` (all (nz, ny, nx) float32), the sigmas of the three DoG levels, and the list of extrema the detector must find in it,
in the reference's order (minima, then maxima, raster order within each).

Planting.  The backgrounds keep every voxel that is not planted from being an extremum, with |v| < 1 throughout:
    Dc in (-0.9, 0.9),   Dp in [0.96, 1),   Dn in (-1, -0.96]
so a background voxel of Dc is neither above all of Dp nor below all of Dn.  A planted voxel p gets Dc[p] = +-(2 + jitter); its six
axis neighbours in Dc set the sub-voxel offset (values a * Dc[p], a < 1: a neighbour of p is never an extremum itself, p beats it);
Dp[p] and Dn[p] set the scale parabola.  Planted voxels sit on a lattice of spacing 3 or more in at least one axis, so the 3x3x3
neighbourhoods of two of them never meet.  Where the peak is not of magnitude 1 (1e-30, 1e30) the whole 3x3x3 neighbourhood of the
three levels is scaled with it, and such neighbourhoods keep a plane of background between them (spacing 4).

Families (`families()` returns all but the first):
  threshold  primaries on the 0.8 threshold (threshold_level; built with the oracle's help, so apart from the rest)
  faces      every face and distance, scales that fix rmax by one rounding, coordinates exactly on the bound
  parabola   offsets 0 and 0.5, peaks of 1e-30, 1 and 1e30, h == l, h or l next to the peak
  symmetric  patches of equal bumps along symmetric directions: tied primaries, the full 11 frames
  rank       rank-1 and rank-2 tensors, and patches without any gradient inside the radius
  dense      white noise, float and quantised
  scale      the smallest and the largest scales a volume admits

Left out on purpose, each as a whole:
  - an `img` that is constant over the WHOLE 11^3 patch.  Normalising it divides by a zero standard deviation, the patch turns to
    NaN, and the orientation splat of the reference (restated by the oracle) then converts a NaN coordinate to int: undefined
    behaviour that indexes outside the histogram on a CPU.  The flat levels of the rank family are constant where the gradients
    inside the 5-sample radius read them, and vary in the corners of the cube.
  - sigmas so large that `(int)(2 * scale + 2)` overflows int: the same kind of undefined conversion, in the bounds test itself.
"""
import numpy as np

CAND = np.dtype([("octave", "<i4"), ("level", "<i4"), ("is_max", "<i4"), ("x", "<i4"), ("y", "<i4"), ("z", "<i4"),
                 ("value", "<f4"), ("h_value", "<f4"), ("l_value", "<f4")])
F = np.float32
SHAPES = [(48, 40, 36), (45, 37, 33)]   # (nx, ny, nz); the second has rows that are no whole 16-byte vectors
RATIO = F(2.0 ** (1.0 / 3.0))


def sigmas(centre):
    """Three sigmas in the pyramid's ratio around `centre`."""
    c = F(centre)
    return (F(c / RATIO), c, F(c * RATIO))


def below(v):
    """The float32 next to v towards zero."""
    return np.nextafter(F(v), F(0))


def vertex(x0, x1, x2, f0, f1, f2):
    """Abscissa of the parabola through three points, in double -- only used to AIM a planted scale; what a case is expected to give
    always comes from the oracle."""
    x0, x1, x2, f0, f1, f2 = (float(v) for v in (x0, x1, x2, f0, f1, f2))
    det = lambda a1, a2, a3, b1, b2, b3, c1, c2, c3: (a1 * b2 * c3) - (a1 * b3 * c2) - (a2 * b1 * c3) + (a3 * b1 * c2) + (a2 * b3 * c1) - (a3 * b2 * c1)
    dx = det(f0, f1, f2, x0, x1, x2, 1, 1, 1)
    dy = det(x0 * x0, x1 * x1, x2 * x2, f0, f1, f2, 1, 1, 1)
    return dy / (-2.0 * dx)


class Level:
    def __init__(self, name, shape, sig, rng, img=None):
        nx, ny, nz = shape
        self.name, self.shape, self.sig = name, shape, tuple(F(s) for s in sig)
        self.Dc = rng.uniform(-0.9, 0.9, (nz, ny, nx)).astype(F)
        self.Dp = rng.uniform(0.96, 0.999, (nz, ny, nx)).astype(F)
        self.Dn = (-rng.uniform(0.96, 0.999, (nz, ny, nx))).astype(F)
        self.img = smooth_img(shape, rng) if img is None else img
        self.rng = rng
        self.eig_thres = (140.0,)   # the thresholds the level is run under
        self._pts = {}
        self.aimed = []        # (target scale, float32 scale the construction achieves) of the candidates planted with aim_scale

    def plant(self, p, is_max, axes=None, h=None, l=None, mag=1.0, peak=None):
        """p = (x, y, z).  axes: six fractions a (x-, x+, y-, y+, z-, z+) of the peak, or callables of the peak; h, l: fractions
        of the peak, or callables; mag: magnitude of the peak."""
        x, y, z = (int(v) for v in p)
        nx, ny, nz = self.shape
        assert 1 <= x < nx - 1 and 1 <= y < ny - 1 and 1 <= z < nz - 1, p
        for q, (_, qmag) in self._pts.items():   # scaled neighbourhoods keep a plane of background between them
            assert max(abs(q[0] - x), abs(q[1] - y), abs(q[2] - z)) >= (3 if mag == 1.0 and qmag == 1.0 else 4), (p, q)
        rng = self.rng
        sgn = 1.0 if is_max else -1.0
        c = F(sgn * mag * (2.0 + rng.uniform(0, 0.5))) if peak is None else F(peak)
        if mag != 1.0:
            for D in (self.Dp, self.Dc, self.Dn):
                D[z - 1:z + 2, y - 1:y + 2, x - 1:x + 2] = (sgn * mag * rng.uniform(0, 0.45, (3, 3, 3))).astype(F)
        val = lambda a: F(a(c)) if callable(a) else F(F(a) * c)
        axes = rng.uniform(0.0, 0.95, 6) if axes is None else axes
        h = rng.uniform(0.3, 0.8) if h is None else h
        l = rng.uniform(0.3, 0.8) if l is None else l
        self.Dc[z, y, x] = c
        for a, (dx, dy, dz) in zip(axes, ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))):
            self.Dc[z + dz, y + dy, x + dx] = val(a)
        self.Dp[z, y, x] = val(h)
        self.Dn[z, y, x] = val(l)
        self._pts[(x, y, z)] = (bool(is_max), mag)

    def candidates(self, level_id=0):
        """The planted list in the reference's order."""
        pts = sorted(self._pts.items(), key=lambda kv: (kv[1][0], kv[0][2], kv[0][1], kv[0][0]))
        out = np.zeros(len(pts), CAND)
        for i, ((x, y, z), (mx, _)) in enumerate(pts):
            out[i] = (level_id // 3, level_id % 3 + 1, int(mx), x, y, z, self.Dc[z, y, x], self.Dp[z, y, x], self.Dn[z, y, x])
        return out

    def aim_scale(self, target, c, l_frac, tries=40):
        """(h, l) as float32 VALUES for a peak c whose scale parabola gives float32(2 * vertex) == target, or the nearest found."""
        c, target = F(c), F(target)
        best = None
        for k in range(tries):
            l = F(F(l_frac) * c)
            for _ in range(k):
                l = np.nextafter(l, F(0))
            sgn = F(1.0) if c > 0 else F(-1.0)
            s = lambda m: F(2 * vertex(self.sig[0], self.sig[1], self.sig[2], sgn * np.int32(m).view(F), c, l))
            a, b = int(F(0.05 * abs(c)).view(np.int32)), int(F(0.98 * abs(c)).view(np.int32))   # |h| as ordered integers
            rising = s(b) > s(a)                       # the vertex moves monotonically with |h| between them
            while b - a > 1:
                m = (a + b) // 2
                if (s(m) < target) == rising:
                    a = m
                else:
                    b = m
            for m in (a, b):
                hm = sgn * np.int32(m).view(F)
                err = abs(float(s(m)) - float(target))
                if best is None or err < best[0]:
                    best = (err, hm, l, s(m))
            if best[0] == 0:
                break
        self.aimed.append((target, best[3]))
        return best[1], best[2]


def smooth_img(shape, rng, noise=0.15):
    """A few random plane waves plus a little noise: generic gradients everywhere."""
    nx, ny, nz = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    v = np.zeros((nz, ny, nx))
    for _ in range(12):
        k = rng.normal(0, 0.9, 3)
        v += rng.uniform(0.3, 1.0) * np.sin(k[0] * x + k[1] * y + k[2] * z + rng.uniform(0, 6.28))
    v += noise * rng.normal(0, 1, v.shape)
    return v.astype(F)


def lattice(lo, hi, step=3):
    return list(range(lo, hi + 1, step))


# ---- faces -----------------------------------------------------------------------------------------------------------------
def faces_level(shape, rmax, seed):
    """Every face, every integer distance 1 .. rmax + 2 from it, offsets on both sides of 0, minima and maxima; the other two
    coordinates stay rmax + 5 or more from their faces, so only the one face decides."""
    rng = np.random.default_rng(seed)
    centre = {3: 0.375, 4: 0.62, 6: 1.12}[rmax]
    lv = Level("faces_r%d_%dx%dx%d" % ((rmax,) + shape), shape, sigmas(centre), rng)
    m = rmax + 5
    slots = [lattice(m, n - 1 - m) for n in shape]
    k = 0
    for axis in range(3):
        t = [a for a in range(3) if a != axis]
        tang = [(u, v) for u in slots[t[0]] for v in slots[t[1]]]
        ndist = rmax + 2
        reps = min(4, len(tang) // ndist)
        assert reps >= 2, (shape, rmax, axis)
        for high in (0, 1):
            it = iter(tang)
            for d in range(1, ndist + 1):
                for r in range(reps):
                    u, v = next(it)
                    p = [0, 0, 0]
                    p[axis] = shape[axis] - 1 - d if high else d
                    p[t[0]], p[t[1]] = u, v
                    ax = list(rng.uniform(0.2, 0.9, 6))
                    a, b = (0.2, 0.9) if r % 2 == 0 else (0.9, 0.2)       # offset towards the lower / the higher neighbour
                    if r >= 2:
                        a, b = (0.70, 0.72) if r == 2 else (0.72, 0.70)   # a small offset on either side
                    ax[2 * axis], ax[2 * axis + 1] = a, b
                    hl = rng.uniform(0.55, 0.65)
                    lv.plant(p, (k + r) % 2, axes=ax, h=hl, l=hl + rng.uniform(-0.03, 0.03))
                k += 1
    return lv


def faces_edge_level(shape, seed):
    """Coordinates that land ON the bound.  The neighbour towards the face is nextafter(peak, 0) and the other one 0: the offset is
    0.5 less a part in 1e7, which the conversion of the refined coordinate to float rounds to 0.5 exactly, so fx is the integer
    ix (low faces) or ix + 1 (high faces).  With rmax = 4, at distance rmax from a high face fx + rmax == X (rejected by >=), at
    distance rmax from a low face fx - rmax == 0 (not < 0: accepted); distances rmax - 1 and rmax + 1 on either side of them."""
    rng = np.random.default_rng(seed)
    rmax = 4
    lv = Level("faces_edge_%dx%dx%d" % shape, shape, sigmas(0.62), rng)
    m = rmax + 5
    slots = [lattice(m, n - 1 - m) for n in shape]
    for axis in range(3):
        t = [a for a in range(3) if a != axis]
        tang = [(u, v) for u in slots[t[0]] for v in slots[t[1]]]
        for high in (0, 1):
            it = iter(tang)
            for d in (rmax - 1, rmax, rmax + 1):
                for is_max in (0, 1):
                    u, v = next(it)
                    p = [0, 0, 0]
                    p[axis] = shape[axis] - 1 - d if high else d
                    p[t[0]], p[t[1]] = u, v
                    ax = [0.5] * 6
                    ax[2 * axis + high], ax[2 * axis + 1 - high] = below, 0.0
                    lv.plant(p, is_max, axes=ax, h=0.6, l=0.6)
    return lv


def faces_ulp_level(shape, seed):
    """Scales aimed at 2 * scale + 2 == 4 to within an ulp (scale 1 and its float neighbours, so rmax is 3 or 4 by one rounding),
    offset 0, at distance 3 from every face: accepted with rmax 3, rejected with rmax 4."""
    rng = np.random.default_rng(seed)
    lv = Level("faces_ulp_%dx%dx%d" % shape, shape, sigmas(0.5), rng)
    m = 9
    slots = [lattice(m, n - 1 - m) for n in shape]
    one = F(1.0)
    targets = [one, np.nextafter(one, F(0)), np.nextafter(np.nextafter(one, F(0)), F(0)), np.nextafter(one, F(2))]
    for axis in range(3):
        t = [a for a in range(3) if a != axis]
        it = iter([(u, v) for u in slots[t[0]] for v in slots[t[1]]])
        for high in (0, 1):
            for i, tg in enumerate(targets):
                u, v = next(it)
                p = [0, 0, 0]
                p[axis] = shape[axis] - 1 - 3 if high else 3
                p[t[0]], p[t[1]] = u, v
                is_max = (i + high) % 2
                c = F((1.0 if is_max else -1.0) * (2.0 + rng.uniform(0, 0.5)))
                h, l = lv.aim_scale(tg, c, rng.uniform(0.5, 0.7))
                ax = [0.5] * 6
                lv.plant(p, is_max, axes=ax, h=lambda c_, h=h: h, l=lambda c_, l=l: l, peak=c)
    return lv


# ---- parabola --------------------------------------------------------------------------------------------------------------
def parabola_level(shape, seed):
    rng = np.random.default_rng(seed)
    lv = Level("parabola_%dx%dx%d" % shape, shape, sigmas(0.5), rng)
    m = 8
    pts = iter([(x, y, z) for z in lattice(m, shape[2] - 1 - m, 4) for y in lattice(m, shape[1] - 1 - m, 4)
                for x in lattice(m, shape[0] - 1 - m, 4)])
    nb = lambda c: below(c)                     # a neighbour one ulp under the peak
    axes_kinds = [
        lambda: [0.5, 0.5, 0.25, 0.25, 0.05, 0.05],         # equal on both sides: offset 0
        lambda: [nb, 0.3, 0.6, nb, nb, 0.1],                # one neighbour at nextafter(peak, 0): offset near +-0.5
        lambda: [0.3, nb, nb, 0.6, 0.1, nb],
        lambda: [nb, nb, nb, nb, nb, nb],                   # both: offset 0 again, curvature of one ulp
    ]
    hl_kinds = [(0.6, 0.6), (nb, 0.4), (0.4, nb), (nb, nb), (0.05, 0.9), (0.9, 0.05)]   # h == l; the scale extremes of the level
    for mag in (1e-30, 1.0, 1e30):
        for ak in axes_kinds:
            for h, l in hl_kinds:
                for is_max in (0, 1):
                    lv.plant(next(pts), is_max, axes=ak(), h=h, l=l, mag=mag)
    return lv


# ---- symmetric patches -----------------------------------------------------------------------------------------------------
AXES6 = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
DIAG8 = [(a, b, c) for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)]
FACE12 = [v for v in [(a, b, 0) for a in (-1, 1) for b in (-1, 1)] + [(a, 0, b) for a in (-1, 1) for b in (-1, 1)] +
          [(0, a, b) for a in (-1, 1) for b in (-1, 1)]]
DIRSETS = {"axes6": AXES6, "diag8": DIAG8, "both14": AXES6 + DIAG8, "face12": FACE12}


def bumps(img, p, dirs, dist, width, amp=1.0, unit=True):
    """Adds equal Gaussian bumps at p + dist * d (d normalised when unit) to img, inside a box around p."""
    x0, y0, z0 = p
    r = int(np.ceil(dist * (1.0 if unit else 1.8) + 3 * width)) + 1
    zz, yy, xx = np.meshgrid(np.arange(-r, r + 1), np.arange(-r, r + 1), np.arange(-r, r + 1), indexing="ij")
    acc = np.zeros(zz.shape)
    for d in dirs:
        d = np.asarray(d, float)
        if unit:
            d = d / np.linalg.norm(d)
        acc += amp * np.exp(-((xx - dist * d[0]) ** 2 + (yy - dist * d[1]) ** 2 + (zz - dist * d[2]) ** 2) / (2 * width * width))
    img[z0 - r:z0 + r + 1, y0 - r:y0 + r + 1, x0 - r:x0 + r + 1] += acc.astype(F)


def symmetric_level(shape, seed, centre=0.75):
    """Integer centre, offset 0, `img` a sum of equal bumps along a symmetric set of directions: tied or nearly tied primary peaks."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    img = np.zeros((nz, ny, nx), F)
    lv = Level("symmetric_%dx%dx%d_s%d" % (shape + (seed,)), shape, sigmas(centre), rng, img=img)
    rad = 4.0 * centre                                   # patch half-width in voxels at the central scale
    step = int(2 * np.ceil(rad * 1.8) + 2)
    m = step // 2 + 1
    pts = [(x, y, z) for z in lattice(m, nz - 1 - m, step) for y in lattice(m, ny - 1 - m, step) for x in lattice(m, nx - 1 - m, step)]
    kinds = [(n, dist, w, unit) for n in DIRSETS for dist, w, unit in ((0.6, 0.35, True), (0.8, 0.25, True), (0.5, 0.3, False))]
    for i, p in enumerate(pts):
        n, dist, w, unit = kinds[(i + seed) % len(kinds)]
        bumps(img, p, DIRSETS[n], dist * rad, w * rad, unit=unit)
        hl = 0.6
        lv.plant(p, i % 2, axes=[0.5] * 6, h=hl, l=hl)
    return lv


_THRESHOLD = {}


def threshold_level(shape, seed, describe):
    """threshold_level_build, once per process."""
    if (shape, seed) not in _THRESHOLD:
        _THRESHOLD[(shape, seed)] = threshold_level_build(shape, seed, describe)
    return _THRESHOLD[(shape, seed)]


def threshold_level_build(shape, seed, describe):
    """Primaries ON the 0.8 threshold.  Each pair of keypoints has bumps of amplitude 1 along one set of directions and of amplitude
    r along another; r is bisected -- with `describe(level, candidates) -> diag` of the oracle deciding -- until the number of
    primaries past the threshold changes between two images that differ in the last bits only, and the pair is planted with the
    r on either side of that flip.  (The only case that needs the oracle to be BUILT; what it must give still comes from the
    oracle alone.)"""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    centre = 0.5
    rad = 4.0 * centre * 1.0268
    step = int(2 * np.ceil(rad * 1.8) + 2)
    m = step // 2 + 1
    pts = [(x, y, z) for z in lattice(m, nz - 1 - m, step) for y in lattice(m, ny - 1 - m, step) for x in lattice(m, nx - 1 - m, step)]
    pts = pts[:len(pts) // 2 * 2]
    sets = [(AXES6[:2], AXES6[2:4]), (AXES6[:2], AXES6[2:]), (DIAG8[:4], DIAG8[4:]), (AXES6, DIAG8), (DIAG8, AXES6), (AXES6[:4], FACE12[:4]),
            (FACE12[:6], FACE12[6:]), (AXES6[:3], AXES6[3:])]
    kinds = [(sets[i % len(sets)], 0.55 + 0.05 * (i % 4), 0.3 + 0.03 * (i % 3)) for i in range(len(pts) // 2)]

    def build(rs):
        img = np.zeros((nz, ny, nx), F)
        lv = Level("threshold_%dx%dx%d" % shape, shape, sigmas(centre), np.random.default_rng(seed + 1), img=img)
        for i, p in enumerate(pts):
            (da, db), dist, w = kinds[i // 2]
            bumps(img, p, da, dist * rad, w * rad)
            bumps(img, p, db, dist * rad, w * rad, amp=rs[i])
            lv.plant(p, (i // 2) % 2, axes=[0.5] * 6, h=0.6, l=0.6)
        return lv

    n = len(pts)
    lo, hi = np.full(n, 0.2), np.full(n, 1.0)
    lv = build(np.where(np.arange(n) % 2 == 0, lo, hi))
    # candidate order -> plant order: position of every planted point in the candidate list
    where = {tuple(int(v) for v in (c["x"], c["y"], c["z"])): j for j, c in enumerate(lv.candidates())}
    at = np.array([where[p] for p in pts])
    kept = lambda lv: describe(lv, lv.candidates())[at, 4]
    k_even, k_odd = kept(lv)[0::2], kept(lv)[1::2]              # even slots hold r = lo, odd slots r = hi
    live = k_even != k_odd                                    # pairs whose bracket holds a flip
    lo2, hi2 = lo[0::2].copy(), hi[0::2].copy()
    klo = k_even.copy()
    for _ in range(30):                                       # to a part in 1e9 of r: well under a bit of the float32 image
        mid = 0.5 * (lo2 + hi2)
        rs = np.empty(n)
        rs[0::2], rs[1::2] = mid, mid
        km = kept(build(rs))[0::2]
        same = km == klo
        lo2 = np.where(same, mid, lo2)
        hi2 = np.where(same, hi2, mid)
    # around the flip, prefer for the second keypoint of a pair an image whose primary sits within half an ulp of the threshold
    best = hi2.copy()
    found = np.zeros(n // 2, bool)
    for k in range(-12, 13):
        rs = np.empty(n)
        rs[0::2], rs[1::2] = lo2, hi2 * (1.0 + 3e-8 * k)
        near = describe(build(rs), build(rs).candidates())[at, 5][1::2] > 0
        best = np.where(near & ~found, rs[1::2], best)
        found |= near
    rs = np.empty(n)
    rs[0::2], rs[1::2] = lo2, best
    lv = build(rs)
    lv.flips = int(live.sum())
    return lv


# ---- rank-deficient --------------------------------------------------------------------------------------------------------
def rank_level(shape, seed):
    """One planar edge through p (rank 1) and two crossing planes (rank 2): sharp and smooth edges, axis-aligned and oblique."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    img = np.zeros((nz, ny, nx), F)
    centre = 0.4
    lv = Level("rank_%dx%dx%d" % shape, shape, sigmas(centre), rng, img=img)
    rad = 4.0 * centre * 1.0268          # h == l puts the vertex midway between the outer sigmas
    r = int(np.ceil(rad * 1.74 + 1))     # a frame's rotated cube and the trilinear footprint of its corners
    step = 2 * r + 1
    m = r + 1
    pts = [(x, y, z) for z in lattice(m, nz - 1 - m, step) for y in lattice(m, ny - 1 - m, step) for x in lattice(m, nx - 1 - m, step)]
    zz, yy, xx = np.meshgrid(np.arange(-r, r + 1), np.arange(-r, r + 1), np.arange(-r, r + 1), indexing="ij")
    normals = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 2, 3), (1, -1, 1)]
    kinds = []
    for n in normals:
        kinds += [("edge", n, None, 0.0), ("edge", n, None, 0.7)]
    for a, b in (((1, 0, 0), (0, 1, 0)), ((0, 1, 0), (0, 0, 1)), ((1, 1, 0), (0, 0, 1)), ((1, 2, 3), (1, -1, 1))):
        kinds += [("cross", a, b, 0.0), ("cross", a, b, 0.7)]
    assert len(pts) >= len(kinds), (shape, len(pts))
    ramp = lambda t, w: np.sign(t) if w == 0 else np.tanh(t / w)
    for i, p in enumerate(pts):
        kind, a, b, w = kinds[(i + seed) % len(kinds)]
        x0, y0, z0 = p
        box = img[z0 - r:z0 + r + 1, y0 - r:y0 + r + 1, x0 - r:x0 + r + 1]
        a = np.asarray(a, float) / np.linalg.norm(a)
        v = ramp(xx * a[0] + yy * a[1] + zz * a[2] + (0.25 if w == 0 else 0.0), w)
        if kind == "cross":
            b = np.asarray(b, float) / np.linalg.norm(b)
            v = v + 0.5 * ramp(xx * b[0] + yy * b[1] + zz * b[2] + (0.25 if w == 0 else 0.0), w)
        box[...] = v.astype(F)
        lv.plant(p, i % 2, axes=[0.5] * 6, h=0.6, l=0.6)
    lv.eig_thres = (140.0, 0.0, 1e30, -1.0)
    return lv


def flat_level(shape, seed):
    """`img` constant wherever the gradients of the in-radius samples read it, and varying in the corners of the 11^3 cube (so the
    patch still has a standard deviation): no gradient, a zero tensor, no histogram peak, no frame.  The samples within the
    5-sample radius and their axis neighbours reach 1.15 * rad from p, the trilinear footprint a voxel more in every axis, the
    corners of the cube 1.73 * rad: that needs rad > 6 voxels."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    centre = 1.75
    rad = 4.0 * centre * 1.0268          # h == l puts the vertex midway between the outer sigmas
    ball = 1.15 * rad + 1.8
    assert 1.73 * rad - 1.8 > ball
    img = smooth_img(shape, rng, noise=0.5)
    lv = Level("flat_%dx%dx%d" % shape, shape, sigmas(centre), rng, img=img)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    m = int(rad + 2) + 2
    for i, p in enumerate(((m, ny // 2, nz // 2), (nx - 1 - m, ny // 2, nz // 2))):
        img[(x - p[0]) ** 2 + (y - p[1]) ** 2 + (z - p[2]) ** 2 <= ball * ball] = F(1.5 + i)
        lv.plant(p, i % 2, axes=[0.5] * 6, h=0.6, l=0.6)
    lv.eig_thres = (140.0, 0.0, 1e30, -1.0)   # the zero tensor: 0 < thres * 0 fails for every thres >= 0
    return lv


# ---- dense -----------------------------------------------------------------------------------------------------------------
def dense_level(shape, seed, quantised):
    """White-noise `img` (float, or quantised to 8-bit steps): dozens of raw histogram peaks per keypoint and, with the quantised
    one, exact ties among their values."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    if quantised:
        img = rng.integers(0, 4, (nz, ny, nx)).astype(F) * F(85.0)       # four grey levels: few distinct gradients, many ties
    else:
        img = rng.uniform(0, 1, (nz, ny, nx)).astype(F)
    lv = Level("dense_%s_%dx%dx%d" % (("u8" if quantised else "f32",) + shape), shape, sigmas(0.3 if quantised else 0.75), rng, img=img)
    m = 8
    pts = [(x, y, z) for z in lattice(m, nz - 1 - m, 4) for y in lattice(m, ny - 1 - m, 4) for x in lattice(m, nx - 1 - m, 4)]
    for i, p in enumerate(pts):
        if quantised:      # integer centre and a scale whose samples fall on voxel centres or exactly between them
            lv.plant(p, i % 2, axes=[0.5] * 6, h=0.6, l=0.6)
        else:
            lv.plant(p, i % 2)
    return lv


# ---- scale extremes --------------------------------------------------------------------------------------------------------
def scale_level(shape, seed, tiny):
    """tiny: the 11^3 samples fall inside one or two source cells.  Otherwise the largest scale the volume admits: the patch
    reaches from face to face, and the candidates one voxel further out on every side are rejected."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    if tiny:
        lv = Level("scale_tiny_%dx%dx%d" % shape, shape, sigmas(0.004), rng)
        pts = [(x, y, z) for z in lattice(3, nz - 4, 5) for y in lattice(3, ny - 4, 5) for x in lattice(3, nx - 4, 5)]
        for i, p in enumerate(pts):
            lv.plant(p, i % 2)
        lv.eig_thres = (140.0, -1.0)   # inside one cell the image is trilinear: the eigen test rejects nearly all of them
        return lv
    half = min(shape) // 2
    centre = (half - 3.5) / 4.0 / 1.02
    lv = Level("scale_large_%dx%dx%d" % shape, shape, sigmas(centre), rng)
    c0 = (nx // 2, ny // 2, nz // 2)
    k = 0
    for dz in (-3, 0, 3):
        for dy in (-3, 0, 3):
            for dx in (-3, 0, 3):
                hl = 0.4 + 0.02 * k
                lv.plant((c0[0] + dx, c0[1] + dy, c0[2] + dz), k % 2, h=hl, l=hl)
                k += 1
    return lv


def small_level(shape, seed, centre=0.5, step=3, margin=6):
    """Generic planted points on a lattice over the interior of a (small) volume."""
    rng = np.random.default_rng(seed)
    lv = Level("small_%dx%dx%d_s%d" % (shape + (seed,)), shape, sigmas(centre), rng)
    nx, ny, nz = shape
    pts = [(x, y, z) for z in lattice(margin, nz - 1 - margin, step) for y in lattice(margin, ny - 1 - margin, step)
           for x in lattice(margin, nx - 1 - margin, step)]
    for i, p in enumerate(pts):
        lv.plant(p, i % 2)
    return lv


# ---- the lot ---------------------------------------------------------------------------------------------------------------
_FAMILIES = None


def families():
    """name -> list of levels.  Built once per process (under a second) and shared: nobody writes to a level."""
    global _FAMILIES
    if _FAMILIES is None:
        _FAMILIES = _build_families()
    return _FAMILIES


def _build_families():
    a, b = SHAPES
    return {
        "faces": [faces_level(a, 3, 101), faces_level(a, 4, 102), faces_level(a, 6, 103), faces_level(b, 3, 104),
                  faces_level(b, 6, 105), faces_ulp_level(a, 106), faces_ulp_level(b, 107), faces_edge_level(a, 108),
                  faces_edge_level(b, 109)],
        "parabola": [parabola_level(a, 201), parabola_level(b, 202)],
        "symmetric": [symmetric_level(a, 301), symmetric_level(b, 302), symmetric_level(a, 303, centre=0.5)],
        "rank": [rank_level(a, 401), rank_level(b, 402), flat_level(a, 403), flat_level(b, 404)],
        "dense": [dense_level(a, 501, False), dense_level(b, 502, True), dense_level(a, 503, True)],
        "scale": [scale_level(a, 601, True), scale_level(b, 602, True), scale_level(a, 603, False), scale_level(b, 604, False)],
    }


def frames_per_keypoint(recs):
    """Frame counts of the keypoints of a record list: a keypoint is one record with the reorient bit clear followed by its frames."""
    re = (recs["info"] & 0x20) != 0
    starts = np.flatnonzero(~re)
    return np.diff(np.append(starts, len(recs))) - 1
