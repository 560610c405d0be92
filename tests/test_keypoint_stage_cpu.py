"""The oracle's stage-level entry o3_describe_level -- the twin of the product's sift3d_describe_dev that
tests/test_gpu_keypoint_stage.py holds the keypoint and descriptor kernels to -- and the planted cases of tests/keypoint_cases.py.

  1. The new entry IS the pinned arithmetic: fed the three detection levels of octave 0 of a blob volume, with the extrema
     o3_pyramid_candidates reports, it returns the leading records of o3_extract byte for byte.
  2. The planted cases are what they claim: the oracle's own detector finds exactly the planted list in every level, and the
     oracle's output alone reaches the edges the cases are built for (reject next to accept on all six faces, scales that decide
     rmax by one rounding, coordinates exactly on the bound, keypoints with 0, 1, 2, 3, 4 and the full 11 frames, tied strongest
     primaries, more primaries than frames, primaries on the 0.8 threshold).
  3. The planted cases are defined behaviour: a stand-alone program (tests/keypoint_stage_san.c + the oracle source, built with
     -fsanitize=address,undefined -fno-sanitize-recover=undefined) runs the stage on every level as a process of its own, exits
     clean, and returns the bytes the unsanitized library returns.  Nothing is loaded into Python under a sanitizer.
"""
import os
import subprocess

import numpy as np
import pytest

import keypoint_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fams():
    return kc.families()


@pytest.fixture(scope="module")
def outputs(fams, oracle):
    """(family, level name, eig_thres) -> (level, candidates, records, diag), for every threshold the level is defined for."""
    out = {}
    for fam, lvs in fams.items():
        for lv in lvs:
            c = lv.candidates()
            for eig in lv.eig_thres:
                recs, dg = oracle.describe_level(lv.img, lv.Dc, lv.sig, c, eig_thres=eig, diag=True)
                out[(fam, lv.name, eig)] = (lv, c, recs, dg)
    return out


def _blob_volume(dims, seed):
    """Plain numpy: a few hundred Gaussian blobs of either sign."""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    v = np.zeros((nz, ny, nx))
    for _ in range(nx * ny * nz // 1500):
        c = rng.uniform(0, 1, 3) * (nx, ny, nz)
        sg = rng.uniform(1.5, 4.0)
        v += rng.uniform(-100, 100) * np.exp(-((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) / (2 * sg * sg))
    return v.astype(np.float32)


def _sigma_schedule():
    """The float recurrences of run_pyramid (oracle/sift3d_oracle.c): the first blur and the sigma of every level of an octave.  A
    wrong value here cannot pass: the comparison below is byte for byte against o3_extract."""
    f32 = np.float32
    extra0 = np.sqrt(f32(f32(1.6) * f32(1.6)) - f32(f32(0.5) * f32(0.5)), dtype=f32)
    factor = f32(2.0 ** (1.0 / 3.0))
    sig = [f32(1.6)]
    for _ in range(5):
        sig.append(f32(sig[-1] * factor))
    return extra0, sig


@pytest.mark.parametrize("dims,seed", [((64, 64, 64), 1), ((80, 64, 48), 2)])
def test_stage_entry_is_the_pinned_arithmetic(oracle, dims, seed):
    extra0, sig = _sigma_schedule()
    vol = _blob_volume(dims, seed)
    cand = oracle.candidates(vol)
    cand = cand[cand["octave"] == 0]
    G, D = oracle.octave_levels(oracle.blur(vol, extra0))
    assert len(cand) > 20 and len(set(cand["level"])) == 3
    for mode in (0, 1, 2, 3):
        for eig in (140.0, -1.0):
            want, _ = oracle.extract(vol, desc_mode=mode, eig_thres=eig)
            got = [oracle.describe_level(G[l], D[l], sig[l - 1:l + 2], cand[cand["level"] == l], eig_thres=eig, desc_mode=mode)
                   for l in (1, 2, 3)]
            got = np.concatenate(got)
            assert len(got) > 20 and got.tobytes() == want[:len(got)].tobytes(), (mode, eig)
            assert len(got) == len(want) or want["scale"][len(got)] > got["scale"].max()   # what follows is the next octave


def test_stage_entry_scales_and_orders(oracle, fams):
    """octave_factor and size_factor are the two multiplications of the reference, in that order; a list that is not
    minima-then-maxima is refused."""
    lv = fams["faces"][1]
    c = lv.candidates()
    base = oracle.describe_level(lv.img, lv.Dc, lv.sig, c)
    got = oracle.describe_level(lv.img, lv.Dc, lv.sig, c, octave_factor=4.0, size_factor=0.5)
    assert len(base) == len(got) > 50
    for f in ("x", "y", "z", "scale"):
        assert (got[f] == (base[f] * np.float32(4.0)) * np.float32(0.5)).all()
    for f in ("ori", "eigs", "info", "desc"):
        assert (got[f] == base[f]).all()
    with pytest.raises(AssertionError):
        oracle.describe_level(lv.img, lv.Dc, lv.sig, c[::-1].copy())


def test_detector_finds_exactly_the_planted_list(oracle, fams):
    for lvs in fams.values():
        for lv in lvs:
            c = lv.candidates()
            mins, maxs = oracle.detect3(lv.Dp, lv.Dc, lv.Dn)
            nmin = int((c["is_max"] == 0).sum())
            assert len(mins) == nmin and len(maxs) == len(c) - nmin, lv.name
            for part, want in ((mins, c[:nmin]), (maxs, c[nmin:])):
                for f in ("x", "y", "z"):
                    assert (part[f] == want[f]).all(), lv.name
                assert part["value"].tobytes() == want["value"].tobytes(), lv.name
            assert 0 < len(c) <= 2000, lv.name
            assert np.abs(lv.Dp).max() < 3 or lv.name.startswith("parabola")


def test_faces_reach_reject_and_accept_on_every_face(outputs):
    """From the oracle's output alone: on each of the six faces, at every rmax, the bounds test rejects a candidate and accepts one
    a voxel further in."""
    seen = 0
    for (fam, name, eig), (lv, c, recs, dg) in outputs.items():
        if not name.startswith("faces_r"):
            continue
        rmax = int(name.split("_r")[1].split("_")[0])
        for axis, f in enumerate(("x", "y", "z")):
            n = lv.shape[axis]
            others = [g for g in ("x", "y", "z") if g != f]
            inner = np.ones(len(c), bool)
            for g in others:
                m = lv.shape["xyz".index(g)]
                inner &= (c[g] >= rmax + 5) & (c[g] <= m - 1 - (rmax + 5))
            for high in (0, 1):
                d = (n - 1 - c[f]) if high else c[f]
                near = inner & (d <= rmax + 2)
                rej = {int(v) for v in d[near & (dg[:, 0] == 0)]}
                acc = {int(v) for v in d[near & (dg[:, 0] != 0)]}
                assert rej and acc, (name, f, high)
                assert max(rej) + 1 >= min(acc) and any(v + 1 in acc for v in rej), (name, f, high, rej, acc)
                assert min(rej) == 1 and max(acc) == rmax + 2, (name, f, high, rej, acc)
                seen += 1
    assert seen == 5 * 6


def test_faces_scales_decide_rmax_by_one_rounding(outputs):
    """The ulp levels: 2 * scale + 2 lands on 4 exactly, on 4 by rounding up a tie (scale one ulp under 1), one ulp over 4, and one
    ulp under it -- only the last gives rmax 3 and passes at distance 3 from a face."""
    one = np.float32(1.0)
    under1 = np.nextafter(one, np.float32(0))
    under2 = np.nextafter(under1, np.float32(0))
    over1 = np.nextafter(one, np.float32(2))
    for (fam, name, eig), (lv, c, recs, dg) in outputs.items():
        if "ulp" not in name:
            continue
        hit = {float(t) for t, s in lv.aimed if t == s}
        assert hit == {float(one), float(under1), float(under2), float(over1)}, (name, lv.aimed)    # the construction hit every aim
        two = np.float32(2.0)
        assert np.float32(two * under1 + two) == np.float32(4.0) and np.float32(two * under2 + two) < np.float32(4.0)
        kept = recs[(recs["info"] & 0x20) == 0]
        assert (dg[:, 0] == 0).sum() == 18 and (dg[:, 0] != 0).sum() == 6, name
        assert len(kept) > 0 and (kept["scale"] == under2).all(), name


def test_faces_coordinates_on_the_bound(outputs):
    """The edge levels: refined coordinates that are integers exactly.  At distance 4 = rmax from a high face fx + rmax == X, which
    >= rejects; one voxel further in it is accepted and its record shows the integer coordinate; at distance rmax from a low face
    fx - rmax == 0, which < 0 accepts."""
    seen = 0
    for (fam, name, eig), (lv, c, recs, dg) in outputs.items():
        if not name.startswith("faces_edge"):
            continue
        kept = recs[(recs["info"] & 0x20) == 0]
        assert (dg[:, 0] != 1).all() and len(kept) == (dg[:, 0] == 2).sum()
        ck = c[dg[:, 0] == 2]
        for axis, f in enumerate("xyz"):
            n = lv.shape[axis]
            for high in (0, 1):
                d = (n - 1 - c[f]) if high else c[f]
                for dist, accepted in ((3, False), (4, not high), (5, True)):
                    sel = d == dist
                    assert sel.sum() == 2 and ((dg[sel, 0] == 2) == accepted).all(), (name, f, high, dist)
                on = ((n - 1 - ck[f]) if high else ck[f]) <= 5
                assert on.sum() == (2 if high else 4) and (kept[f][on] == ck[f][on] + high).all(), (name, f, high)   # fx = ix (+ 1) exactly
                seen += 1
    assert seen == 12


@pytest.fixture(scope="module")
def thr(oracle):
    lv = kc.threshold_level(kc.SHAPES[0], 701, lambda l, c: oracle.describe_level(l.img, l.Dc, l.sig, c, diag=True)[1])
    return lv, lv.candidates(), oracle.describe_level(lv.img, lv.Dc, lv.sig, lv.candidates(), diag=True)


def test_threshold_level_sits_on_the_threshold(oracle, thr):
    """Pairs of keypoints whose images differ in the last bits and whose count of primaries past 0.8 * max differs; and primaries so
    close under the threshold that taking it in float would keep them."""
    lv, c, (recs, dg) = thr
    mins, maxs = oracle.detect3(lv.Dp, lv.Dc, lv.Dn)
    assert len(mins) + len(maxs) == len(c) == 36 and (mins["x"] == c["x"][:len(mins)]).all() and (maxs["x"] == c["x"][len(mins):]).all()
    assert lv.flips >= 8
    assert (dg[:, 0] == 2).all() and (dg[:, 5] > 0).sum() >= 1


def test_orientation_reach(outputs):
    """Frame counts 0, 1, 2, 3, 4 and the full 11; a keypoint whose two strongest primaries hold the same bits; more primaries
    than the 11 that are looked at; the eigen test on both sides for rank-deficient tensors."""
    frames, ties, many = set(), 0, 0
    for (fam, name, eig), (lv, c, recs, dg) in outputs.items():
        kept = dg[:, 0] == 2
        assert (kc.frames_per_keypoint(recs) == dg[kept, 3]).all() and len(recs) == int((dg[kept, 3] + 1).sum()), name
        frames |= {int(v) for v in dg[kept, 3]}
        ties += int(dg[kept, 2].sum())
        many += int((dg[kept, 1] > 11).sum())
        if fam == "symmetric":
            assert (dg[kept, 3] == 11).sum() >= 5 and dg[kept, 2].sum() >= 1, name
        if fam == "rank" and name.startswith("rank"):
            # threshold 0 rejects everything and -1 nothing; a tensor with a zero eigenvalue fails 140 and even 1e30, one whose
            # smallest eigenvalue is rounding residue passes 1e30
            fates = set(int(v) for v in dg[:, 0])
            assert {140.0: 1 in fates, 0.0: fates == {1}, 1e30: fates == {1, 2}, -1.0: fates == {2}}[eig], (name, eig, fates)
            if eig == -1.0:
                assert (recs["eigs"][:, 2] == 0).sum() >= 3 and (recs["eigs"][:, 1] == 0).sum() >= 3, name    # rank 2 and rank 1, exactly
        if name.startswith("flat"):       # no gradient at all: a zero tensor, no peak, no frame -- and a finite descriptor
            # es^3 = 0 and es * ep = 0: "0 < thres * 0" fails under 140, 0 and 1e30 alike; only the switched-off test keeps it
            assert set(dg[:, 0]) == ({2} if eig == -1.0 else {1}), (name, eig)
            assert len(recs) == (2 if eig == -1.0 else 0), (name, eig)
            if eig == -1.0:
                assert len(recs) == 2 and (recs["eigs"] == 0).all() and (dg[:, 1] == 0).all() and (dg[:, 3] == 0).all(), name
        if fam == "dense":
            assert (dg[:, 1] >= 12).sum() >= 5, name
        assert not np.isnan(recs["desc"]).any() and not np.isnan(recs["ori"]).any(), name
    assert frames >= {0, 1, 2, 3, 4, 11}, frames
    assert ties >= 1 and many >= 10


def _case_file(path, lv, c):
    cf = np.stack([c[f].astype(np.float32) for f in ("x", "y", "z", "is_max", "value", "h_value", "l_value")], axis=1)
    with open(path, "wb") as f:
        f.write(np.ascontiguousarray(lv.img, np.float32).tobytes())
        f.write(np.ascontiguousarray(lv.Dc, np.float32).tobytes())
        f.write(np.ascontiguousarray(cf, np.float32).tobytes())


def test_planted_families_are_defined_behaviour(oracle, fams, outputs, thr, tmp_path):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "kpstage_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    prog = os.path.join(ROOT, "oracle", "_build", "keypoint_stage_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    import _oracle
    outputs = dict(outputs)
    outputs[("threshold", thr[0].name, 140.0)] = (thr[0], thr[1]) + thr[2]
    for fam, lvs in list(fams.items()) + [("threshold", [thr[0]])]:
        for lv in lvs:
            c = lv.candidates()
            case, out = str(tmp_path / (lv.name + ".f32")), str(tmp_path / (lv.name + ".rec"))
            _case_file(case, lv, c)
            cfgs = [(e, 0, 1.0, 1.0) for e in lv.eig_thres] + [(lv.eig_thres[-1], m, 0.5, 2.0) for m in (1, 2, 3)]
            nx, ny, nz = lv.shape
            args = [prog, case, str(nx), str(ny), str(nz), str(len(c))] + [repr(float(s)) for s in lv.sig] + [out] + \
                ["%r:%d:%r:%r" % (float(e), m, s, o) for e, m, s, o in cfgs]
            r = subprocess.run(args, capture_output=True, text=True, env=env)
            assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (lv.name, r.stderr[-3000:])
            got = np.fromfile(out, _oracle.REC)
            want = [outputs[(fam, lv.name, e)][2] for e in lv.eig_thres] + \
                [oracle.describe_level(lv.img, lv.Dc, lv.sig, c, eig_thres=lv.eig_thres[-1], desc_mode=m, size_factor=0.5, octave_factor=2.0)
                 for m in (1, 2, 3)]
            assert [int(l.split()[1]) for l in r.stdout.splitlines()] == [len(w) for w in want], lv.name
            assert got.tobytes() == np.concatenate(want).tobytes(), lv.name
