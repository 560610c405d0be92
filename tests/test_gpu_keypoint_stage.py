"""GPU suite: keypoint_kernel + descriptor_kernel (and the extrema pass, sort, record prefix sum and placement in front of and
behind them) against the oracle's stage-level entry o3_describe_level, on the planted levels of tests/keypoint_cases.py.

Every test hands caller-owned device buffers (img, Dp, Dc, Dn) to a slab context: candidates_reset, extrema_append_dev,
candidates_dev, describe_dev.  Bar: the candidates ARE the planted list (positions, is_max exact; value, h_value, l_value
bit-identical), the records are the oracle's byte for byte -- count, info, desc, and every float field bit-identical -- and the
group words are level_id * 2 + is_max.  What the families reach (reject / accept on every face, tied primaries, 0..4 and 11
frames, rank-deficient tensors, ...) is asserted from the oracle's output alone in tests/test_keypoint_stage_cpu.py.
"""
import numpy as np
import pytest

import keypoint_cases as kc

pytestmark = pytest.mark.gpu

def level(name):
    for lvs in kc.families().values():
        for lv in lvs:
            if lv.name == name:
                return lv
    raise KeyError(name)


# the names kc.families() gives its levels (test_level_names_are_the_built_ones), so that collecting this file builds nothing
NAMES = ["faces_r3_48x40x36", "faces_r4_48x40x36", "faces_r6_48x40x36", "faces_r3_45x37x33", "faces_r6_45x37x33", "faces_ulp_48x40x36",
         "faces_ulp_45x37x33", "faces_edge_48x40x36", "faces_edge_45x37x33", "parabola_48x40x36", "parabola_45x37x33",
         "symmetric_48x40x36_s301", "symmetric_45x37x33_s302", "symmetric_48x40x36_s303", "rank_48x40x36", "rank_45x37x33",
         "flat_48x40x36", "flat_45x37x33", "dense_f32_48x40x36", "dense_u8_45x37x33", "dense_u8_48x40x36", "scale_tiny_48x40x36",
         "scale_tiny_45x37x33", "scale_large_48x40x36", "scale_large_45x37x33"]
REPRESENTATIVE = ["faces_r4_48x40x36", "parabola_45x37x33", "symmetric_48x40x36_s301", "rank_45x37x33", "dense_u8_45x37x33",
                  "scale_large_48x40x36"]
assert set(REPRESENTATIVE) <= set(NAMES)


def test_level_names_are_the_built_ones():
    assert NAMES == [lv.name for lvs in kc.families().values() for lv in lvs]


_WANT = {}


def want(oracle, lv, eig=140.0, mode=0, size_factor=1.0, octave_factor=1.0):
    """The oracle's records (and per-candidate diagnostics) of a level, computed once per configuration."""
    key = (lv.name, eig, mode, size_factor, octave_factor)
    if key not in _WANT:
        _WANT[key] = oracle.describe_level(lv.img, lv.Dc, lv.sig, lv.candidates(), octave_factor=octave_factor, eig_thres=eig,
                                           desc_mode=mode, size_factor=size_factor, diag=True)
    return _WANT[key]


_DEV = {}


def dev(lv):
    """The level's four volumes on the device, uploaded once."""
    import torch
    if lv.name not in _DEV:
        _DEV[lv.name] = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (lv.img, lv.Dp, lv.Dc, lv.Dn))
        torch.cuda.synchronize()
    return _DEV[lv.name]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def compare_records(got, want_recs):
    """The bar of test_gpu_parity._compare_records with `exact` required."""
    assert len(got) == len(want_recs), (len(got), len(want_recs))
    assert (got["info"] == want_recs["info"]).all()
    assert (bits(got["desc"]) == bits(want_recs["desc"])).all()
    for f in ("x", "y", "z", "scale", "ori", "eigs"):
        assert (bits(got[f]) == bits(want_recs[f])).all(), f
    assert got.tobytes() == want_recs.tobytes()


def groups_of(lv, dg, level_id):
    """Group word of every record the oracle returns for the level: level_id * 2 + is_max, once per record of a kept candidate."""
    c = lv.candidates()
    per = np.where(dg[:, 0] == 2, dg[:, 3] + 1, 0)
    return np.repeat(level_id * 2 + c["is_max"], per).astype(np.int32)


def desc_of(lv, level_id, octave_factor=1.0, cut=None):
    """Level-table entry and extrema-pass arguments of a level, whole (cut None) or as planes [z0, z1) keeping [z_lo, z_hi)."""
    img, dp, dc, dn = dev(lv)
    nx, ny, nz = lv.shape
    z0, z1, z_lo, z_hi = (0, nz, 0, nz) if cut is None else cut
    if cut is not None:
        img, dp, dc, dn = (t[z0:z1] for t in (img, dp, dc, dn))
        assert all(t.is_contiguous() for t in (img, dp, dc, dn))
    d = {"img": img.data_ptr(), "dogc": dc.data_ptr(), "nx": nx, "ny": ny, "nz_local": z1 - z0, "nz_global": nz, "z_offset": z0,
         "sigma_h": float(lv.sig[0]), "sigma_c": float(lv.sig[1]), "sigma_l": float(lv.sig[2]), "octave_factor": float(octave_factor)}
    app = (dp.data_ptr(), dc.data_ptr(), dn.data_ptr(), nx, ny, z1 - z0, level_id, z_lo - z0, z_hi - z0)
    return d, app, (img, dp, dc, dn)


def run(built, specs, mode=0, eig=140.0, size_factor=1.0, tune=(), candidates=True):
    """specs: [(level, level_id, octave_factor, cut)].  Returns (candidates or None, records, group words)."""
    n_ids = max(s[1] for s in specs) + 1
    table, apps, keep = [None] * n_ids, [], []
    for lv, level_id, of, cut in specs:
        d, app, bufs = desc_of(lv, level_id, of, cut)
        table[level_id] = d
        apps.append(app)
        keep.append(bufs)
    filler = next(d for d in table if d is not None)      # ids nobody appends to are never read
    table = [d if d is not None else filler for d in table]
    dims = [max(s[0].shape[a] for s in specs) for a in range(3)]
    with built.Context(dims[0], dims[1], dims[2], slab=True) as ctx:
        for knob, value in tune:
            ctx.set_tuning(knob, value)
        ctx.candidates_reset()
        for app in apps:
            ctx.extrema_append_dev(*app)
        cand = ctx.candidates_dev(table) if candidates else None
        recs, grp = ctx.describe_dev(table, desc_mode=mode, eig_thres=eig, size_factor=size_factor)
    return cand, recs, grp


def check_candidates(got, lv, level_id, keep=None):
    c = lv.candidates(level_id)
    if keep is not None:
        c = c[keep]
    assert got.dtype == c.dtype and len(got) == len(c), (len(got), len(c))
    for f in ("octave", "level", "is_max", "x", "y", "z"):
        assert (got[f] == c[f]).all(), f
    for f in ("value", "h_value", "l_value"):
        assert (bits(got[f]) == bits(c[f])).all(), f


@pytest.mark.parametrize("name", NAMES)
def test_family_level_matches_the_oracle(built, oracle, name):
    """Every planted level, under every threshold it is defined for (rank-deficient tensors: 140, 0, 1e30 and -1)."""
    lv = level(name)
    level_id = NAMES.index(name) % 7            # also a level id other than 0: octave / level of the candidates, group words
    for i, eig in enumerate(lv.eig_thres):
        w, dg = want(oracle, lv, eig)
        cand, recs, grp = run(built, [(lv, level_id, 1.0, None)], eig=eig, candidates=(i == 0))
        if i == 0:
            check_candidates(cand, lv, level_id)
        compare_records(recs, w)
        assert (grp == groups_of(lv, dg, level_id)).all()


def test_threshold_level_matches_the_oracle(built, oracle):
    """Primaries on the 0.8 threshold (taken in double): pairs of keypoints a last-bit change of the image moves across it, and
    primaries that a threshold taken in float would keep."""
    lv = kc.threshold_level(kc.SHAPES[0], 701, lambda l, c: oracle.describe_level(l.img, l.Dc, l.sig, c, diag=True)[1])
    w, dg = want(oracle, lv)
    assert (dg[:, 5] > 0).any()
    cand, recs, grp = run(built, [(lv, 0, 1.0, None)])
    check_candidates(cand, lv, 0)
    compare_records(recs, w)
    assert (grp == groups_of(lv, dg, 0)).all()


@pytest.mark.parametrize("name", REPRESENTATIVE)
def test_modes_and_factors(built, oracle, name):
    """desc_mode 0 - 3 under three (size_factor, octave_factor) pairs, and every pair of {1, 0.5, 2} x {1, 2, 4} under mode 0."""
    lv = level(name)
    eig = lv.eig_thres[-1]
    pairs = [(1.0, 1.0), (0.5, 2.0), (2.0, 4.0)]
    combos = [(m, sf, of) for m in (0, 1, 2, 3) for sf, of in pairs]
    combos += [(0, sf, of) for sf in (1.0, 0.5, 2.0) for of in (1.0, 2.0, 4.0) if (sf, of) not in pairs]
    for mode, sf, of in combos:
        w, dg = want(oracle, lv, eig, mode, sf, of)
        _, recs, grp = run(built, [(lv, 0, of, None)], mode=mode, eig=eig, size_factor=sf, candidates=False)
        compare_records(recs, w)
        assert (grp == groups_of(lv, dg, 0)).all()


@pytest.mark.parametrize("name", ["dense_f32_48x40x36", "faces_r6_45x37x33", "symmetric_48x40x36_s303"])
def test_schedules_give_the_same_bytes(built, oracle, name):
    """TUNE_KP_CHUNKS 1, 3, 16 and 0, TUNE_DESC_SEGMENT 0, 1 and 7, TUNE_SAMPLER_CAP 0: how the stage is cut into launches and
    dealt to the XCDs changes no byte (the dense level has 2 500 records: more than one segment, more than one chunk)."""
    lv = level(name)
    w, dg = want(oracle, lv)
    schedules = [[(built.TUNE_KP_CHUNKS, v)] for v in (1, 3, 16, 0)] + [[(built.TUNE_DESC_SEGMENT, v)] for v in (0, 1, 7)] + \
        [[(built.TUNE_SAMPLER_CAP, 0)], [(built.TUNE_KP_CHUNKS, 3), (built.TUNE_DESC_SEGMENT, 1), (built.TUNE_SAMPLER_CAP, 0)]]
    for tune in schedules:
        _, recs, grp = run(built, [(lv, 2, 1.0, None)], tune=tune, candidates=False)
        compare_records(recs, w)
        assert (grp == groups_of(lv, dg, 2)).all(), tune


def test_list_sizes_none_one_and_all_rejected(built, oracle):
    """No candidate at all (nothing planted), a single one, and a list the bounds test rejects whole: zero records, with the
    records-per-keypoint prefix sum behind them."""
    rng = np.random.default_rng(5)
    shape = (45, 37, 33)
    empty = kc.Level("none", shape, kc.sigmas(0.62), rng)
    one = kc.Level("one", shape, kc.sigmas(0.62), rng)
    one.plant((20, 18, 16), 1)
    rejected = kc.Level("rejected", shape, kc.sigmas(0.62), rng)
    for i, p in enumerate([(1, 10, 10), (43, 14, 10), (10, 2, 14), (14, 35, 14), (20, 20, 1), (24, 20, 31), (3, 3, 3), (41, 33, 29)]):
        rejected.plant(p, i % 2)
    for lv, n_cand, any_recs in ((empty, 0, False), (one, 1, True), (rejected, 8, False)):
        mins, maxs = oracle.detect3(lv.Dp, lv.Dc, lv.Dn)
        assert len(mins) + len(maxs) == n_cand
        w, dg = want(oracle, lv)
        assert (len(w) > 0) == any_recs and (not n_cand or any_recs or (dg[:, 0] == 0).all())
        for chunks in (0, 3):
            cand, recs, grp = run(built, [(lv, 1, 1.0, None)], tune=[(built.TUNE_KP_CHUNKS, chunks)])
            check_candidates(cand, lv, 1)
            compare_records(recs, w)
            assert (grp == groups_of(lv, dg, 1)).all()
        _DEV.pop(lv.name)
    # and the rejected list in front of and behind lists that yield records, in one call
    specs = [(rejected, 0, 1.0, None), (one, 1, 1.0, None), (rejected, 2, 1.0, None), (level("faces_r3_45x37x33"), 3, 1.0, None)]
    _, recs, grp = run(built, specs, candidates=False)
    w3, dg3 = want(oracle, specs[3][0])
    compare_records(recs, np.concatenate([want(oracle, one)[0], w3]))
    assert (grp == np.concatenate([groups_of(one, want(oracle, one)[1], 1), groups_of(specs[3][0], dg3, 3)])).all()
    for lv in (one, rejected):
        _DEV.pop(lv.name)


def test_several_levels_in_one_call(built, oracle):
    """Three level ids with three shapes (one of them an octave down, factor 2) in one describe_dev: records group-major, each
    level's run the bytes of its single-level run."""
    a = level("faces_r4_48x40x36")
    b = kc.small_level((24, 20, 18), 77)
    c = level("faces_r3_45x37x33")
    specs = [(a, 0, 1.0, None), (b, 4, 2.0, None), (c, 5, 1.0, None)]
    cand, recs, grp = run(built, specs)
    ws = [want(oracle, lv, octave_factor=of) for lv, _, of, _ in specs]
    assert all(len(w) > 20 for w, _ in ws)
    want_c = np.concatenate([lv.candidates(i) for lv, i, _, _ in specs])
    assert cand.tobytes() == want_c.tobytes()
    compare_records(recs, np.concatenate([w for w, _ in ws]))
    assert (grp == np.concatenate([groups_of(lv, dg, i) for (lv, i, _, _), (_, dg) in zip(specs, ws)])).all()
    assert (np.diff(grp) >= 0).all()
    at = 0
    for (lv, i, of, _), (w, _) in zip(specs, ws):
        _, single, _ = run(built, [(lv, i, of, None)], candidates=False)
        assert single.tobytes() == recs[at:at + len(w)].tobytes()
        at += len(w)
    _DEV.pop(b.name)


@pytest.mark.parametrize("name,rmax", [("faces_r4_48x40x36", 4), ("faces_r3_45x37x33", 3)])
def test_slab_presentation(built, oracle, name, rmax):
    """The same level handed over as planes [z0, z1) with z_offset = z0 and nz_global = nz, extrema kept in [z_lo, z_hi), halos of
    rmax + 2 planes (at these scales, 2 * scale <= 4.1, that covers a rotated patch's reach 2 * scale * sqrt(3) + 1): three cuts,
    the first touching z = 0, the last the far face.  The records are those of the full-volume run whose candidate lies in the
    kept planes -- geometry and the bounds test on all six faces in whole-volume coordinates."""
    lv = level(name)
    nx, ny, nz = lv.shape
    w, dg = want(oracle, lv)
    _, full, full_grp = run(built, [(lv, 1, 1.0, None)], candidates=False)
    compare_records(full, w)
    c = lv.candidates(1)
    per = np.where(dg[:, 0] == 2, dg[:, 3] + 1, 0)
    rec_z = np.repeat(c["z"], per)                       # the candidate plane of every record
    halo = rmax + 2
    cuts = [(0, nz // 3), (nz // 3, 2 * nz // 3 + 1), (2 * nz // 3 + 1, nz)]
    total = 0
    for z_lo, z_hi in cuts:
        z0, z1 = max(0, z_lo - halo), min(nz, z_hi + halo)
        cand, recs, grp = run(built, [(lv, 1, 1.0, (z0, z1, z_lo, z_hi))])
        keep = (c["z"] >= z_lo) & (c["z"] < z_hi)
        assert keep.sum() > 10
        check_candidates(cand, lv, 1, keep)
        sel = (rec_z >= z_lo) & (rec_z < z_hi)
        assert sel.sum() > 10 and (per[keep] == 0).any()  # records, and candidates that yield none, on every slab
        assert recs.tobytes() == full[sel].tobytes()
        assert (grp == full_grp[sel]).all()
        total += len(recs)
    assert total == len(full)
