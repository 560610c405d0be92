"""GPU suite: the order in which descriptor_kernel takes a re-oriented record's samples (TUNE_DESC_ORDER; csrc/sample_order.h).

1: the lanes take the samples sorted by the image row they read (a counting sort in LDS before the sampling); 0: in patch order.
A patch value is the same whichever lane computes it, so both orders must give the oracle's records byte for byte: on the planted
levels of tests/keypoint_cases.py whose patches reach the volume's faces and leave it in x (faces, faces-edge), at both ends of
the scale range (the bins of a small and of a large footprint; the large one joins planes), and on the dense level (2 500
records: the tokens are waited for), at 48 x 40 x 36 and at 45 x 37 x 33, whose rows are no whole vectors -- in all four
descriptor modes, with the sampler cap at 0, 1 and 4, and with the level handed over as a slab with a z offset.  Then one 64^3
extraction under both orders.
"""
import numpy as np
import pytest

from test_gpu_keypoint_stage import compare_records, groups_of, level, run, want

pytestmark = pytest.mark.gpu

LEVELS = ["faces_r3_48x40x36", "faces_r6_48x40x36", "faces_r6_45x37x33", "faces_edge_48x40x36", "faces_edge_45x37x33",
          "scale_tiny_48x40x36", "scale_tiny_45x37x33", "scale_large_48x40x36", "scale_large_45x37x33", "dense_f32_48x40x36",
          "dense_u8_45x37x33"]
ORDERS = (1, 0)


def test_knob_follows_fused_stagger_and_takes_0_and_1(built):
    assert built.TUNE_DESC_ORDER == built.TUNE_FUSED_STAGGER + 1
    with built.Context(16, 16, 16) as ctx:
        for bad in (-1, 2):
            with pytest.raises(Exception):
                ctx.set_tuning(built.TUNE_DESC_ORDER, bad)


@pytest.mark.parametrize("name", LEVELS)
def test_both_orders_give_the_oracles_records(built, oracle, name):
    lv = level(name)
    for eig in lv.eig_thres:
        w, dg = want(oracle, lv, eig)
        # re-oriented records are the only ones the kernel samples; the tiny scale (patches inside one voxel) yields no record
        assert (dg[:, 3] > 0).any() or name.startswith("scale_tiny")
        for order in ORDERS:
            _, recs, grp = run(built, [(lv, 1, 1.0, None)], eig=eig, tune=[(built.TUNE_DESC_ORDER, order)], candidates=False)
            compare_records(recs, w)
            assert (grp == groups_of(lv, dg, 1)).all(), order


@pytest.mark.parametrize("name", ["faces_edge_45x37x33", "scale_large_48x40x36", "dense_u8_45x37x33"])
def test_modes_and_sampler_caps(built, oracle, name):
    """Modes 0 - 3 (the BRIEF family overlays the order on its blur buffer) x sampler cap 0 (no tokens), 1 and 4 x both orders."""
    lv = level(name)
    for mode in (0, 1, 2, 3):
        w, _ = want(oracle, lv, mode=mode)
        got = {}
        for cap in (0, 1, 4):
            for order in ORDERS:
                tune = [(built.TUNE_DESC_ORDER, order), (built.TUNE_SAMPLER_CAP, cap)]
                _, recs, _ = run(built, [(lv, 0, 1.0, None)], mode=mode, tune=tune, candidates=False)
                compare_records(recs, w)
                got[cap, order] = recs.tobytes()
        assert len(set(got.values())) == 1


@pytest.mark.parametrize("name,rmax", [("faces_r4_48x40x36", 4), ("faces_r3_45x37x33", 3)])
def test_slab_presentation_with_a_z_offset(built, oracle, name, rmax):
    """The middle and the last third of the level as planes [z0, z1) with z_offset = z0 > 0: the keys come from whole-volume
    cells, the addresses from the slab's."""
    lv = level(name)
    nz = lv.shape[2]
    w, dg = want(oracle, lv)
    c = lv.candidates(1)
    per = np.where(dg[:, 0] == 2, dg[:, 3] + 1, 0)
    rec_z = np.repeat(c["z"], per)
    halo = rmax + 2
    for z_lo, z_hi in ((nz // 3, 2 * nz // 3 + 1), (2 * nz // 3 + 1, nz)):
        z0, z1 = max(0, z_lo - halo), min(nz, z_hi + halo)
        assert z0 > 0
        sel = (rec_z >= z_lo) & (rec_z < z_hi)
        assert sel.sum() > 10
        for order in ORDERS:
            _, recs, _ = run(built, [(lv, 1, 1.0, (z0, z1, z_lo, z_hi))], tune=[(built.TUNE_DESC_ORDER, order)], candidates=False)
            assert recs.tobytes() == w[sel].tobytes(), order


def test_extraction_is_the_same_under_both_orders(built):
    vol = built.synth_blobs(64, 64, 64, seed=12345)
    got = []
    for order in ORDERS:
        with built.Context(64, 64, 64) as ctx:
            ctx.set_tuning(built.TUNE_DESC_ORDER, order)
            ctx.set_volume(vol)
            got.append(ctx.extract())
    assert len(got[0]) == 74 and got[0].tobytes() == got[1].tobytes()
