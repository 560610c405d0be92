"""pyramid_cases.oracle_pyramid is the oracle's own pyramid: the extrema of its DoG levels are oracle.candidates, entry for entry.

That ties the level volumes tests/test_gpu_pyramid_levels.py compares the resident pyramid with to the candidate lists every
other pipeline test trusts.  CPU only.
"""
import numpy as np
import pytest

import pyramid_cases as pc


@pytest.mark.parametrize("dims,seed,scale", [((64, 64, 64), 12345, 1.0), ((100, 100, 100), 21, 1.0), ((50, 47, 45), 8, 0.5),
                                             ((67, 45, 38), 5, 1.0), ((128, 128, 128), 3, 1.0)])
def test_oracle_pyramid_levels_give_the_oracles_candidates(built, oracle, dims, seed, scale):
    vol = built.synth_blobs(*dims, seed=seed)
    want = oracle.candidates(vol, init_scale=scale)
    pyr = pc.oracle_pyramid(oracle, vol, scale)
    assert [G.shape[1:] for G, _ in pyr] == [(z, y, x) for x, y, z in pc.octave_shapes(dims)]
    assert len(want) > 0 and want["octave"].max() >= 1
    n = 0
    for o, (G, D) in enumerate(pyr):
        for j in range(5):
            assert (pc.bits(D[j]) == pc.bits(oracle.dog(G[j], G[j + 1]))).all(), (o, j)
        for lvl in (1, 2, 3):
            mins, maxs = oracle.detect3(D[lvl - 1], D[lvl], D[lvl + 1])
            for is_max, got in ((0, mins), (1, maxs)):
                w = want[(want["octave"] == o) & (want["level"] == lvl) & (want["is_max"] == is_max)]
                assert len(got) == len(w), (o, lvl, is_max, len(got), len(w))
                for f in ("x", "y", "z"):
                    assert (got[f] == w[f]).all(), (o, lvl, is_max, f)
                assert (pc.bits(got["value"]) == pc.bits(w["value"])).all(), (o, lvl, is_max)
                at = (w["z"], w["y"], w["x"])
                assert (pc.bits(D[lvl - 1][at]) == pc.bits(w["h_value"])).all(), (o, lvl, is_max, "h_value")
                assert (pc.bits(D[lvl + 1][at]) == pc.bits(w["l_value"])).all(), (o, lvl, is_max, "l_value")
                n += len(got)
    assert n == len(want)


def test_initial_sigma_is_the_schedules():
    """1.6^2 - 0.5^2 and 1.6^2 - 1^2 under float32 rounding: the two first blurs the suite uses"""
    assert pc.initial_sigma(1.0) == float(np.sqrt(np.float32(np.float32(1.6) * np.float32(1.6)) - np.float32(0.25), dtype=np.float32))
    assert abs(pc.initial_sigma(1.0) - 1.5198684930801392) < 1e-12     # test_gpu_parity.SIGMAS[3]
    assert abs(pc.initial_sigma(0.5) - 1.2489995956420898) < 1e-6


def test_case_helpers():
    assert pc.octave_shapes((100, 100, 100)) == [(100,) * 3, (50,) * 3, (25,) * 3, (12,) * 3, (6,) * 3, (3,) * 3]
    assert pc.octave_shapes((3, 3, 400)) == [(3, 3, 400)]
    assert pc.tiny_octaves((16, 16, 16)) == 3 and pc.tiny_octaves((17, 16, 16)) == 2 and pc.tiny_octaves((72, 72, 72)) == 2
    a, b = pc.signed_blobs((20, 12, 9), 4), pc.signed_blobs((20, 12, 9), 4)
    assert a.shape == (9, 12, 20) and a.dtype == np.float32 and a.tobytes() == b.tobytes()
    assert (a > 0).any() and (a < 0).any()
    got = [{"L": [a] * 5, "D": [a, None, a + np.float32(1), a, a]}]
    lines, missing = pc.compare_levels(got, [(np.stack([a] * 6), np.stack([a] * 5))], "case")
    assert missing == [(0, "D", 1)] and len(lines) == 1 and "octave 0 D_2: 2160 of 2160 voxels differ, first at (z, y, x) = (0, 0, 0)" in lines[0]
