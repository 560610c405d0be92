"""GPU suite: every case of tests/blur_cases.py against the oracle, bit for bit ("Blur ledger").

tests/test_blur_ledger.py (CPU) holds the table to reach every blur kernel the library builds: the 94 forms of the fused launch, the
16 + 64 instantiations of the three-pass kernels, the generic kernel through its DoG branch.  Here each case runs through its
operator-level entry point; level, DoG and half-size volume are compared with oracle.blur, oracle.dog and oracle.subsample
without a tolerance -- the kernels claim the reference's operations in its order -- and the launch log says
whether the fused launch or the three passes ran, as the case expects.  Then the pipeline with a first blur of 3 taps.
"""
import collections

import numpy as np
import pytest

import blur_cases as bc
import pyramid_cases as pc

pytestmark = pytest.mark.gpu

KNOB_DEFAULTS = {"BLUR_FUSED": 1, "FUSED_CHUNKS": 0, "FUSED_ROWS": 0, "FUSED_TILE": 0, "FUSED_STAGGER": 0, "FUSED_SUB": 1}   # sift3d_create's
SENTINEL = 123.0

GROUPS = collections.OrderedDict()
for _c in bc.CASES:
    GROUPS.setdefault((_c.family, _c.dims), []).append(_c)

_WANT = {}


def want_of(oracle, case):
    """(taps, level, DoG) of the oracle for a case's input and filter, computed once and left unchanged"""
    key = (case.dims, case.sigma, case.nonfinite)
    if key not in _WANT:
        vol = bc.volume(case.dims, case.nonfinite)
        level = oracle.blur(vol, case.sigma)
        dog = oracle.dog(vol, level)
        for a in (level, dog):
            a.setflags(write=False)
        _WANT[key] = (len(oracle.taps(case.sigma)), level, dog)
    return _WANT[key]


def differing(got, want, nan_aware):
    """the voxels where got has not want's bits; with nan_aware a NaN matches a NaN (and only a NaN), as
    test_gpu_image_like.same_floats has it: sign and payload of a NaN are what x86 and the GPU may encode differently"""
    bad = pc.bits(got) != pc.bits(want)
    if nan_aware:
        bad &= ~(np.isnan(got) & np.isnan(want))
    return bad


def hold(got, want, case, what):
    assert got.shape == want.shape, (bc.describe(case), what)
    bad = differing(got, want, case.nonfinite)
    if bad.any():
        zyx = tuple(int(i) for i in np.argwhere(bad)[0])
        pytest.fail("%s: %s differs from the oracle in %d of %d voxels, first at (z, y, x) = %s: %r, the oracle's %r"
                    % (bc.describe(case), what, int(bad.sum()), bad.size, zyx, float(got[zyx]), float(want[zyx])))


@pytest.mark.parametrize("family,dims", list(GROUPS), ids=["%s-%dx%dx%d" % ((f.replace(" ", "_"),) + d) for f, d in GROUPS])
def test_every_case_gives_the_oracles_bits(built, oracle, family, dims):
    """One context and one set of device buffers per (family, shape); every filter, output set and knob setting of the table in
    turn.  An output the call does not ask for keeps what it held."""
    import torch
    nx, ny, nz = dims
    stage = {s: built.STAGES.index(s) for s in ("blur_x", "blur_y", "blur_z_dog", "blur_fused")}
    with built.Context(*dims) as ctx:
        d_in = {nf: torch.from_numpy(bc.volume(dims, nf).copy()).cuda() for nf in {c.nonfinite for c in GROUPS[family, dims]}}   # the table's volume is read-only
        d_out, d_dog = (torch.empty((nz, ny, nx), dtype=torch.float32, device="cuda") for _ in range(2))
        d_half = torch.empty((nz // 2, ny // 2, nx // 2), dtype=torch.float32, device="cuda")
        for case in GROUPS[family, dims]:
            ntaps, level, dog = want_of(oracle, case)
            has_out, has_dog = bc.OUTPUTS[case.entry]
            for knob, value in dict(KNOB_DEFAULTS, **case.knobs).items():
                ctx.set_tuning(getattr(built, "TUNE_" + knob), value)
            for d in (d_out, d_dog, d_half):
                d.fill_(SENTINEL)
            torch.cuda.synchronize()   # torch's stream and the context's stream are not ordered with each other
            ctx.enable_timing(True)    # a fresh launch log
            src = d_in[case.nonfinite].data_ptr()
            if case.entry == bc.HOST:
                got_level = ctx.gauss_blur(bc.volume(dims, case.nonfinite), case.sigma)
            elif case.entry == bc.LEVEL:
                ctx.gauss_blur_dev(src, d_out.data_ptr(), nx, ny, nz, case.sigma)
            elif case.entry == bc.HALF:
                assert ctx.gauss_blur_dog_half_dev(src, d_out.data_ptr(), d_dog.data_ptr(), d_half.data_ptr(), nx, ny, nz, case.sigma), \
                    "%s: the launch did not carry the half-size volume" % bc.describe(case)
            else:
                ctx.gauss_blur_dog_dev(src, d_out.data_ptr() if has_out else 0, d_dog.data_ptr(), nx, ny, nz, case.sigma)
            ctx.sync()
            log = ctx.launch_log()
            if case.entry != bc.HOST:
                got_level = d_out.cpu().numpy()
            if has_out:
                hold(got_level, level, case, "the level")
            else:
                assert (got_level == SENTINEL).all(), bc.describe(case)
            if has_dog:
                hold(d_dog.cpu().numpy(), dog, case, "the DoG")
            else:
                assert (d_dog.cpu().numpy() == SENTINEL).all(), bc.describe(case)
            if case.entry == bc.HALF:
                hold(d_half.cpu().numpy(), oracle.subsample(level), case, "the half-size volume")
            else:
                assert (d_half.cpu().numpy() == SENTINEL).all(), bc.describe(case)
            # the kernels that ran
            assert (log["ntaps"] == ntaps).all() and (log["nvox"] == nx * ny * nz).all(), (bc.describe(case), log)
            if case.fused:
                assert log["stage"].tolist() == [stage["blur_fused"]], (bc.describe(case), log["stage"])
            else:
                assert log["stage"].tolist() == [stage["blur_x"], stage["blur_y"], stage["blur_z_dog"]], (bc.describe(case), log["stage"])


@pytest.mark.parametrize("dims,seed", bc.PIPELINE_CASES)
def test_pipeline_with_a_first_blur_of_three_taps(built, oracle, dims, seed):
    """initial_image_scale 0.33 makes the pipeline's own first blur one of 3 taps: at 2^18 voxels the fused 3-tap level-only launch,
    below it three passes over rows padded to whole vectors.  Candidates equal in every field, records byte for byte."""
    vol = built.synth_blobs(*dims, seed=seed)
    nx, ny, nz = dims
    xp = -(-nx // 4) * 4
    with built.Context(*dims) as ctx:
        ctx.set_volume(vol)
        ctx.enable_timing(True)
        cands = ctx.detect(initial_image_scale=bc.PIPELINE_SCALE)
        log = ctx.launch_log()
        recs = ctx.extract(initial_image_scale=bc.PIPELINE_SCALE)
    first = ["blur_fused"] if nx * ny * nz >= 2 ** 18 else ["blur_x", "blur_y", "blur_z_dog"]
    assert [built.STAGES[s] for s in log["stage"][:len(first)]] == first
    assert (log["ntaps"][:len(first)] == 3).all() and (log["nvox"][:len(first)] == xp * ny * nz).all()
    want = oracle.candidates(vol, init_scale=bc.PIPELINE_SCALE)
    assert len(cands) == len(want) >= 20
    for f in ("octave", "level", "is_max", "x", "y", "z"):
        assert (cands[f] == want[f]).all(), f
    for f in ("value", "h_value", "l_value"):
        assert (pc.bits(cands[f]) == pc.bits(want[f])).all(), f
    want_recs, _ = oracle.extract(vol, init_scale=bc.PIPELINE_SCALE)
    assert len(recs) == len(want_recs) > 0
    for f in ("info", "desc", "x", "y", "z", "scale", "ori", "eigs"):
        assert recs[f].tobytes() == want_recs[f].tobytes(), f
    assert recs.tobytes() == want_recs.tobytes()
