"""GPU suite: the device-pointer entry points on a caller's stream (sift3d_set_stream), held to the CPU oracle.

include/sift3d.h promises two ways of ordering device buffers handed to the *_dev entry points.  While the context runs on
its own stream every call is fenced against the legacy default stream; test_gpu_parity.py covers that mode for the blur,
subsample, extrema-append and describe calls, and test_volume_from_the_device_is_fenced here adds sift3d_set_volume_dev.
A caller on another stream hands that stream over with sift3d_set_stream: the context then runs ON it, the fences are
skipped and stream order alone protects the caller's buffers -- although the pipeline itself fans out over side streams
(extrema, per-keypoint stage) that must wait for, and be waited for by, the caller's stream.  That second mode is what the
rest of this module pins.

Every ordering test has the shape of test_dev_entry_points_are_ordered_with_the_default_stream, moved onto a stream S the
test made itself (hipStreamCreateWithFlags through ctypes: non-blocking, so nothing orders it with the default stream; a
torch.cuda.Stream() is a blocking stream on ROCm and would hide a missing dependency): outputs filled with NaN on S, S kept
busy ahead of the producer, the producer queued on S, the library called with no synchronisation, the outputs cloned on S,
the input overwritten on S straight away, and only then the clones read back -- while the default stream carries unrelated
work nothing orders S against.  Expected values come from the CPU oracle and are compared bit for bit.

A race is timing-dependent: these tests cannot prove the absence of one.  What they can detect was measured once on an
MI355X with the core sequence of the first test (blur, blur + DoG, subsample) and the context deliberately left on its own
stream (producer and consumers on S, no sift3d_set_stream, so nothing orders the two): wrong in 11 of 12 calls, every output
of such a call stale.  test_sync_waits_for_the_callers_stream is the one assertion here that does not depend on timing.
"""
import contextlib
import importlib

import numpy as np
import pytest

import image_like as il
from _helpers import caller_stream, hip_memcpy_to_host
from resample_cases import ResampleOracle, about_centre, rot

pytestmark = pytest.mark.gpu

SIGMA11 = 1.9465880393981934          # 11 taps: the filter of the pyramid's level 3, the one that can carry the half-size volume
OP_DIMS = (96, 80, 72)                # (nx, ny, nz), nx % 8 == 0
OP_DIMS_ODD = (92, 40, 36)            # nx % 8 != 0: the half-size volume takes a subsample launch of its own
WINDOW = (20, 41)                     # one interior window of output planes
RES_OUT = (37, 45, 53)                # (oz, oy, ox) of the warp
JUNK = (64, 1024, 1024)               # 256 MB: the size the default-stream tests keep their stream busy with

# (nx, ny, nz), synth_blobs seed: rows that are not whole 16-byte vectors (pitched copy, pad columns cleared), a smaller dense
# shape, and the first shape again with another volume (the geometry changed in between: cleared again).  Seeds chosen on the
# CPU so that the oracle finds at least 30 records in each (54, 45, 40).
VOLUMES = [((61, 56, 48), 17), ((64, 48, 40), 3), ((61, 56, 48), 21)]
NAN_DIMS, NAN_SEED = (88, 72, 64), 11     # image_like.nan_voxels: 82 records, none with a NaN field
CTX_DIMS = (88, 72, 64)                   # one context for all of them
SLAB_DIMS, SLAB_SEED = (96, 88, 80), 21


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def scaled(base, k):
    """what the producer `d_in.copy_(d_base * (1 + k) + k)` leaves in d_in, in float32 like torch"""
    return (base * np.float32(1 + k) + np.float32(k)).astype(np.float32)


def on(torch, S):
    """queue on the caller's stream S; S None: on the default stream"""
    return contextlib.nullcontext() if S is None else torch.cuda.stream(S.torch)


def same_records(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    if got.tobytes() != want.tobytes():
        bad = [f for f in want.dtype.names if got[f].tobytes() != want[f].tobytes()]
        raise AssertionError("%r: records differ from the expected bytes in %s" % (what, bad))


def finite_timings(ctx):
    """timings and the launch log: finite and non-negative, never judged"""
    tm, log = ctx.timings(), ctx.launch_log()
    vals = [tm["total_ms"]] + [st[f] for st in tm["stages"].values() for f in ("ms", "launches", "alg_bytes")]
    vals += log["ms"].tolist() + log["start_ms"].tolist() + log["alg_bytes"].tolist()
    assert np.isfinite(vals).all() and min(vals) >= 0.0, vals
    return tm, log


@pytest.fixture(scope="module")
def rorc(tmp_path_factory):
    return ResampleOracle(tmp_path_factory.mktemp("resample_oracle"))


@pytest.fixture(scope="module")
def op_map():
    """an oblique map, output voxel -> source voxel, that also leaves the source (fill) at the corners"""
    nx, ny, nz = OP_DIMS
    return about_centre(2.1 * rot((1, 2, 3), 20.0), (nz, ny, nx), RES_OUT, (0.7, -1.3, 2.1))


@pytest.fixture(scope="module")
def op_want(built, oracle, rorc, op_map):
    """the oracle's outputs of every operator call of the first test, for the four inputs of its rounds; computed once"""
    base = built.synth_blobs(*OP_DIMS, seed=8)
    want = {}
    for k in range(4):
        v = scaled(base, k)
        b = oracle.blur(v, SIGMA11)
        want[k] = {"level": b, "dog": oracle.dog(v, b), "half": oracle.subsample(b),
                   "linear": rorc.resample(v, RES_OUT, op_map, "linear", -7.0),
                   "nearest": rorc.resample(v, RES_OUT, op_map, "nearest", -7.0)}
    return base, want


@pytest.fixture(scope="module")
def odd_want(built, oracle):
    base = built.synth_blobs(*OP_DIMS_ODD, seed=9)
    want = {}
    for k in range(4):
        v = scaled(base, k)
        b = oracle.blur(v, SIGMA11)
        want[k] = {"level": b, "dog": oracle.dog(v, b), "half": oracle.subsample(b)}
    return base, want


@pytest.fixture(scope="module")
def vol_want(built, oracle):
    """[(dims, volume, the oracle's records)] of VOLUMES, then the NaN-voxel volume"""
    out = []
    for dims, seed in VOLUMES:
        v = built.synth_blobs(*dims, seed=seed)
        out.append((dims, v, oracle.extract(v)[0]))
    v = il.nan_voxels(built.synth_blobs(*NAN_DIMS, seed=NAN_SEED), seed=NAN_SEED)
    out.append((NAN_DIMS, v, oracle.extract(v)[0]))
    return out


def blur_rounds(torch, ctx, S, t, want, ks, rounds=1):
    """The ordering round with the blur alone, on the caller's stream S (or, S None, on the default stream with the context
    fenced against it): t = device tensors base, in, out, junk."""
    nz, ny, nx = t["base"].shape
    for rnd in range(rounds):
        for k in ks:
            with on(torch, S):
                t["out"].fill_(float("nan"))
                for _ in range(3):
                    t["junk"].normal_()
                t["in"].copy_(t["base"] * float(1 + k) + float(k))
                ctx.gauss_blur_dev(t["in"].data_ptr(), t["out"].data_ptr(), nx, ny, nz, SIGMA11)
                got = t["out"].clone()
                t["in"].fill_(-1.0)
                assert (bits(got.cpu().numpy()) == bits(want[k]["level"])).all(), (rnd, k)


# ---- 1: the operator entry points on the caller's stream ---------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, 2], ids=["three_pass", "fused"])
@pytest.mark.parametrize("flags", [1, 0], ids=["nonblocking", "blocking"])
def test_operator_entry_points_on_the_callers_stream(built, op_want, odd_want, op_map, flags, fused):
    """gauss_blur_dev, gauss_blur_dog_dev, gauss_blur_dog_half_dev, gauss_blur_dog_window_dev, dog_dev, subsample2_dev and
    resample_affine_dev after sift3d_set_stream(S): producer, calls and consumers all on S with no synchronisation anywhere,
    three rounds over four inputs, every output the oracle's bits.  Through the three-pass blur (the default at this size:
    it goes through the context's two intermediates) and through the one-launch kernel (TUNE_BLUR_FUSED 2, two rows per
    thread), where the launch carries the half-size volume when nx % 8 == 0 and a subsample launch follows when it is not:
    in_one_launch must tell the two apart.  On a non-blocking stream and on a blocking one (the contract names no flag).

    Measured once with the context left on its own stream and the rest as here (non-blocking S, three-pass; the blur, the
    blur + DoG and the subsample call): wrong in 11 of 12 calls -- the sequence does see a missing dependency.  It remains
    timing-dependent: a pass is no proof."""
    import torch
    base, want = op_want
    nx, ny, nz = OP_DIMS
    lo, hi = WINDOW
    names = ("blur", "level", "dog", "h_level", "h_dog", "h_half", "w_level", "w_dog", "dog2", "half", "linear", "nearest")
    with caller_stream(flags) as S, built.Context(*OP_DIMS) as ctx:
        ctx.set_tuning(built.TUNE_BLUR_FUSED, fused)
        ctx.set_tuning(built.TUNE_FUSED_ROWS, 2 if fused == 2 else 0)
        d_base = torch.from_numpy(base).cuda()
        d_in = torch.empty_like(d_base)
        shape_of = {"h_half": (nz // 2, ny // 2, nx // 2), "half": (nz // 2, ny // 2, nx // 2), "linear": RES_OUT, "nearest": RES_OUT}
        o = {n: torch.empty(shape_of.get(n, (nz, ny, nx)), dtype=torch.float32, device="cuda") for n in names}
        junk = torch.empty(JUNK, dtype=torch.float32, device="cuda")
        other = torch.empty(JUNK, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()                   # the set-up above ran on the default stream: done before S starts
        ctx.set_stream(S.handle)
        assert ctx.blur_window_supported(nx, ny, SIGMA11)
        for rnd in range(3):
            for k in range(4):
                other.normal_()                    # the default stream's own work: nothing orders S against it
                with torch.cuda.stream(S.torch):
                    for t in o.values():
                        t.fill_(float("nan"))
                    for _ in range(3):
                        junk.normal_()             # S is busy ahead of the producer
                    d_in.copy_(d_base * float(1 + k) + float(k))          # producer: queued, not finished
                    p = d_in.data_ptr()
                    ctx.gauss_blur_dev(p, o["blur"].data_ptr(), nx, ny, nz, SIGMA11)
                    ctx.gauss_blur_dog_dev(p, o["level"].data_ptr(), o["dog"].data_ptr(), nx, ny, nz, SIGMA11)
                    one = ctx.gauss_blur_dog_half_dev(p, o["h_level"].data_ptr(), o["h_dog"].data_ptr(), o["h_half"].data_ptr(),
                                                      nx, ny, nz, SIGMA11)
                    ctx.gauss_blur_dog_window_dev(p, o["w_level"].data_ptr(), o["w_dog"].data_ptr(), nx, ny, nz, lo, hi, SIGMA11)
                    ctx.dog_dev(p, o["level"].data_ptr(), o["dog2"].data_ptr(), nx * ny * nz)   # reads what the call before last wrote
                    ctx.subsample2_dev(o["level"].data_ptr(), nx, ny, nz, o["half"].data_ptr())
                    ctx.resample_affine_dev(p, (nz, ny, nx), o["linear"].data_ptr(), RES_OUT, op_map, "linear", -7.0)
                    ctx.resample_affine_dev(p, (nz, ny, nx), o["nearest"].data_ptr(), RES_OUT, op_map, "nearest", -7.0)
                    got = {n: o[n].clone() for n in names}                # consumers on S, no ctx.sync()
                    d_in.fill_(-1.0)                                      # and the input is overwritten straight away
                    got = {n: g.cpu().numpy() for n, g in got.items()}
                assert one == (fused == 2), (rnd, k)
                w = want[k]
                for n, key in (("blur", "level"), ("level", "level"), ("dog", "dog"), ("h_level", "level"), ("h_dog", "dog"),
                               ("h_half", "half"), ("dog2", "dog"), ("half", "half"), ("linear", "linear"), ("nearest", "nearest")):
                    assert (bits(got[n]) == bits(w[key])).all(), (rnd, k, n)
                for n, key in (("w_level", "level"), ("w_dog", "dog")):
                    assert (bits(got[n][lo:hi]) == bits(w[key][lo:hi])).all(), (rnd, k, n)
                    assert np.isnan(got[n][:lo]).all() and np.isnan(got[n][hi:]).all(), (rnd, k, n)   # planes outside the window keep the fill
        # rows of nx % 8 != 0: the launch cannot carry the half-size volume, a subsample launch follows on the same stream
        obase, owant = odd_want
        ox, oy, oz = OP_DIMS_ODD
        with torch.cuda.stream(S.torch):
            e_base = torch.from_numpy(obase).cuda()
            e_in, e_lvl, e_dog = torch.empty_like(e_base), torch.empty_like(e_base), torch.empty_like(e_base)
            e_half = torch.empty((oz // 2, oy // 2, ox // 2), dtype=torch.float32, device="cuda")
        for k in range(4):
            other.normal_()
            with torch.cuda.stream(S.torch):
                for t in (e_lvl, e_dog, e_half):
                    t.fill_(float("nan"))
                for _ in range(3):
                    junk.normal_()
                e_in.copy_(e_base * float(1 + k) + float(k))
                one = ctx.gauss_blur_dog_half_dev(e_in.data_ptr(), e_lvl.data_ptr(), e_dog.data_ptr(), e_half.data_ptr(), ox, oy, oz, SIGMA11)
                got = (e_lvl.clone(), e_dog.clone(), e_half.clone())
                e_in.fill_(-1.0)
                got = [g.cpu().numpy() for g in got]
            assert one is False, k
            for g, key in zip(got, ("level", "dog", "half")):
                assert (bits(g) == bits(owant[k][key])).all(), (k, key)
        torch.cuda.synchronize()


def test_sync_waits_for_the_callers_stream(built):
    """The guard that does not depend on timing: after sift3d_set_stream(S), sift3d_sync waits for S.  Three fills of 256 MB
    and a final fill of a small tensor are queued on S; after ctx.sync() a plain hipMemcpy -- which no torch stream orders --
    must read the final value."""
    import torch
    with caller_stream(1) as S, built.Context(32, 32, 32) as ctx:
        junk = torch.empty(JUNK, dtype=torch.float32, device="cuda")
        small = torch.zeros(64, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.set_stream(S.handle)
        with torch.cuda.stream(S.torch):
            for _ in range(3):
                junk.normal_()
            small.fill_(5.0)
        ctx.sync()
        host = np.zeros(64, np.float32)
        hip_memcpy_to_host(host, small.data_ptr(), host.nbytes)
        assert (host == 5.0).all(), host
        assert S.idle()
        torch.cuda.synchronize()


# ---- 2, 3: sift3d_set_volume_dev + extraction --------------------------------------------------------------------------
def volumes_through_one_context(torch, built, ctx, S, vol_want, copy=True, timed=False, kp_launches=None):
    """Every volume of vol_want through ctx from ONE device buffer: produced behind junk work by queued torch kernels, handed to
    set_volume_dev with no synchronisation, overwritten right after the call returns -- all on the caller's stream S, or (S None)
    on the default stream with the context fenced against it.  The records must be the oracle's bytes."""
    d_src = [torch.from_numpy(v).cuda() for _, v, _ in vol_want]
    d_buf = torch.empty(max(v.size for _, v, _ in vol_want), dtype=torch.float32, device="cuda")
    junk = torch.empty(JUNK, dtype=torch.float32, device="cuda")
    other = torch.empty(JUNK, dtype=torch.float32, device="cuda") if S is not None else None
    torch.cuda.synchronize()
    for i, ((nx, ny, nz), v, want) in enumerate(vol_want):
        assert len(want) >= 30, (i, len(want))
        if other is not None:
            other.normal_()                        # the default stream's own work
        with on(torch, S):
            d_vol = d_buf[:v.size].view(nz, ny, nx)
            d_buf.fill_(float("nan"))
            for _ in range(3):
                junk.normal_()
            d_vol.copy_(d_src[i] * 1.0)            # producer: queued, not finished
            ctx.set_volume_dev(d_vol.data_ptr(), nx, ny, nz)
            d_vol.fill_(-1.0)                      # the caller's volume is overwritten as soon as the call has returned
            for _ in range(3):
                junk.normal_()                     # set_volume_dev ends with a read-back: the stream is busy again when the pyramid is
                                                   # queued behind this, and the pipeline's idle side streams could run ahead of it
        got = ctx.extract(copy=copy)
        same_records(got, want, (i, (nx, ny, nz)))   # (a view of the pinned buffer: read before the next call)
        tm = ctx.timings()
        assert tm["n_octaves"] >= 3 and tm["n_records"] == len(want)   # three octaves: the split candidate list applies
        if kp_launches is not None:
            assert tm["stages"]["keypoint"]["launches"] == kp_launches, i
        if timed:
            assert len(finite_timings(ctx)[1]) > 0
    torch.cuda.synchronize()


def test_volume_from_the_device_is_fenced(built, vol_want):
    """sift3d_set_volume_dev with the context on its own stream and the caller on the default stream (the fenced mode; the call
    test_dev_entry_points_are_ordered_with_the_default_stream leaves out): a pitched shape (hipMemcpy2DAsync, pad columns
    cleared), a smaller dense one, the pitched shape again with another volume, and a volume with NaN voxels, whose scan on the
    device must select the strict first extrema pass -- through one context, each volume still being produced when the call is
    made and overwritten when it returns.  The records are the oracle's bytes and those of sift3d_set_volume of the host array
    on a second context."""
    import torch
    with built.Context(*CTX_DIMS) as ctx:
        volumes_through_one_context(torch, built, ctx, None, vol_want)
    with built.Context(*CTX_DIMS) as host_ctx:
        for dims, v, want in vol_want:
            host_ctx.set_volume(v)
            same_records(host_ctx.extract(), want, ("host", dims))


SETTINGS = {"default": {}, "kp_chunks_3": {"tune": [("TUNE_KP_CHUNKS", 3)]}, "one_list": {"tune": [("TUNE_SPLIT_TAIL", 0)]},
            "split_tail": {"tune": [("TUNE_SPLIT_TAIL", 1)]}, "timing_1": {"timing": 1}, "timing_2": {"timing": 2}, "timing_3": {"timing": 3}}


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_volume_from_the_device_on_the_callers_stream(built, vol_want, setting):
    """The same sequence after sift3d_set_stream(S), producer and overwrite on S, the records read from the view of the pinned
    buffer (extract(copy=False)).  The pipeline leaves S for its side streams: the extrema passes (ex_stream, ex_stream2), and
    the per-keypoint stage in three chunks (descriptor launches on kp_stream beside the main stream), with the candidate list
    in one part and in two (the first part's keypoint kernel on kp_stream while S still builds the coarse octaves), and with
    every launch bracketed by events recorded on the caller's stream (timing modes 1 - 3).  The same bytes under every
    setting: the oracle's.

    Tried once against a build whose extrema streams did not wait for the event recorded on the main stream: every setting
    here failed except timing_3 (which keeps the extrema on the main stream), while test_gpu_parity.py::test_pipeline_records
    passed -- there the main stream is idle when the pyramid is queued and the side streams cannot get ahead of it."""
    import torch
    s = SETTINGS[setting]
    with caller_stream(1) as S, built.Context(*CTX_DIMS) as ctx:
        for knob, value in s.get("tune", ()):
            ctx.set_tuning(getattr(built, knob), value)
        ctx.set_stream(S.handle)
        if "timing" in s:
            ctx.enable_timing(s["timing"])
        volumes_through_one_context(torch, built, ctx, S, vol_want, copy=False, timed="timing" in s,
                                    kp_launches=3 if setting == "kp_chunks_3" else None)


# ---- 4: the slab building blocks on the caller's stream ---------------------------------------------------------------
@pytest.fixture(scope="module")
def slab_want(built, oracle):
    """The first octave of the single-context extraction, which is what the oracle extracts from that octave: records are
    octave-major, so it is the leading part of the oracle's list, and it ends where the oracle's octave-0 candidates end."""
    vol = built.synth_blobs(*SLAB_DIMS, seed=SLAB_SEED)
    with built.Context(*SLAB_DIMS) as ctx:
        ctx.set_volume(vol)
        ctx.set_max_octaves(1)
        want = ctx.extract()
        n_extrema = ctx.timings()["n_extrema"]
    full = oracle.extract(vol)[0]
    cand = oracle.candidates(vol)
    assert 100 < len(want) < len(full) and want.tobytes() == full[:len(want)].tobytes()
    assert n_extrema == int((cand["octave"] == 0).sum()) < len(cand)
    return vol, want


@pytest.mark.parametrize("lazy", [False, True], ids=["stored", "lazy"])
def test_slab_building_blocks_on_the_callers_stream(built, slab_want, lazy):
    """test_slab_entry_points_are_ordered_with_the_default_stream run entirely on S: blur chain, candidates_reset,
    extrema_append_dev / _append_lazy_dev, describe_dev, the levels produced by queued work on S, the DoG levels only the
    appends read overwritten on S right after them.  Then the per-keypoint stage in two parts (describe_dev_counts +
    describe_dev_place) into a list shared with an imaginary rank in front, at made-up shifts.  Expected: the first octave of
    the single-context extraction, byte for byte (slab_want holds that to the oracle)."""
    import torch
    zs = importlib.import_module("3d_sift_cuda_amd.zslab")
    vol, want = slab_want
    nx, ny, nz = SLAB_DIMS
    extra0, extras, sig = zs.sigma_schedule(1.0)
    with caller_stream(1) as S, built.Context(nx, ny, nz, slab=True) as ctx:
        d_vol = torch.from_numpy(vol).cuda()
        junk = torch.empty(JUNK, dtype=torch.float32, device="cuda")
        other = torch.empty(JUNK, dtype=torch.float32, device="cuda")
        L = [torch.empty_like(d_vol) for _ in range(6)]
        D = [torch.empty_like(d_vol) for _ in range(5)]
        torch.cuda.synchronize()
        ctx.set_stream(S.handle)
        levels = [{"img": L[l + 1].data_ptr(), "dogc": D[l + 1].data_ptr(), "nx": nx, "ny": ny, "nz_local": nz,
                   "nz_global": nz, "z_offset": 0, "sigma_h": sig[l], "sigma_c": sig[l + 1], "sigma_l": sig[l + 2],
                   "octave_factor": 1.0} for l in range(3)]

        def pyramid_and_appends():
            """queued on S, which is busy ahead of everything; the input itself is still being produced"""
            for t in L + D:
                t.fill_(float("nan"))
            for _ in range(3):
                junk.normal_()
            src = d_vol * 1.0
            ctx.gauss_blur_dev(src.data_ptr(), L[0].data_ptr(), nx, ny, nz, extra0)
            for j in range(1, 6):
                ctx.gauss_blur_dog_dev(L[j - 1].data_ptr(), L[j].data_ptr(), D[j - 1].data_ptr(), nx, ny, nz, extras[j - 1])
            ctx.candidates_reset()
            if lazy:
                assert ctx.lazy_levels_supported(nx, ny, nz, extras[4])
                ctx.extrema_append_lazy_dev(0, L[0].data_ptr(), L[1].data_ptr(), D[1].data_ptr(), D[2].data_ptr(), 0, 0.0,
                                            nx, ny, nz, 0, 0, nz)
                ctx.extrema_append_dev(D[1].data_ptr(), D[2].data_ptr(), D[3].data_ptr(), nx, ny, nz, 1, 0, nz)
                ctx.extrema_append_lazy_dev(D[2].data_ptr(), 0, 0, D[3].data_ptr(), 0, L[4].data_ptr(), extras[4],
                                            nx, ny, nz, 2, 0, nz)
            else:
                for l in range(3):
                    ctx.extrema_append_dev(D[l].data_ptr(), D[l + 1].data_ptr(), D[l + 2].data_ptr(), nx, ny, nz, l, 0, nz)
            D[0].fill_(-7.0); D[4].fill_(7.0); L[5].fill_(0.0)            # nothing after the appends reads them
            if not lazy:
                L[0].fill_(3.0)
            return src

        wgrp = None
        for rnd in range(3):
            other.normal_()                                              # the default stream's own work
            with torch.cuda.stream(S.torch):
                src = pyramid_and_appends()
                got, grp = ctx.describe_dev(levels)
            assert got.tobytes() == want.tobytes(), (lazy, rnd)
            wgrp = grp
        # the stage in two parts, the records placed in a list this context shares with a rank in front of it
        other.normal_()
        with torch.cuda.stream(S.torch):
            src = pyramid_and_appends()
            counts, n = ctx.describe_dev_counts(levels)
        assert n == len(want) and (counts == np.bincount(wgrp, minlength=built.GROUPS)).all()
        rng = np.random.default_rng(1)
        front = np.where(counts > 0, rng.integers(0, 7, built.GROUPS), 0).astype(np.int32)
        shift1, total = zs.placed_shifts(np.stack([front, counts]), 1)
        assert total == n + int(front.sum())
        lst = np.zeros(total + 5, built.FEATURE_DTYPE)
        lst["scale"] = -1.0                                              # what nobody stores stays as it is
        built.host_register(lst.ctypes.data, lst.nbytes)
        try:
            assert ctx.describe_dev_place(lst.ctypes.data, shift1) == n
            at, pos, mine = 0, 0, np.zeros(total + 5, bool)
            for g in range(built.GROUPS):
                pos += int(front[g])                                     # the other rank's run of the group comes first
                k = int(counts[g])
                assert lst[pos:pos + k].tobytes() == want[at:at + k].tobytes(), g
                mine[pos:pos + k] = True
                pos += k; at += k
            assert at == n and (lst["scale"][~mine] == -1.0).all()
        finally:
            torch.cuda.synchronize()
            built.host_unregister(lst.ctypes.data)
        del src


# ---- 5: moving between streams ----------------------------------------------------------------------------------------
def test_moving_between_streams(built, op_want):
    """One context: its own stream -> S1 -> its own -> S2 -> S2 again -> its own.  After every move one ordering round of the
    blur: on the caller's stream while the context runs on it, and in the fenced default-stream form whenever it is back on a
    stream of its own (own_stream, and with it the fences, must have come back).  sift3d_set_stream with work still queued on
    the old stream must not lose it.  After the context is closed S1 and S2 are still the caller's: the library destroys only
    a stream it owns."""
    import torch
    base, want = op_want
    nx, ny, nz = OP_DIMS
    with caller_stream(1) as S1, caller_stream(1) as S2:
        ctx = built.Context(*OP_DIMS)
        try:
            t = {"base": torch.from_numpy(base).cuda()}
            t["in"], t["out"] = torch.empty_like(t["base"]), torch.empty_like(t["base"])
            t["junk"] = torch.empty(JUNK, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            blur_rounds(torch, ctx, None, t, want, (0, 1))
            for step, S in enumerate((S1, None, S2, S2, None)):
                ctx.set_stream(S.handle if S is not None else 0)
                torch.cuda.synchronize()       # the caller changes streams: what it queued on the old one is done
                blur_rounds(torch, ctx, S, t, want, ((step + 2) % 4, (step + 3) % 4))
            # work queued on the context's own stream, and the stream changed at once
            torch.cuda.synchronize()
            t["in"].copy_(t["base"] * 3.0 + 2.0)
            t["out"].fill_(float("nan"))
            ctx.gauss_blur_dev(t["in"].data_ptr(), t["out"].data_ptr(), nx, ny, nz, SIGMA11)
            ctx.set_stream(S1.handle)
            torch.cuda.synchronize()
            assert (bits(t["out"].cpu().numpy()) == bits(want[2]["level"])).all()
        finally:
            ctx.close()
        for S in (S1, S2):
            with torch.cuda.stream(S.torch):
                probe = torch.zeros(1024, dtype=torch.float32, device="cuda")
                probe.fill_(9.0)
                S.torch.synchronize()
                assert float(probe.sum().item()) == 9.0 * 1024
            assert S.idle()                    # hipStreamQuery: hipSuccess, the handle is still a stream
        torch.cuda.synchronize()


# ---- 6: what sift3d_set_volume_dev refuses ----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["own_stream", "callers_stream"])
def test_volume_from_the_device_refusals(built, oracle, vol_want, mode):
    """A null pointer, nz <= 1, a shape beyond the context and a slab context: each an error with the library's text, each
    leaving the context usable -- the next good call gives the oracle's bytes."""
    import torch
    (nx, ny, nz), v, want = vol_want[1]
    with (caller_stream(1) if mode == "callers_stream" else contextlib.nullcontext()) as S:
        d_vol = torch.from_numpy(v).cuda()
        torch.cuda.synchronize()
        with built.Context(nx, ny, nz) as ctx:
            if S is not None:
                ctx.set_stream(S.handle)
            for args, text in (((0, nx, ny, nz), "null volume"), ((d_vol.data_ptr(), nx, ny, 1), "z <= 1"),
                               ((d_vol.data_ptr(), nx, ny, 0), "does not fit"), ((d_vol.data_ptr(), nx + 4, ny, nz), "does not fit"),
                               ((d_vol.data_ptr(), nz, ny, 2 * nx), "does not fit")):
                with pytest.raises(built.Sift3DError, match=text):
                    ctx.set_volume_dev(*args)
                with on(torch, S):
                    ctx.set_volume_dev(d_vol.data_ptr(), nx, ny, nz)
                same_records(ctx.extract(), want, args[1:])
        with built.Context(nx, ny, nz, slab=True) as ctx:
            if S is not None:
                ctx.set_stream(S.handle)
            with pytest.raises(built.Sift3DError, match="needs a full context"):
                ctx.set_volume_dev(d_vol.data_ptr(), nx, ny, nz)
            with on(torch, S):
                d_out = torch.empty_like(d_vol)
                ctx.gauss_blur_dev(d_vol.data_ptr(), d_out.data_ptr(), nx, ny, nz, SIGMA11)
                got = d_out.clone().cpu().numpy()
            assert (bits(got) == bits(oracle.blur(v, SIGMA11))).all()
        torch.cuda.synchronize()
