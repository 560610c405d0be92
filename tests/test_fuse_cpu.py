"""CPU suite: multi-atlas label fusion by locally weighted voting without a GPU -- the oracle
tests/fuse_oracle.c against a numpy restatement of the patch sums and against its own contract (identical atlases, gain and
offset, ties, flat patches, unlabelled voxels, no voter), the product's host helpers against the oracle and at their bounds, the
host file under the sanitizers as a stand-alone program, and the five-atlas scenario."""
import os
import re
import subprocess

import numpy as np
import pytest

from field_cases import FieldOracle
from blockmatch_cases import lattice_numpy
from blockmatch_ncc_cases import NccOracle
from fuse_cases import (ENDS, ENDS_SHAPE, FALLBACK, NONE, SUM_MAX_B6, U_ONE, ZERO_SHIFT_SHAPE, FuseOracle, assert_zero_shift_identity, cpu_fuse, ends_volumes,
                        fused_labels, leg, mean_dice, pair, scenario)
from resample_cases import ResampleOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fz(tmp_path_factory):
    return FuseOracle(tmp_path_factory.mktemp("fuse_oracle"))


@pytest.fixture(scope="module")
def ro(tmp_path_factory):
    return ResampleOracle(tmp_path_factory.mktemp("resample_oracle"))


@pytest.fixture(scope="module")
def fo(tmp_path_factory):
    return FieldOracle(tmp_path_factory.mktemp("field_oracle"))


@pytest.fixture(scope="module")
def scen(built, ro, tmp_path_factory):
    return scenario(built, ro, tmp_path_factory.mktemp("fuse_scenario"))


def sums_numpy(qt, qw, b):
    """the six sums of every voxel with numpy: zero padding and one shifted slice per patch offset"""
    qt, qw = np.asarray(qt, np.int64), np.asarray(qw, np.int64)
    ok = (qt >= 0) & (qw >= 0)
    f, w = np.where(ok, qt, 0), np.where(ok, qw, 0)
    terms = [np.pad(t, b) for t in (ok.astype(np.int64), f, f * f, w, w * w, f * w)]
    nz, ny, nx = qt.shape
    out = np.zeros(qt.shape + (6,), np.int64)
    for dz in range(2 * b + 1):
        for dy in range(2 * b + 1):
            for dx in range(2 * b + 1):
                for i, t in enumerate(terms):
                    out[..., i] += t[dz:dz + nz, dy:dy + ny, dx:dx + nx]
    return out


def u_python(metric, n, sf, sff, sw, sww, sfw):
    """the similarity in Python integers and floats (IEEE double, one operation at a time; round() is ties-to-even)"""
    if n <= 0:
        return 0
    if metric == "ssd":
        return (n << 15) // (sff - 2 * sfw + sww + n)
    A, Vf, Vw = n * sfw - sf * sw, n * sff - sf * sf, n * sww - sw * sw
    rho2 = (float(A) * float(A)) / (float(Vf) * float(Vw)) if A > 0 and Vf > 0 and Vw > 0 else 0.0
    return ((1 << 31) - round((1.0 - min(rho2, 1.0)) * 2147483648.0)) >> 16


@pytest.mark.parametrize("metric", ["ssd", "ncc"])
@pytest.mark.parametrize("shape,b,holes,kind", [pytest.param(*c, "pair", id="shape%d-%d-%s" % (i, c[1], c[2])) for i, c in enumerate(
    [((2, 3, 4), 2, False), ((5, 9, 33), 2, False), ((11, 19, 21), 1, True), ((9, 14, 17), 6, True)])] +     # the ids these cases have always had
    [pytest.param(ENDS_SHAPE, b, k == "speckled_holes", k, id="%s-%d" % (k, b)) for k in ENDS for b in (2, 6)])
def test_oracle_equals_numpy(fz, metric, shape, b, holes, kind):
    """kind "pair": fuse_cases.pair.  The others are fuse_cases.ends_volumes on a shape with unclipped patches at b = 6: the restatement's
    sums are int64 and cannot wrap, so it settles the sums and u where they pass 2^31."""
    T, W = pair(shape, 5, holes) if kind == "pair" else ends_volumes(kind, shape, 5)
    qt, qw = fz.quantize(T, *fz.range(T)), fz.quantize(W, *(fz.range(T) if metric == "ssd" else fz.range(W)))
    assert qt.max() == 1023 and qt.min() == (-1 if holes else 0)
    u, sums = fz.weights_q(qt, qw, b, metric, sums=True)
    want = sums_numpy(qt, qw, b)
    assert np.array_equal(sums, want)
    assert sums[..., 0].max() <= (2 * b + 1) ** 3 and sums.max() < 2 ** 32
    flat = want.reshape(-1, 6)
    assert np.array_equal(u.reshape(-1), np.array([u_python(metric, *(int(v) for v in s)) for s in flat], np.uint16))
    if kind == "pair":
        assert u.max() <= U_ONE and 0 < u.max() and len(np.unique(u)) > 1
        return
    # the ends: what test_gpu_integer_ends.py relies on, asserted on the oracle's sums
    D = sums[..., 2] - 2 * sums[..., 5] + sums[..., 4]
    print("%s %s b %d: largest sum %d, D %d .. %d, u %d .. %d" % (kind, metric, b, sums.max(), D.min(), D.max(), u.min(), u.max()))
    assert set(np.unique(qt)) - {-1} == {0, 1023} and set(np.unique(qw)) - {-1} == {0, 1023} and u.max() <= U_ONE
    if b == 6:
        assert 2 ** 31 <= sums.max() <= SUM_MAX_B6 < 2 ** 32
    if kind.startswith("speckled"):
        assert (metric == "ncc" or (u == 0).all()) and (b < 6 or D.max() >= 2 ** 31) and (sums[..., 0].min() < (2 * b + 1) ** 3) and D.max() < 2 ** 32
    if kind == "bright_same":
        assert ((u == U_ONE) | ((u == 0) & (metric == "ncc"))).all() and (u == U_ONE).mean() > 0.9 and (D == 0).all() and (b < 6 or min(sums[..., i].max() for i in (2, 4, 5)) >= 2 ** 31)
    if kind == "bright" and metric == "ncc" and b == 6:   # A, Vf and Vw are small differences of large products, and no patch is flat
        assert ((u > 0) & (u < U_ONE)).mean() > 0.9 and len(np.unique(u)) > 100


def test_weights_equal_the_block_matchers_cost_at_the_zero_shift(fz, tmp_path):
    """The fusion's similarity and the block matcher's cost come from the same sums (patch_cost.h in the product): at an unflagged
    lattice node the patch is whole (n = N = 125 at b = 2) and word 5 is the cost at the zero shift, so u = (2^31 - cost) >> 16
    under NCC and (125 << 15) // (cost + 125) under SSD.  Here between the oracles alone (fuse_oracle.c, blockmatch_oracle.c,
    blockmatch_ncc_oracle.c); test_gpu_fuse.py holds the kernels to the same identity."""
    T, W = pair(ZERO_SHIFT_SHAPE, 5)
    first, count = lattice_numpy(ZERO_SHIFT_SHAPE, 1, 2, 1)
    no = NccOracle(tmp_path)
    for metric, oracle in (("ssd", no.ssd), ("ncc", no)):
        assert_zero_shift_identity(metric, fz.weights(T, W, 2, metric), oracle.match(T, W, first, 1, count, 2, 1), first)


@pytest.mark.parametrize("metric", ["ssd", "ncc"])
def test_identical_atlases_give_their_labels_with_full_confidence(fz, metric):
    T, _ = pair((7, 12, 35), 2)
    labels = (np.arange(T.size).reshape(T.shape) % 7).astype(np.float32)
    u = fz.weights(T, T, 2, metric)
    assert (u == U_ONE).all()
    for power in (0, 1, 2):
        words = fz.vote([u] * 3, [labels] * 3, power)
        assert np.array_equal(words[..., 0], labels.astype(np.uint32) | (3 << 16)) and (words[..., 1] == 65535).all()


@pytest.mark.parametrize("g,o", [(0.5, 0.0), (4.0, -1024.0), (2.0, 512.0)])
def test_gain_and_offset_leave_ncc_alone_and_lower_ssd(fz, g, o):
    """W integer-valued, g and o powers of two: g W + o is exact in float32 and quantises, with its own range, to the same integers"""
    rng = np.random.default_rng(12)
    T, _ = pair((9, 13, 20), 3)
    T = np.rint(T).astype(np.float32)
    W = np.rint(T + rng.normal(0, 12.0, T.shape)).astype(np.float32)
    W[0, 0, 0], W[-1, -1, -1] = T.min(), T.max()           # W keeps T's range: under SSD it is on T's scale exactly
    W2 = (np.float32(g) * W + np.float32(o)).astype(np.float32)
    assert np.array_equal(W2.astype(np.float64), g * W.astype(np.float64) + o)
    a, b = fz.weights(T, W, 2, "ncc"), fz.weights(T, W2, 2, "ncc")
    assert np.array_equal(a, b) and len(np.unique(a)) > 10 and a.min() > 0
    s, s2 = fz.weights(T, W, 2, "ssd"), fz.weights(T, W2, 2, "ssd")
    assert (s2 < s).mean() > 0.9 and s2.astype(np.int64).sum() < 0.5 * s.astype(np.int64).sum() and s.min() > 0


def test_vote_ties_flat_patches_unlabelled_voxels_and_no_voter(fz):
    nan = np.float32(np.nan)
    # five voxels, three atlases: a tie of two labels; a tie of three; weights that overturn the majority; one unlabelled; none labelled
    labels = [np.array([9, 5, 1, 4, nan], np.float32), np.array([3, 65535, 1, nan, nan], np.float32), np.array([3, 7, 2, 4, np.inf], np.float32)]
    u = [np.array([20, 10, 10, 0, 5], np.uint16), np.array([10, 10, 10, 7, 5], np.uint16), np.array([10, 10, 30, 0, 5], np.uint16)]
    w1 = fz.vote(u, labels, 1)
    assert [int(x) & 0xffff for x in w1[:, 0]] == [3, 5, 2, 4, 0]                # 20 = 10 + 10: the smaller label; 10 = 10 = 10: the smallest
    assert [(int(x) >> 16) & 63 for x in w1[:, 0]] == [3, 3, 3, 2, 0]
    assert [int(x) for x in w1[:, 1]] == [65535 * 20 // 40, 65535 * 10 // 30, 65535 * 30 // 50, 65535, 0]
    assert int(w1[4, 0]) == NONE and int(w1[3, 0]) & FALLBACK and not any(int(x) & FALLBACK for x in w1[:3, 0])
    w0 = fz.vote(u, labels, 0)
    assert [int(x) & 0xffff for x in w0[:, 0]] == [3, 5, 1, 4, 0] and not (w0[:, 0] & FALLBACK).any()
    assert [int(x) for x in w0[:, 1]] == [65535 * 2 // 3, 65535 // 3, 65535 * 2 // 3, 65535, 0]
    w2 = fz.vote(u, labels, 2)
    assert [int(x) & 0xffff for x in w2[:, 0]] == [9, 5, 2, 4, 0]                # 400 > 100 + 100
    assert int(w2[0, 1]) == 65535 * 400 // 600 and int(w2[2, 1]) == 65535 * 900 // 1100
    # thirty-two voters of the largest weight: S = 2^35 fits, conf is exact
    words = fz.vote([np.array([U_ONE], np.uint16)] * 32, [np.array([65535], np.float32)] * 32, 2)
    assert int(words[0, 0]) == 65535 | (32 << 16) and int(words[0, 1]) == 65535


def test_flat_patches_under_ncc_fall_back_to_majority(fz):
    T, _ = pair((6, 10, 12), 4)
    T[:, :, :7] = 300.0                                     # every patch of x <= 4 is flat at b = 2
    W = np.roll(T, 1, 1)
    W[:, :, :7] = 120.0
    u = fz.weights(T, W, 2, "ncc")
    assert (u[:, :, :5] == 0).all() and (u[:, :, 8:] > 0).any()
    labels = [np.full(T.shape, 2, np.float32), np.full(T.shape, 2, np.float32), np.full(T.shape, 1, np.float32)]
    words = fz.vote([u, u, u], labels, 2)
    assert ((words[:, :, :5, 0] & FALLBACK) != 0).all() and ((words[:, :, :5, 0] & 0xffff) == 2).all() and (words[:, :, :5, 1] == 65535 * 2 // 3).all()
    assert ((words[..., 0] & FALLBACK) != 0).sum() == int((u == 0).sum())
    # the sum of squared differences has no flat case: equal flat patches are identical ones
    assert (fz.weights(T, T, 2, "ssd") == U_ONE).all()


def test_host_helpers_against_the_oracle_and_at_their_bounds(built, fz):
    N, q = 13 ** 3, 1023
    h = N // 2
    for metric in ("ssd", "ncc"):
        # D = 0 on the widest sums; n = 1; the largest D; n = 0
        assert built.fuse_similarity(metric, N, q * h, q * q * h, q * h, q * q * h, q * q * h) == U_ONE
        assert built.fuse_similarity(metric, 1, 5, 25, 5, 25, 25) == (U_ONE if metric == "ssd" else 0)
        assert built.fuse_similarity(metric, N, q * h, q * q * h, q * (N - h), q * q * (N - h), 0) == 0
        assert built.fuse_similarity(metric, 0, 0, 0, 0, 0, 0) == 0
    assert built.fuse_similarity("ssd", N, 0, 0, N, N, 0) == U_ONE // 2           # one quantisation step everywhere: n 2^15 / (n + n)
    rng = np.random.default_rng(3)
    for _ in range(4000):
        n = int(rng.integers(1, N + 1))
        f, w = rng.integers(0, 1024, n).astype(np.int64), rng.integers(0, 1024, n).astype(np.int64)
        if rng.random() < 0.5:
            w = np.clip(f + rng.integers(-2, 3, n), 0, 1023)
        a = (n, int(f.sum()), int((f * f).sum()), int(w.sum()), int((w * w).sum()), int((f * w).sum()))
        for metric in ("ssd", "ncc"):
            got = built.fuse_similarity(metric, *a)
            assert got == fz.similarity(metric, *a) == u_python(metric, *a) and got <= U_ONE, (metric, a)
    # the overlap
    a = rng.integers(0, 6, (5, 6, 7)).astype(np.float32)
    b = np.where(rng.random(a.shape) < 0.7, a, 65535).astype(np.float32)
    a[0, 0, :3], b[1, 1, :3] = np.nan, np.inf
    labels, ca, cb, cc = built.label_overlap(a, b)
    oa, ob, oc = fz.overlap(a, b)
    assert list(labels) == list(np.nonzero((oa > 0) | (ob > 0))[0]) and 65535 in labels
    assert np.array_equal(ca, oa[labels]) and np.array_equal(cb, ob[labels]) and np.array_equal(cc, oc[labels])
    assert ca.sum() == a.size - 3 and cb.sum() == b.size - 3 and (cc <= np.minimum(ca, cb)).all()
    for bad in (0.5, -1.0, 65536.0):
        with pytest.raises(built.Sift3DError):
            built.label_overlap(a, np.full(a.shape, bad, np.float32))
    p = built.fuse_params()
    assert (p.block, p.metric, p.power, p.fill, p.max_voxels) == (2, 0, 2, 0.0, 1 << 28)


def test_host_file_under_sanitizers(built, fz, tmp_path):
    """fuse_host.c and tests/fuse_host_san.c as one program, with and without -fsanitize=address,undefined: both exit clean and
    print the same lines, and the similarities among them are the oracle's"""
    src = [os.path.join(ROOT, "tests", "fuse_host_san.c"), os.path.join(ROOT, "3d_sift_cuda_amd", "csrc", "fuse_host.c")]
    base = ["cc", "-std=c11", "-ffp-contract=off", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include")]
    out = {}
    for name, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])):
        exe = str(tmp_path / ("fuse_host_" + name))
        subprocess.run(base + flags + ["-o", exe] + src + ["-lm"], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
        out[name] = r.stdout
    assert out["san"] == out["plain"] and "overlap 4\n" in out["san"] and "overlap bad -1\n" in out["san"]
    N, q = 2197, 1023
    h = N // 2
    case1 = (N, q * h, q * q * h, q * h, q * q * h, q * q * h)
    assert "u 1 0 %d\n" % fz.similarity("ssd", *case1) in out["san"] and "u 1 1 %d\n" % fz.similarity("ncc", *case1) in out["san"]
    assert re.search(r"^check bad 0 0$", out["san"], re.M) and "check -1\n" in out["san"]


# The scenario's Dice (mean over the labels 0 .. 4) on the oracle when this was written; DESIGN.md section 7j has the table.
SCENARIO_DICE = {"ssd": {"single": [0.6506, 0.6812, 0.6128, 0.6120, 0.6278], 0: 0.8453, 1: 0.9041, 2: 0.9029},
                 "ncc": {"single": [0.6506, 0.6812, 0.6128, 0.6120, 0.6278], 0: 0.8453, 1: 0.8989, 2: 0.9020}}


@pytest.mark.parametrize("metric", ["ssd", "ncc"])
def test_scenario_weighted_voting_beats_majority_and_every_atlas(built, fz, ro, fo, scen, metric):
    """40^3, five atlases, each misregistered by three voxels in three of the target's five z slabs, a different three each: in
    every slab three of five atlases are wrong.  Under "ncc" every atlas also has its own gain and offset.  Asserted: power 2
    exceeds majority voting (power 0) and every single atlas by at least half the gap measured on the oracle when this was
    written (SCENARIO_DICE); the GPU equals the oracle to the bit (test_gpu_fuse.py), so the same holds there."""
    rec = SCENARIO_DICE[metric]
    atlases = leg(scen, metric)
    dice = {}
    for power in (0, 1, 2):
        words, rep = cpu_fuse(built, fz, ro, fo, scen["target"], atlases, scen["vox2key"], metric=metric, power=power)
        dice[power] = mean_dice(fz, fused_labels(words), scen["truth"])[0]
        assert rep["none"] == 0 and rep["fallback"] == 0 and all(r["voters"] > 0.97 * scen["target"].size for r in rep["atlas"])
    single = [mean_dice(fz, fused_labels(cpu_fuse(built, fz, ro, fo, scen["target"], [a], scen["vox2key"], metric=metric, power=0)[0]), scen["truth"])[0]
              for a in atlases]
    print("fuse scenario %s: single %s power 0 %.4f power 1 %.4f power 2 %.4f" % (metric, " ".join("%.4f" % d for d in single), dice[0], dice[1], dice[2]))
    assert dice[2] >= dice[0] + 0.5 * (rec[2] - rec[0]), (dice, rec)
    assert dice[2] >= max(single) + 0.5 * (rec[2] - max(rec["single"])), (dice, single)
    assert rec[2] - rec[0] > 0.05 and rec[2] - max(rec["single"]) > 0.2
    # a single atlas is only as good as its registration: the three misregistered slabs cost it a third of its overlap
    assert max(single) < 0.7
