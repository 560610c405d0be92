"""CPU suite: the image similarity without a GPU -- the oracle tests/similarity_oracle.c against a numpy
restatement that shares no code with it, the product's host measures (similarity_host.c) against the oracle bit for bit and against
a Python restatement, the hand cases, the registration scenario that the joint histogram is there for, the shape that takes the GPU
kernel past its launch cap, and the host file under the sanitizers as a stand-alone program."""
import math
import os
import subprocess

import numpy as np
import pytest

from blockmatch_cases import volume
from similarity_cases import (BIG, BINS, CAP, COUNT_SHAPES, EXCESS, MEASURES, PAIRS, STRETCH, VPT, SimilarityOracle, bits, count_numpy, holes, kernel_constants,
                              measures_python, pair, rho_rms_python, same_measure)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def so(tmp_path_factory):
    return SimilarityOracle(tmp_path_factory.mktemp("similarity_oracle"))


# ---- the oracle against numpy -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_holes", [False, True], ids=["whole", "holes"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 4), (5, 9, 33)])
def test_oracle_counts_equal_numpy(so, shape, with_holes):
    """n = 1, 24 and 1485 voxels, all four bins, both same_scale settings: the histogram, the six sums and excluded"""
    rng = np.random.default_rng(shape[2])
    A, B = volume("random", shape, 1), (np.float32(0.5) * volume("random", shape, 2) + np.float32(20.0)).astype(np.float32)
    if with_holes:
        A, B = holes(A, rng, 0.2), holes(B, rng, 0.2)
        A.reshape(-1)[0] = np.nan                        # the single voxel is a hole too
    for same_scale in (False, True):
        ra = (np.float32(10.0), np.float32(190.0)) if A.size == 1 else so.range(A)[0]      # one voxel has no range of its own: a given one
        rb = ra if same_scale else ((np.float32(0.0), np.float32(100.0)) if A.size == 1 else so.range(B)[0])
        for bins in BINS:
            hist, sums, excluded, _ = so.count(A, B, ra, rb, bins)
            want = count_numpy(A, B, ra, rb, bins)
            assert np.array_equal(hist, want[0]) and sums == want[1] and excluded == want[2], (bins, same_scale)
            assert hist.sum() == sums[0] == A.size - excluded
    assert not with_holes or excluded > 0


def test_oracle_range_and_quantiser(so):
    v = np.array([np.nan, 2.0, -np.inf, -3.0, np.inf, 2.0], np.float32)
    assert so.range(v) == ((np.float32(-3.0), np.float32(2.0)), True)
    assert so.range(np.full(5, 2.5, np.float32))[1] is False and so.range(np.full(5, np.nan, np.float32))[1] is False
    q = lambda x: so.L.osim_q(x, 0.0, 1023.0)
    assert [q(v) for v in (0.5, 1.5, 2.5, -0.0, -7.0, 1022.5, 1023.0, 5000.0)] == [0, 2, 2, 0, 0, 1022, 1023, 1023]    # ties to even, the ends clamp
    assert [q(v) for v in (math.nan, math.inf, -math.inf)] == [-1, -1, -1]


# ---- the host measures ---------------------------------------------------------------------------------------------------------------
def close(got, want, rel=1e-12):
    return (math.isnan(got) and math.isnan(want)) or abs(got - want) <= rel * max(abs(want), 1e-300)


@pytest.mark.parametrize("kind", PAIRS)
def test_host_measures_equal_the_oracle_and_python(built, so, kind):
    """similarity_host.c against the oracle: equal bits.  Against math.log and big integers: 1e-12 relative -- a sum of at most 4096
    terms each good to 2^-52 is good to 1e-12 with two orders of magnitude to spare.  mi is a difference of entropies and is held to
    1e-12 of their size."""
    A, B = pair(kind, (5, 9, 33))
    for same_scale in (False, True):
        ra = so.range(A)[0]
        rb = ra if same_scale else so.range(B)[0]
        for bins in BINS:
            hist, sums, _, _ = so.count(A, B, ra, rb, bins)
            got = built.similarity_measures(hist, sums, ra[0], ra[1], same_scale)
            want, py = so.measures(hist, sums, ra[0], ra[1], same_scale), measures_python(hist, sums, ra[0], ra[1], same_scale)
            for k in MEASURES:
                assert same_measure(got[k], want[k]), (kind, bins, same_scale, k, got[k], want[k])
            for k in ("nmi", "rho", "rms", "h_a", "h_b", "h_ab"):
                assert close(got[k], py[k]), (kind, bins, same_scale, k, got[k], py[k])
            assert abs(got["mi"] - py["mi"]) <= 1e-12 * max(got["h_a"] + got["h_b"], 1.0)
            assert math.isnan(got["rms"]) == (not same_scale)
    rows = {"one": [1, 5, 9, 25, 81, 45], "line": [3, 6, 12, 14, 56, 28], "anti": [2, 1023, 1023, 1023 * 1023, 1023 * 1023, 0], "none": [0] * 6,
            "wide": [1 << 30, 1023 << 29, 1023 << 29, (1023 * 1023) << 29, (1023 * 1023) << 29, 0]}
    for name, s in rows.items():
        for same_scale in (False, True):
            got, want, py = built.similarity_label_measures(7, s, -2.0, 3.0, same_scale), so.rho_rms(s, -2.0, 3.0, same_scale), rho_rms_python(s, -2.0, 3.0, same_scale)
            assert all(same_measure(g, w) for g, w in zip(got, want)) and all(close(g, p) for g, p in zip(got, py)), (name, got, want, py)
    # three voxels on a line: Va = 6, Vb = 24, and sqrt(6) sqrt(24) is 12 only to the last bit; two opposite voxels: both roots are exact
    assert abs(built.similarity_label_measures(7, rows["line"], 0, 1)[0] - 1.0) < 1e-15 and built.similarity_label_measures(7, rows["anti"], 0, 1)[0] == -1.0
    assert built.similarity_label_measures(7, rows["wide"], 0, 1)[0] == -1.0        # the products reach 2^80: exact in 128 bits


# ---- hand cases ----------------------------------------------------------------------------------------------------------------------
def test_equal_images_fill_the_diagonal(built, so):
    A, _ = pair("equal", (5, 9, 33))
    for bins in BINS:
        r = so.similarity(A, A.copy(), bins=bins)
        assert r["n"] == A.size and np.array_equal(r["hist"], np.diag(np.diag(r["hist"])))
        m = built.similarity_measures(r["hist"], r["sums"])
        assert bits(m["h_a"]) == bits(m["h_b"]) == bits(m["h_ab"]) == bits(m["mi"]) and m["nmi"] == 2.0 and m["h_a"] > 0
        assert all(same_measure(m[k], r[k]) for k in MEASURES) and abs(m["rho"] - 1.0) < 1e-15


def test_product_histogram_has_no_information(built, so):
    for bins in BINS:
        u, v = np.arange(1, bins + 1, dtype=np.int64), np.arange(2, bins + 2, dtype=np.int64)[::-1]
        hist = np.outer(u, v)
        for m in (built.similarity_measures(hist, [int(hist.sum()), 0, 0, 0, 0, 0]), so.measures(hist, [int(hist.sum()), 0, 0, 0, 0, 0], 0, 1, False)):
            assert abs(m["mi"]) < 1e-12 and abs(m["nmi"] - 1.0) < 1e-12 and math.isnan(m["rho"])


def test_single_voxel_no_voxel_and_empty_ranges(built, so):
    # a single counted voxel: no spread, so no entropy, no correlation; the RMS difference is its difference
    A = np.array([[[0.0, 4.0, np.nan]]], np.float32)
    B = np.array([[[np.inf, 1.0, 4.0]]], np.float32)
    r = so.similarity(A, B, same_scale=True)
    assert r["n"] == 1 and r["excluded"] == 2 and r["sums"] == [1, 1023, 256, 1023 * 1023, 256 * 256, 1023 * 256] and r["hist"][63, 16] == 1
    m = built.similarity_measures(r["hist"], r["sums"], 0.0, 4.0, True)
    assert (m["h_a"], m["h_b"], m["h_ab"], m["mi"]) == (0.0, 0.0, 0.0, 0.0) and math.isnan(m["nmi"]) and math.isnan(m["rho"])
    assert m["rms"] == math.sqrt(float(767 * 767)) * (4.0 / 1023.0) and same_measure(m["rms"], r["rms"])
    # no voxel: NaN throughout
    r = so.similarity(A, np.array([[[np.inf, np.nan, 4.0]]], np.float32), same_scale=True)
    assert r["n"] == 0 and r["excluded"] == 3 and not r["hist"].any() and all(math.isnan(r[k]) for k in MEASURES)
    assert all(math.isnan(v) for v in built.similarity_measures(r["hist"], r["sums"], 0.0, 4.0, True).values())
    # each empty_range value: an image without two distinct finite values, where it needs a range
    flat, nans, ok = np.full((2, 3, 4), 2.5, np.float32), np.full((2, 3, 4), np.nan, np.float32), volume("random", (2, 3, 4), 1)
    for a, b, same_scale, want in ((flat, ok, False, 1), (ok, nans, False, 2), (nans, flat, False, 3), (flat, ok, True, 1), (ok, flat, True, 0), (ok, ok, False, 0)):
        r = so.similarity(a, b, same_scale=same_scale)
        assert r["empty_range"] == want
        if want:
            assert r["n"] == 0 and r["excluded"] == 24 and not r["hist"].any() and all(math.isnan(r[k]) for k in MEASURES)
    r = so.similarity(ok, flat, same_scale=True)        # B needs no range of its own under same_scale: every voxel of it lands in one column
    assert r["n"] == 24 and (r["hist"].sum(0) > 0).sum() == 1


@pytest.mark.parametrize("where", ["a", "b", "both"])
def test_special_values_are_counted_by_hand(so, where):
    """-0 is a finite value like 0; NaN, +inf and -inf are excluded wherever they stand"""
    base = np.linspace(-4.0, 9.0, 24).astype(np.float32).reshape(2, 3, 4)
    special = np.array([-0.0, np.nan, np.inf, -np.inf], np.float32)
    A, B = base.copy(), base[::-1].copy()
    if where in ("a", "both"):
        A.reshape(-1)[2:6] = special
    if where in ("b", "both"):
        B.reshape(-1)[4:8] = special                    # overlaps A's at voxels 4 and 5 (+inf and -inf there; -0 and NaN here)
    want_excluded = {"a": 3, "b": 3, "both": 5}[where]   # A loses voxels 3, 4, 5; B 5, 6, 7; together 3 .. 7
    for same_scale in (False, True):
        r = so.similarity(A, B, same_scale=same_scale)
        assert r["excluded"] == want_excluded and r["n"] == 24 - want_excluded and r["hist"].sum() == r["n"]
        assert r["range_a"] == (np.float32(-4.0), np.float32(9.0))
        hist, sums, excluded = count_numpy(A, B, r["range_a"], r["range_b"], 64)
        assert np.array_equal(hist, r["hist"]) and sums == r["sums"] and excluded == r["excluded"]
    if where != "b":
        assert so.L.osim_q(float(A.reshape(-1)[2]), -4.0, 9.0) == so.L.osim_q(0.0, -4.0, 9.0) == 315      # -0: rint(4 / 13 * 1023) = rint(314.77)


# ---- the scenario: the reason the histogram is there -----------------------------------------------------------------------------------
SHIFTS = (0, 1, 2, 3, 5)
# the oracle's figures when this was written (64 bins, own ranges), to the digits printed: mi and rho per shift
SCENARIO = {
    "as_it_is": {"mi": (3.963, 1.439, 0.812, 0.477, 0.168), "rho": (1.000, 0.967, 0.872, 0.723, 0.324)},
    "folded": {"mi": (3.203, 0.890, 0.388, 0.182, 0.058), "rho": (0.019, 0.024, 0.026, 0.023, 0.006)},
}


def scenario_pairs():
    """A: the x-crop [5, -5) of blockmatch_cases.volume("smooth", (40, 44, 48), 5); B: the same crop moved by 0, 1, 2, 3, 5 voxels along
    x, as it is and folded about the middle of its range, |v - mid|: a relation between the intensities that is not monotone"""
    v = volume("smooth", (40, 44, 48), 5)
    A = np.ascontiguousarray(v[:, :, 5:-5])
    out = {"as_it_is": [], "folded": []}
    for s in SHIFTS:
        B = np.ascontiguousarray(v[:, :, 5 + s:48 - 5 + s])
        mid = (B.min() + B.max()) / np.float32(2.0)
        out["as_it_is"].append((A, B))
        out["folded"].append((A, np.abs(B - mid).astype(np.float32)))
    return out


def test_scenario_mutual_information_follows_the_shift(so):
    """On the oracle: mi falls strictly with the shift in both cases; under the fold |rho| stays below 0.1 at every shift, so a
    correlation coefficient says nothing there while mi still finds the shift; mi(0) - mi(1) is at least half the recorded gap."""
    for case, pairs in scenario_pairs().items():
        got = [so.similarity(A, B) for A, B in pairs]
        mi, rho = [r["mi"] for r in got], [r["rho"] for r in got]
        print("similarity scenario %s: mi %s rho %s" % (case, " ".join("%.3f" % v for v in mi), " ".join("%.3f" % v for v in rho)))
        assert all(r["n"] == 40 * 44 * 38 and r["excluded"] == 0 for r in got)
        assert all(a > b for a, b in zip(mi, mi[1:])), (case, mi)
        want = SCENARIO[case]
        assert all(abs(g - w) < 5e-4 for g, w in zip(mi, want["mi"])) and all(abs(g - w) < 5e-4 for g, w in zip(rho, want["rho"])), (case, mi, rho)
        gap = want["mi"][0] - want["mi"][1]
        assert gap > 0 and mi[0] - mi[1] >= 0.5 * gap
        if case == "folded":
            assert all(abs(v) < 0.1 for v in rho), rho
        else:
            assert all(a > b for a, b in zip(rho, rho[1:]))


# ---- the shapes of the GPU suite --------------------------------------------------------------------------------------------------------
def test_shapes_follow_the_kernel_file():
    K = kernel_constants()
    assert (K["SIM_VPT"], K["SIM_THREADS"] * K["SIM_VPT"], K["SIM_MAX_BLOCKS"]) == (VPT, STRETCH, CAP)
    assert K["SIM_MAX_BINS"] == 64 and K["SIM_MAX_LABELS"] == 64 and K["SIM_THREADS"] == 256
    assert 4 * K["SIM_MAX_BINS"] ** 2 + 8 * 6 * (1 + K["SIM_MAX_LABELS"]) <= 65536      # the workgroup's LDS
    count = lambda s: s[0] * s[1] * s[2]
    assert all(max(s) <= 4096 for s in COUNT_SHAPES + [BIG])
    counts = [count(s) for s in COUNT_SHAPES]
    assert counts[:2] == [1, 24] and {c % VPT for c in counts} == {0, 1, 2, 3}
    assert {STRETCH - 1, STRETCH, STRETCH + 1} <= set(counts) and max(counts) > 4 * STRETCH
    # past the launch cap: more than cap x 256 x voxels-per-thread voxels by at least 32 workgroups' worth, and a last thread with a part load
    assert count(BIG) >= (CAP + EXCESS) * STRETCH and count(BIG) % VPT != 0


# ---- similarity_host.c under the sanitizers -------------------------------------------------------------------------------------------------
def fmt(v):
    return "nan" if math.isnan(v) else "%.17g" % v


def report_text(rec, labels=None):
    """sift3d_similarity_report_text restated"""
    g = lambda v: "nan" if math.isnan(v) else "%.12g" % v
    t = "# range_a %.9g %.9g\n# range_b %.9g %.9g\n# same_scale %d\n# voxels %d %d\n" % (rec["range_a"] + rec["range_b"] + (rec["same_scale"], rec["n"], rec["excluded"]))
    t += " ".join(g(rec[k]) for k in MEASURES) + "\n"
    if labels is not None:
        t += "# label n rho rms\n" + "".join("%d %d %s %s\n" % (l["label"], l["n"], g(l["rho"]), g(l["rms"])) for l in labels)
    return t


def test_host_file_under_sanitizers(built, so, tmp_path):
    """similarity_host.c and tests/similarity_host_san.c as one program, with and without -fsanitize=address,undefined: both exit
    clean and print the same lines, and those are the restatement's"""
    src = [os.path.join(ROOT, "tests", "similarity_host_san.c"), os.path.join(ROOT, "3d_sift_cuda_amd", "csrc", "similarity_host.c")]
    base = ["cc", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-ffp-contract=off", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include")]
    out = {}
    for name, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])):
        exe = str(tmp_path / ("similarity_host_" + name))
        subprocess.run(base + flags + ["-o", exe] + src + ["-lm"], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
        out[name] = r.stdout
    text = out["san"]
    assert text == out["plain"] and "defaults 64 0 64 0 1\n" in text
    for line in ("check null -1 null pointer", "check bins 8 0 ", "check bins 64 0 ", "check bins 0 -1 bins = 0: 8, 16, 32 or 64", "check bins 7 -1 bins = 7: 8, 16, 32 or 64",
                 "check bins 128 -1 bins = 128: 8, 16, 32 or 64", "check bins -8 -1 bins = -8: 8, 16, 32 or 64", "check same_scale 1 0 ",
                 "check same_scale 2 -1 same_scale = 2: 0 or 1", "check max_labels 0 -1 max_labels = 0: 1 .. 64", "check max_labels 64 0 ",
                 "check max_labels 65 -1 max_labels = 65: 1 .. 64", "check flush 1 0 ", "check flush 2 -1 flush = 2: 0 or 1", "check short_err -1 bins =",
                 "check no_err -1 ", "measures refused -1 -1 -1", "report null -1"):
        assert line + "\n" in text, line
    # the measures of the program's histograms, restated here from the same recipes
    for bins in BINS:
        q = [i * (1024 // bins) for i in range(bins)]
        c = list(range(1, bins + 1))
        s1, s2 = sum(a * b for a, b in zip(c, q)), sum(a * b * b for a, b in zip(c, q))
        n30 = 1 << 30
        cases = (("diagonal", np.diag(c), [sum(c), s1, s1, s2, s2, s2], -2.0, 3.0, 1),
                 ("product", np.outer(np.arange(1, bins + 1), np.arange(2, bins + 2)), [int(np.outer(np.arange(1, bins + 1), np.arange(2, bins + 2)).sum()), 0, 0, 0, 0, 0], 0.0, 1.0, 0),
                 ("one_cell", np.zeros((bins, bins), np.int64), [n30, 1023 * n30, 0, 1023 * 1023 * n30, 0, 0], 0.0, 1023.0, 1),
                 ("empty", np.zeros((bins, bins), np.int64), [0] * 6, 0.0, 1.0, 1))
        for name, hist, sums, lo, hi, same_scale in cases:
            hist = np.array(hist, np.int64)
            if name == "one_cell":
                hist[bins - 1, 0] = n30
            want = so.measures(hist, sums, lo, hi, same_scale)
            assert "measures %s %d %d %s\n" % (name, bins, same_scale, " ".join(fmt(want[k]) for k in MEASURES)) in text, (name, bins)
            py = measures_python(hist, sums, lo, hi, same_scale)
            assert all(close(want[k], py[k]) for k in MEASURES if k != "mi"), (name, bins, want, py)
            assert math.isnan(py["mi"]) if math.isnan(want["mi"]) else abs(want["mi"] - py["mi"]) < 1e-11, (name, bins, want, py)
    half, sq = 1 << 29, 1023 * 1023
    hist = np.zeros((64, 64), np.int64)
    hist[0, 63] = hist[63, 0] = half
    want = so.measures(hist, [2 * half, 1023 * half, 1023 * half, sq * half, sq * half, 0], -1.0e30, 1.0e30, 1)
    assert want["rho"] == -1.0 and want["h_a"] == want["h_b"] == want["h_ab"] == want["mi"] and abs(want["mi"] - math.log(2.0)) < 1e-14
    for name in ("widest", "in_place"):
        assert "measures %s 64 1 %s\n" % (name, " ".join(fmt(want[k]) for k in MEASURES)) in text, name
    rows = ([1, 5, 9, 25, 81, 45], [3, 6, 12, 14, 56, 28], [2, 1023, 1023, sq, sq, 0], [0] * 6)
    for k, s in enumerate(rows):
        for same_scale in (0, 1):
            rho, rms = so.rho_rms(s, -2.0, 3.0, same_scale)
            assert "label %d %d %s %s\n" % (65535 - k, s[0], fmt(rho), fmt(rms)) in text, (k, same_scale)
    # the report, restated
    f32 = lambda v: float(np.float32(v))
    rec = {"range_a": (f32(-1.0e30), f32(3.4028234e38)), "range_b": (-0.0, f32(1.17549435e-38)), "same_scale": 1, "n": 1 << 30, "excluded": (1 << 30) - 1,
           "mi": 4.1588830833596715, "nmi": 2.0, "rho": -1.0, "rms": math.nan, "h_a": 1.0e-300, "h_b": 1.0e-300, "h_ab": math.nan}
    labels = [{"label": 65535 - 64 + k, "n": (1 << 30) - k, "rho": math.nan if k % 3 == 0 else -1.0 + k / 64.0, "rms": math.nan if k % 5 == 0 else 1.0e30 / (k + 1)}
              for k in range(64)]
    bare, want = report_text(rec), report_text(rec, labels)
    assert "-nan" not in text and len(want) < 8192
    assert "report bare %d\n%s" % (len(bare), bare) in text and "report full %d\n%s" % (len(want), want) in text
    # a buffer that is too short holds the text's beginning and a terminator, and the length is the whole text's
    for room in (0, 1, 2, 100, len(want), len(want) + 1):
        assert "report room %d %d [%s]\n" % (room, len(want), want[:max(min(room - 1, len(want)), 0)]) in text, room
    assert "report over %d\n" % len(want) in text          # n_labels beyond 64 is read as 64


def test_python_mirror_of_the_host_helpers(built):
    p = built.similarity_params()
    assert (p.bins, p.same_scale, p.max_labels, p.device, p.flush) == (64, 0, 64, 0, 1) and built.similarity_check(p) is None
    assert built.similarity_check(built.similarity_params(bins=12)) == "bins = 12: 8, 16, 32 or 64"
    assert built.similarity_check(built.similarity_params(flush="atomics", bins=8, same_scale=1, max_labels=1)) is None
    assert built.similarity_check(built.similarity_params(max_labels=65)) == "max_labels = 65: 1 .. 64"
    with pytest.raises(ValueError):
        built.similarity_params(bin=8)
    with pytest.raises(built.Sift3DError):
        built.similarity_measures(np.zeros((7, 7), np.int64), [0] * 6)
