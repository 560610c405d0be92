"""CPU suite: the order in which descriptor_kernel takes a re-oriented record's samples (3d_sift_cuda_amd/csrc/sample_order.h).

The kernel sorts the 1331 samples of a patch by the image row they read before it samples them.  tests/sample_order_check.cpp
runs the header's functions with the host compiler -- orthonormal frames, the identity, axis permutations with sign flips,
slightly skewed frames, frames with a NaN or an infinite entry, scales 0.5 .. 8, centres in the interior and within a radius of
every face, a slab context's octave, and centres and radii that are not finite -- and checks that every key lies inside the
bins, that it follows from the cells trilinear takes, and that the emulated counting sort is a permutation of 0 .. 1330 whatever
order the samples arrive in.  It also restates the line model: the 128-byte lines a quad of lanes touches per gather, summed
over a record, for the patch order and for the image order.  Here it is built once plain and once under AddressSanitizer +
UndefinedBehaviorSanitizer, and its report is read.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3d_sift_cuda_amd", "csrc")
FAMILIES = {"orthonormal": 2000, "identity": 200, "permutation": 400, "skewed": 1000, "nonfinite": 600, "odd_record": 20}
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def build_and_run(tmp, name, opt):
    exe = str(tmp / name)
    cmd = [os.environ.get("CXX", "c++"), "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra"] + opt + \
          ["-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "sample_order_check.cpp"), "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("name,opt", [("plain", ["-O2"]), ("sanitized", SAN)])
def test_order_is_a_permutation_in_image_rows(tmp_path, name, opt):
    code, out, err = build_and_run(tmp_path, "sample_order_check_" + name, opt)
    assert code == 0 and not err, (code, out, err[-3000:])
    rows = [line.split() for line in out.splitlines()]
    got = {r[0]: (int(r[1]), int(r[2])) for r in rows if r[0] != "lines"}
    assert got == {f: (n, 0) for f, n in FAMILIES.items()}, got
    lines = {r[1]: (float(r[2]), float(r[3])) for r in rows if r[0] == "lines"}
    assert set(lines) == {"1.3", "2.6"}, lines
    for step, (patch_order, image_order) in lines.items():
        print("step %s: %.0f lines per record over quads in patch order, %.0f in image order" % (step, patch_order, image_order))
        assert image_order < patch_order, (step, patch_order, image_order)
