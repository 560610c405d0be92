"""CPU suite: the box walk of the SIFT-rank descriptor's bins (3d_sift_cuda_amd/csrc/desc_bins.h).

descriptor_kernel<true> sums every bin over the 5 x 5 x 5 box on which the bin's trilinear weights are not zero instead of over
every voxel of its octant.  tests/desc_bins_check.cpp runs the header's walk with the host compiler on patches fed directly --
random ones, gradients all in one octant, flat except on the centre planes, mostly zero gradients, faint and denormal magnitudes,
all NaN, infinite values -- and holds the 64 bins to the oracle's o3_desc_sift bit for bit and the ranks to o3_rank; here it is
built with the oracle's source, once plain and once under AddressSanitizer + UndefinedBehaviorSanitizer, and its report is read.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3d_sift_cuda_amd", "csrc")
ORACLE = os.path.join(ROOT, "oracle")
# family -> (patches, patches that must have taken the walk over all voxels: None = every one of them)
FAMILIES = {"random": (400, 0), "one_octant": (64, 0), "centre_planes": (64, 0), "mostly_zero": (64, 0), "faint": (64, 0),
            "denormal_planted": (200, 0), "all_nan": (1, 0), "infinite": (32, None)}
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def build_and_run(tmp, name, opt):
    """The oracle as C with its binding flags (no contraction), the check as C++17, one stand-alone program."""
    obj, exe = str(tmp / (name + "_oracle.o")), str(tmp / name)
    common = ["-ffp-contract=off", "-Wall", "-Wextra"] + opt
    for cmd in ([os.environ.get("CC", "cc"), "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-Wno-unused-parameter"] + common +
                ["-c", os.path.join(ORACLE, "sift3d_oracle.c"), "-o", obj],
                [os.environ.get("CXX", "c++"), "-std=c++17"] + common + ["-I", CSRC, "-I", ORACLE, "-o", exe,
                 os.path.join(ROOT, "tests", "desc_bins_check.cpp"), obj, "-lm"]):
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("name,opt", [("plain", ["-O2"]), ("sanitized", SAN)])
def test_box_walk_equals_the_oracle(tmp_path, name, opt):
    code, out, err = build_and_run(tmp_path, "desc_bins_check_" + name, opt)
    assert code == 0 and not err, (code, out, err[-3000:])
    got = {f: (int(n), int(bad), int(walked_all)) for f, n, bad, walked_all in (line.split() for line in out.splitlines())}
    assert set(got) == set(FAMILIES), sorted(got)
    for family, (n, walked_all) in FAMILIES.items():
        assert got[family] == (n, 0, n if walked_all is None else walked_all), (family, got[family])
