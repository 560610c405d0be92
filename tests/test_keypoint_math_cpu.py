"""CPU suite: the scalar arithmetic of the per-keypoint kernels (3d_sift_cuda_amd/csrc/keypoint_math.h).

keypoint_kernel and descriptor_kernel take every bit of a record's frame from the scalar routines of this header: the
sub-voxel refinement, the 3x3 singular value decomposition and its sort, the 3x3 inverse, the vector helpers.  The header is
plain C++ for host and device, so tests/keypoint_math_check.cpp runs the same text with the host compiler.

Against the oracle, bit for bit: svd3 + sort_eig against o3_svd3 + o3_sort_eig (200 000 structure tensors, rank-deficient and
zero ones among them), invert3 against o3_invert3 (their eigenvector matrices and 2 000 nearly singular matrices),
interp_quadratic against o3_interp_quadratic (200 000 triples over the abscissae the kernel uses, degenerate ordinates among
them), interp_point_patch against o3_interp_point (every interior voxel of 20 grids of 11^3).

Against a property, there being no oracle export: in_radius marks 485 voxels, all interior, symmetric under the negation of
each axis.  (485 lattice points lie strictly inside radius 5, which is the reference's test; 515, the figure the kernel's NRAD
once carried, counts the points inside or on it, and the six of those on the axes are not interior.)

No comparison here is against a restatement of the kernel's text.  The header's eigen test decision and octant choice, and
the statements that stayed in keypoint_kernel (the frame of two peak directions, the two splat positions), are held to the
oracle on the GPU by tests/test_gpu_keypoint_stage.py and tests/test_gpu_parity.py.

Here the program is built with the oracle's source, once plain and once under AddressSanitizer + UndefinedBehaviorSanitizer,
and its report is read.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3d_sift_cuda_amd", "csrc")
ORACLE = os.path.join(ROOT, "oracle")
FAMILIES = {"svd3_sort_eig": 200000, "invert3": 202000, "interp_quadratic": 200000, "interp_point_patch": 729 * 20, "in_radius": 1331}
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def build_and_run(tmp, name, opt):
    """The oracle as C with its binding flags (no contraction), the check as C++17, one stand-alone program."""
    obj, exe = str(tmp / (name + "_oracle.o")), str(tmp / name)
    common = ["-ffp-contract=off", "-Wall", "-Wextra"] + opt
    for cmd in ([os.environ.get("CC", "cc"), "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-Wno-unused-parameter"] + common +
                ["-c", os.path.join(ORACLE, "sift3d_oracle.c"), "-o", obj],
                [os.environ.get("CXX", "c++"), "-std=c++17"] + common + ["-I", CSRC, "-I", ORACLE, "-o", exe,
                 os.path.join(ROOT, "tests", "keypoint_math_check.cpp"), obj, "-lm"]):
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("name,opt", [("plain", ["-O2"]), ("sanitized", SAN)])
def test_scalar_routines_equal_the_oracle(tmp_path, name, opt):
    code, out, err = build_and_run(tmp_path, "keypoint_math_check_" + name, opt)
    assert code == 0 and not err, (code, out, err[-3000:])
    got = {family: (int(n), int(bad)) for family, n, bad in (line.split() for line in out.splitlines())}
    assert got == {f: (n, 0) for f, n in FAMILIES.items()}, got
