"""Shared pieces of the resampling tests (test_resample_cpu.py, test_gpu_resample.py): the CPU oracle tests/resample_oracle.c,
built with cc -O2 -ffp-contract=off into a temporary directory and bound with ctypes, and the maps and volumes the tests use."""
import ctypes as C

import numpy as np

from _helpers import c_oracle

MODES = {"linear": 0, "nearest": 1}


class ResampleOracle:
    def __init__(self, tmpdir):
        L = c_oracle("resample_oracle", tmpdir)
        P, I64 = C.c_void_p, C.c_int64
        L.orc_resample.restype = C.c_int
        L.orc_resample.argtypes = [P, I64, I64, I64, P, I64, I64, I64, P, C.c_int, C.c_float, I64, I64]
        self.L = L

    def resample(self, vol, out_shape, A, interp="linear", fill=0.0, z0=0, z1=None):
        """output planes [z0, z1) of out_shape = (oz, oy, ox)"""
        v = np.ascontiguousarray(vol, np.float32)
        nz, ny, nx = v.shape
        oz, oy, ox = out_shape
        z1 = oz if z1 is None else z1
        out = np.empty((z1 - z0, oy, ox), np.float32)
        a = np.ascontiguousarray(A, np.float32).reshape(12)
        assert self.L.orc_resample(v.ctypes.data, nx, ny, nz, out.ctypes.data, ox, oy, oz, a.ctypes.data, MODES[interp], float(fill), z0, z1) == 0
        return out


def rot(axis, deg):
    """3 x 3 rotation about a unit axis (float64)"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def affine(R, t, s=1.0):
    """4 x 4 float64 of x -> s R x + t"""
    m = np.eye(4)
    m[:3, :3] = s * np.asarray(R, np.float64)
    m[:3, 3] = t
    return m


def about_centre(M3, shape_src, shape_out, shift=(0, 0, 0)):
    """3 x 4 float32 map: output voxel -> source voxel, M3 applied about the two volumes' centres, plus a shift (x, y, z)"""
    cs = (np.array(shape_src[::-1], np.float64) - 1) / 2
    co = (np.array(shape_out[::-1], np.float64) - 1) / 2
    A = np.zeros((3, 4))
    A[:, :3] = M3
    A[:, 3] = cs - M3 @ co + np.asarray(shift, np.float64)
    return A.astype(np.float32)


def special_volume(shape, seed):
    """a float32 volume with NaN, +-inf, denormals and -0 sprinkled over a smooth ramp"""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    v = (np.sin(x * 0.21) + np.cos(y * 0.17) * 2 + z * 0.05).astype(np.float32)
    flat = v.reshape(-1)
    n = flat.size
    for val, frac in ((np.nan, 0.01), (np.inf, 0.005), (-np.inf, 0.005), (np.float32(1e-40), 0.02), (np.float32(-0.0), 0.02),
                      (np.float32(-3e-39), 0.01)):
        idx = rng.choice(n, max(1, int(n * frac)), replace=False)
        flat[idx] = val
    return v
