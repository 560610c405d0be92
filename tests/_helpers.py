"""Helpers the alignment, guided re-matching and resampling tests share: the build of their CPU oracles, an extraction on the
GPU, and a command line that must succeed."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def c_oracle(name, tmpdir):
    """tests/<name>.c built with cc -O2 -ffp-contract=off into tmpdir, loaded with ctypes"""
    so = os.path.join(str(tmpdir), "lib%s.so" % name)
    subprocess.run(["cc", "-O2", "-ffp-contract=off", "-std=c11", "-fPIC", "-shared", "-o", so, os.path.join(HERE, name + ".c"), "-lm"],
                   check=True)
    return C.CDLL(so)


def extract(built, vol):
    """the records of one volume (nz, ny, nx), extracted on device 0"""
    nz, ny, nx = vol.shape
    with built.Context(nx, ny, nz, device=0) as ctx:
        ctx.set_volume(vol)
        return ctx.extract()


def run(argv, cwd):
    """run a command line in cwd; it must exit with 0"""
    argv = [str(a) for a in argv]
    r = subprocess.run(argv, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, " ".join(argv) + "\n" + r.stdout[-3000:] + r.stderr[-3000:]
    return r
