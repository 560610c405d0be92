"""Helpers the alignment, guided re-matching and resampling tests share: the build of their CPU oracles, an extraction on the
GPU, and a command line that must succeed."""
import contextlib
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


class CallerStream:
    """A hipStream_t the test owns, as a caller of the library would: .handle for sift3d_set_stream, .torch (a
    torch.cuda.ExternalStream over the same handle) to queue producers and consumers on it with torch.cuda.stream()."""

    def __init__(self, hip, handle, torch_stream):
        self.hip, self.handle, self.torch = hip, handle, torch_stream

    def idle(self):
        """hipStreamQuery: True when everything queued on the stream has run (and the handle is still a stream)"""
        return self.hip.hipStreamQuery(C.c_void_p(self.handle)) == 0


@contextlib.contextmanager
def caller_stream(flags=1):
    """A stream made with hipStreamCreateWithFlags(flags): 1 = hipStreamNonBlocking, which nothing orders with the legacy default
    stream (a torch.cuda.Stream() is a blocking stream on ROCm and would hide a missing dependency), 0 = blocking.  Destroyed
    with hipStreamDestroy when the block ends: open the library context INSIDE the block, so that it is closed first."""
    import torch                                   # loaded first: the process keeps ONE HIP runtime, torch's
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    hip.hipStreamQuery.argtypes = hip.hipStreamSynchronize.argtypes = hip.hipStreamDestroy.argtypes = [C.c_void_p]
    torch.cuda.init()
    s = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(s), flags) == 0 and s.value
    try:
        yield CallerStream(hip, s.value, torch.cuda.ExternalStream(s.value))
    finally:
        rc = hip.hipStreamSynchronize(s) or hip.hipStreamDestroy(s)
    assert rc == 0                                 # (after a clean block only: a failure inside it is what gets reported)


def hip_memcpy_to_host(dst, dev_ptr, nbytes):
    """a plain hipMemcpy (device to host) into the numpy array dst: the runtime's own copy, which torch does not order with
    any of its streams"""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(dst.ctypes.data, C.c_void_p(int(dev_ptr)), nbytes, 2) == 0   # 2 = hipMemcpyDeviceToHost


def run(argv, cwd):
    """run a command line in cwd; it must exit with 0"""
    argv = [str(a) for a in argv]
    r = subprocess.run(argv, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, " ".join(argv) + "\n" + r.stdout[-3000:] + r.stderr[-3000:]
    return r
