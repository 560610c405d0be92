"""CPU suite: every device and pinned host allocation of the library goes through csrc/alloc_fill.hip.

The fill hook of sift3d_selftest_alloc_fill (include/sift3d_dev.h, tests/test_gpu_alloc_fill.py) can only poison the blocks
it sees.  A buffer allocated with the runtime's own call beside it would be exactly the buffer the GPU suite cannot check,
so a file of csrc/ that names one of the runtime's allocators in code fails here."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3d_sift_cuda_amd", "csrc")
ALLOCATOR = "alloc_fill.hip"
# hipMalloc, hipHostMalloc, hipMallocAsync, hipMallocManaged and their kin (hipMallocPitch, hipMalloc3D, hipExtMallocWithFlags,
# hipMallocFromPoolAsync, hipHostAlloc, hipMemAllocHost, ...): called, or taken as a function pointer
RUNTIME_ALLOC = re.compile(r"\bhip\w*(?:Malloc|Alloc)\w*\s*(?:\(|[;,)])")
FLAG = re.compile(r"\bhipHostMalloc(?:Default|Portable|Mapped|WriteCombined|NumaUser|Coherent|NonCoherent)\b")


def code_of(text):
    """the text without comments and string literals"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return re.sub(r'"(?:\\.|[^"\\\n])*"', '""', text)


def sources():
    out = []
    for d, dirs, fs in os.walk(CSRC):
        dirs[:] = [x for x in dirs if not x.startswith("_build")]
        out += [os.path.join(d, f) for f in sorted(fs) if f.endswith((".hip", ".h", ".c", ".cpp", ".hpp", ".cc"))]
    return out


def direct_allocations(text):
    return RUNTIME_ALLOC.findall(FLAG.sub(" ", code_of(text)))


def test_the_pattern_sees_what_it_must():
    """the ledger's own eyes: the four calls the hook replaces, a kin, a pointer to one -- and not the flags or a comment"""
    for call in ("hipMalloc(&p, n)", "hipMalloc ((void **)&p, n)", "hipHostMalloc(&p, n, 0)", "hipMallocAsync(&p, n, s)", "hipMallocManaged(&p, n)",
                 "hipMallocPitch(&p, &pitch, w, h)", "hipExtMallocWithFlags(&p, n, 0)", "hipHostAlloc(&p, n, 0)", "auto f = hipMalloc;"):
        assert direct_allocations("x = " + call), call
    for clean in ("sift3d_alloc_host(&p, n, hipHostMallocPortable | hipHostMallocMapped)", "/* what hipMalloc( hands back */", "// hipMalloc(x)",
                  'fail("hipMalloc(%d) failed")', "sift3d_alloc_device(&p, n)"):
        assert not direct_allocations(clean), clean


def test_only_the_allocator_calls_the_runtime_allocators():
    files = sources()
    assert any(os.path.basename(f) == ALLOCATOR for f in files) and len(files) > 40
    bad = {}
    for f in files:
        hits = direct_allocations(open(f, errors="ignore").read())
        if os.path.basename(f) == ALLOCATOR:
            assert hits, "the allocator no longer allocates: the ledger watches the wrong file"
        elif hits:
            bad[os.path.relpath(f, ROOT)] = hits
    assert not bad, "allocate through sift3d_alloc_device / sift3d_alloc_host (alloc_fill.hip): %r" % bad


def test_the_hook_is_off_by_default_and_turning_it_off_needs_no_device(built):
    """-1 touches no device and has nothing to report (the counters only run while a byte is set); a byte outside 0 .. 255 is refused"""
    import ctypes as C
    stats = (C.c_uint64 * 2)(7, 7)
    L = built.hip_lib()
    assert L.sift3d_selftest_alloc_fill(-1, stats) == 0 and tuple(stats) == (0, 0)
    assert L.sift3d_selftest_alloc_fill(-1, None) == 0
    assert L.sift3d_selftest_alloc_fill(256, stats) != 0 and L.sift3d_selftest_alloc_fill(-2, stats) != 0
    with pytest.raises(ValueError):
        with built.alloc_fill(300):
            pass


def test_the_allocator_is_linked_and_covers_the_arena():
    """alloc_fill.o is linked into libsift3d_hip.so, and the slab rank fills the pieces of its reused arena"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "$(B)/alloc_fill.o" in mk
    assert "sift3d_alloc_reused(" in code_of(open(os.path.join(CSRC, "zslab_driver.hip")).read())
