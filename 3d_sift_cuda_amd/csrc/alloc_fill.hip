/*
 * alloc_fill.hip -- the one place the library takes device and pinned host memory from the runtime, and the fill hook
 * the GPU suite turns on there (sift3d_selftest_alloc_fill, include/sift3d_dev.h).
 *
 * Nothing may depend on what an allocation holds when it is handed out.  A young process mostly gets zero pages, so a
 * missing clear passes every test that only hopes for garbage; with a fill byte set, every block -- and every piece a slab
 * rank cuts from its reused arena -- holds that byte over its whole length before the caller sees it.  Off (the default)
 * the hook costs one relaxed load per allocation.  tests/test_alloc_ledger.py keeps every other file of csrc/ from calling
 * the runtime's allocators itself.
 */
#include <atomic>
#include <cstring>

#include "sift3d_internal.h"

namespace {
std::atomic<int> g_fill{-1};          /* -1: off, else the byte */
std::atomic<uint64_t> g_blocks{0};    /* blocks and bytes filled since the last sift3d_selftest_alloc_fill */
std::atomic<uint64_t> g_bytes{0};

/* The fill is complete when this returns: hipMemset runs on the null stream, which the library's non-blocking streams are
 * not ordered with, so without the wait it could still be running when the caller's own clear or first kernel has finished
 * -- and wipe it.  The hook is never on in a timed run. */
hipError_t fill_device(void *p, size_t bytes, int byte, bool counted)
{
    if (!p || bytes == 0) return hipSuccess;
    hipError_t e = hipMemset(p, byte, bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess && counted) {
        g_blocks.fetch_add(1, std::memory_order_relaxed);
        g_bytes.fetch_add((uint64_t)bytes, std::memory_order_relaxed);
    }
    return e;
}

hipError_t alloc_device(void **p, size_t bytes, bool counted)
{
    const hipError_t e = hipMalloc(p, bytes);
    const int byte = g_fill.load(std::memory_order_relaxed);
    if (e != hipSuccess || byte < 0) return e;
    const hipError_t f = fill_device(*p, bytes, byte, counted);
    if (f != hipSuccess) {
        hipFree(*p);
        *p = nullptr;
    }
    return f;
}
} // namespace

hipError_t sift3d_alloc_device(void **p, size_t bytes) { return alloc_device(p, bytes, true); }

hipError_t sift3d_alloc_host(void **p, size_t bytes, unsigned flags)
{
    const hipError_t e = hipHostMalloc(p, bytes, flags);
    const int byte = g_fill.load(std::memory_order_relaxed);
    if (e != hipSuccess || byte < 0) return e;
    memset(*p, byte, bytes); /* pinned memory is the host's to write: done when memset returns */
    g_blocks.fetch_add(1, std::memory_order_relaxed);
    g_bytes.fetch_add((uint64_t)bytes, std::memory_order_relaxed);
    return hipSuccess;
}

hipError_t sift3d_alloc_reused(void *p, size_t bytes)
{
    const int byte = g_fill.load(std::memory_order_relaxed);
    return byte < 0 ? hipSuccess : fill_device(p, bytes, byte, true);
}

extern "C" int sift3d_selftest_alloc_fill(int byte, uint64_t stats[2])
{
    if (byte < -1 || byte > 255) return SIFT3D_ERR_ARG;
    g_fill.store(byte, std::memory_order_relaxed);
    const uint64_t blocks = g_blocks.exchange(0, std::memory_order_relaxed), bytes = g_bytes.exchange(0, std::memory_order_relaxed);
    if (stats) {
        stats[0] = blocks;
        stats[1] = bytes;
    }
    if (byte < 0) return SIFT3D_OK;
    /* the setter proves itself: a block from the same allocator (not counted) holds the pattern in every byte */
    enum { PROBE = 4096 };
    unsigned char *d = nullptr, h[PROBE];
    memset(h, byte ^ 0xff, PROBE);
    hipError_t e = alloc_device((void **)&d, PROBE, false);
    if (e == hipSuccess) e = hipMemcpy(h, d, PROBE, hipMemcpyDeviceToHost);
    hipFree(d);
    bool same = e == hipSuccess;
    for (int i = 0; i < PROBE && same; i++) same = h[i] == (unsigned char)byte;
    if (!same) {
        (void)hipGetLastError();
        g_fill.store(-1, std::memory_order_relaxed);
        return SIFT3D_ERR_DEVICE;
    }
    return SIFT3D_OK;
}
