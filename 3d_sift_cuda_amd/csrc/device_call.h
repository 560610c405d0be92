/*
 * device_call.h -- what one call of a host-array entry point (sift3d_knn64, the alignment, resampling and guided re-matching
 * calls) holds on the device: a non-blocking stream, two timing events and its device buffers, released together when the
 * call returns, the messages those entry points write into the caller's err, and the RMS their reports give.  Internal: nothing here is part of the C-ABI.
 */
#ifndef SIFT3D_DEVICE_CALL_H
#define SIFT3D_DEVICE_CALL_H
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <vector>

#include "sift3d_internal.h"

#pragma GCC visibility push(hidden)

/* printf into err (when there is room for it); returns rc */
__attribute__((format(printf, 4, 5))) inline int call_fail(char *err, int64_t err_len, int rc, const char *fmt, ...)
{
    if (err && err_len > 0) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, (size_t)err_len, fmt, ap);
        va_end(ap);
    }
    return rc;
}

/* the root mean square of the residuals r, as the refinement reports give it; 0 for none */
inline double rms_of(const std::vector<double> &r)
{
    double s = 0;
    for (double x : r) s += x * x;
    return r.empty() ? 0.0 : std::sqrt(s / (double)r.size());
}

struct device_call {
    char *err;
    int64_t err_len;
    int device = 0;
    hipStream_t s = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    std::vector<void *> bufs;

    device_call(char *err_, int64_t err_len_) : err(err_), err_len(err_len_) {}
    device_call(const device_call &) = delete;
    void operator=(const device_call &) = delete;
    ~device_call()
    {
        for (void *p : bufs) hipFree(p);
        if (e0) hipEventDestroy(e0);
        if (e1) hipEventDestroy(e1);
        if (s) hipStreamDestroy(s);
    }
    /* SIFT3D_OK, or SIFT3D_ERR_DEVICE and "<call> failed: <hip error>" in err */
    int check(hipError_t e, const char *call) { return e == hipSuccess ? SIFT3D_OK : call_fail(err, err_len, SIFT3D_ERR_DEVICE, "%s failed: %s", call, hipGetErrorString(e)); }
    /* make dev current and create the stream, and the two events when the call is timed */
    hipError_t open(int dev, bool timed = true)
    {
        device = dev;
        hipError_t e = hipSetDevice(dev);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        if (e == hipSuccess && timed) e = hipEventCreate(&e0);
        if (e == hipSuccess && timed) e = hipEventCreate(&e1);
        return e;
    }
    /* n elements, freed with the call */
    template <class T> hipError_t alloc(T **d, size_t n)
    {
        const hipError_t e = sift3d_alloc_device((void **)d, sizeof(T) * n);
        if (e == hipSuccess) bufs.push_back((void *)*d);
        return e;
    }
    template <class T> hipError_t to_device(T *d, const T *h, size_t n) { return hipMemcpyAsync(d, h, sizeof(T) * n, hipMemcpyHostToDevice, s); }
    template <class T> hipError_t upload(T **d, const T *h, size_t n)
    {
        const hipError_t e = alloc(d, n);
        return e == hipSuccess ? to_device(*d, h, n) : e;
    }
    template <class T> hipError_t download(T *h, const T *d, size_t n) { return hipMemcpyAsync(h, d, sizeof(T) * n, hipMemcpyDeviceToHost, s); }
    hipError_t sync() { return hipStreamSynchronize(s); }
    /* the e0 .. e1 interval over runs into *ms, where ms is given */
    hipError_t elapsed_ms(double *ms, int runs = 1)
    {
        float t = 0;
        const hipError_t e = ms ? hipEventElapsedTime(&t, e0, e1) : hipSuccess;
        if (ms && e == hipSuccess) *ms = (double)t / runs;
        return e;
    }
};

/* return the call's error code when a HIP call fails */
#define DEVCHK(dc, call)                                      \
    do {                                                      \
        const int rc_ = (dc).check((call), #call);            \
        if (rc_ != SIFT3D_OK) return rc_;                     \
    } while (0)

#pragma GCC visibility pop
#endif
