/*
 * device_call.h -- what one call of a host-array entry point (sift3d_knn64, the alignment, resampling and guided re-matching
 * calls, the label tools) holds on the device: a non-blocking stream, a set of timing events (stage_events: two in the call, or
 * as many as the entry point's stages need beside it) and its device buffers with the bytes asked for, released together when
 * the call returns; the messages those entry points write into the caller's err, among them the out-of-memory report and the
 * refusal of a volume that holds no labels; and the RMS their reports give.  Internal: nothing here is part of the C-ABI.
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

/* SIFT3D_OK, or SIFT3D_ERR_ARG and the first voxel of labels (n values) that is neither non-finite nor an integer 0 .. 65535;
 * who: "" or what names the volume ("atlas 3: ", "volume a: ") */
inline int check_labels(const char *who, const float *labels, int64_t n, char *err, int64_t err_len)
{
    const int64_t at = sift3d_fuse_check_labels(labels, n);
    if (at < 0) return SIFT3D_OK;
    return call_fail(err, err_len, SIFT3D_ERR_ARG, "%sthe label %g at voxel %lld is neither non-finite nor an integer 0 .. 65535", who, (double)labels[at],
                     (long long)at);
}

/* kernels_label.hip: labels (n floats) to the uint16 plane lab and the validity bits valid ((n + 63) / 64 words) */
hipError_t sift3d_launch_label_plane(hipStream_t s, const float *labels, int64_t n, unsigned short *lab, unsigned long long *valid);

/* N events around the stages of a call; which pairs of them make a stage is the caller's table */
template <int N> struct stage_events {
    hipEvent_t e[N] = {};
    stage_events() = default;
    stage_events(const stage_events &) = delete;
    void operator=(const stage_events &) = delete;
    ~stage_events()
    {
        for (hipEvent_t x : e)
            if (x) hipEventDestroy(x);
    }
    hipError_t create()
    {
        hipError_t rc = hipSuccess;
        for (int i = 0; i < N && rc == hipSuccess; i++) rc = hipEventCreate(&e[i]);
        return rc;
    }
    hipError_t record(int i, hipStream_t s) const { return hipEventRecord(e[i], s); }
    /* the time between two recorded events into *ms; the stream has been synchronised */
    hipError_t elapsed(int from, int to, double *ms) const
    {
        float t = 0;
        const hipError_t rc = hipEventElapsedTime(&t, e[from], e[to]);
        if (rc == hipSuccess) *ms = (double)t;
        return rc;
    }
};

struct device_call {
    char *err;
    int64_t err_len;
    int device = 0;
    hipStream_t s = nullptr;
    stage_events<2> ev;
    std::vector<void *> bufs;
    size_t asked = 0; /* the bytes of every alloc so far, the one that failed included */

    device_call(char *err_, int64_t err_len_) : err(err_), err_len(err_len_) {}
    device_call(const device_call &) = delete;
    void operator=(const device_call &) = delete;
    ~device_call()
    {
        for (void *p : bufs) hipFree(p);
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
        if (e == hipSuccess && timed) e = ev.create();
        return e;
    }
    /* n elements, freed with the call */
    template <class T> hipError_t alloc(T **d, size_t n)
    {
        asked += sizeof(T) * n;
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
    /* the call's two events: mark(0) before what is timed, mark(1) after it */
    hipError_t mark(int i) { return ev.record(i, s); }
    /* the interval between the two marks over runs into *ms, where ms is given */
    hipError_t elapsed_ms(double *ms, int runs = 1)
    {
        const hipError_t e = ms ? ev.elapsed(0, 1, ms) : hipSuccess;
        if (ms && e == hipSuccess) *ms /= runs;
        return e;
    }
    /* an alloc has failed: SIFT3D_ERR_MEMORY and the bytes the call has asked for in err; clause (printf): what they were for */
    __attribute__((format(printf, 2, 3))) int no_memory(const char *clause = nullptr, ...)
    {
        (void)hipGetLastError();
        char what[128] = "";
        if (clause) {
            va_list ap;
            va_start(ap, clause);
            vsnprintf(what, sizeof what, clause, ap);
            va_end(ap);
        }
        return call_fail(err, err_len, SIFT3D_ERR_MEMORY, "cannot allocate %zu bytes on device %d%s", asked, device, what);
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
