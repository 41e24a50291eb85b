// host_common.h — the host-side frame every component of libatgpu shares:
// the growable device buffer, the per-component error slot with its
// "try a HIP call" macro, and the base of the single-stream codec handles.
// Host code only; nothing here is seen by a kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <initializer_list>
#include <mutex>
#include <string>

#include "../../include/atgpu.h"

// A device allocation that only grows.  No destructor on purpose: several
// components keep these in static per-device contexts, and a hipFree from a
// static destructor at process exit races the runtime's own teardown
// (DESIGN.md section 8).  The owner calls release().
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap && p)
            return hipSuccess;
        release();
        const size_t want = std::max<size_t>(bytes, 256);
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess)
            cap = want;
        return e;
    }
    void release()
    {
        if (p)
            (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// One component's last error message.  Every translation unit keeps its own
// thread_local slot, so atg_*_last_error() reports that component alone.
struct ErrSlot {
    std::string msg;
    atg_status fail(atg_status s, std::string m)
    {
        msg = std::move(m);
        return s;
    }
};

// Try a HIP call; on failure record "<text>: <hipGetErrorString>" in the slot
// and return ATG_ERR_DEVICE.  The text is a parameter because each file wraps
// this as `#define XHIP(expr) ATG_HIP_TRY(g_x_err, expr, #expr)`: stringifying
// in the wrapper keeps the expression as written, where a `#expr` in here
// would see it after macro expansion (hipStreamNonBlocking as 0x01).
#define ATG_HIP_TRY(slot, expr, text)                                                    \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess)                                                            \
            return (slot).fail(ATG_ERR_DEVICE,                                           \
                               std::string(text ": ") + hipGetErrorString(e_));          \
    } while (0)

// Base of the codec handles that run one batch at a time on one non-blocking
// stream and time its N-1 stages with N events: times[k] is ev[k] -> ev[k+1],
// times[N-1] the whole run.  The codec's struct derives from this and adds
// its buffers; open_handle() below creates one.
template <int N> struct StageHandle {
    std::recursive_mutex mu; // held by every public entry point (handle_lock.h)
    int device = 0;
    hipStream_t s = nullptr;
    hipEvent_t ev[N] = {};
    float times[N] = {};
    bool have_times = false;

    // after the run's last synchronise
    void finish_times()
    {
        for (int k = 0; k < N - 1; ++k)
            (void)hipEventElapsedTime(&times[k], ev[k], ev[k + 1]);
        (void)hipEventElapsedTime(&times[N - 1], ev[0], ev[N - 1]);
        have_times = true;
    }

    // the body of *_kernel_times
    int report(const char *const (&stage)[N], const char **names, float *ms, int cap) const
    {
        if (!have_times)
            return 0;
        const int k = cap < N ? cap : N;
        for (int i = 0; i < k; ++i) {
            if (names)
                names[i] = stage[i];
            if (ms)
                ms[i] = times[i];
        }
        return k;
    }

    // Drain the stream, free the codec's buffers, then the events and the
    // stream; any of them may still be null after a failed create.
    void close(std::initializer_list<DevBuf *> bufs)
    {
        (void)hipSetDevice(device);
        if (s)
            (void)hipStreamSynchronize(s);
        for (DevBuf *b : bufs)
            b->release();
        for (hipEvent_t &e : ev)
            if (e)
                (void)hipEventDestroy(e);
        if (s)
            (void)hipStreamDestroy(s);
    }
};

// The shared part of *_create: the argument checks, then a new H on `device`
// with its stream and events.  On failure *out stays null and nothing is
// left allocated.  What else the codec needs it makes afterwards.
template <class H> atg_status open_handle(int device, H **out, ErrSlot &slot, const char *what)
{
    if (!out)
        return slot.fail(ATG_ERR_INVALID, "out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return slot.fail(ATG_ERR_DEVICE, "no HIP device available");
    if (device < 0 || device >= n)
        return slot.fail(ATG_ERR_INVALID, "device index out of range");
    ATG_HIP_TRY(slot, hipSetDevice(device), "hipSetDevice(device)");
    H *h = new H();
    h->device = device;
    hipError_t err = hipStreamCreateWithFlags(&h->s, hipStreamNonBlocking);
    for (hipEvent_t &e : h->ev)
        if (err == hipSuccess)
            err = hipEventCreate(&e);
    if (err != hipSuccess) {
        h->close({});
        delete h;
        return slot.fail(ATG_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(err));
    }
    *out = h;
    return ATG_OK;
}
