// host_common.h — the host-side frame every component of libatgpu shares:
// the growable device and pinned buffers, the per-component error slot with its
// "try a HIP call" macro, the stage times, the base of the single-stream
// codec handles, and what a component without a handle is made of: its
// per-device contexts, its one timed launch, the device it runs on and the
// staging of its *_host entries.  Host code only; nothing here is seen by a kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <initializer_list>
#include <mutex>
#include <string>
#include <vector>

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

// The pinned-host counterpart: n elements of T, at least 16, growing only.
// No destructor either, for DevBuf's reason (teardown);
// the owner calls release().
template <class T> struct PinBuf {
    T *p = nullptr;
    size_t cap = 0; // elements
    hipError_t ensure(size_t n)
    {
        if (p && n <= cap)
            return hipSuccess;
        release();
        const size_t want = std::max<size_t>(n, 16);
        hipError_t e = hipHostMalloc((void **)&p, want * sizeof(T), hipHostMallocDefault);
        if (e == hipSuccess)
            cap = want;
        return e;
    }
    void release()
    {
        if (p)
            (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};

// release() on every buffer named, DevBufs and PinBufs alike
template <class... B> void release_all(B &...b) { (b.release(), ...); }

// A non-blocking stream at the device's highest stream priority.
inline hipError_t high_priority_stream(hipStream_t *s)
{
    int prio_lo = 0, prio_hi = 0;
    hipError_t e = hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    if (e == hipSuccess)
        e = hipStreamCreateWithPriority(s, hipStreamNonBlocking, prio_hi);
    return e;
}

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

// The body of every *_kernel_times: the first min(cap, n) names and values.
// A second call with at = what the first returned appends its stages as far
// as cap still allows.  Returns the entries written so far.
inline int copy_times(const char *const *stage, const float *times, int n, const char **names,
                      float *ms, int cap, int at = 0)
{
    const int k = std::max(0, std::min(cap - at, n));
    for (int i = 0; i < k; ++i) {
        if (names)
            names[at + i] = stage[i];
        if (ms)
            ms[at + i] = times[i];
    }
    return at + k;
}

// The stage times of a component without a handle: one thread_local per
// component, so a thread reads its own last call.  n counts the valid
// entries, 0 before the thread's first call.
template <int N> struct StageTimes {
    float ms[N] = {};
    int n = 0;
};

// Create the events of an array that are still null.
template <int N> hipError_t ensure_events(hipEvent_t (&ev)[N])
{
    hipError_t err = hipSuccess;
    for (hipEvent_t &e : ev)
        if (!e && err == hipSuccess)
            err = hipEventCreate(&e);
    return err;
}

// The events of a handle that only order streams: no timestamps taken.
template <size_t N> hipError_t create_fences(std::array<hipEvent_t *, N> evs)
{
    hipError_t err = hipSuccess;
    for (hipEvent_t *e : evs)
        if (err == hipSuccess)
            err = hipEventCreateWithFlags(e, hipEventDisableTiming);
    return err;
}

// Destroy an event that may still be null (a create that failed part-way).
inline void destroy_event(hipEvent_t &e)
{
    if (e)
        (void)hipEventDestroy(e);
    e = nullptr;
}

// The context of a component that keeps one table per device: the table and
// the two events that time its launch.
struct TableCtx {
    DevBuf table;
    hipEvent_t ev[2] = {nullptr, nullptr};
};

// One timed launch on a held context's table buffer and two events: the host
// table goes up, launch(device table) enqueues the kernel(s) on s between the
// events, before_sync() the device-to-host copies, then s is synchronised.
// *ms is the time between the events, negative where HIP could not tell.
template <class Row, class Launch, class Hook = hipError_t (*)()>
atg_status timed_launch(DevBuf &table, hipEvent_t (&ev)[2], const std::vector<Row> &tab,
                        hipStream_t s, ErrSlot &slot, float *ms, Launch launch,
                        Hook before_sync = [] { return hipSuccess; })
{
    const size_t bytes = sizeof(Row) * tab.size();
    ATG_HIP_TRY(slot, ensure_events(ev), "hipEventCreate(&e)");
    ATG_HIP_TRY(slot, table.ensure(bytes), "table.ensure(bytes)");
    ATG_HIP_TRY(slot, hipMemcpyAsync(table.p, tab.data(), bytes, hipMemcpyHostToDevice, s),
                "hipMemcpyAsync(table.p, tab.data(), bytes, hipMemcpyHostToDevice, s)");
    ATG_HIP_TRY(slot, hipEventRecord(ev[0], s), "hipEventRecord(ev[0], s)");
    launch((const Row *)table.p);
    ATG_HIP_TRY(slot, hipGetLastError(), "hipGetLastError()");
    ATG_HIP_TRY(slot, hipEventRecord(ev[1], s), "hipEventRecord(ev[1], s)");
    ATG_HIP_TRY(slot, before_sync(), "before_sync()");
    ATG_HIP_TRY(slot, hipStreamSynchronize(s), "hipStreamSynchronize(s)");
    if (hipEventElapsedTime(ms, ev[0], ev[1]) != hipSuccess)
        *ms = -1.f;
    return ATG_OK;
}

// The head of every entry that takes a device index: the index checked, the
// device made current.
inline atg_status use_device(int device, ErrSlot &slot)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return slot.fail(ATG_ERR_DEVICE, "no HIP device available");
    if (device < 0 || device >= n)
        return slot.fail(ATG_ERR_INVALID, "device index out of range");
    ATG_HIP_TRY(slot, hipSetDevice(device), "hipSetDevice(device)");
    return ATG_OK;
}

// A device allocation of one call, freed at scope exit: the staging buffers
// of the *_host entries.  Always a local, so DevBuf's reason to have no
// destructor does not reach it.  alloc() hands back HIP's error and the
// caller words it, each component in its own status and text.
struct DevTemp {
    void *p = nullptr;
    DevTemp() = default;
    DevTemp(const DevTemp &) = delete;
    DevTemp &operator=(const DevTemp &) = delete;
    ~DevTemp()
    {
        if (p)
            (void)hipFree(p);
    }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
};

// The static per-device state of a component without a handle: one Ctx per
// device, each behind a mutex, and the only way to one is hold(), which
// returns it locked.  Ctx keeps DevBufs and events and has no destructor,
// like DevBuf and for its reason.
constexpr int kMaxDevices = 64;

template <class Ctx> class DeviceContexts {
    struct Slot {
        std::mutex mu;
        Ctx ctx;
    };
    Slot slots_[kMaxDevices];

  public:
    // a context for as long as this lives
    class Held {
        friend class DeviceContexts;
        std::unique_lock<std::mutex> lock_;
        Ctx *c_ = nullptr;

      public:
        Ctx &operator*() const { return *c_; }
        Ctx *operator->() const { return c_; }
    };

    // Run where the buffers are: a sharded caller's thread may sit elsewhere.
    // The device that holds d_ptr is made current; for NULL or a pointer HIP
    // does not know, the current device stands.  Then that device's context,
    // locked, into `out`.
    atg_status hold(const void *d_ptr, ErrSlot &slot, Held &out)
    {
        int dev = 0;
        hipPointerAttribute_t attr;
        if (d_ptr && hipPointerGetAttributes(&attr, d_ptr) == hipSuccess &&
            attr.type == hipMemoryTypeDevice) {
            dev = attr.device;
            ATG_HIP_TRY(slot, hipSetDevice(dev), "hipSetDevice(dev)");
        } else {
            (void)hipGetLastError();
            ATG_HIP_TRY(slot, hipGetDevice(&dev), "hipGetDevice(&dev)");
        }
        if (dev < 0 || dev >= kMaxDevices)
            return slot.fail(ATG_ERR_UNSUPPORTED, "device index too large");
        out.lock_ = std::unique_lock<std::mutex>(slots_[dev].mu);
        out.c_ = &slots_[dev].ctx;
        return ATG_OK;
    }
};

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
        return have_times ? copy_times(stage, times, N, names, ms, cap) : 0;
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
            destroy_event(e);
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
    const atg_status st = use_device(device, slot);
    if (st != ATG_OK)
        return st;
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
