// aidfp_buffers.h -- the owners of every device block, page-locked block and event of libaidfp.so's host code. This
// header is the one place that calls hipMalloc / hipFree, hipHostMalloc / hipHostFree and hipEventCreate* /
// hipEventDestroy: whatever holds a DevBuf, a HostBuf or an Event frees it by being destroyed, and the three counts
// below (aid_live_allocations) say how many are alive in the process.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <type_traits>
#include <utility>

#pragma GCC visibility push(hidden)

namespace aid {

struct LiveCounts {
    std::atomic<int64_t> device{0}, pinned{0}, events{0};
};
inline LiveCounts g_live;  // one instance per library

// device buffer. kFloor: the least capacity an allocation gets (1 for the engine's buffers, 64 for the vector
// catalog's, as before they shared this type)
template <typename T, size_t kFloor = 1>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;  // capacity in elements
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), n(std::exchange(o.n, 0)) {}
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            n = std::exchange(o.n, 0);
        }
        return *this;
    }
    ~DevBuf() { release(); }
    // contents are lost on growth; after a failed growth the buffer is empty
    hipError_t reserve(size_t want) {
        if (want <= n) return hipSuccess;
        if (p) (void)hipDeviceSynchronize();  // growing: in-flight work of earlier calls may still use the old buffer
        release();
        const size_t cap = std::max(want, kFloor);
        hipError_t e = hipMalloc((void **)&p, cap * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            return e;
        }
        n = cap;
        ++g_live.device;
        return hipSuccess;
    }
    // grow to hold `want` elements (at least doubling), keeping the first `keep` by a copy on `s`, which is
    // synchronised before the old block goes. A failure leaves the buffer as it was
    hipError_t grow_keep(size_t keep, size_t want, hipStream_t s) {
        if (want <= n) return hipSuccess;
        DevBuf nb;
        hipError_t e = nb.reserve(std::max(want, n * 2));
        keep = p ? std::min(keep, n) : 0;  // nothing stored yet on the first growth
        if (e == hipSuccess && keep) e = hipMemcpyAsync(nb.p, p, keep * sizeof(T), hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e == hipSuccess) std::swap(*this, nb);
        return e;  // nb frees the old block, or the new one after a failure
    }
    void release() {
        if (p) {
            (void)hipFree(p);
            --g_live.device;
        }
        p = nullptr;
        n = 0;
    }
};

// page-locked host buffer (hipHostMalloc): copies to and from it are asynchronous, so a call can queue its
// result copies behind its kernels and wait once. `flags` matter when the block is allocated (hipHostMallocMapped:
// the device can address it)
template <typename T>
struct HostBuf {
    T *p = nullptr;
    size_t n = 0;  // capacity in elements
    HostBuf() = default;
    HostBuf(const HostBuf &) = delete;
    HostBuf &operator=(const HostBuf &) = delete;
    HostBuf(HostBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), n(std::exchange(o.n, 0)) {}
    HostBuf &operator=(HostBuf &&o) noexcept {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            n = std::exchange(o.n, 0);
        }
        return *this;
    }
    ~HostBuf() { release(); }
    // callers have synchronised any copy still using the old buffer; contents are lost on growth
    hipError_t reserve(size_t want, unsigned flags = hipHostMallocDefault) {
        if (want <= n) return hipSuccess;
        release();
        const size_t cap = std::max(want, (size_t)64);
        hipError_t e = hipHostMalloc((void **)&p, cap * sizeof(T), flags);
        if (e != hipSuccess) {
            p = nullptr;
            return e;
        }
        n = cap;
        ++g_live.pinned;
        return hipSuccess;
    }
    void release() {
        if (p) {
            (void)hipHostFree(p);
            --g_live.pinned;
        }
        p = nullptr;
        n = 0;
    }
};

// counted creation and destruction of a raw event (the profiling events, which move between a pool and a list)
inline hipError_t event_create(hipEvent_t *ev, unsigned flags) {
    hipError_t e = hipEventCreateWithFlags(ev, flags);
    if (e == hipSuccess) ++g_live.events;
    return e;
}
inline void event_destroy(hipEvent_t ev) {
    if (!ev) return;
    (void)hipEventDestroy(ev);
    --g_live.events;
}

// an event that orders the reuse of a buffer: record() after the work that uses it, wait() before the reuse.
// live = recorded and not yet waited for
struct Event {
    hipEvent_t ev = nullptr;
    bool live = false;
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event() { event_destroy(ev); }
    hipError_t record(hipStream_t s) {
        if (!ev)
            if (hipError_t e = event_create(&ev, hipEventDisableTiming)) return e;
        hipError_t e = hipEventRecord(ev, s);
        if (e == hipSuccess) live = true;
        return e;
    }
    hipError_t wait() {
        if (!live) return hipSuccess;
        hipError_t e = hipEventSynchronize(ev);
        if (e == hipSuccess) live = false;
        return e;
    }
};

static_assert(!std::is_copy_constructible<DevBuf<float>>::value && !std::is_copy_assignable<DevBuf<float>>::value &&
                  !std::is_copy_constructible<HostBuf<float>>::value && !std::is_copy_assignable<HostBuf<float>>::value &&
                  !std::is_copy_constructible<Event>::value && !std::is_copy_assignable<Event>::value,
              "an owner that could be copied would free its block twice");

}  // namespace aid

#pragma GCC visibility pop
