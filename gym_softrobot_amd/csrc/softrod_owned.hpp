// softrod_owned.hpp — who releases what the host side allocates (host only: no kernel, no device code).
//
// Every device buffer, pinned buffer and event of a handle is a member of one of these move-only owners, or sits in
// a struct or vector of them, and is released by the owner's destructor: there is no release code to keep in step
// with the features (softrod_capi.hip's softrod_destroy is `delete h`).  Each HIP allocation and release call of the
// library is written once, here; softrod_capi.hip has none outside its softrod_exchange_* functions, whose memory
// belongs to the caller.
//
// The same types make a set-up safe to fail: an entry point builds what it needs in LOCAL owners and moves them into
// the handle only after its last fallible call has succeeded ("Owners and set-ups"), so an early return
// releases exactly what the attempt made and leaves the handle as it was.
//
// Assigning to an owner releases what it held at that point, under the caller's device guard; hipFree waits for the
// device, so no kernel still uses the old buffer.  These are owners and nothing more — no pool, no registry, no sizes.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace softrod {

// device memory
template <class T>
class DeviceBuf {
    T* p_ = nullptr;
public:
    DeviceBuf() = default;
    DeviceBuf(DeviceBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
    DeviceBuf& operator=(DeviceBuf&& o) noexcept {
        DeviceBuf old(std::move(*this));        // released when this operator returns
        p_ = std::exchange(o.p_, nullptr);
        return *this;
    }
    ~DeviceBuf() { if (p_) (void)hipFree(p_); }
    // For an empty owner.  zeroed: hipMemset behind the allocation; if that fails the owner still holds the buffer
    // (get() tells an allocation that failed from a fill that did).
    hipError_t alloc(size_t bytes, bool zeroed = false) {
        const hipError_t e = hipMalloc((void**)&p_, bytes);
        if (e != hipSuccess) { p_ = nullptr; return e; }
        return zeroed ? hipMemset(p_, 0, bytes) : hipSuccess;
    }
    T* get() const { return p_; }
};

// pinned host memory
template <class T>
class PinnedBuf {
    T* p_ = nullptr;
public:
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
    PinnedBuf& operator=(PinnedBuf&& o) noexcept {
        PinnedBuf old(std::move(*this));
        p_ = std::exchange(o.p_, nullptr);
        return *this;
    }
    ~PinnedBuf() { if (p_) (void)hipHostFree(p_); }
    hipError_t alloc(size_t bytes) {
        const hipError_t e = hipHostMalloc((void**)&p_, bytes, hipHostMallocDefault);
        if (e != hipSuccess) p_ = nullptr;
        return e;
    }
    T* get() const { return p_; }
};

// an event, created with the flags given
class Event {
    hipEvent_t ev_ = nullptr;
public:
    Event() = default;
    Event(Event&& o) noexcept : ev_(std::exchange(o.ev_, nullptr)) {}
    Event& operator=(Event&& o) noexcept {
        Event old(std::move(*this));
        ev_ = std::exchange(o.ev_, nullptr);
        return *this;
    }
    ~Event() { if (ev_) (void)hipEventDestroy(ev_); }
    hipError_t create(unsigned flags) {
        const hipError_t e = hipEventCreateWithFlags(&ev_, flags);
        if (e != hipSuccess) ev_ = nullptr;
        return e;
    }
    hipEvent_t get() const { return ev_; }
};

// Rows on their way to the device: the pinned staging buffer the host fills, its device twin, and the event that
// guards reuse of the pinned side.  The three are allocated by the set-up that owns the triple, one call each.
template <class T>
struct Upload {
    DeviceBuf<T> dev;
    PinnedBuf<T> host;
    Event ev;
    // the previous upload has left the pinned side: the host may write it again
    hipError_t wait() const { return hipEventSynchronize(ev.get()); }
    // the first n rows go out on `st`; the guard is recorded behind them
    hipError_t send(size_t n, hipStream_t st) const {
        const hipError_t e = hipMemcpyAsync(dev.get(), host.get(), n * sizeof(T), hipMemcpyHostToDevice, st);
        return e != hipSuccess ? e : hipEventRecord(ev.get(), st);
    }
};

}  // namespace softrod
