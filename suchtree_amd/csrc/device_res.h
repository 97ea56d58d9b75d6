// device_res.h -- host-only owners of HIP resources: device memory (DevBuf), pinned host memory (PinnedBuf), a stream
// (Stream, DrainedStream), an event (Event).  Move-only (a declared move constructor deletes copying).  Each reads as the
// raw pointer or handle it owns, so kernel arguments, null tests and pointer arithmetic are written as on a raw field.
// What the code around them relies on:
//   * a destructor only releases: it reports nothing and leaves the thread's error message alone;
//   * a destructor runs with the owning device current: call-scoped owners are declared after ST_DEVICE(...), owners
//     inside a heap object die in a `delete` under a DeviceScope;
//   * no owner has static storage duration (the runtime may be gone before a static destructor runs);
//   * Stream's destructor does not synchronise: whoever owns memory that the stream's work touches drains it first.  A
//     call's own stream is a DrainedStream, whose destructor does: memory that the stream's work touches is declared
//     before the DrainedStream; reverse destruction order does the rest.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace st {

template <typename T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(o.release()) {}
    DevBuf &operator=(DevBuf &&o) noexcept { std::swap(p_, o.p_); return *this; }      // (what was held dies with o)
    ~DevBuf() { reset(); }

    // `count` elements; what was held goes first, and a failure leaves null
    hipError_t alloc(size_t count)
    {
        reset();
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&p_), count * sizeof(T));
        if (e != hipSuccess) p_ = nullptr;
        return e;
    }
    void reset() { if (p_) (void)hipFree(release()); }
    T *release() { return std::exchange(p_, nullptr); }
    T *get() const { return p_; }
    operator T *() const { return p_; }

private:
    T *p_ = nullptr;
};

template <typename T>
class PinnedBuf {
public:
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf &&o) noexcept : p_(o.release()) {}
    PinnedBuf &operator=(PinnedBuf &&o) noexcept { std::swap(p_, o.p_); return *this; }
    ~PinnedBuf() { reset(); }

    hipError_t alloc(size_t count, unsigned flags)
    {
        reset();
        const hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&p_), count * sizeof(T), flags);
        if (e != hipSuccess) p_ = nullptr;
        return e;
    }
    void reset() { if (p_) (void)hipHostFree(release()); }
    T *release() { return std::exchange(p_, nullptr); }
    T *get() const { return p_; }
    operator T *() const { return p_; }

private:
    T *p_ = nullptr;
};

// a stream of its own beside the caller's: hipStreamNonBlocking
class Stream {
public:
    Stream() = default;
    Stream(Stream &&o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
    Stream &operator=(Stream &&o) noexcept { std::swap(s_, o.s_); return *this; }
    ~Stream() { reset(); }

    hipError_t create()
    {
        reset();
        const hipError_t e = hipStreamCreateWithFlags(&s_, hipStreamNonBlocking);
        if (e != hipSuccess) s_ = nullptr;
        return e;
    }
    void reset() { if (s_) (void)hipStreamDestroy(std::exchange(s_, nullptr)); }
    operator hipStream_t() const { return s_; }

private:
    hipStream_t s_ = nullptr;
};

struct DrainedStream : Stream {      // the stream of one call, not moved: drained, then destroyed
    ~DrainedStream() { if (*this) (void)hipStreamSynchronize(*this); }
};

class Event {
public:
    Event() = default;
    Event(Event &&o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    Event &operator=(Event &&o) noexcept { std::swap(e_, o.e_); return *this; }
    ~Event() { reset(); }

    // (no flags: hipEventCreate's event, which can be timed)
    hipError_t create(unsigned flags = hipEventDefault)
    {
        reset();
        const hipError_t e = hipEventCreateWithFlags(&e_, flags);
        if (e != hipSuccess) e_ = nullptr;
        return e;
    }
    void reset() { if (e_) (void)hipEventDestroy(std::exchange(e_, nullptr)); }
    operator hipEvent_t() const { return e_; }

private:
    hipEvent_t e_ = nullptr;
};

}  // namespace st
