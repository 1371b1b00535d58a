// device_owner.h — the one owner of each kind of HIP resource the host side of libptrt.so holds: device buffer, event, stream, pinned
// host block. All are move-only (a move leaves the source empty) and release in their destructor, on whatever device is current then:
// whoever destroys an owner sets the device first. No other file of the library frees or creates these resources.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <utility>

namespace ptrt {

// Counts DevBuf allocations of the calling thread: a frame that had to allocate is a cold frame (its rate is not a measurement). Only ever
// compared between the start and the end of one pt_render, so what other calls (a commit, the LBVH builder's scratch, pt_comm) add is harmless.
inline thread_local uint64_t g_device_allocs = 0;

template <typename T> struct DevBuf {
    T *p = nullptr; size_t n = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), n(std::exchange(o.n, 0)) {}
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { release(); p = std::exchange(o.p, nullptr); n = std::exchange(o.n, 0); } return *this; }
    ~DevBuf() { release(); }
    hipError_t ensure(size_t count)
    {
        if (p && count <= n && (n <= (1u << 20) || count >= n / 4)) return hipSuccess; // big enough, and not more than 4x too big
        ++g_device_allocs;
        release();
        hipError_t e = hipMalloc((void **)&p, (count ? count : 1) * sizeof(T));
        if (e == hipSuccess) n = count ? count : 1;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};

// An event or a stream. `borrowed`: the handle is the caller's (pt_device_desc::stream) and is left alone.
template <typename H, hipError_t (*Destroy)(H)> struct Handle {
    H h = nullptr; bool borrowed = false;
    Handle() = default;
    Handle(Handle &&o) noexcept : h(std::exchange(o.h, nullptr)), borrowed(o.borrowed) {}
    Handle &operator=(Handle &&o) noexcept { if (this != &o) { reset(); h = std::exchange(o.h, nullptr); borrowed = o.borrowed; } return *this; }
    ~Handle() { reset(); }
    void reset() { if (h && !borrowed) (void)Destroy(h); h = nullptr; }
    operator H() const { return h; }
};
struct Event : Handle<hipEvent_t, hipEventDestroy> {
    // on first use (a later call is a no-op); timing = false: an event that only orders streams
    hipError_t create(bool timing = true) { return h ? hipSuccess : timing ? hipEventCreate(&h) : hipEventCreateWithFlags(&h, hipEventDisableTiming); }
};
struct Stream : Handle<hipStream_t, hipStreamDestroy> {
    hipError_t create() { return hipStreamCreateWithFlags(&h, hipStreamNonBlocking); }
    void borrow(hipStream_t s) { reset(); h = s; borrowed = true; }
};

// Pinned host memory: p is the host address, d the device address of a mapped block (null for a plain one).
template <typename T> struct Pinned {
    T *p = nullptr, *d = nullptr;
    Pinned() = default;
    Pinned(Pinned &&o) noexcept : p(std::exchange(o.p, nullptr)), d(std::exchange(o.d, nullptr)) {}
    Pinned &operator=(Pinned &&o) noexcept { if (this != &o) { release(); p = std::exchange(o.p, nullptr); d = std::exchange(o.d, nullptr); } return *this; }
    ~Pinned() { release(); }
    hipError_t alloc(size_t count, bool mapped = false) // mapped: all or nothing, a block the device cannot address is given back
    {
        release();
        hipError_t e = hipHostMalloc((void **)&p, count * sizeof(T), mapped ? hipHostMallocMapped : hipHostMallocDefault);
        if (mapped && e == hipSuccess && ((e = hipHostGetDevicePointer((void **)&d, p, 0)) != hipSuccess || !d)) { release(); if (e == hipSuccess) e = hipErrorNotSupported; }
        return e;
    }
    void release() { if (p) (void)hipHostFree(p); p = d = nullptr; }
};

} // namespace ptrt
