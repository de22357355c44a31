// The owning buffer types of the library: device memory (DevBuf) and pinned host memory (PinnedBuf). A buffer belongs to the object or
// scope that declares it and is freed with it: a destroy function sets the device and deletes, nothing is released by enumeration. Whoever
// deletes an owner must have made its device current first (hipFree of another device's memory is an error).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <type_traits>
#include <utility>
#include <vector>

namespace iba {

template <class T>
struct DevBuf {
    T* p = nullptr; size_t n = 0;   // n: elements asked for (at least one is allocated)
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), n(std::exchange(o.n, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { release(); p = std::exchange(o.p, nullptr); n = std::exchange(o.n, 0); } return *this; }
    ~DevBuf() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
    // frees what it held; on failure the buffer is empty (the sticky error is the caller's to clear)
    hipError_t alloc(size_t count) {
        release();
        const hipError_t e = hipMalloc((void**)&p, std::max<size_t>(count, 1) * sizeof(T));
        if (e != hipSuccess) p = nullptr; else n = count;
        return e;
    }
    // buffers that only grow: a quarter of headroom, nothing kept of the old contents
    hipError_t grow(size_t count) { return (p && n >= count) ? hipSuccess : alloc(count + count / 4); }
    hipError_t upload(const T* src, size_t count) {   // blocking
        const hipError_t e = alloc(count);
        if (e != hipSuccess || !count) return e;
        return hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice);
    }
    hipError_t upload(const std::vector<T>& v) { return upload(v.data(), v.size()); }
};

template <class T>
struct PinnedBuf {
    T* p = nullptr; size_t n = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    PinnedBuf(PinnedBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), n(std::exchange(o.n, 0)) {}
    PinnedBuf& operator=(PinnedBuf&& o) noexcept { if (this != &o) { release(); p = std::exchange(o.p, nullptr); n = std::exchange(o.n, 0); } return *this; }
    ~PinnedBuf() { release(); }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; n = 0; }
    hipError_t alloc(size_t count, unsigned flags = hipHostMallocDefault) {
        release();
        const hipError_t e = hipHostMalloc((void**)&p, std::max<size_t>(count, 1) * sizeof(T), flags);
        if (e != hipSuccess) p = nullptr; else n = count;
        return e;
    }
    // staging that only grows: at least 64 elements, a quarter of headroom, nothing kept of the old contents
    hipError_t grow(size_t count) { return (p && n >= count) ? hipSuccess : alloc(std::max<size_t>(64, count + count / 4)); }
};

static_assert(!std::is_copy_constructible<DevBuf<int>>::value && std::is_nothrow_move_constructible<DevBuf<int>>::value, "DevBuf is move-only");
static_assert(!std::is_copy_constructible<PinnedBuf<int>>::value && std::is_nothrow_move_constructible<PinnedBuf<int>>::value, "PinnedBuf is move-only");

}  // namespace iba
