// avt_host.h (private, host only) — the three conventions every C ABI of libavatar_hip.so shares: the HIP status macro,
// the guard that keeps C++ exceptions inside the library, and the owner of one device allocation.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <exception>
#include <string>

void avt_set_error(const std::string& s);

// on a HIP error: the last-error text becomes "<expression>: <hipGetErrorString>" and the enclosing function returns 1
#define AVT_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { avt_set_error(std::string(#x) + ": " + hipGetErrorString(e_)); return 1; } } while (0)

// no C++ exception crosses the C ABI: an entry point is `return avt_guard("avt_x", [&]() -> int { ... });`
template <class F>
int avt_guard(const char* name, F&& body) {
    try { return body(); }
    catch (const std::exception& e) { avt_set_error(std::string(name) + ": " + e.what()); return 1; }
    catch (...) { avt_set_error(std::string(name) + ": unknown exception"); return 1; }
}

// Move-only owner of one device allocation of `cap` elements.  A buffer that was never allocated makes no HIP call, so a
// handle without a device can hold one.  hipFree synchronises the device: a DevBuf that goes away while work on it is
// still queued waits for that work first.
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~DevBuf() { release(); }
    operator T*() const { return p; }     // launch wrappers and hipMemcpy calls take the raw pointer
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    // discard: too small -> free FIRST (the peak footprint must not rise), then exactly n elements (+ pad_bytes); the contents are lost
    int reserve(size_t n, size_t pad_bytes = 0) {
        if (n <= cap) return 0;
        release();
        AVT_HIP(hipMalloc((void**)&p, n * sizeof(T) + pad_bytes));
        cap = n;
        return 0;
    }
    // keep: too small -> max(n, 2 cap) elements (exactly n without `doubling`), the first `keep` copied over on `s`; the old
    // block goes after the stream has drained, and a failed copy frees the new block
    int grow(size_t n, size_t keep, hipStream_t s, bool doubling = true) {
        if (n <= cap) return 0;
        DevBuf q;
        if (q.reserve(doubling ? std::max(n, 2 * cap) : n)) return 1;
        if (keep) AVT_HIP(hipMemcpyAsync(q.p, p, keep * sizeof(T), hipMemcpyDeviceToDevice, s));
        AVT_HIP(hipStreamSynchronize(s));
        *this = std::move(q);             // q leaves with the old block
        return 0;
    }
};
