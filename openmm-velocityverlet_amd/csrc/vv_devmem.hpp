// vv_devmem.hpp -- who owns the plan's memory: move-only owners of device buffers, pinned host words and hipIpc mappings that free
// in their destructor.  Host only; sizes are BYTES everywhere (half of the plan's buffers change their element with the precision).
// The HIP allocation and free calls of libvvhip live here and in the caller-owned vvhip_malloc / vvhip_free, nowhere else.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <utility>
#include <vector>

namespace vv {

// What the owners below hold at this moment, process-wide (vvhip_debug_live_buffers): buffers and mappings / bytes of the buffers
inline std::atomic<long long> live_buffers{0}, live_bytes{0};

// Device memory.  alloc / alloc_uncached replace what the buffer held; a request of 0 bytes leaves it empty (as hipMalloc does).
template <class T>
class DevBuf {
    T* ptr_ = nullptr;
    size_t bytes_ = 0;
    hipError_t take(size_t bytes, bool uncached) {
        reset();
        void* q = nullptr;
        const hipError_t e = uncached ? hipExtMallocWithFlags(&q, bytes, hipDeviceMallocUncached) : hipMalloc(&q, bytes);
        if (e != hipSuccess || !q) return e;
        ptr_ = (T*) q; bytes_ = bytes;
        live_buffers++; live_bytes += (long long) bytes;
        return hipSuccess;
    }
public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : ptr_(std::exchange(o.ptr_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); ptr_ = std::exchange(o.ptr_, nullptr); bytes_ = std::exchange(o.bytes_, 0); } return *this; }
    ~DevBuf() { reset(); }
    T* get() const { return ptr_; }
    explicit operator bool() const { return ptr_ != nullptr; }
    size_t bytes() const { return bytes_; }
    void reset() {
        if (!ptr_) return;
        (void) hipFree((void*) ptr_);
        live_buffers--; live_bytes -= (long long) bytes_;
        ptr_ = nullptr; bytes_ = 0;
    }
    hipError_t alloc(size_t bytes) { return take(bytes, false); }
    hipError_t alloc_uncached(size_t bytes) { return take(bytes, true); }      // polled across XCDs / written by peers: never served from an L2
    // keeps a buffer that already holds `bytes`, replaces a smaller one (its contents go)
    hipError_t ensure(size_t bytes) { return ptr_ && bytes_ >= bytes ? hipSuccess : alloc(bytes); }
};

// Pinned host memory; `mapped`: the device reaches the same words (hipHostGetDevicePointer)
template <class T>
class PinnedBuf {
    T* ptr_ = nullptr;
    size_t bytes_ = 0;
public:
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&& o) noexcept : ptr_(std::exchange(o.ptr_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    PinnedBuf& operator=(PinnedBuf&& o) noexcept { if (this != &o) { reset(); ptr_ = std::exchange(o.ptr_, nullptr); bytes_ = std::exchange(o.bytes_, 0); } return *this; }
    ~PinnedBuf() { reset(); }
    T* get() const { return ptr_; }
    explicit operator bool() const { return ptr_ != nullptr; }
    T& operator[](size_t i) const { return ptr_[i]; }
    size_t bytes() const { return bytes_; }
    void reset() {
        if (!ptr_) return;
        (void) hipHostFree((void*) ptr_);
        live_buffers--; live_bytes -= (long long) bytes_;
        ptr_ = nullptr; bytes_ = 0;
    }
    hipError_t alloc(size_t bytes, bool mapped = false) {
        reset();
        void* q = nullptr;
        const hipError_t e = hipHostMalloc(&q, bytes, mapped ? hipHostMallocMapped : hipHostMallocDefault);
        if (e != hipSuccess || !q) return e;
        ptr_ = (T*) q; bytes_ = bytes;
        live_buffers++; live_bytes += (long long) bytes;
        return hipSuccess;
    }
};

// Another process's buffer mapped into this one (hipIpcOpenMemHandle); closed, not freed
class IpcMapping {
    void* ptr_ = nullptr;
public:
    IpcMapping() = default;
    IpcMapping(IpcMapping&& o) noexcept : ptr_(std::exchange(o.ptr_, nullptr)) {}
    IpcMapping& operator=(IpcMapping&& o) noexcept { if (this != &o) { reset(); ptr_ = std::exchange(o.ptr_, nullptr); } return *this; }
    ~IpcMapping() { reset(); }
    void* get() const { return ptr_; }
    void reset() {
        if (!ptr_) return;
        (void) hipIpcCloseMemHandle(ptr_);
        live_buffers--;
        ptr_ = nullptr;
    }
    hipError_t open(const hipIpcMemHandle_t& h) {
        reset();
        const hipError_t e = hipIpcOpenMemHandle(&ptr_, h, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) { ptr_ = nullptr; return e; }
        live_buffers++;
        return hipSuccess;
    }
};

// A table as the host built it: allocation (of `floor` bytes at least) + blocking copy
template <class T, class U>
hipError_t upload(DevBuf<T>& buf, const std::vector<U>& v, size_t floor = 0) {
    const size_t bytes = v.size() * sizeof(U);
    const hipError_t e = buf.alloc(bytes > floor ? bytes : floor);
    if (e != hipSuccess || !bytes) return e;
    return hipMemcpy((void*) buf.get(), v.data(), bytes, hipMemcpyHostToDevice);
}
// Zero-filled scratch: allocation + fill ON THE PLAN'S STREAM.  (Every fill of a plan buffer goes there: a plain hipMemset only enqueues
// on the null stream, which a non-blocking stream does not wait for -- the reset of both accumulator copies at a switch of the cos
// perturbation (vvhip_set_params) could land a step later and wipe kernel A's sums; found by the adapter fuzz when a host stall changed
// the timing, tests/test_cpp_plugin.py)
template <class T>
hipError_t zeros(DevBuf<T>& buf, size_t bytes, hipStream_t stream, bool uncached = false) {
    const hipError_t e = uncached ? buf.alloc_uncached(bytes) : buf.alloc(bytes);
    if (e != hipSuccess || !bytes) return e;
    return hipMemsetAsync((void*) buf.get(), 0, bytes, stream);
}

}  // namespace vv
