// Error reporting and the buffers that own their memory: the part of sq_common.hpp that needs nothing of the runtime
// but its allocation, free and copy calls (tests/host compiles it against a stand-in <hip/hip_runtime.h>).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <utility>

#include "../../include/smqtk_hip.h"

namespace sq {

// ------------------------------------------------------------------ errors
extern thread_local char g_err[512];
inline int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define SQ_HIP(expr)                                                                  \
    do {                                                                              \
        hipError_t e_ = (expr);                                                       \
        if (e_ != hipSuccess)                                                         \
            return sq::fail(e_ == hipErrorOutOfMemory ? SQ_ERR_NOMEM : SQ_ERR_HIP,    \
                            "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),   \
                            __FILE__, __LINE__);                                      \
    } while (0)

// (variadic: an expression such as launch<kernel<A, B>>(...) has commas of its own)
#define SQ_TRY(...)                   \
    do {                              \
        int rc_ = (__VA_ARGS__);      \
        if (rc_ != SQ_OK) return rc_; \
    } while (0)

// ----------------------------------------------------------- owning buffers
// DevBuf, HostPinned and PinnedStage own their memory: move-only, freed by the destructor.  A struct that declares
// one owns it -- a handle, a per-call slot or a function's locals need no list of what to free -- and release() is for
// giving memory back early.

// Device memory.  reserve() never shrinks and does not keep the contents (grow_keep does); alloc_exact() replaces it.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            cap = std::exchange(o.cap, 0);
        }
        return *this;
    }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    // (a local may go out of scope while a kernel that reads it is still queued -- an error return between a launch and
    // its wait: hipFree waits for the device first, which the explicit release() calls have always relied on)
    ~DevBuf() { release(); }
    int reserve(size_t bytes) { return bytes <= cap ? SQ_OK : alloc_exact(bytes + (bytes >> 3) + 256); }
    // a new block of exactly `want` bytes (16 for none), whatever the buffer held: arrays that are replaced whole, not grown
    int alloc_exact(size_t want) {
        release();
        if (want == 0) want = 16;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(SQ_ERR_NOMEM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
        }
        cap = want;
        return SQ_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T* as() const { return reinterpret_cast<T*>(p); }
};

// Room for `need` bytes in b with its first `used` bytes kept (grown by half again at least, so a stream of small
// appends copies the contents O(log) times).  b is untouched when the allocation or the copy fails.
inline int grow_keep(DevBuf& b, size_t used, size_t need) {
    if (need <= b.cap) return SQ_OK;
    DevBuf nb;
    SQ_TRY(nb.reserve(std::max(need, used + used / 2)));
    if (used && b.p && hipMemcpy(nb.p, b.p, used, hipMemcpyDeviceToDevice) != hipSuccess)
        return fail(SQ_ERR_HIP, "device copy failed while growing a buffer");
    b = std::move(nb);
    return SQ_OK;
}

// Pinned host memory the device can address.
struct HostPinned {
    void* p = nullptr;
    size_t cap = 0;
    void* dev = nullptr;   // the block's device address (looked up once per allocation: device_ptr)
    HostPinned() = default;
    HostPinned(HostPinned&& o) noexcept
        : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)), dev(std::exchange(o.dev, nullptr)) {}
    HostPinned& operator=(HostPinned&& o) noexcept {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            cap = std::exchange(o.cap, 0);
            dev = std::exchange(o.dev, nullptr);
        }
        return *this;
    }
    HostPinned(const HostPinned&) = delete;
    HostPinned& operator=(const HostPinned&) = delete;
    ~HostPinned() { release(); }
    int reserve(size_t bytes) {
        if (bytes <= cap) return SQ_OK;
        release();
        hipError_t e = hipHostMalloc(&p, bytes + 256, hipHostMallocDefault);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(SQ_ERR_NOMEM, "hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        }
        cap = bytes + 256;
        return SQ_OK;
    }
    // device address of the block (a runtime call of a few microseconds: cached per allocation)
    int device_ptr(void** out) {
        if (!dev) {
            hipError_t e = hipHostGetDevicePointer(&dev, p, 0);
            if (e != hipSuccess) {
                dev = nullptr;
                return fail(SQ_ERR_HIP, "hipHostGetDevicePointer failed: %s", hipGetErrorString(e));
            }
        }
        *out = dev;
        return SQ_OK;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        dev = nullptr;
        cap = 0;
    }
};

// Small host buffers travel through pinned staging: an "asynchronous" copy from or to pageable memory is a
// blocking staged copy inside the runtime (~10-15 us each; a one-query search makes three to five of them).
// in(): memcpy into the pinned block, asynchronous H2D from there.  out(): asynchronous D2H into the block;
// finish() -- after the stream has drained -- copies the pieces to the caller's buffers.  Calls above
// kStageMax bytes in total copy directly.  (Owns its block through `pin`: moving one empties the source's.)
struct PinnedStage {
    static constexpr size_t kStageMax = 1u << 20;
    HostPinned pin;
    size_t used = 0;
    bool on = false;
    struct Out {
        void* dst;
        size_t off, bytes;
    };
    Out outs[4];
    int n_out = 0;
    int begin(size_t total_bytes) {
        used = 0;
        n_out = 0;
        on = total_bytes <= kStageMax;
        return on ? pin.reserve(total_bytes + 64 * 8) : SQ_OK;
    }
    hipError_t in(void* dev, const void* host, size_t bytes, hipStream_t st) {
        if (!on) return hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, st);
        char* at = static_cast<char*>(pin.p) + used;
        memcpy(at, host, bytes);
        used += (bytes + 63) / 64 * 64;
        return hipMemcpyAsync(dev, at, bytes, hipMemcpyHostToDevice, st);
    }
    hipError_t out(void* host, const void* dev, size_t bytes, hipStream_t st) {
        if (!on || n_out >= 4) return hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st);
        outs[n_out++] = Out{host, used, bytes};
        char* at = static_cast<char*>(pin.p) + used;
        used += (bytes + 63) / 64 * 64;
        return hipMemcpyAsync(at, dev, bytes, hipMemcpyDeviceToHost, st);
    }
    void finish() {  // the stream has been waited for
        for (int i = 0; i < n_out; ++i) memcpy(outs[i].dst, static_cast<char*>(pin.p) + outs[i].off, outs[i].bytes);
        n_out = 0;
    }
    void release() { pin.release(); }
};

template <class T>
inline constexpr bool is_move_only_owner = !std::is_copy_constructible<T>::value && !std::is_copy_assignable<T>::value &&
                                           std::is_nothrow_move_constructible<T>::value && std::is_nothrow_move_assignable<T>::value;
static_assert(is_move_only_owner<DevBuf>, "DevBuf: not copyable, nothrow-movable");
static_assert(is_move_only_owner<HostPinned>, "HostPinned: not copyable, nothrow-movable");
static_assert(is_move_only_owner<PinnedStage>, "PinnedStage: not copyable, nothrow-movable");

}  // namespace sq
