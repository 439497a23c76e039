// Stand-in for <hip/hip_runtime.h>, for the host programs of tests/host only: the allocation, free and copy calls that
// smqtk_indexing_amd/csrc/sq_buffers.hpp uses, on malloc / free / memcpy, so that the owning buffer types run on a CPU
// under the host sanitizers.  "Device" and pinned memory are plain heap blocks; every copy is done when it returns.
// For smqtk_indexing_amd/csrc/sq_pairwise.hpp (tests/host/pairwise_main.cpp): the function qualifiers as nothing, the
// round-to-nearest adds as plain adds (the programs are compiled with -ffp-contract=off), and a cross-lane exchange
// that only has to compile -- the eight-lane leaf that uses it is not instantiated on a host.
// For smqtk_indexing_amd/csrc/sq_pipeline.hpp (tests/host/pipeline_main.cpp): streams and events as counted heap objects
// (a forgotten destroy is a leak, a second one an address error) and a log of what was recorded and waited for on them.
#pragma once
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <vector>

#define __host__
#define __device__
#define __forceinline__ inline
inline float __fadd_rn(float a, float b) { return a + b; }
inline double __dadd_rn(double a, double b) { return a + b; }
template <class T>
inline T __shfl_xor(T, int) {
    abort();   // one thread has no neighbouring lanes
}

typedef int hipError_t;
enum : int { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2 };
typedef struct hipStubStream* hipStream_t;
typedef struct hipStubEvent* hipEvent_t;
struct hipStubStream {
    unsigned flags;
};
struct hipStubEvent {
    unsigned flags;
};
enum : unsigned { hipStreamNonBlocking = 1, hipEventDisableTiming = 2 };
enum hipMemcpyKind { hipMemcpyHostToHost, hipMemcpyHostToDevice, hipMemcpyDeviceToHost, hipMemcpyDeviceToDevice };
enum : unsigned { hipHostMallocDefault = 0 };

namespace hip_stub {
inline long fail_in = 0;      // N > 0: the N-th allocation from now fails (device and pinned ones count alike)
inline long allocs = 0, frees = 0, device_ptr_calls = 0;
inline void* const kPoison = reinterpret_cast<void*>(0x5a5a5a5a5a5a5a50ull);   // what a failed allocation leaves in *p

inline hipError_t alloc(void** p, size_t bytes) {
    if (fail_in > 0 && --fail_in == 0) {
        *p = kPoison;
        return hipErrorOutOfMemory;
    }
    *p = malloc(bytes ? bytes : 1);
    if (!*p) return hipErrorOutOfMemory;
    memset(*p, 0xcd, bytes);
    ++allocs;
    return hipSuccess;
}
inline hipError_t release(void* p) {
    if (p) ++frees;
    free(p);
    return hipSuccess;
}

inline long streams_created = 0, streams_destroyed = 0, events_created = 0, events_destroyed = 0;
// append-only: an event recorded on a stream (null: the default stream), a stream made to wait for an event; the
// programs add waits and marks of their own
enum Op { kRecord, kStreamWaitEvent, kStreamWait, kEventWait, kMark };
struct Logged {
    Op op;
    hipStream_t stream;
    hipEvent_t event;
    bool operator==(const Logged& o) const { return op == o.op && stream == o.stream && event == o.event; }
};
inline std::vector<Logged> log;
}  // namespace hip_stub

inline hipError_t hipStreamCreateWithFlags(hipStream_t* st, unsigned flags) {
    *st = new hipStubStream{flags};
    ++hip_stub::streams_created;
    return hipSuccess;
}
inline hipError_t hipStreamDestroy(hipStream_t st) {
    ++hip_stub::streams_destroyed;
    delete st;
    return hipSuccess;
}
inline hipError_t hipEventCreateWithFlags(hipEvent_t* ev, unsigned flags) {
    *ev = new hipStubEvent{flags};
    ++hip_stub::events_created;
    return hipSuccess;
}
inline hipError_t hipEventDestroy(hipEvent_t ev) {
    ++hip_stub::events_destroyed;
    delete ev;
    return hipSuccess;
}
inline hipError_t hipEventRecord(hipEvent_t ev, hipStream_t st) {
    if (!ev) return hipErrorInvalidValue;
    hip_stub::log.push_back({hip_stub::kRecord, st, ev});
    return hipSuccess;
}
inline hipError_t hipStreamWaitEvent(hipStream_t st, hipEvent_t ev, unsigned) {
    if (!ev) return hipErrorInvalidValue;
    hip_stub::log.push_back({hip_stub::kStreamWaitEvent, st, ev});
    return hipSuccess;
}

inline hipError_t hipMalloc(void** p, size_t bytes) { return hip_stub::alloc(p, bytes); }
inline hipError_t hipFree(void* p) { return hip_stub::release(p); }
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return hip_stub::alloc(p, bytes); }
inline hipError_t hipHostFree(void* p) { return hip_stub::release(p); }
inline hipError_t hipHostGetDevicePointer(void** dev, void* host, unsigned) {
    ++hip_stub::device_ptr_calls;
    *dev = host;
    return host ? hipSuccess : hipErrorInvalidValue;
}
inline hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
    memcpy(dst, src, bytes);
    return hipSuccess;
}
inline hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t) {
    return hipMemcpy(dst, src, bytes, kind);
}
inline const char* hipGetErrorString(hipError_t e) {
    return e == hipSuccess ? "no error" : e == hipErrorOutOfMemory ? "out of memory" : "invalid value";
}
