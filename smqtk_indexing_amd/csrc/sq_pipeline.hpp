// The asynchronous call pipeline and the host-memory call, shared by every index kind: plain host logic over the
// runtime's stream and event calls (tests/host/pipeline_main.cpp runs it against the stand-in <hip/hip_runtime.h>).
// stream_wait and event_wait are the including translation unit's (sq_common.hpp: poll, then block).
#pragma once
#include <hip/hip_runtime.h>

#include "sq_buffers.hpp"

namespace sq {

// What orders one call slot's work: `ev_in` puts a call behind the caller's stream, `ev_done` is what resolving the call
// waits for, `own` is the slot's internal stream.  Each is created at first use and destroyed once.
struct SlotSync {
    hipEvent_t ev_in = nullptr, ev_done = nullptr;
    hipStream_t own = nullptr;
    SlotSync() = default;
    SlotSync(SlotSync&& o) noexcept
        : ev_in(std::exchange(o.ev_in, nullptr)), ev_done(std::exchange(o.ev_done, nullptr)), own(std::exchange(o.own, nullptr)) {}
    SlotSync& operator=(SlotSync&& o) noexcept {
        if (this != &o) {
            release();
            ev_in = std::exchange(o.ev_in, nullptr);
            ev_done = std::exchange(o.ev_done, nullptr);
            own = std::exchange(o.own, nullptr);
        }
        return *this;
    }
    SlotSync(const SlotSync&) = delete;
    SlotSync& operator=(const SlotSync&) = delete;
    ~SlotSync() { release(); }
    int stream(hipStream_t* out) {
        if (!own) SQ_HIP(hipStreamCreateWithFlags(&own, hipStreamNonBlocking));
        *out = own;
        return SQ_OK;
    }
    // the caller's earlier work on `caller` (the queries) comes before what `run` (this slot's stream or another's) is given next
    int order_behind(hipStream_t caller, hipStream_t run) {
        if (!ev_in) SQ_HIP(hipEventCreateWithFlags(&ev_in, hipEventDisableTiming));
        SQ_HIP(hipEventRecord(ev_in, caller));
        SQ_HIP(hipStreamWaitEvent(run, ev_in, 0));
        return SQ_OK;
    }
    int mark_done(hipStream_t run) {
        if (!ev_done) SQ_HIP(hipEventCreateWithFlags(&ev_done, hipEventDisableTiming));
        SQ_HIP(hipEventRecord(ev_done, run));
        return SQ_OK;
    }
    // the call has drained: the one marked done (use_event), or everything on `st`
    int wait(bool use_event, hipStream_t st) const {
        SQ_HIP(use_event ? event_wait(ev_done) : stream_wait(st));
        return SQ_OK;
    }
    void release() {
        if (ev_in) (void)hipEventDestroy(std::exchange(ev_in, nullptr));
        if (ev_done) (void)hipEventDestroy(std::exchange(ev_done, nullptr));
        if (own) (void)hipStreamDestroy(std::exchange(own, nullptr));
    }
};
static_assert(is_move_only_owner<SlotSync>, "SlotSync: not copyable, nothrow-movable");

// Asynchronous calls rotate through `depth` of the slots (slot = calls % depth): call i is enqueued before call i - 1 is
// waited for, and a call is final once the (depth - 1)-th call after it has resolved it.  A blocking call drains the ring
// and uses slot 0.  `resolve(slot)` finishes the call enqueued on a slot (a slot without one: nothing) and returns an
// SQ_* code; the first failure ends a drain.
template <class Slot, int kMaxDepth>
struct CallRing {
    static_assert(kMaxDepth >= 2, "a pipeline is two calls deep at least");
    Slot slot[kMaxDepth];
    int depth = 2;                 // asynchronous calls in flight (fixed while any is)
    unsigned long long calls = 0;  // asynchronous calls so far
    // the slot the next call takes: it holds the call `depth` back, the oldest in flight
    Slot& next() { return slot[calls % (unsigned)depth]; }
    // the call on next() has been enqueued: the slot of the oldest call now in flight (resolved before returning: final depth - 1 calls later)
    Slot& advance() {
        ++calls;
        return next();
    }
    template <class Resolve>
    int drain(Resolve&& resolve) {   // finish every call in flight, oldest first
        for (int j = 0; j < depth; ++j) SQ_TRY(resolve(slot[(calls + (unsigned)j) % (unsigned)depth]));
        return SQ_OK;
    }
    template <class Resolve>
    int set_depth(int want, Resolve&& resolve) {   // 2 .. kMaxDepth; a new depth starts from an empty pipeline
        want = want < 2 ? 2 : want > kMaxDepth ? kMaxDepth : want;
        if (want == depth) return SQ_OK;
        SQ_TRY(drain(resolve));
        depth = want;
        calls = 0;
        return SQ_OK;
    }
};

// A call whose inputs and outputs are in host memory: the device buffers reserved, the inputs copied in, `run()` (which
// enqueues the work on `st` and returns an SQ_* code), the outputs copied out, the stream waited for.  Up to
// PinnedStage::kStageMax bytes in total travel through `stage`.  Nothing is copied out when run() fails.
struct StagedIn { DevBuf& dev; const void* host; size_t bytes; };
struct StagedOut { void* host; DevBuf& dev; size_t bytes; };
template <size_t NI, size_t NO, class Run>
inline int staged_call(PinnedStage& stage, hipStream_t st, const StagedIn (&ins)[NI], const StagedOut (&outs)[NO], Run&& run) {
    static_assert(NO <= sizeof(PinnedStage::outs) / sizeof(PinnedStage::Out), "PinnedStage::outs holds no more outputs than that");
    size_t total = 0;
    for (const StagedIn& i : ins) total += i.bytes;
    for (const StagedOut& o : outs) total += o.bytes;
    for (const StagedIn& i : ins) SQ_TRY(i.dev.reserve(i.bytes));
    for (const StagedOut& o : outs) SQ_TRY(o.dev.reserve(o.bytes));
    SQ_TRY(stage.begin(total));
    for (const StagedIn& i : ins) SQ_HIP(stage.in(i.dev.p, i.host, i.bytes, st));
    SQ_TRY(run());
    for (const StagedOut& o : outs) SQ_HIP(stage.out(o.host, o.dev.p, o.bytes, st));
    SQ_HIP(stream_wait(st));
    stage.finish();
    return SQ_OK;
}

}  // namespace sq
