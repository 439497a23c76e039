// The call pipeline of smqtk_indexing_amd/csrc/sq_pipeline.hpp on a CPU: SlotSync, CallRing and staged_call, compiled
// against the stand-in runtime in hip_stub/ with -fsanitize=address,undefined and run by
// tests/test_host_logic_pipeline.py.  Streams and events are heap objects there: a dropped destroy shows as a leak, a
// second one as an address error; the stand-in's log says in which order they were recorded and waited for.
#include "../../smqtk_indexing_amd/csrc/sq_buffers.hpp"

#include <cstdio>
#include <cstdlib>
#include <functional>
#include <utility>
#include <vector>

thread_local char sq::g_err[512];

// what sq_common.hpp declares for the library: here the waits are logged, and a test may look around while one "blocks"
namespace sq {
static std::function<void()> g_during_wait;
inline hipError_t stream_wait(hipStream_t st) {
    hip_stub::log.push_back({hip_stub::kStreamWait, st, nullptr});
    if (g_during_wait) g_during_wait();
    return hipSuccess;
}
inline hipError_t event_wait(hipEvent_t ev) {
    hip_stub::log.push_back({hip_stub::kEventWait, nullptr, ev});
    return hipSuccess;
}
}  // namespace sq

#include "../../smqtk_indexing_amd/csrc/sq_pipeline.hpp"

using namespace sq;
using hip_stub::Logged;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

static long live() { return hip_stub::allocs - hip_stub::frees; }
static long live_events() { return hip_stub::events_created - hip_stub::events_destroyed; }
static long live_streams() { return hip_stub::streams_created - hip_stub::streams_destroyed; }

// ------------------------------------------------------------------ the ring
struct TestSlot {
    int pending = -1;   // number of the call in flight on the slot
};

// The drivers' sequence around a ring (sq_dense_search, sq_hamming_search): set the depth, resolve the slot about to be
// reused, enqueue, advance, resolve the oldest call in flight unless the caller does not wait.
template <int kMaxDepth>
struct Driver {
    CallRing<TestSlot, kMaxDepth> ring;
    int made = 0;                          // calls enqueued so far: the next call's number
    std::vector<int> resolved;             // call numbers, in the order they were resolved
    int fail_resolve_of = -1, fail_enqueue_of = -1;
    int used_slot = -1, oldest_slot = -1;  // of the last call

    int resolve(TestSlot& s) {
        if (s.pending < 0) return SQ_OK;
        const int call = std::exchange(s.pending, -1);   // (as the drivers: a call is given up once its resolve fails)
        if (call == fail_resolve_of) return fail(SQ_ERR_HIP, "resolve of call %d", call);
        resolved.push_back(call);
        return SQ_OK;
    }
    int oldest_pending() const {
        int o = -1;
        for (int j = 0; j < kMaxDepth; ++j)
            if (ring.slot[j].pending >= 0 && (o < 0 || ring.slot[j].pending < o)) o = ring.slot[j].pending;
        return o;
    }
    int drain() {
        return ring.drain([this](TestSlot& s) { return resolve(s); });
    }
    int call(int want_depth, bool wait) {
        const auto r = [this](TestSlot& s) { return resolve(s); };
        SQ_TRY(ring.set_depth(want_depth, r));
        TestSlot& s = ring.next();
        SQ_TRY(r(s));
        if (made == fail_enqueue_of) return fail(SQ_ERR_HIP, "enqueue of call %d", made);
        CHECK(s.pending < 0);
        s.pending = made++;
        used_slot = (int)(&s - ring.slot);
        TestSlot& oldest = ring.advance();
        oldest_slot = (int)(&oldest - ring.slot);
        // "final after this call" is the oldest call in flight (or, with fewer than depth calls made, an empty slot)
        CHECK(oldest.pending < 0 ? ring.calls < (unsigned)ring.depth : oldest.pending == oldest_pending());
        return wait ? r(oldest) : SQ_OK;
    }
};

template <int kMaxDepth>
static void ring_rotation(int depth, bool wait) {
    Driver<kMaxDepth> d;
    const int n = 3 * depth + 1;
    for (int i = 0; i < n; ++i) {
        const size_t before = d.resolved.size();
        CHECK(d.call(depth, wait) == SQ_OK);
        CHECK(d.ring.depth == depth && d.ring.calls == (unsigned long long)(i + 1));
        CHECK(d.used_slot == i % depth && d.oldest_slot == (i + 1) % depth);
        if (wait) {
            // final depth - 1 calls later: everything up to call i - (depth - 1) is resolved, nothing younger
            CHECK((int)d.resolved.size() == std::max(0, i - depth + 2));
        } else {
            // one more call of lag: the slot resolved before reuse held the call `depth` back
            CHECK(d.resolved.size() == before + (i >= depth ? 1 : 0));
            if (i >= depth) CHECK(d.resolved.back() == i - depth);
        }
        for (size_t j = 0; j < d.resolved.size(); ++j) CHECK(d.resolved[j] == (int)j);   // oldest first, none skipped
    }
    // drain after wrap-around: the calls still in flight, oldest first
    CHECK(d.drain() == SQ_OK && (int)d.resolved.size() == n);
    for (int j = 0; j < n; ++j) CHECK(d.resolved[(size_t)j] == j);
    CHECK(d.drain() == SQ_OK && (int)d.resolved.size() == n);   // nothing in flight: nothing happens
}

template <int kMaxDepth>
static void ring_drain_and_depth() {
    for (int depth = 2; depth <= kMaxDepth; ++depth) {
        // fewer calls than slots
        Driver<kMaxDepth> d;
        for (int i = 0; i < depth - 1; ++i) CHECK(d.call(depth, false) == SQ_OK);
        CHECK(d.resolved.empty() && d.drain() == SQ_OK && (int)d.resolved.size() == depth - 1);
        for (int j = 0; j < depth - 1; ++j) CHECK(d.resolved[(size_t)j] == j);
    }
    Driver<kMaxDepth> d;
    CHECK(d.ring.depth == 2);
    for (int i = 0; i < 5; ++i) CHECK(d.call(3, false) == SQ_OK);   // calls 0 and 1 resolved by reuse, 2 3 4 in flight
    CHECK(d.ring.depth == 3 && d.ring.calls == 5 && d.resolved.size() == 2);
    const auto r = [&d](TestSlot& s) { return d.resolve(s); };
    CHECK(d.ring.set_depth(3, r) == SQ_OK && d.resolved.size() == 2 && d.ring.calls == 5);   // the same depth: nothing
    CHECK(d.call(2, false) == SQ_OK);   // a new depth: everything pending resolved oldest first, then slot 0
    CHECK(d.ring.depth == 2 && d.ring.calls == 1 && d.used_slot == 0 && d.resolved.size() == 5);
    for (int j = 0; j < 5; ++j) CHECK(d.resolved[(size_t)j] == j);
    CHECK(d.call(2, false) == SQ_OK && d.used_slot == 1);
    // clamping
    const int wants[4] = {0, 1, kMaxDepth + 1, -7}, gives[4] = {2, 2, kMaxDepth, 2};
    for (int j = 0; j < 4; ++j) {
        CHECK(d.ring.set_depth(kMaxDepth == 2 ? 2 : 3, r) == SQ_OK);
        CHECK(d.ring.set_depth(wants[j], r) == SQ_OK && d.ring.depth == gives[j] && d.ring.calls == 0);
    }
    CHECK(d.ring.set_depth(kMaxDepth, r) == SQ_OK && d.ring.depth == kMaxDepth);
}

template <int kMaxDepth>
static void ring_failures() {
    Driver<kMaxDepth> d;
    for (int i = 0; i < 4; ++i) CHECK(d.call(2, false) == SQ_OK);   // 0 1 resolved; 2 3 in flight
    // the resolve of the slot about to be reused fails: nothing is enqueued, the ring does not move
    d.fail_resolve_of = 2;
    CHECK(d.call(2, false) == SQ_ERR_HIP && d.made == 4 && d.ring.calls == 4 && d.resolved.size() == 2);
    CHECK(d.call(2, false) == SQ_OK && d.made == 5 && d.used_slot == 0 && d.ring.calls == 5);   // the next call takes that slot
    // a failing enqueue: the slot was resolved, the ring does not move, the next call takes the same slot
    d.fail_enqueue_of = 5;
    CHECK(d.call(2, false) == SQ_ERR_HIP && d.made == 5 && d.ring.calls == 5 && d.resolved.back() == 3);
    d.fail_enqueue_of = -1;
    CHECK(d.call(2, false) == SQ_OK && d.used_slot == 1 && d.ring.calls == 6);
    // a failing resolve ends a drain, and a change of depth with it: depth and calls stay
    d.fail_resolve_of = 4;
    CHECK(d.call(3, false) == SQ_ERR_HIP && d.ring.depth == 2 && d.ring.calls == 6 && d.made == 6);
    CHECK(d.call(3, false) == SQ_OK && d.ring.depth == 3 && d.used_slot == 0 && d.resolved.back() == 5);
}

// ------------------------------------------------------------------ the per-slot state
static void slot_sync() {
    hip_stub::log.clear();
    const long ev0 = live_events(), st0 = live_streams(), ev_made = hip_stub::events_created, st_made = hip_stub::streams_created;
    hipStubStream caller_obj{0};
    hipStream_t caller = &caller_obj;
    {
        SlotSync a, b;
        CHECK(!a.ev_in && !a.ev_done && !a.own);
        hipStream_t run = nullptr;
        for (int call = 0; call < 5; ++call) {
            const size_t at = hip_stub::log.size();
            CHECK(a.stream(&run) == SQ_OK && run && run == a.own);
            CHECK(a.order_behind(caller, run) == SQ_OK);
            hip_stub::log.push_back({hip_stub::kMark, run, nullptr});   // the enqueue
            CHECK(a.mark_done(run) == SQ_OK);
            CHECK(hip_stub::log.size() == at + 4);
            CHECK((hip_stub::log[at] == Logged{hip_stub::kRecord, caller, a.ev_in}));
            CHECK((hip_stub::log[at + 1] == Logged{hip_stub::kStreamWaitEvent, run, a.ev_in}));
            CHECK(hip_stub::log[at + 2].op == hip_stub::kMark);
            CHECK((hip_stub::log[at + 3] == Logged{hip_stub::kRecord, run, a.ev_done}));
            CHECK(live_events() == ev0 + 2 && live_streams() == st0 + 1);   // created once, however many calls
        }
        CHECK(a.ev_in != a.ev_done && a.own->flags == hipStreamNonBlocking && a.ev_in->flags == hipEventDisableTiming);
        // resolve waits for the event of the call, or for the whole stream of a blocking one
        size_t at = hip_stub::log.size();
        CHECK(a.wait(true, run) == SQ_OK && (hip_stub::log[at] == Logged{hip_stub::kEventWait, nullptr, a.ev_done}));
        CHECK(a.wait(false, caller) == SQ_OK && (hip_stub::log[at + 1] == Logged{hip_stub::kStreamWait, caller, nullptr}));
        // another slot's stream as the run stream: b's event, a's stream, no stream of b's own
        at = hip_stub::log.size();
        CHECK(b.order_behind(caller, a.own) == SQ_OK && b.mark_done(a.own) == SQ_OK);
        CHECK((hip_stub::log[at] == Logged{hip_stub::kRecord, caller, b.ev_in}));
        CHECK((hip_stub::log[at + 1] == Logged{hip_stub::kStreamWaitEvent, a.own, b.ev_in}));
        CHECK((hip_stub::log[at + 2] == Logged{hip_stub::kRecord, a.own, b.ev_done}));
        CHECK(b.own == nullptr && b.ev_in != a.ev_in && live_events() == ev0 + 4 && live_streams() == st0 + 1);
        // the default stream as the caller's
        CHECK(b.order_behind(nullptr, a.own) == SQ_OK && hip_stub::log[hip_stub::log.size() - 2].stream == nullptr);
        // moves: the source is empty, each object is destroyed once
        hipEvent_t in = a.ev_in, done = a.ev_done;
        SlotSync c(std::move(a));
        CHECK(!a.ev_in && !a.ev_done && !a.own && c.ev_in == in && c.ev_done == done && c.own == run);
        CHECK(live_events() == ev0 + 4 && live_streams() == st0 + 1);
        b = std::move(c);   // b's two events go, c's three objects arrive
        CHECK(!c.own && b.own == run && b.ev_in == in && live_events() == ev0 + 2 && live_streams() == st0 + 1);
        SlotSync& self = b;
        b = std::move(self);
        CHECK(b.own == run && live_events() == ev0 + 2);
        CHECK(a.stream(&run) == SQ_OK && run != b.own && live_streams() == st0 + 2);   // a moved-from slot is an empty one
        a.release();
        a.release();
        CHECK(live_streams() == st0 + 1);
    }
    CHECK(live_events() == ev0 && live_streams() == st0);
    CHECK(hip_stub::events_created == ev_made + 4 && hip_stub::streams_created == st_made + 2);   // the counters agree with the leak check
}

// ------------------------------------------------------------------ the staged host call
static void fill(void* p, size_t bytes, unsigned seed) {
    unsigned char* c = static_cast<unsigned char*>(p);
    for (size_t i = 0; i < bytes; ++i) c[i] = (unsigned char)((i * 131u + seed) >> 3);
}
static bool filled(const void* p, size_t bytes, unsigned seed) {
    const unsigned char* c = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < bytes; ++i)
        if (c[i] != (unsigned char)((i * 131u + seed) >> 3)) return false;
    return true;
}
static bool all_are(const std::vector<unsigned char>& v, unsigned char x) {
    for (unsigned char c : v)
        if (c != x) return false;
    return true;
}

// What a handle keeps for its host-memory calls, and one call through it: two inputs, the "kernel" (input bytes become
// output bytes), two outputs; `total` bytes in all.
struct Staged {
    PinnedStage stage;
    DevBuf in_a, in_b, out_a, out_b;
    std::vector<unsigned char> back_a, back_b;   // the caller's output buffers
    bool staged_at_wait = false, direct_at_wait = false;

    int call(size_t total, unsigned seed, bool run_fails = false) {
        const size_t a = 1001, b = (total - 2 * a + 1) / 2, b_out = (total - 2 * a) / 2;
        std::vector<unsigned char> src_a(a), src_b(b);
        fill(src_a.data(), a, seed);
        fill(src_b.data(), b, seed + 1);
        back_a.assign(a, 0xee);
        back_b.assign(b_out, 0xee);
        hipStubStream st_obj{0};
        hipStream_t st = &st_obj;
        g_during_wait = [&] {   // the stream drains: outputs that travel through the stage have not reached the caller yet
            staged_at_wait = all_are(back_a, 0xee) && all_are(back_b, 0xee);
            direct_at_wait = filled(back_a.data(), a, seed) && filled(back_b.data(), b_out, seed + 1);
        };
        const size_t waits = hip_stub::log.size();
        const int rc = staged_call(stage, st, {{in_a, src_a.data(), a}, {in_b, src_b.data(), b}},
                                   {{back_a.data(), out_a, a}, {back_b.data(), out_b, b_out}}, [&] {
                                       CHECK(filled(in_a.p, a, seed) && filled(in_b.p, b, seed + 1));   // the inputs are in
                                       CHECK(out_a.cap >= a && out_b.cap >= b_out);
                                       if (run_fails) return fail(SQ_ERR_HIP, "the work failed");
                                       memcpy(out_a.p, in_a.p, a);
                                       memcpy(out_b.p, in_b.p, b_out);
                                       return (int)SQ_OK;
                                   });
        g_during_wait = nullptr;
        if (rc == SQ_OK) {
            CHECK(hip_stub::log.size() == waits + 1 && (hip_stub::log[waits] == Logged{hip_stub::kStreamWait, st, nullptr}));
            CHECK(filled(back_a.data(), a, seed) && filled(back_b.data(), b_out, seed + 1) && stage.n_out == 0);
        } else {
            CHECK(hip_stub::log.size() == waits);   // no wait: nothing was copied out
        }
        return rc;
    }
};

static void staged_calls() {
    const long base = live();
    {
        Staged s;
        CHECK(s.call(PinnedStage::kStageMax - 1, 10) == SQ_OK && s.stage.on && s.staged_at_wait && !s.direct_at_wait);
        CHECK(s.call(PinnedStage::kStageMax, 20) == SQ_OK && s.stage.on && s.staged_at_wait && !s.direct_at_wait);
        CHECK(s.call(PinnedStage::kStageMax + 1, 30) == SQ_OK && !s.stage.on && !s.staged_at_wait && s.direct_at_wait);
        CHECK(s.call(4097, 40) == SQ_OK && s.stage.on && s.staged_at_wait);
        // the work fails: the caller's buffers are untouched, and nothing is left for the next call's finish() to copy
        for (size_t total : {(size_t)5000, PinnedStage::kStageMax + 1}) {
            CHECK(s.call(total, 50, /*run_fails*/ true) == SQ_ERR_HIP && g_err[0] != 0);
            CHECK(all_are(s.back_a, 0xee) && all_are(s.back_b, 0xee) && s.stage.n_out == 0);
            std::vector<unsigned char> failed_a, failed_b;
            failed_a.swap(s.back_a), failed_b.swap(s.back_b);
            CHECK(s.call(6000, 60) == SQ_OK);
            CHECK(all_are(failed_a, 0xee) && all_are(failed_b, 0xee));
        }
        CHECK(live() == base + 5);   // four device buffers and the stage's block
    }
    CHECK(live() == base);
    // every allocation of a first call fails in turn: four device buffers, then the pinned block
    const int n_allocs = 5;
    for (int n = 1; n <= n_allocs + 1; ++n) {
        {
            Staged s;
            hip_stub::fail_in = n;
            const int rc = s.call(20000, 70 + n);
            if (n <= n_allocs) {
                CHECK(rc == SQ_ERR_NOMEM && hip_stub::fail_in == 0 && live() == base + n - 1);
                CHECK(all_are(s.back_a, 0xee) && all_are(s.back_b, 0xee));
                CHECK(s.call(20000, 80 + n) == SQ_OK && live() == base + n_allocs);   // the following call succeeds
            } else {
                CHECK(rc == SQ_OK && hip_stub::fail_in == 1);   // ... and there is no sixth
                hip_stub::fail_in = 0;
            }
        }
        CHECK(live() == base);
    }
    // direct copies need no pinned block
    {
        Staged s;
        hip_stub::fail_in = 5;
        CHECK(s.call(PinnedStage::kStageMax + 4096, 90) == SQ_OK && hip_stub::fail_in == 1 && live() == base + 4);
        hip_stub::fail_in = 0;
    }
    CHECK(live() == base);
}

int main() {
    for (int wait = 0; wait < 2; ++wait) {
        for (int depth : {2, 3, 6}) ring_rotation<6>(depth, wait != 0);   // the dense index: kMaxDepth = 6
        for (int depth : {2, 3, 4}) ring_rotation<4>(depth, wait != 0);   // the Hamming index: kMaxDepth = 4
    }
    ring_drain_and_depth<6>();
    ring_drain_and_depth<4>();
    ring_failures<6>();
    ring_failures<4>();
    slot_sync();
    staged_calls();
    CHECK(live() == 0 && live_events() == 0 && live_streams() == 0 && hip_stub::allocs > 0);
    printf("pipeline ok: %ld events, %ld streams, %ld allocations, %zu operations logged\n", hip_stub::events_created,
           hip_stub::streams_created, hip_stub::allocs, hip_stub::log.size());
    return 0;
}
