// The owning buffer types of smqtk_indexing_amd/csrc/sq_buffers.hpp on a CPU: compiled against the stand-in runtime in
// hip_stub/ with -fsanitize=address,undefined and run by tests/test_host_logic_buffers.py.  A dropped free shows as a
// leak, a second free or a use after a move as an address error; the counters of the stand-in check the rest.
#include "../../smqtk_indexing_amd/csrc/sq_buffers.hpp"

#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

thread_local char sq::g_err[512];

using namespace sq;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

static long live() { return hip_stub::allocs - hip_stub::frees; }

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

// reserve, grow, scope exit; moves; release twice; a failed allocation -- the same for both allocating types
template <class Buf>
static void lifetime() {
    const long base = live();
    {
        Buf b;
        CHECK(b.p == nullptr && b.cap == 0);
        CHECK(b.reserve(1000) == SQ_OK);
        CHECK(b.p && b.cap >= 1000 && live() == base + 1);
        void* first = b.p;
        const size_t cap = b.cap;
        fill(b.p, b.cap, 1);                       // the whole block is ours to write
        CHECK(b.reserve(cap) == SQ_OK && b.p == first && b.cap == cap);   // fits: nothing happens
        CHECK(b.reserve(cap + 1) == SQ_OK);        // grows: the old block is freed, one block is live
        CHECK(b.cap >= cap + 1 && live() == base + 1);
        fill(b.p, b.cap, 2);
    }
    CHECK(live() == base);   // scope exit freed it
    {
        Buf a;
        CHECK(a.reserve(300) == SQ_OK);
        fill(a.p, 300, 3);
        void* p = a.p;
        const size_t cap = a.cap;
        Buf b(std::move(a));   // move construction empties the source
        CHECK(a.p == nullptr && a.cap == 0 && b.p == p && b.cap == cap && filled(b.p, 300, 3));
        Buf c;
        CHECK(c.reserve(700) == SQ_OK && live() == base + 2);
        c = std::move(b);      // move assignment onto a buffer that holds memory: its block is freed once
        CHECK(live() == base + 1 && b.p == nullptr && b.cap == 0 && c.p == p && c.cap == cap && filled(c.p, 300, 3));
        Buf& self = c;
        c = std::move(self);   // onto itself: nothing happens
        CHECK(c.p == p && c.cap == cap && live() == base + 1);
        CHECK(a.reserve(10) == SQ_OK && live() == base + 2);   // a moved-from buffer is an empty one
        c.release();
        CHECK(c.p == nullptr && c.cap == 0 && live() == base + 1);
        c.release();           // twice is harmless
        CHECK(c.p == nullptr && c.cap == 0 && live() == base + 1);
        CHECK(c.reserve(20) == SQ_OK && live() == base + 2);   // ... and it can be used again
    }
    CHECK(live() == base);
    {
        Buf b;
        hip_stub::fail_in = 1;
        CHECK(b.reserve(100) == SQ_ERR_NOMEM);     // a failed first allocation leaves it empty
        CHECK(b.p == nullptr && b.cap == 0 && live() == base && g_err[0] != 0);
        CHECK(b.reserve(100) == SQ_OK && live() == base + 1);
        hip_stub::fail_in = 1;
        CHECK(b.reserve(100000) == SQ_ERR_NOMEM);  // a failed growth too (the old block went first: free, then allocate)
        CHECK(b.p == nullptr && b.cap == 0 && live() == base);
        CHECK(b.reserve(50) == SQ_OK && live() == base + 1);
        fill(b.p, b.cap, 4);
    }
    CHECK(live() == base);
}

static void sizes() {
    DevBuf d;
    CHECK(d.reserve(4096) == SQ_OK && d.cap == 4096 + 512 + 256);   // 1/8 + 256 over the request (sq_dense_info reports cap)
    CHECK(d.as<float>() == static_cast<float*>(d.p));
    HostPinned h;
    CHECK(h.reserve(4096) == SQ_OK && h.cap == 4096 + 256);
}

// DevBuf::alloc_exact: the bytes asked for and no more, a new block every time
static void exact() {
    const long base = live();
    {
        DevBuf b;
        CHECK(b.alloc_exact(4096) == SQ_OK && b.p && b.cap == 4096 && live() == base + 1);   // no eighth on top
        fill(b.p, 4096, 8);
        const long made = hip_stub::allocs;
        CHECK(b.alloc_exact(100) == SQ_OK && b.cap == 100 && hip_stub::allocs == made + 1 && live() == base + 1);   // replaced, although it fitted
        fill(b.p, 100, 9);
        CHECK(b.alloc_exact(0) == SQ_OK && b.p && b.cap == 16 && live() == base + 1);       // nothing is 16 bytes
        fill(b.p, 16, 10);
        CHECK(b.reserve(16) == SQ_OK && b.cap == 16 && b.reserve(17) == SQ_OK && b.cap == 17 + 2 + 256);   // reserve() goes on from it
        hip_stub::fail_in = 1;
        CHECK(b.alloc_exact(5000) == SQ_ERR_NOMEM);   // DevBuf's failure contract: empty, the old block freed
        CHECK(b.p == nullptr && b.cap == 0 && live() == base && g_err[0] != 0);
        DevBuf c;
        hip_stub::fail_in = 1;
        CHECK(c.alloc_exact(0) == SQ_ERR_NOMEM && c.p == nullptr && c.cap == 0 && live() == base);   // a failed first allocation
        hip_stub::fail_in = 2;
        CHECK(b.alloc_exact(64) == SQ_OK && c.alloc_exact(64) == SQ_ERR_NOMEM && live() == base + 1);
        CHECK(c.alloc_exact(64) == SQ_OK && c.cap == 64 && live() == base + 2);           // ... and it can be used again
        DevBuf d(std::move(c));
        CHECK(c.p == nullptr && d.cap == 64 && live() == base + 2);
    }
    CHECK(live() == base);
}

static void device_pointer() {
    HostPinned h;
    CHECK(h.reserve(64) == SQ_OK);
    const long calls = hip_stub::device_ptr_calls;
    void* d = nullptr;
    CHECK(h.device_ptr(&d) == SQ_OK && d == h.p && h.device_ptr(&d) == SQ_OK && d == h.p);
    CHECK(hip_stub::device_ptr_calls == calls + 1);   // looked up once per allocation
    HostPinned g(std::move(h));
    CHECK(h.dev == nullptr && g.dev == d);
    CHECK(g.reserve(100000) == SQ_OK && g.dev == nullptr);   // a new block: looked up again
    CHECK(g.device_ptr(&d) == SQ_OK && d == g.p && hip_stub::device_ptr_calls == calls + 2);
    g.release();
    CHECK(g.dev == nullptr);
}

static void growing() {
    const long base = live();
    {
        DevBuf b;
        CHECK(grow_keep(b, 0, 1000) == SQ_OK && b.cap >= 1000 && live() == base + 1);   // from nothing
        fill(b.p, 1000, 5);
        void* p = b.p;
        CHECK(grow_keep(b, 1000, b.cap) == SQ_OK && b.p == p);                        // fits: nothing happens
        const size_t cap = b.cap;
        CHECK(grow_keep(b, 1000, cap + 1) == SQ_OK && live() == base + 1);           // grows by half again at least ...
        CHECK(b.cap >= 1500 && b.cap >= cap + 1 && filled(b.p, 1000, 5));             // ... and keeps the first `used` bytes
        CHECK(grow_keep(b, 1000, 100000) == SQ_OK && b.cap >= 100000 && filled(b.p, 1000, 5) && live() == base + 1);
        p = b.p;
        const size_t cap2 = b.cap;
        hip_stub::fail_in = 1;
        CHECK(grow_keep(b, 1000, cap2 + 1) == SQ_ERR_NOMEM);                           // no memory: the buffer is as it was
        CHECK(b.p == p && b.cap == cap2 && filled(b.p, 1000, 5) && live() == base + 1);
    }
    CHECK(live() == base);
}

// bytes through the stage and back: `total` is what the call announces, split into two pieces in and two pieces out
static void stage_round_trip(PinnedStage& s, size_t total) {
    const size_t a = 1001, rest = total - 2 * a, b_in = (rest + 1) / 2, b_out = rest / 2;
    std::vector<unsigned char> src_a(a), src_b(b_in), back_a(a), back_b(b_out);
    fill(src_a.data(), a, 6);
    fill(src_b.data(), b_in, 7);
    DevBuf dev_a, dev_b;
    CHECK(dev_a.reserve(a) == SQ_OK && dev_b.reserve(b_in) == SQ_OK);
    CHECK(s.begin(total) == SQ_OK);
    CHECK(s.on == (total <= PinnedStage::kStageMax));
    CHECK(s.in(dev_a.p, src_a.data(), a, nullptr) == hipSuccess);
    CHECK(s.in(dev_b.p, src_b.data(), b_in, nullptr) == hipSuccess);
    CHECK(filled(dev_a.p, a, 6) && filled(dev_b.p, b_in, 7));
    CHECK(s.out(back_a.data(), dev_a.p, a, nullptr) == hipSuccess);
    CHECK(s.out(back_b.data(), dev_b.p, b_out, nullptr) == hipSuccess);
    CHECK(s.n_out == (s.on ? 2 : 0));
    s.finish();
    CHECK(s.n_out == 0 && filled(back_a.data(), a, 6) && filled(back_b.data(), b_out, 7));
}

static void staging() {
    const long base = live();
    {
        PinnedStage s;
        stage_round_trip(s, 4096);
        stage_round_trip(s, PinnedStage::kStageMax - 1);   // just under: staged (the block grows)
        stage_round_trip(s, PinnedStage::kStageMax);
        CHECK(live() == base + 1);
        stage_round_trip(s, PinnedStage::kStageMax + 1);   // just over: direct copies, the block is left alone
        CHECK(live() == base + 1);
        void* p = s.pin.p;
        PinnedStage t(std::move(s));
        CHECK(s.pin.p == nullptr && t.pin.p == p);
        stage_round_trip(s, 4096);                         // the moved-from stage allocates anew
        CHECK(live() == base + 2);
        s = std::move(t);                                  // ... and gives that block up for the one it is assigned
        CHECK(live() == base + 1 && s.pin.p == p && t.pin.p == nullptr);
        stage_round_trip(s, 70000);
        s.release();
        s.release();
        CHECK(live() == base);
        stage_round_trip(s, 4096);
    }
    CHECK(live() == base);
}

// what the handles are: several buffers, no destructor of their own
struct Several {
    DevBuf a, b;
    HostPinned c;
    PinnedStage d;
    DevBuf more[3];
};

static void implicit_destructor() {
    const long base = live();
    {
        Several s;
        CHECK(s.a.reserve(10) == SQ_OK && s.b.reserve(20) == SQ_OK && s.c.reserve(30) == SQ_OK && s.d.begin(40) == SQ_OK);
        for (auto& m : s.more) CHECK(m.reserve(50) == SQ_OK);
        CHECK(live() == base + 7);
        Several t(std::move(s));   // memberwise move
        CHECK(live() == base + 7 && s.a.p == nullptr && s.more[2].p == nullptr && t.more[2].p != nullptr);
        hip_stub::fail_in = 1;
        CHECK(t.b.reserve(100000) == SQ_ERR_NOMEM && live() == base + 6);   // one member empty, the rest still owned
    }
    CHECK(live() == base);
}

int main() {
    lifetime<DevBuf>();
    lifetime<HostPinned>();
    sizes();
    exact();
    device_pointer();
    growing();
    staging();
    implicit_destructor();
    CHECK(live() == 0 && hip_stub::allocs > 0);
    printf("buffers ok: %ld allocations, %ld frees\n", hip_stub::allocs, hip_stub::frees);
    return 0;
}
