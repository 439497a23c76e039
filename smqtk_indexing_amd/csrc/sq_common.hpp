// Internal helpers shared by the libsmqtk_hip translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/smqtk_hip.h"
#include "sq_buffers.hpp"   // errors (fail, SQ_HIP, SQ_TRY) and the owning buffers (DevBuf, HostPinned, PinnedStage, grow_keep)

typedef unsigned long long u64;
typedef unsigned int u32;

namespace sq {

// ----------------------------------------------------------------- options
struct Options {
    int profile = 0;         // 1: hipEvent timing of the search stages into sq_stats_t; N > 1: only every N-th asynchronous dense search is timed (the others report scan_ms = 0)
    int sample_stride = 0;   // 0 = auto
    int candidate_cap = 0;   // 0 = auto
    int force_fallback = 0;
    int dense_stages = 0;    // 0 = auto (LDS ring depth of the dense scan)
    int dense_blocks = 0;    // 0 = auto (row blocks of the dense scan grid)
    int dense_sample_blocks = 0;  // pipelined one-group searches: workgroups of the SAMPLE pass; 0 = auto (the CUs the full pass leaves free), -1 = as many as the full pass, N = N
    int dense_debug = 0;     // measurement only (see DenseScanArgs::debug)
    int dense_waves = 0;     // 0 = auto, 4 or 8 waves per scan workgroup
    int dense_qt = 0;        // 0 = auto, 1 / 2 / 4 query tiles per scan wave
    int itq_exact = 0;       // 1 = every row through the float64 ITQ kernel (no bf16 filter)
    int dense_qplanes = 0;       // 0 = auto, 2 = keep q_hi + q_lo also in the multi-tile scan
    int dense_no_center = 0;     // 1 = the dense L2 filter scores the rows as given (no column-mean origin; measurement)
    int dense_rerank_segments = 0;  // survivor segments per re-rank workgroup (0 = all waves of a scan workgroup; measurement)
    int merge_threads = 0;       // host threads of the shard merge (0 = by size)
    int spin_wait_us = 2000;     // searches poll the stream this long before blocking (0 = block at once)
    int dense_async_streams = 2; // asynchronous dense searches: 2 = the two call slots run on streams of their own (tail of call i overlaps the head of call i + 1), 1 = everything on the caller's stream
    int dense_async_depth = 2;   // asynchronous dense searches in flight (2..4): the results of a call are final when the (depth - 1)-th call after it returns
    int dense_async_wait = 1;    // 1: an asynchronous dense search returns once the oldest call in flight is final; 0: it returns right after enqueueing (the wait moves to the start of the next call: one more call of lag, host work between calls overlaps the device)
    int dense_async_order = 1;   // 1: an asynchronous dense search on internal streams starts behind the work already on the caller's stream (an event per call); 0: the caller guarantees its queries are complete -- no event, the call starts as soon as the device has room
    int dense_nt = -1;           // non-temporal LDS-DMA of the dense scan's row stream (launches of one query group): -1 = automatic, 0 = never, 1 = every byte
    int dense_nt_keep_mb = 0;    // one-tile dense scan, automatic mode: MB at the head of the scan copy that keep the default cache policy (0 = 192)
    int hamming_no_permute = 0;  // 1 = keep the Hamming code array in caller order on the device (measurement)
    int dense_fused_prep = 1;    // 1 = L2 searches of one query tile build the query planes inside the scan kernels (no prep launch); 0 = dense_prep_queries_kernel
    int dense_int8_batch = 64;   // largest batch the int8 filter takes (33 .. 64: two query tiles per wave, 128-byte rows; up to 256: four tiles, which only ties with the bf16 kernels; 32 = one tile only)
    int dense_fused = 1;         // int8 calls of one query tile as three launches (head: query prep + sample pass + threshold by the last workgroup; full pass with the re-rank as its tail; select) instead of six; 0 = the six-launch chain
    int dense_tighten = 1;       // fused int8 calls: the full pass histograms its entries' scores and its tail re-ranks only those under the tightened threshold (sq_dense_i8.hpp); rows beyond 512 dimensions: the second-level threshold of sq_dense_tighten.hpp between the pass and the re-rank; 0 = every entry is re-ranked (measurement)
    int dense_graph = 1;         // pipelined int8 calls: the call's kernels as one captured graph launch (0 = eager launches)
    int dense_int8 = -1;         // int8 first-stage filter (L2, d <= 128, one query tile): -1 = automatic, 0 = never (bf16 filter), 1 = whenever the copy exists
    int dense_int8_wide = 0;     // int8 first-stage filter for rows of 513 to 8192 dimensions (sq_dense_i8_wide.hpp; L2 and cosine, one query tile): read when an index is created, appended to or compacted -- 1 = such an index of at least 65536 rows keeps the int8 copy and its calls of up to 32 queries stream it ("dense_int8" = 0 on the handle turns the stage off); 0 = no copy, the bfloat16 filter as before
    int dense_bf16 = 1;          // the bfloat16 scan copy of a dense index (rows of up to 8192 dimensions), read when copies are built (create, compact, the first search that wants the copy): 1 = built at create / compact; -1 = on demand -- built by the first search that takes the bfloat16 chain, kept from then on, shed again by sq_dense_compact; 0 = never -- calls the int8 stage does not take go to the later tiers (set on a handle that has the copy: the copy is left alone, not freed)
    int dense_mid_tier = 1;      // 1 = queries the first filter could not certify get a second, tighter filter pass (L2 and cosine: bf16 planes of the float32 rows built on the fly) before the exact all-rows path, and calls start there once the first filter's lists overflow call after call; 0 = straight to the exact path
    int hamming_async_depth = 2; // asynchronous Hamming searches in flight (2..4), as dense_async_depth
    int hamming_async_wait = 1;  // as dense_async_wait
    int hamming_async_order = 1; // as dense_async_order
    int hamming_ring = -1;       // Hamming stream kernel: -1 = automatic (LDS-DMA ring for arrays beyond the MALL), 0 = register loads, 1 = ring (1 .. 7, 8, 16 words, 16-byte aligned arrays; the register kernel otherwise)
    int hamming_tighten = 1;     // fused Hamming searches: stream threshold from a lower sample rank than k (far fewer candidates); a bet the pick kernel checks -- a lost one redoes the call with the safe rule; 0 = the safe rank-k rule
    int ivf_key_budget_mb = 0;   // IVF search: MB of key scratch a call may hold -- a batch runs in query slices under it (0 = 256; sq_ivf_plan.hpp)
    int hamming_fused = 1;       // Hamming searches of up to 32 queries (64 .. 448-bit codes, k <= 2048) as three launches (head: sampled histogram + thresholds by the last workgroup; stream; pick: exact k-th distance + gather + sort per query) instead of a memset and five; 0 = the general chain
};
extern Options g_opt;   // process-wide defaults (sq_set_option); a handle may override any of them (sq_handle_set_option)
// name -> member, shared by sq_set_option and sq_handle_set_option (sq_core.hip)
int Options::*option_member(const char* name);

// Wait the way a latency-bound caller wants to: poll `query` for a while (a search is a fraction of a millisecond;
// the blocking wait's wake-up costs tens of microseconds of it), then `block`.
// Option "spin_wait_us" (default 2000; 0 = always block).
template <class Query, class Block>
inline hipError_t poll_then_block(Query query, Block block) {
    const long long budget_us = g_opt.spin_wait_us;
    if (budget_us > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            for (int i = 0; i < 64; ++i) {
                const hipError_t e = query();
                if (e != hipErrorNotReady) return e;
            }
            if (std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() > budget_us)
                break;
        }
    }
    return block();
}
inline hipError_t stream_wait(hipStream_t st) {
    return poll_then_block([st] { return hipStreamQuery(st); }, [st] { return hipStreamSynchronize(st); });
}
inline hipError_t event_wait(hipEvent_t ev) {
    return poll_then_block([ev] { return hipEventQuery(ev); }, [ev] { return hipEventSynchronize(ev); });
}
}  // namespace sq
#include "sq_pipeline.hpp"   // the call slots' events and streams, the ring of slots, the host-memory call: they wait with the two above
namespace sq {

// ------------------------------------------------------------------ handles
enum HandleKind { H_HAMMING = 1, H_DENSE = 2, H_ROWS = 3, H_FIT = 4, H_ITQ = 5, H_IVF = 6, H_PQ = 7 };

struct HandleBase {
    int kind = 0;
    int device = 0;
    std::mutex mu;
    sq_stats_t stats{};
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    // Options of THIS handle: the process-wide values with the handle's own overrides on top, re-read under the
    // handle's lock at every API entry (refresh_options).  Two indexes searched from two threads therefore keep their
    // own pipeline depth, candidate lists, profiling ... (the reference's contract: "implementations should be
    // thread safe", interfaces/nearest_neighbor_index.py:22-23).
    std::vector<std::pair<int Options::*, int>> overrides;
    Options opt;
    void refresh_options() {
        opt = g_opt;
        for (const auto& o : overrides) opt.*(o.first) = o.second;
    }
    virtual ~HandleBase() {
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

sq_handle_t register_handle(HandleBase* h);
HandleBase* lookup_handle(sq_handle_t id, int kind);
HandleBase* remove_handle(sq_handle_t id, int kind);

// The bodies of sq_*_sync / sq_*_destroy of a handle with pipelined calls: `drain(h)` finishes every call in flight; a null `h`: no such handle.
template <class H, class Drain>
inline int handle_sync(H* h, const char* who, Drain drain) {
    if (!h) return fail(SQ_ERR_INVALID, "%s: unknown handle", who);
    std::lock_guard<std::mutex> lock(h->mu);
    h->refresh_options();
    SQ_HIP(hipSetDevice(h->device));
    return drain(h);
}
template <class H, class Drain>
inline int handle_destroy(H* h, const char* who, Drain drain) {
    if (!h) return fail(SQ_ERR_INVALID, "%s: unknown handle", who);
    (void)handle_sync(h, who, drain);  // nothing of this handle is left on the device when its buffers go
    delete h;
    return SQ_OK;
}

inline int cu_count(int device) {
    static int cached[64] = {0};
    if (device >= 0 && device < 64 && cached[device]) return cached[device];
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, device) != hipSuccess) return 256;
    if (device >= 0 && device < 64) cached[device] = p.multiProcessorCount;
    return p.multiProcessorCount;
}

// ----------------------------------------------------------------- launches
// Launch `Kernel` and report a bad launch configuration where it happens, not at the next wait.
template <auto Kernel, class... Args>
inline int launch(dim3 grid, dim3 block, size_t lds, hipStream_t st, Args&&... args) {
    Kernel<<<grid, block, lds, st>>>(std::forward<Args>(args)...);
    SQ_HIP(hipGetLastError());
    return SQ_OK;
}

// launch() for a kernel that may take more than 64 KiB of dynamic LDS.  `max_dyn_lds` is the largest `lds` the kernel
// is ever launched with (a kernel with static LDS of its own asks for its ring, not the CU's 160 KiB).
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) applies to the CURRENT device's copy of a kernel: once per (kernel
// instantiation, device), the mask below being this instantiation's (a second GPU used from the same process otherwise
// never gets the attribute and its launches with more than 64 KiB of LDS fail).
template <auto Kernel, class... Args>
inline int launch_lds(int max_dyn_lds, dim3 grid, dim3 block, size_t lds, hipStream_t st, Args&&... args) {
    static std::atomic<unsigned long long> done_devices{0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    const unsigned long long bit = dev >= 0 && dev < 64 ? 1ull << dev : 0ull;
    if (!bit || !(done_devices.load(std::memory_order_relaxed) & bit)) {
        SQ_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, max_dyn_lds));
        if (bit) done_devices.fetch_or(bit, std::memory_order_relaxed);
    }
    return launch<Kernel>(grid, block, lds, st, std::forward<Args>(args)...);
}

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace sq
