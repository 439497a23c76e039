// The host's arithmetic around the IVF-Flat index (sq_ivf.hip): the row stride, the offsets of the counting sort an add
// performs, the chunks of the list scan, and how many queries of a batch share the key scratch.  Everything in 64-bit.
// Plain C++, no runtime header: tests/host/ivf_plan_main.cpp runs it on the CPU.  ivf_locate is also what the scan kernel
// calls, so the walk the host program checks is the one the device makes.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SQ_IVF_HD __host__ __device__
#else
#define SQ_IVF_HD
#endif

namespace sq {

static constexpr int kIvfMaxLists = 65536;        // the coarse index answers from exact keys of every centroid up to here
static constexpr int kIvfAssignSlice = 1024;      // rows assigned per call of the coarse index
static constexpr int kIvfChunk = 256;             // candidates per work item of the scan: one per lane of a 256-thread workgroup
static constexpr long long kIvfMaxRows = 0xffffffffll;      // keys carry a 32-bit row number; all ones is the padding key's
static constexpr long long kIvfKeyBudget = 256ll << 20;     // bytes of key scratch a search may hold (option "ivf_key_budget_mb")
static constexpr long long kIvfSelectLdsKeys = 16384;       // k up to here: the one-workgroup select; beyond: a full sort
static constexpr long long kIvfSortChunk = 4096;            // keys per LDS chunk of that sort (SortLarge<u64>::CH)

// floats per stored row: whole 16-byte pieces, zero padded
inline long long ivf_row_stride(int d) { return ((long long)d + 3) / 4 * 4; }
inline bool ivf_rows_ok(long long n) { return n >= 0 && n <= kIvfMaxRows; }
inline long long ivf_rows_bytes(long long n, int d) { return n * ivf_row_stride(d) * 4; }

// Offsets of the stable counting sort of an add: list l of the new buffer holds its old rows (old_off[l] .. old_off[l + 1])
// and behind them the add_cnt[l] new ones.  new_off[nlist + 1]: where the lists start; add_at[nlist]: where the new rows
// of a list start; add_pre[nlist]: rows of the add that belong to lower lists (the position of a list's first new row in
// the add's rows sorted by (list, insertion number)).  Returns the rows in total.
inline long long ivf_merge_offsets(const long long* old_off, const long long* add_cnt, int nlist, long long* new_off,
                                   long long* add_at, long long* add_pre) {
    long long run = 0, pre = 0;
    for (int l = 0; l < nlist; ++l) {
        const long long old_n = old_off[l + 1] - old_off[l];
        new_off[l] = run;
        add_at[l] = run + old_n;
        add_pre[l] = pre;
        run += old_n + add_cnt[l];
        pre += add_cnt[l];
    }
    new_off[nlist] = run;
    return run;
}

// The list of position p in a query's concatenated candidate range: pre[0 .. np] are the exclusive prefix sums of the
// probed lists' sizes (pre[np] = the candidates in total, p < pre[np]); the answer is the last j with pre[j] <= p, which
// skips empty lists (their pre[j] == pre[j + 1]).
SQ_IVF_HD inline int ivf_locate(const long long* pre, int np, long long p) {
    int lo = 0, hi = np;   // invariant: pre[lo] <= p < pre[hi]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (pre[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// work items of the scan for a query of `cands` candidates
inline long long ivf_chunks(long long cands) { return (cands + kIvfChunk - 1) / kIvfChunk; }

// keys the full sort works on for lists of up to maxc keys (a power of two of at least one chunk)
inline long long ivf_sort_span(long long maxc) {
    long long p = kIvfSortChunk;
    while (p < maxc) p <<= 1;
    return p;
}
// results the select is asked for: k, but no more than the longest candidate list (the rest is padding)
inline long long ivf_select_k(long long maxc, long long k) { return k < maxc ? k : (maxc > 0 ? maxc : 1); }
// scratch bytes one query of a slice takes: its keys, the selected keys and, beyond the one-workgroup select, the two
// buffers of the full sort
inline long long ivf_query_scratch_bytes(long long maxc, long long k) {
    const long long mc = maxc > 0 ? maxc : 1, ks = ivf_select_k(maxc, k);
    long long b = (mc + ks) * 8;
    if (ks > kIvfSelectLdsKeys) b += 2 * ivf_sort_span(mc) * 8;
    return b;
}
// queries per slice: as many as the budget holds, one at least (a single query beyond the budget still runs)
inline long long ivf_slice_queries(long long nq, long long maxc, long long k, long long budget_bytes) {
    const long long per = ivf_query_scratch_bytes(maxc, k);
    long long s = budget_bytes / per;
    if (s < 1) s = 1;
    return s < nq ? s : nq;
}

}  // namespace sq
