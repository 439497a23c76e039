// The host arithmetic of the IVF-Flat index (smqtk_indexing_amd/csrc/sq_ivf_plan.hpp) on a CPU: compiled with
// -fsanitize=address,undefined and run by tests/test_host_logic_ivf.py.  Checked here: the counting sort's offsets
// against a direct stable sort; the scan's chunks covering every candidate once, through the same ivf_locate the kernel
// calls, at list lengths 0, 1, chunk - 1, chunk and chunk + 1; ivf_locate over prefix arrays of 65, 257 and 700 entries
// with runs of empty lists; slice sizes that keep the key scratch under the budget; 64-bit products at 2^32 - 1 rows.
#include "../../smqtk_indexing_amd/csrc/sq_ivf_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace sq;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

static unsigned long long g_state = 0x9e3779b97f4a7c15ull;
static unsigned rnd(unsigned m) {   // xorshift64*
    g_state ^= g_state >> 12, g_state ^= g_state << 25, g_state ^= g_state >> 27;
    return (unsigned)((g_state * 0x2545f4914f6cdd1dull) >> 33) % m;
}

// Two adds into nlist lists, the second through ivf_merge_offsets: the slot of every row equals its place in a stable
// sort of all rows by list.
static void counting_sort(int nlist, int n_old, int n_add, int empty_every) {
    auto pick = [&](void) {
        int l = (int)rnd((unsigned)nlist);
        if (empty_every && l % empty_every == 0) l = (l + 1) % nlist;   // some lists stay empty
        return l;
    };
    std::vector<int> list_of((size_t)(n_old + n_add));
    for (auto& l : list_of) l = pick();
    // the old index: rows 0 .. n_old by a direct stable sort
    std::vector<long long> old_off((size_t)nlist + 1, 0), add_cnt((size_t)nlist, 0);
    for (int i = 0; i < n_old; ++i) old_off[(size_t)list_of[(size_t)i] + 1]++;
    for (int l = 0; l < nlist; ++l) old_off[(size_t)l + 1] += old_off[(size_t)l];
    for (int i = n_old; i < n_old + n_add; ++i) add_cnt[(size_t)list_of[(size_t)i]]++;
    std::vector<long long> new_off((size_t)nlist + 1), add_at((size_t)nlist), add_pre((size_t)nlist);
    const long long total = ivf_merge_offsets(old_off.data(), add_cnt.data(), nlist, new_off.data(), add_at.data(), add_pre.data());
    CHECK(total == n_old + n_add && new_off[0] == 0 && new_off[(size_t)nlist] == total);
    // where the scatter kernels put every row
    std::vector<long long> slot((size_t)(n_old + n_add), -1);
    {
        std::vector<long long> seen((size_t)nlist, 0);   // old rows: slot s of list l -> new_off[l] + (s - old_off[l])
        for (int i = 0; i < n_old; ++i) {
            const int l = list_of[(size_t)i];
            slot[(size_t)i] = new_off[(size_t)l] + seen[(size_t)l]++;
        }
        for (int l = 0; l < nlist; ++l) CHECK(seen[(size_t)l] == old_off[(size_t)l + 1] - old_off[(size_t)l]);
        // new rows: t-th in (list, insertion) order -> add_at[l] + (t - add_pre[l])
        std::vector<std::pair<int, int>> keys;
        for (int i = 0; i < n_add; ++i) keys.push_back({list_of[(size_t)(n_old + i)], i});
        std::sort(keys.begin(), keys.end());
        for (long long t = 0; t < (long long)keys.size(); ++t) {
            const int l = keys[(size_t)t].first;
            CHECK(t >= add_pre[(size_t)l] && t - add_pre[(size_t)l] < add_cnt[(size_t)l]);
            slot[(size_t)(n_old + keys[(size_t)t].second)] = add_at[(size_t)l] + (t - add_pre[(size_t)l]);
        }
    }
    // the direct sort
    std::vector<int> order((size_t)(n_old + n_add));
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return list_of[(size_t)a] < list_of[(size_t)b]; });
    for (size_t p = 0; p < order.size(); ++p) CHECK(slot[(size_t)order[p]] == (long long)p);
    for (int l = 0; l < nlist; ++l)
        for (long long p = new_off[(size_t)l]; p < new_off[(size_t)l + 1]; ++p) CHECK(list_of[(size_t)order[(size_t)p]] == l);
}

// every candidate of a query is visited exactly once by the chunks, in the list and at the offset the prefix array says
static void chunks(const std::vector<long long>& sizes) {
    const int np = (int)sizes.size();
    std::vector<long long> pre((size_t)np + 1, 0);
    for (int j = 0; j < np; ++j) pre[(size_t)j + 1] = pre[(size_t)j] + sizes[(size_t)j];
    const long long total = pre[(size_t)np];
    CHECK(ivf_chunks(total) * kIvfChunk >= total && (ivf_chunks(total) - 1) * kIvfChunk < total + (total == 0 ? kIvfChunk : 0));
    std::vector<std::vector<int>> hits((size_t)np);
    for (int j = 0; j < np; ++j) hits[(size_t)j].assign((size_t)sizes[(size_t)j], 0);
    long long visited = 0;
    for (long long c = 0; c < ivf_chunks(total); ++c)
        for (int lane = 0; lane < kIvfChunk; ++lane) {
            const long long p = c * kIvfChunk + lane;
            if (p >= total) continue;
            const int j = ivf_locate(pre.data(), np, p);
            CHECK(j >= 0 && j < np && pre[(size_t)j] <= p && p < pre[(size_t)j + 1]);
            hits[(size_t)j][(size_t)(p - pre[(size_t)j])]++;
            ++visited;
        }
    CHECK(visited == total);
    for (const auto& h : hits)
        for (int v : h) CHECK(v == 1);
}

// A prefix array of np entries as a query probing more lists than a wave has lanes meets it: lists of 1 to 48 rows with
// runs of empty ones (equal prefix values) at the front, across entries 63 / 64 and 255 / 256, at the end, and one
// scattered in every 11.  Every position is located in the LAST list whose prefix is at or below it -- found here by
// walking down from the end -- and that list is not empty.
static void long_prefix(int np) {
    std::vector<long long> sizes((size_t)np);
    for (int j = 0; j < np; ++j) {
        const bool empty = j < 3 || (j >= 62 && j <= 65) || (j >= 254 && j <= 257) || j >= np - 3 || rnd(11) == 0;
        sizes[(size_t)j] = empty ? 0 : 1 + (long long)rnd(48);
    }
    std::vector<long long> pre((size_t)np + 1, 0);
    for (int j = 0; j < np; ++j) pre[(size_t)j + 1] = pre[(size_t)j] + sizes[(size_t)j];
    const long long total = pre[(size_t)np];
    CHECK(total > 0 && pre[3] == 0 && pre[(size_t)np - 3] == total);
    if (np > 66) CHECK(pre[62] == pre[66]);
    if (np > 258) CHECK(pre[254] == pre[258]);
    for (long long p = 0; p < total; ++p) {
        int want = np - 1;
        while (pre[(size_t)want] > p) --want;
        const int j = ivf_locate(pre.data(), np, p);
        CHECK(j == want && sizes[(size_t)j] > 0 && p - pre[(size_t)j] < sizes[(size_t)j]);
    }
    chunks(sizes);
}

static void slices() {
    const long long budget = kIvfKeyBudget;
    const long long ks[] = {1, 100, 16384, 16385, 30000, 1000000};
    const long long cs[] = {0, 1, 255, 2441, 20011, 156250, 10000000, 33554432, 4294967295ll};
    const long long nqs[] = {1, 32, 33, 4096, 100000};
    for (long long k : ks)
        for (long long maxc : cs)
            for (long long nq : nqs) {
                const long long per = ivf_query_scratch_bytes(maxc, k), s = ivf_slice_queries(nq, maxc, k, budget);
                CHECK(per > 0 && s >= 1 && s <= nq);
                CHECK(s * per <= budget || s == 1);                  // under the budget, or the one query that must run
                CHECK(s == nq || (s + 1) * per > budget);            // and no smaller than the budget asks
                const long long ksel = ivf_select_k(maxc, k);
                CHECK(ksel >= 1 && ksel <= k && (maxc == 0 || ksel <= maxc));
                CHECK(per >= ((maxc > 0 ? maxc : 1) + ksel) * 8);
                if (ksel > kIvfSelectLdsKeys) {
                    const long long span = ivf_sort_span(maxc);
                    CHECK(span >= maxc && span >= kIvfSortChunk && (span & (span - 1)) == 0 && (span == kIvfSortChunk || span / 2 < maxc));
                    CHECK(per == (maxc + ksel + 2 * span) * 8);
                }
            }
    // a small budget: 33 queries of 20011 candidates run in slices of 6 under 1 MiB
    CHECK(ivf_slice_queries(33, 20011, 10, 1ll << 20) == 6);
    CHECK(ivf_slice_queries(33, 20011, 30000, 1ll << 20) == 1);
}

static void wide() {
    const long long n = kIvfMaxRows;   // 2^32 - 1
    CHECK(ivf_rows_ok(n) && !ivf_rows_ok(n + 1) && ivf_rows_ok(0) && !ivf_rows_ok(-1));
    CHECK(ivf_row_stride(1) == 4 && ivf_row_stride(4) == 4 && ivf_row_stride(5) == 8 && ivf_row_stride(36) == 36 && ivf_row_stride(127) == 128);
    CHECK(ivf_row_stride(2147483647) == 2147483648ll);
    CHECK(ivf_rows_bytes(n, 128) == 4294967295ll * 512 && ivf_rows_bytes(n, 8190) == 4294967295ll * 8192 * 4);
    CHECK(ivf_chunks(n) == 16777216 && ivf_chunks(n) * kIvfChunk >= n);
    CHECK(ivf_query_scratch_bytes(n, 1) == (n + 1) * 8 && ivf_query_scratch_bytes(n, n) == (n + n + 2 * 4294967296ll) * 8);
    CHECK(ivf_slice_queries(1000, n, 10, kIvfKeyBudget) == 1);
    // offsets at that size: one list with everything, the add on top
    const long long old_off[3] = {0, n - 5, n - 5}, add_cnt[2] = {2, 3};
    long long new_off[3], add_at[2], add_pre[2];
    CHECK(ivf_merge_offsets(old_off, add_cnt, 2, new_off, add_at, add_pre) == n);
    CHECK(new_off[0] == 0 && new_off[1] == n - 3 && new_off[2] == n && add_at[0] == n - 5 && add_at[1] == n - 3 && add_pre[0] == 0 && add_pre[1] == 2);
    // a prefix array that ends at 2^32 - 1
    const long long pre[4] = {0, 1, 1, n};
    CHECK(ivf_locate(pre, 3, 0) == 0 && ivf_locate(pre, 3, 1) == 2 && ivf_locate(pre, 3, n - 1) == 2);
}

int main() {
    counting_sort(1, 0, 17, 0);
    counting_sort(1, 9, 1, 0);
    counting_sort(7, 0, 500, 0);
    counting_sort(64, 3000, 1, 5);
    counting_sort(64, 1, 7000, 5);
    counting_sort(300, 2000, 2000, 3);
    counting_sort(4096, 100, 100, 0);   // most lists empty
    const long long C = kIvfChunk;
    const long long lens[] = {0, 1, C - 1, C, C + 1};
    for (long long a : lens)
        for (long long b : lens)
            for (long long c : lens) {
                chunks({a});
                chunks({a, b});
                chunks({a, b, c});
                chunks({0, a, 0, 0, b, 4 * C + 3, c, 0});
            }
    for (int np : {65, 257, 700})
        for (int rep = 0; rep < 4; ++rep) long_prefix(np);
    slices();
    wide();
    printf("ivf plan ok: chunk=%d budget=%lld max_lists=%d\n", kIvfChunk, kIvfKeyBudget, kIvfMaxLists);
    return 0;
}
