// The host arithmetic of the list-major IVF-Flat scan (smqtk_indexing_amd/csrc/sq_ivf_plan.hpp) on a CPU: compiled with
// -fsanitize=address,undefined and run by tests/test_host_logic_ivf_shared.py.  The groups and the prefix of work items
// are built as ivf_pair_groups_kernel builds them and walked as ivf_scan_shared_kernel walks them (ivf_locate over the
// prefix): for list lengths 0 .. 1025 and 1 .. 3 G + 1 pairs on a list, every row of every pair is covered by exactly
// one (work item, lane, slot), and the grid bound the host launches with is never below the true count.  Then the route.
#include "../../smqtk_indexing_amd/csrc/sq_ivf_plan.hpp"

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

struct Group {
    long long first, count, list;
};

// lists of these lengths, list l probed by pairs[l] pairs: the cover
static void cover(const std::vector<long long>& len, const std::vector<long long>& pairs) {
    constexpr int G = kIvfSharedGroup;
    const int nlist = (int)len.size();
    std::vector<Group> groups;
    std::vector<long long> item;   // exclusive prefix of the groups' chunks
    long long first = 0, items = 0, cands = 0, live = 0;
    for (int l = 0; l < nlist; ++l) {
        const long long c = len[(size_t)l] > 0 ? pairs[(size_t)l] : 0;   // pairs of an empty list are dropped before the cut
        for (long long g = 0; g < ivf_pair_groups(c, G); ++g) {
            groups.push_back({first + g * G, ivf_pair_group_size(c, g, G), l});
            item.push_back(items);
            items += ivf_row_chunks(len[(size_t)l]);
        }
        first += c;
        live += c;
        cands += pairs[(size_t)l] * len[(size_t)l];
    }
    item.push_back(items);
    long long all_pairs = 0;
    for (long long c : pairs) all_pairs += c;
    CHECK(ivf_shared_items_bound(cands, all_pairs) >= items);
    CHECK((long long)groups.size() <= live);
    std::vector<std::vector<int>> hits((size_t)live);   // per live pair, per row
    {
        long long p = 0;
        for (int l = 0; l < nlist; ++l)
            for (long long c = 0; c < (len[(size_t)l] > 0 ? pairs[(size_t)l] : 0); ++c) hits[(size_t)p++].assign((size_t)len[(size_t)l], 0);
    }
    for (long long b = 0; b < ivf_shared_items_bound(cands, all_pairs); ++b) {
        if (b >= items) continue;   // blocks beyond the device-side count return at once
        const int g = ivf_locate(item.data(), (int)groups.size(), b);
        CHECK(g >= 0 && g < (int)groups.size() && item[(size_t)g] <= b && b < item[(size_t)g + 1]);
        const Group& gr = groups[(size_t)g];
        CHECK(gr.count >= 1 && gr.count <= G);
        const long long chunk = b - item[(size_t)g];
        for (int lane = 0; lane < kIvfChunk; ++lane) {
            const long long r = chunk * kIvfChunk + lane;
            if (r >= len[(size_t)gr.list]) continue;
            for (int slot = 0; slot < G; ++slot)
                if (slot < gr.count) hits[(size_t)(gr.first + slot)][(size_t)r]++;
        }
    }
    for (const auto& h : hits)
        for (int v : h) CHECK(v == 1);
}

static void route() {
    const long long big = 1ll << 40;
    // option 0 never; option 1 wherever the kernel can run
    CHECK(!ivf_scan_route(0, 128, 0, 1024, 16, 1024, big) && ivf_scan_route(1, 128, 0, 1, 1, 65536, 10));
    // eight staged queries in 160 KiB - 256 bytes: round_up(d, 4) <= 5112; a tree of depth 7 is declined
    CHECK(ivf_scan_route(1, 5112, 6, 33, 8, 8, 1000) && ivf_scan_route(1, 5109, 6, 33, 8, 8, 1000) && !ivf_scan_route(1, 5113, 6, 33, 8, 8, 1000));
    CHECK(!ivf_scan_route(1, 4000, 7, 33, 8, 8, 1000));
    // the pair index rides in 32 bits and one sort takes 2^24 pairs; the grid is one-dimensional
    CHECK(ivf_scan_route(1, 8, 0, 1 << 12, 1 << 12, 8, 1000) && !ivf_scan_route(1, 8, 0, (1 << 12) + 1, 1 << 12, 8, 1000));
    CHECK(!ivf_scan_route(1, 8, 0, 1000, 16, 1024, kIvfSharedMaxItems * kIvfChunk));
    // automatic: from kIvfSharedAutoRatio pairs per list of the index
    const long long R = kIvfSharedAutoRatio;
    CHECK(ivf_scan_route(-1, 128, 0, 256 * R, 16, 4096, 1000) && !ivf_scan_route(-1, 128, 0, 256 * R - 1, 16, 4096, 1000));
    CHECK(!ivf_scan_route(-1, 128, 0, 1, 64, 4096, 100) && !ivf_scan_route(-1, 128, 0, 32, 16, 4096, 100));
    CHECK(ivf_scan_route(-1, 8, 0, 70000, 2, 8, 1000) && ivf_scan_route(-1, 36, 0, 33, 64, 64, 1000));
    CHECK(!ivf_scan_route(-1, 5113, 6, 1024, 8, 8, 1000));   // the automatic rule never widens what the kernel takes
}

int main() {
    constexpr int G = kIvfSharedGroup;
    for (long long len = 0; len <= 1025; ++len)
        for (long long c = 1; c <= 3 * G + 1; ++c) cover({len}, {c});
    // several lists in one prefix: empty ones between, lists nobody probes, a long list shared by many
    cover({5, 0, 256, 257, 0, 1025, 1}, {1, 4, G, G + 1, 9, 3 * G + 1, 2 * G});
    cover({300, 300, 300}, {0, G + 3, 0});
    cover({0, 0}, {3, G});
    route();
    printf("ivf shared plan ok: group=%d chunk=%d auto_ratio=%lld\n", G, kIvfChunk, kIvfSharedAutoRatio);
    return 0;
}
