// The host arithmetic of the list-major IVF-SQ scan (smqtk_indexing_amd/csrc/sq_isq_plan.hpp) on a CPU: compiled with
// -fsanitize=address,undefined and run by tests/test_host_logic_isq_shared.py.  The LDS the scan stages per kind, the
// edges of the route per kind, and that the automatic rule never widens what the kernel takes.  (The cut into groups and
// work items is sq_ivf_plan.hpp's: tests/host/ivf_shared_plan_main.cpp walks it.)
#include "../../smqtk_indexing_amd/csrc/sq_isq_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <initializer_list>

using namespace sq;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

int main() {
    constexpr int G = kIvfSharedGroup;
    const long long big = 1ll << 40;
    for (int kind : {kIsqSq8, kIsqF16}) {
        const int extra = kind == kIsqSq8 ? 2 : 0;   // SQ8 stages vmin and step once beside the G queries
        const long long R = isq_shared_auto_ratio(kind);
        CHECK(R == 0 || R == 1 || R == 2 || R == 4 || R == 8);
        for (int d = 1; d <= 8192; ++d) {
            const long long dq = (d + 3) / 4 * 4, lds = (extra + G) * dq * 4;
            CHECK(isq_shared_lds_bytes(d, kind) == lds && isq_stage_bytes(d, kind) == (extra + 1) * dq * 4);
            // option 1 takes a width exactly while the staging fits; -1 never widens what option 1 takes
            CHECK(isq_scan_route(1, kind, d, 6, 33, 8, 8, 1000) == (lds <= kIvfSharedLdsBytes));
            CHECK(isq_scan_route(-1, kind, d, 6, 1024, 64, 8, 1000) == (R > 0 && lds <= kIvfSharedLdsBytes));
        }
        const int edge = kind == kIsqSq8 ? 4088 : 5112;   // for G = 8
        CHECK(isq_scan_route(1, kind, edge - 3, 6, 33, 8, 8, 1000) && isq_scan_route(1, kind, edge, 6, 33, 8, 8, 1000));
        CHECK(!isq_scan_route(1, kind, edge + 1, 6, 33, 8, 8, 1000) && !isq_scan_route(1, kind, edge + 4, 6, 33, 8, 8, 1000));
        // option 0 never; option 1 wherever the kernel can run; a tree of depth 7 is declined under both
        CHECK(!isq_scan_route(0, kind, 128, 0, 1024, 16, 1024, big) && isq_scan_route(1, kind, 128, 0, 1, 1, 65536, 10));
        CHECK(!isq_scan_route(1, kind, 4000, kIvfSharedDepth + 1, 33, 8, 8, 1000) && !isq_scan_route(-1, kind, 128, 7, 1024, 8, 8, 1000));
        // one sort takes 2^24 pairs; the grid is one-dimensional
        CHECK(isq_scan_route(1, kind, 8, 0, 1 << 12, 1 << 12, 8, 1000) && !isq_scan_route(1, kind, 8, 0, (1 << 12) + 1, 1 << 12, 8, 1000));
        CHECK(!isq_scan_route(-1, kind, 8, 0, (1 << 12) + 1, 1 << 12, 8, 1000) && !isq_scan_route(1, kind, 8, 0, 0, 16, 1024, 0));
        CHECK(!isq_scan_route(1, kind, 8, 0, 1000, 16, 1024, kIvfSharedMaxItems * kIvfChunk));
        // automatic: from R pairs per list of the index; R = 0 is "never"
        CHECK(isq_scan_route(-1, kind, 128, 0, 256 * R, 16, 4096, 1000) == (R > 0) && !isq_scan_route(-1, kind, 128, 0, 256 * R - 1, 16, 4096, 1000));
    }
    printf("isq shared plan ok: group=%d lds=%lld auto_ratio sq8=%lld f16=%lld\n", G, kIvfSharedLdsBytes, kIsqSharedAutoRatioSq8, kIsqSharedAutoRatioF16);
    return 0;
}
