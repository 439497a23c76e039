// sq_opq_plan.hpp walked on the CPU under AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_host_logic_opq.py):
// for every width the LDS a workgroup asks for, the pitches' bank rule, and -- on arrays of exactly the planned size --
// every LDS index opq_apply_kernel's staging writes and its operand reads form (a read element must have been written).
#include <cstdio>
#include <vector>

#include "../../smqtk_indexing_amd/csrc/sq_opq_plan.hpp"

using namespace sq;

static int d = 0;
#define CHECK(c) do { if (!(c)) { std::printf("opq plan: %s failed at d = %d (line %d)\n", #c, d, __LINE__); return 1; } } while (0)

int main() {
    int widest = 0, switch_at = 0;
    for (d = 1; d <= kOpqMaxD; ++d) {
        const OpqPlan p = opq_plan(d);
        CHECK(p.lds_bytes <= kOpqLdsMax && p.sx % 8 == 4 && p.sa % 8 == 4 && p.lda % 4 == 0 && p.lda >= d && p.lda < d + 4);
        CHECK(p.nslab == (d + 31) / 32 && p.ncb == (d + 127) / 128 && p.resident == (d <= kOpqResidentMaxD));
        if (p.resident) switch_at = d;
        if (p.lds_bytes > widest) widest = p.lds_bytes;
        std::vector<char> xs((size_t)kOpqTileRows * p.sx, 0), as((size_t)kOpqColBlock * p.sa, 0);
        CHECK((int)((xs.size() + as.size()) * 4) == p.lds_bytes);
        const int pieces = (p.sx - 4) / 4;
        for (int tid = 0; tid < 256; ++tid) {
            const int sr = tid >> 3, sc = (tid & 7) * 4;
            for (int e = 0; e < 4; ++e) {
                for (int u = 0; u < 4; ++u) as.at((size_t)(sr + 32 * u) * p.sa + sc + e) = 1;
                for (int u = 0; u < 2 && !p.resident; ++u) xs.at((size_t)(sr + 32 * u) * p.sx + sc + e) = 1;
                for (int idx = tid; p.resident && idx < kOpqTileRows * pieces; idx += 256) xs.at((size_t)(idx / pieces) * p.sx + 4 * (idx % pieces) + e) = 1;
            }
        }
        for (int s = 0; s < p.nslab; ++s) {
            const int steps = opq_slab_steps(d, s);
            CHECK(steps >= 1 && steps * kOpqKStep <= kOpqSlabK);
            for (int row : {0, 31, 32, kOpqTileRows - 1})   // (every row has the same k offsets)
                for (int k = 0; k < steps * kOpqKStep; ++k) {
                    CHECK(xs.at((size_t)row * p.sx + (p.resident ? s * kOpqSlabK : 0) + k) == 1);
                    CHECK(as.at((size_t)row * p.sa + k) == 1 && as.at((size_t)(row + 64) * p.sa + k) == 1);
                }
        }
    }
    CHECK(opq_tiles(0) == 0 && opq_tiles(64) == 1 && opq_tiles(65) == 2 && opq_tiles(10000000) == 156250);
    CHECK(opq_grid(156250, 256) == 2048u && opq_grid(0, 256) == 1u && opq_grid(7, 256) == 7u && opq_grid(1ll << 56, 0) == (unsigned)kOpqBlocksPerCu);
    std::printf("opq plan ok: widest_lds=%d resident_up_to=%d\n", widest, switch_at);
    return 0;
}
