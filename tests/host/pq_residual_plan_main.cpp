// The host arithmetic of the IVF-PQ index's residual mode (smqtk_indexing_amd/csrc/sq_pq_plan.hpp) on a CPU: compiled
// with -fsanitize=address,undefined and run by tests/test_host_logic_pq_residual.py.  Checked here: the pairs per launch
// inside 1 .. 65535; the budget invariant -- keys of the slice and tables of a launch within the budget whenever one
// query's keys and one pair's tables fit --; room for one pair per query of the slice; the ranges of a slice covering
// its pairs once, in order, counted by pq_res_launches; the longest list.  It prints
// "plan <nq> <np> <maxc> <k> <m> <ksub> <budget> <slice> <pairs per launch> <launches>" lines that the Python
// restatement (tests/pq_residual_cases.py) is compared with.
#include "../../smqtk_indexing_amd/csrc/sq_pq_plan.hpp"

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

static long long g_lines = 0;

static void one(long long nq, long long np, long long maxc, long long k, int m, int ksub, long long budget, bool print) {
    const long long per = ivf_query_scratch_bytes(maxc, k), tb = pq_table_bytes(m, ksub);
    const long long slice = pq_slice_queries(nq, maxc, k, m, ksub, budget);
    const long long ppl = pq_res_pairs_per_launch(slice, maxc, k, m, ksub, budget);
    const long long launches = pq_res_launches(nq, np, maxc, k, m, ksub, budget);
    CHECK(slice >= 1 && slice <= nq && ppl >= 1 && ppl <= kPqMaxPairsPerLaunch);
    if (per + tb <= budget) {
        // the budget invariant, and room for the tables of one pair per query of the slice (unless the grid's limit cuts it)
        CHECK(pq_res_scratch_bytes(slice, ppl, maxc, k, m, ksub) <= budget);
        CHECK(ppl >= slice || ppl == kPqMaxPairsPerLaunch);
        // no larger count would do
        CHECK(ppl == kPqMaxPairsPerLaunch || pq_res_scratch_bytes(slice, ppl + 1, maxc, k, m, ksub) > budget);
    } else {
        CHECK(slice == 1 && ppl == 1);   // a single query beyond the budget still runs, one pair at a time
    }
    // the walk sq_pq.hip makes: every pair of every slice in exactly one range, ranges in order
    const long long eff = ppl < slice * np ? ppl : slice * np;
    long long walked = 0, pairs_seen = 0;
    if (maxc > 0 && nq * np <= 2000000) {
        for (long long q0 = 0; q0 < nq; q0 += slice) {
            const long long ns = nq - q0 < slice ? nq - q0 : slice, pairs = ns * np;
            long long next = 0;
            for (long long p0 = 0; p0 < pairs; p0 += eff) {
                const long long pl = pairs - p0 < eff ? pairs - p0 : eff;
                CHECK(p0 == next && pl >= 1 && pl <= kPqMaxPairsPerLaunch && pl * tb <= (eff * tb));
                next = p0 + pl;
                ++walked;
            }
            CHECK(next == pairs);
            pairs_seen += pairs;
        }
        CHECK(walked == launches && pairs_seen == nq * np);
    }
    if (maxc == 0) CHECK(launches == 0);
    if (print) {
        printf("plan %lld %lld %lld %lld %d %d %lld %lld %lld %lld\n", nq, np, maxc, k, m, ksub, budget, slice, ppl, launches);
        ++g_lines;
    }
}

static void sweep() {
    const long long budgets[] = {1ll << 20, 3ll << 20, kIvfKeyBudget};
    const long long ks[] = {1, 10, 100, 5000, 16385};
    const long long cs[] = {0, 1, 5, 3001, 12000, 156250, 10000000};
    const long long nqs[] = {1, 3, 5, 33, 64, 600, 70000};
    const long long nps[] = {1, 3, 8, 64, 700};
    const int shapes[][2] = {{1, 1}, {8, 64}, {16, 16}, {6, 16}, {64, 256}, {32, 256}, {5, 13}};
    for (long long b : budgets)
        for (long long k : ks)
            for (long long maxc : cs)
                for (long long nq : nqs)
                    for (long long np : nps)
                        for (const auto& s : shapes) one(nq, np, maxc, k, s[0], s[1], b, true);
}

static void by_hand() {
    // 3 queries, 8 lists of 3001 rows in all, k = 10, 64 KiB of tables, 1 MiB: 3011 * 8 bytes of keys per query; what is
    // left of the budget beside three queries' keys holds 14 table sets: 24 pairs in ranges of 14 and 10
    CHECK(pq_slice_queries(3, 3001, 10, 64, 256, 1ll << 20) == 3);
    CHECK(pq_res_pairs_per_launch(3, 3001, 10, 64, 256, 1ll << 20) == 14 && pq_res_launches(3, 8, 3001, 10, 64, 256, 1ll << 20) == 2);
    CHECK(pq_res_launches(5, 8, 3001, 10, 64, 256, 1ll << 20) == 3);
    // the default budget and small tables: the grid's second dimension is the limit
    CHECK(pq_res_pairs_per_launch(32, 156250, 100, 8, 16, kIvfKeyBudget) == kPqMaxPairsPerLaunch);
    CHECK(pq_res_pairs_per_launch(32, 156250, 100, 8, 256, kIvfKeyBudget) == (kIvfKeyBudget - 32 * 156350ll * 8) / 8192);
    CHECK(pq_res_launches(70000, 1, 10, 1, 1, 1, kIvfKeyBudget) == 2 && pq_res_launches(65535, 1, 10, 1, 1, 1, kIvfKeyBudget) == 1);
    CHECK(pq_res_launches(600, 3, 12000, 100, 16, 16, kIvfKeyBudget) == 1 && pq_res_launches(0, 3, 10, 1, 1, 1, kIvfKeyBudget) == 0);
    // 2^32 - 1 candidates: 64-bit throughout
    CHECK(pq_res_pairs_per_launch(1, kIvfMaxRows, 1, 64, 256, kIvfKeyBudget) == 1 && pq_res_launches(2, 3, kIvfMaxRows, 1, 64, 256, kIvfKeyBudget) == 6);
    const long long off[] = {0, 0, 5, 5, 8105, 8105, 12000};
    CHECK(pq_longest_list(off, 6) == 8100 && pq_longest_list(off, 1) == 0 && pq_longest_list(off, 3) == 5 && pq_longest_list(off, 0) == 0);
    CHECK(pq_residual_blocks_max() * 256 > 0 && pq_residual_blocks_max() <= 0x7fffffffll);
}

int main() {
    by_hand();
    sweep();
    printf("pq residual plan ok: lines=%lld max_pairs=%lld\n", g_lines, kPqMaxPairsPerLaunch);
    return 0;
}
