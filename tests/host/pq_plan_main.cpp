// The host arithmetic of the IVF-PQ index (smqtk_indexing_amd/csrc/sq_pq_plan.hpp) on a CPU: compiled with
// -fsanitize=address,undefined and run by tests/test_host_logic_pq.py.  Checked here: which shapes an index takes; the
// code stride as the scan reads it (whole dwords, every byte of a row inside its stride, rows packed back to back); the
// LDS bytes of a query's tables at m = 1 and m = 64; the workgroups per query covering every chunk once; the slice sizes
// with the tables counted; the 64-bit products at 2^32 - 1 rows.
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

static void shapes() {
    CHECK(pq_shape_error(128, 8, 256) == 0 && pq_shape_error(128, 32, 256) == 0 && pq_shape_error(12, 12, 1) == 0);
    CHECK(pq_shape_error(516, 4, 64) == 0 && pq_shape_error(1, 1, 1) == 0 && pq_shape_error(64, 64, 256) == 0);
    CHECK(pq_shape_error(128, 7, 256) == 1 && pq_shape_error(10, 4, 16) == 1);
    CHECK(pq_shape_error(128, 0, 256) == 2 && pq_shape_error(128, -1, 256) == 2 && pq_shape_error(130, 65, 256) == 2);
    CHECK(pq_shape_error(16384, 1, 256) == 0 && pq_shape_error(16385, 1, 256) == 4 && pq_shape_error(64ll * 16384, 64, 1) == 0);
    CHECK(pq_shape_error(64ll * 16385, 64, 1) == 4 && pq_entry_stride(kPqMaxDsub) * 4 == 65536);
    CHECK(pq_shape_error(128, 8, 0) == 3 && pq_shape_error(128, 8, 257) == 3 && pq_shape_error(128, 8, -5) == 3);
}

// the scan reads row s as stride / 4 dwords from byte s * stride and takes byte j of the row for j < m: every such
// byte lies inside the row's own stride, and the bytes of n rows are exactly the buffer
static void stride() {
    for (int m = 1; m <= kPqMaxM; ++m) {
        const long long cs = pq_code_stride(m);
        CHECK(cs % 4 == 0 && cs >= m && cs - m < 4);
        std::vector<unsigned char> buf((size_t)pq_codes_bytes(5, m), 0);
        CHECK((long long)buf.size() == 5 * cs);
        for (long long s = 0; s < 5; ++s)
            for (long long w = 0; w < cs / 4; ++w)
                for (int b = 0; b < 4; ++b) {
                    const long long j = w * 4 + b;
                    if (j < m) buf[(size_t)(s * cs + w * 4 + b)]++;   // (under AddressSanitizer: inside the buffer)
                }
        for (long long s = 0; s < 5; ++s)
            for (long long j = 0; j < cs; ++j) CHECK(buf[(size_t)(s * cs + j)] == (j < m ? 1 : 0));
    }
    CHECK(pq_code_stride(8) == 8 && pq_code_stride(32) == 32 && pq_code_stride(12) == 12 && pq_code_stride(1) == 4 && pq_code_stride(63) == 64);
    CHECK(pq_entry_stride(1) == 4 && pq_entry_stride(4) == 4 && pq_entry_stride(129) == 132 && pq_entry_stride(16) == 16);
}

static void lds() {
    CHECK(pq_table_bytes(1, 1) == 4 && pq_table_bytes(1, 256) == 1024 && pq_table_bytes(64, 256) == 65536);
    CHECK(pq_table_bytes(kPqMaxM, kPqMaxKsub) <= 64 * 1024);     // what a plain launch takes
    CHECK(pq_table_bytes(32, 256) == 32768 && pq_table_bytes(12, 3) == 144);
}

// workgroup g of `groups` walks chunks g, g + groups, ...: every chunk once, no workgroup without one
static void groups() {
    const long long cus[] = {1, 64, 256, 304};
    const long long nqs[] = {1, 2, 32, 33, 70, 4096, 70000};
    const long long chunks[] = {1, 2, 15, 16, 17, 255, 611, 4096, 16777216};
    for (long long cu : cus)
        for (long long nq : nqs)
            for (long long ch : chunks) {
                const long long g = pq_scan_groups(ch, nq, cu);
                CHECK(g >= 1 && g <= ch);
                // a workgroup stages the tables once per kPqChunksPerGroup chunks at least, unless the call is spread to fill the device
                const long long per = (ch + g - 1) / g;
                CHECK(per >= 1 && (per <= kPqChunksPerGroup || g * nq >= kPqGroupsPerCu * cu || g == ch));
                CHECK(g == ch || g * kPqChunksPerGroup >= ch);
                if (ch <= 4096) {
                    std::vector<int> hit((size_t)ch, 0);
                    for (long long w = 0; w < g; ++w)
                        for (long long c = w; c < ch; c += g) hit[(size_t)c]++;
                    for (int v : hit) CHECK(v == 1);
                }
            }
    CHECK(pq_scan_groups(0, 1, 256) == 1 && pq_scan_groups(611, 1, 256) == 512 && pq_scan_groups(611, 32, 256) == 39);
    CHECK(pq_scan_groups(4096, 70000, 256) == 256);
}

static void slices() {
    const long long budget = kIvfKeyBudget;
    const long long ks[] = {1, 100, 16384, 16385, 30000};
    const long long cs[] = {0, 1, 255, 3001, 156250, 10000000, 4294967295ll};
    const long long nqs[] = {1, 32, 33, 70, 100000};
    const int ms[] = {1, 8, 32, 64};
    const int ksubs[] = {1, 3, 256};
    for (long long k : ks)
        for (long long maxc : cs)
            for (long long nq : nqs)
                for (int m : ms)
                    for (int ksub : ksubs) {
                        const long long per = pq_query_scratch_bytes(maxc, k, m, ksub), s = pq_slice_queries(nq, maxc, k, m, ksub, budget);
                        CHECK(per == ivf_query_scratch_bytes(maxc, k) + (long long)m * ksub * 4);
                        CHECK(s >= 1 && s <= nq && s <= ivf_slice_queries(nq, maxc, k, budget));   // the tables count
                        CHECK(s * per <= budget || s == 1);
                        CHECK(s == nq || (s + 1) * per > budget);
                    }
    // 70 queries of 3001 candidates, k = 10, m = 8, ksub = 64 under 1 MiB: (3011 * 8 + 2048) bytes each, 40 per slice
    CHECK(pq_slice_queries(70, 3001, 10, 8, 64, 1ll << 20) == 40);
    CHECK(pq_slice_queries(70, 3001, 10, 64, 256, 1ll << 20) == 11);
}

static void wide() {
    const long long n = kIvfMaxRows;   // 2^32 - 1
    CHECK(pq_codes_bytes(n, 64) == 4294967295ll * 64 && pq_codes_bytes(n, 1) == 4294967295ll * 4 && pq_codes_bytes(n, 33) == 4294967295ll * 36);
    CHECK(pq_codes_bytes(10000000, 32) + 10000000ll * 4 == 360000000ll);      // 0.36 GB at 10 M x 128, m = 32
    CHECK(pq_query_scratch_bytes(n, 1, 64, 256) == (n + 1) * 8 + 65536);
    CHECK(pq_slice_queries(1000, n, 10, 64, 256, kIvfKeyBudget) == 1);
    CHECK(pq_scan_groups(ivf_chunks(n), 1, 256) == 1048576 && pq_scan_groups(ivf_chunks(n), 1, 256) * kPqChunksPerGroup * kIvfChunk >= n);
}

// pq_scan_groups on the triples the strided-scan tests are cut for (tests/pq_cases.py restates the function in Python;
// tests/test_host_logic_pq.py compares the two line by line): "groups <chunks> <nq> <cus> <value>"
static void print_groups() {
    const long long cus[] = {1, 64, 80, 128, 256, 304};
    const long long nqs[] = {0, 1, 33, 50, 64, 70, 600, 70000};
    for (long long cu : cus)
        for (long long nq : nqs) {
            for (long long ch = 0; ch <= 64; ++ch) printf("groups %lld %lld %lld %lld\n", ch, nq, cu, pq_scan_groups(ch, nq, cu));
            printf("groups 611 %lld %lld %lld\n", nq, cu, pq_scan_groups(611, nq, cu));
            printf("groups 16777216 %lld %lld %lld\n", nq, cu, pq_scan_groups(16777216, nq, cu));
        }
}

int main() {
    shapes();
    stride();
    lds();
    groups();
    slices();
    wide();
    print_groups();
    printf("pq plan ok: max_m=%d max_ksub=%d chunks_per_group=%d lds_max=%lld\n", kPqMaxM, kPqMaxKsub, kPqChunksPerGroup,
           pq_table_bytes(kPqMaxM, kPqMaxKsub));
    return 0;
}
