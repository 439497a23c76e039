// The host's arithmetic around the IVF-PQ index (sq_pq.hip): which (d, m, ksub) an index takes, the stride of a coded
// row, the LDS a scan workgroup stages a query's tables in, how many workgroups walk one query's candidates, and how
// many queries of a batch share the scratch once the tables are counted; for residual mode, how many (query, probed
// list) pairs one launch takes and how many launches a search makes.  Everything in 64-bit.  Plain C++ on top of
// sq_ivf_plan.hpp, no runtime header: tests/host/pq_plan_main.cpp and pq_residual_plan_main.cpp run it on the CPU.
#pragma once
#include "sq_ivf_plan.hpp"

namespace sq {

static constexpr int kPqMaxM = 64;               // sub-quantisers: a query's tables are at most 64 * 256 * 4 = 64 KiB of LDS
static constexpr int kPqMaxKsub = 256;           // entries per codebook: a code is one byte
static constexpr int kPqMaxDsub = 16384;          // floats of a sub-vector: pq_tables_kernel stages one in round_up(dsub, 4) * 4 <= 64 KiB of LDS
static constexpr int kPqChunksPerGroup = 16;     // chunks of 256 candidates a scan workgroup walks per staging of the tables, at least
static constexpr int kPqGroupsPerCu = 2;         // ... unless the call would leave the device idle: then this many workgroups per CU

// 0: the shape is taken; 1: d is no multiple of m; 2: m out of range; 3: ksub out of range; 4: d / m beyond kPqMaxDsub
inline int pq_shape_error(long long d, long long m, long long ksub) {
    if (m < 1 || m > kPqMaxM) return 2;
    if (ksub < 1 || ksub > kPqMaxKsub) return 3;
    if (d < 1 || d % m != 0) return 1;
    if (d / m > kPqMaxDsub) return 4;
    return 0;
}

// Bytes of a coded row: its m code bytes, padded with zeros to whole dwords.  A lane reads its row as m / 4 dwords
// (16-byte loads when the stride is a multiple of 16), neighbouring lanes read neighbouring rows.
inline long long pq_code_stride(int m) { return ((long long)m + 3) / 4 * 4; }
inline long long pq_codes_bytes(long long n, int m) { return n * pq_code_stride(m); }
// floats per codebook entry as the tables kernel reads it: whole 16-byte pieces, zero padded (ivf_row_stride's rule)
inline long long pq_entry_stride(int dsub) { return ivf_row_stride(dsub); }

// a query's distance tables: [m][ksub] float32, in global memory per query of a slice and in a scan workgroup's LDS
inline long long pq_table_bytes(int m, int ksub) { return (long long)m * ksub * 4; }

// Workgroups that share one query's chunks (the scan grid's first dimension).  A workgroup stages the tables once and
// walks chunks g, g + groups, ...: with kPqChunksPerGroup chunks each the table bytes are 1/4 of the code bytes at
// ksub = 256.  A call too small to fill the device that way is spread over kPqGroupsPerCu workgroups per CU instead.
inline long long pq_scan_groups(long long chunks, long long nq, long long cus) {
    if (chunks < 1) return 1;
    const long long want = (chunks + kPqChunksPerGroup - 1) / kPqChunksPerGroup;
    const long long fill = nq > 0 ? (kPqGroupsPerCu * cus + nq - 1) / nq : 1;
    const long long g = want > fill ? want : fill;
    return g < chunks ? (g > 0 ? g : 1) : chunks;
}

// scratch bytes one query of a slice takes: IVF-Flat's keys, selected keys and sort buffers, and its tables
inline long long pq_query_scratch_bytes(long long maxc, long long k, int m, int ksub) {
    return ivf_query_scratch_bytes(maxc, k) + pq_table_bytes(m, ksub);
}
// queries per slice: as many as the budget holds, one at least
inline long long pq_slice_queries(long long nq, long long maxc, long long k, int m, int ksub, long long budget_bytes) {
    long long s = budget_bytes / pq_query_scratch_bytes(maxc, k, m, ksub);
    if (s < 1) s = 1;
    return s < nq ? s : nq;
}

// ---- residual mode: one table set per pair (query of the slice, probe position), so np times the tables per query.
// The queries per slice are pq_slice_queries' -- each query's keys and ONE pair's tables --; what the budget has left
// beside the slice's keys holds the tables of `pairs per launch` pairs, and a slice's ns * np pairs are taken in ranges
// of that many, row-major in (query, position): a range is one tables launch and one scan launch.
static constexpr long long kPqMaxPairsPerLaunch = 65535;   // the scan grid's second dimension

inline long long pq_res_pairs_per_launch(long long slice, long long maxc, long long k, int m, int ksub, long long budget_bytes) {
    long long p = (budget_bytes - slice * ivf_query_scratch_bytes(maxc, k)) / pq_table_bytes(m, ksub);
    if (p < 1) p = 1;
    return p < kPqMaxPairsPerLaunch ? p : kPqMaxPairsPerLaunch;
}
// scratch bytes of a residual search: the slice's keys and the tables of the pairs of one launch
inline long long pq_res_scratch_bytes(long long slice, long long ppl, long long maxc, long long k, int m, int ksub) {
    return slice * ivf_query_scratch_bytes(maxc, k) + ppl * pq_table_bytes(m, ksub);
}
// launches (ranges) of a residual search of nq queries at np probed lists each: what scan_launches counts
inline long long pq_res_launches(long long nq, long long np, long long maxc, long long k, int m, int ksub, long long budget_bytes) {
    if (maxc < 1 || nq < 1 || np < 1) return 0;
    const long long slice = pq_slice_queries(nq, maxc, k, m, ksub, budget_bytes);
    long long ppl = pq_res_pairs_per_launch(slice, maxc, k, m, ksub, budget_bytes);
    if (ppl > slice * np) ppl = slice * np;
    const long long full = nq / slice, rest = nq % slice;   // whole slices, and the queries of a last shorter one
    return full * ((slice * np + ppl - 1) / ppl) + (rest * np + ppl - 1) / ppl;
}
// rows of the longest list: the chunks a pair's scan workgroups share (pq_scan_groups with a pair in a query's place)
inline long long pq_longest_list(const long long* list_off, int nlist) {
    long long mx = 0;
    for (int l = 0; l < nlist; ++l) {
        const long long len = list_off[l + 1] - list_off[l];
        mx = len > mx ? len : mx;
    }
    return mx;
}
// workgroups of pq_residual_kernel at most: it strides over the elements beyond that
inline long long pq_residual_blocks_max() { return 1ll << 20; }

}  // namespace sq
