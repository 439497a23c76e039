// The host's arithmetic around the IVF-PQ index (sq_pq.hip): which (d, m, ksub) an index takes, the stride of a coded
// row, the LDS a scan workgroup stages a query's tables in, how many workgroups walk one query's candidates, and how
// many queries of a batch share the scratch once the tables are counted.  Everything in 64-bit.  Plain C++ on top of
// sq_ivf_plan.hpp, no runtime header: tests/host/pq_plan_main.cpp runs it on the CPU.
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

}  // namespace sq
