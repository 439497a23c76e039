// Removal of rows from a dense index on the device, and its compaction.
//
// What it replaces: FaissNearestNeighborsIndex._remove_from_index (smqtk_indexing/impls/nn_index/faiss.py:644-694,
// remove_ids at :675) -- rows leave the resident index in place and a search afterwards costs what it cost before.
//
// Removal is data, not code, for the filters: every scan compares a row's score with its query's threshold by an
// ordered `<=`, so a row whose stored per-row term makes the score NaN (or +inf under a finite threshold) is never
// emitted -- the representation rows holding a non-finite element have had all along.  dense_remove_apply_kernel
// writes that term into every copy the handle keeps:
//   bfloat16 scan, L2      norms / norms1 (the MFMA's C operand)                    <- NaN
//   bfloat16 scan, cosine  the first 16-byte chunk of the row's scan copy            <- NaN (x^.q^ is then NaN)
//   int8 scan              N_row (sq_dense_i8.hpp; integer products: never NaN)      <- +inf, as its padding rows
//   middle tier, cosine    1/|x| and u of the row (sq_dense_mid.hpp)                 <- NaN
// (the L2 middle tier starts from `norms`).  A +inf int8 term passes a +inf threshold; that threshold admits the
// padding rows as well, so every list of the call then holds more than `cap` entries and is discarded (n > cap on
// the filter path): a removed row never reaches an answer that is kept.
// The kernels that score EVERY row from the float32 matrix (sq_dense_exact.hpp, the middle tier's sample) read the
// bitmap of removed rows this file maintains.  No kernel here writes to the float32 rows: an index that borrows the
// caller's matrix leaves the caller's memory alone.
#pragma once
#include "sq_dense_exact.hpp"

namespace sq {

// every per-row term of a handle (null: the handle keeps no such copy)
struct DenseDeadTerms {
    float* norms;         // L2 [n_pad]
    float* norms1;        // L2 [n_pad]
    float* nrow8;         // int8 row terms
    uint4* scan;          // cosine: bfloat16 copy, `scan_cpr` 16-byte chunks per row
    long long scan_cpr;
    float* mid_cos;       // cosine middle tier [2][mid_cos_ld]
    long long mid_cos_ld;
};

__device__ __forceinline__ void dense_dead_write(const DenseDeadTerms& t, long long row) {
    const float nanv = __builtin_nanf("");
    if (t.norms) t.norms[row] = nanv;
    if (t.norms1) t.norms1[row] = nanv;
    if (t.nrow8) t.nrow8[row] = __builtin_inff();
    if (t.scan) {
        const u32 w = 0x7fc07fc0u;   // two bfloat16 NaN
        t.scan[row * t.scan_cpr] = make_uint4(w, w, w, w);
    }
    if (t.mid_cos) {
        t.mid_cos[row] = nanv;
        t.mid_cos[t.mid_cos_ld + row] = nanv;
    }
}

// status word of a removal: bit 0 an id outside [id_base, id_base + n), bit 1 an id that is already removed or listed twice
static constexpr u32 DENSE_REMOVE_RANGE = 1u, DENSE_REMOVE_DEAD = 2u;

// Pass 1 of sq_dense_remove: validate each id and set its bit.  atomicOr's return value says whether the bit was
// clear: a set bit is a row removed earlier or the same id met twice in this call (the second thread to arrive sees
// the first one's bit).  `won[i]` = this thread set the bit -- what the undo pass needs to restore the bitmap exactly
// when the call is refused.  Relaxed device-scope atomics: the words are only read by later kernels.
static __global__ __launch_bounds__(256) void dense_remove_kernel(const long long* __restrict__ ids, long long m, long long id_base,
                                                                   long long n, u32* __restrict__ dead, u32* __restrict__ won,
                                                                   u32* __restrict__ status) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const long long row = ids[i] - id_base;
    u32 mine = 0u;
    if (row < 0 || row >= n) {
        atomicOr(status, DENSE_REMOVE_RANGE);
    } else {
        const u32 bit = 1u << (u32)(row & 31);
        const u32 old = atomicOr(&dead[row >> 5], bit);
        if (old & bit)
            atomicOr(status, DENSE_REMOVE_DEAD);
        else
            mine = 1u;
    }
    won[i] = mine;
}

// Pass 2, the call was refused: clear exactly the bits pass 1 set.
static __global__ __launch_bounds__(256) void dense_remove_undo_kernel(const long long* __restrict__ ids, long long m, long long id_base,
                                                                        u32* __restrict__ dead, const u32* __restrict__ won) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= m || !won[i]) return;
    const long long row = ids[i] - id_base;
    atomicAnd(&dead[row >> 5], ~(1u << (u32)(row & 31)));
}

// Pass 2, the call stands: the "never emitted" value into every per-row term of the removed rows.
static __global__ __launch_bounds__(256) void dense_remove_apply_kernel(const long long* __restrict__ ids, long long m, long long id_base,
                                                                         DenseDeadTerms t) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < m) dense_dead_write(t, ids[i] - id_base);
}

// The same for every removed row of [row_from, n): after a kernel of the build has rewritten terms (an append redoes
// the tile and the int8 unit the old rows ended in; the cosine middle tier builds its terms at first use).
static __global__ __launch_bounds__(256) void dense_dead_reapply_kernel(const u32* __restrict__ dead, long long row_from, long long n,
                                                                         DenseDeadTerms t) {
    const long long row = row_from + (long long)blockIdx.x * 256 + threadIdx.x;
    if (row < n && dense_row_dead(dead, row)) dense_dead_write(t, row);
}

// ------------------------------------------------------------------------------------------------- compaction
// new row of old row r = prefix[r >> 5] + (live rows of word r >> 5 below bit r & 31).
// dense_compact_scan_kernel: ONE workgroup of 1024 threads; thread t owns the words [t W, (t + 1) W): it counts their
// live rows (bits beyond n count as removed), the 1024 sums are scanned in LDS (Hillis-Steele, ten steps), and the
// thread walks its words again writing the exclusive prefix of each.  The bitmap is n / 8 bytes (1.25 MB at 10 M
// rows): two passes of one workgroup over it are microseconds beside the gather.  total[0] = live rows.
__device__ __forceinline__ u32 dense_live_word(const u32* __restrict__ dead, long long w, long long n) {
    u32 live = ~dead[w];
    const long long first = w << 5;
    if (first + 32 > n) live &= n > first ? (0xffffffffu >> (u32)(32 - (n - first))) : 0u;
    return live;
}

static __global__ __launch_bounds__(1024) void dense_compact_scan_kernel(const u32* __restrict__ dead, long long n, long long n_words,
                                                                          unsigned long long* __restrict__ prefix,
                                                                          unsigned long long* __restrict__ total) {
    __shared__ unsigned long long s_sum[1024];
    const long long W = (n_words + 1023) / 1024;
    const long long w0 = (long long)threadIdx.x * W, w1 = w0 + W < n_words ? w0 + W : n_words;
    unsigned long long mine = 0;
    for (long long w = w0; w < w1; ++w) mine += (unsigned long long)__popc(dense_live_word(dead, w, n));
    s_sum[threadIdx.x] = mine;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const unsigned long long add = (int)threadIdx.x >= o ? s_sum[threadIdx.x - o] : 0ull;
        __syncthreads();
        s_sum[threadIdx.x] += add;
        __syncthreads();
    }
    unsigned long long run = s_sum[threadIdx.x] - mine;   // exclusive
    for (long long w = w0; w < w1; ++w) {
        prefix[w] = run;
        run += (unsigned long long)__popc(dense_live_word(dead, w, n));
    }
    if (threadIdx.x == 1023) total[0] = s_sum[1023];
}

__device__ __forceinline__ long long dense_new_row(const u32* __restrict__ dead, const unsigned long long* __restrict__ prefix,
                                                   long long row) {
    const u32 below = ~dead[row >> 5] & ((1u << (u32)(row & 31)) - 1u);
    return (long long)prefix[row >> 5] + (long long)__popc(below);
}

// Surviving rows of [row0, row1) to their new place, 16 bytes per thread and copy (`cpr` chunks per row: the owned
// matrix has a row stride of whole 16-byte chunks).  dst row = new row - dst_row0.  Source and destination are
// DIFFERENT buffers: workgroups run in no particular order, so a row's new place may not overlap a row another
// workgroup has yet to read (sq_dense_compact gathers into a second buffer, or through a bounce buffer piece by piece).
static __global__ __launch_bounds__(256) void dense_compact_gather_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                                           long long cpr, long long row0, long long row1,
                                                                           long long dst_row0, const u32* __restrict__ dead,
                                                                           const unsigned long long* __restrict__ prefix) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long row = row0 + idx / cpr;
    if (row >= row1 || dense_row_dead(dead, row)) return;
    const long long c = idx % cpr;
    dst[(dense_new_row(dead, prefix, row) - dst_row0) * cpr + c] = src[row * cpr + c];
}

// old_to_new[i] = id_base + new row of old row i, or -1 for a removed row
static __global__ __launch_bounds__(256) void dense_compact_map_kernel(const u32* __restrict__ dead,
                                                                        const unsigned long long* __restrict__ prefix, long long n,
                                                                        long long id_base, long long* __restrict__ old_to_new) {
    const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    old_to_new[row] = dense_row_dead(dead, row) ? -1ll : id_base + dense_new_row(dead, prefix, row);
}

}  // namespace sq
