// IVF-PQ, packed mode (sq_pq_create_packed): ksub <= 16 entries per codebook, two codes per byte (gfx950).
//
// Included by sq_pq.hip behind PqPair / pq_pair.  The arithmetic is the one-byte index's (include/smqtk_hip_pq.h); what
// differs is the storage -- byte b of a row holds code[2b] in its low nibble and code[2b + 1] in its high nibble, the
// row is w = ceil(m / 8) dwords -- and, following from 16 entries, where the tables live during the scan:
//
//   pq4_tables_kernel  [unit][m][ksub] tables for codebooks of at most 16 entries: a workgroup takes one unit (a query of
//                      the slice, or a (query, probed list) pair) and 16 sub-quantisers, 16 lanes each, where
//                      pq_tables_kernel would leave 240 of its 256 lanes idle.  The same SqLeafLane sum, the same bits.
//   pq4_scan_kernel    a sub-quantiser's table is 16 lanes of ONE register, so a wave keeps its unit's m tables in m
//                      VGPRs and a lookup is a cross-lane read (ds_bpermute_b32: the LDS crossbar, no LDS memory, no bank
//                      conflict of random table addresses).  No LDS allocation, no barrier.
//
// The active-lane rule of the scan: ds_bpermute_b32 returns garbage from a lane that is switched off, so every lane of a
// wave stays active through every lookup of every trip.  A lane behind the end of its list (or of its query's
// candidates) computes on the last valid row and only skips the store; no lane leaves the loop on its own.
#pragma once
#include "sq_pq_plan.hpp"

namespace sq {

// ------------------------------------------------------------------ tables
// What a tables launch works on.  Plain mode: unit u is query q0 + u of `queries`.  Residual mode: unit u is pair p0 + u,
// its sub-vectors are q_j - cent[l]_j; a pair whose list is empty is skipped.
struct Pq4Tables {
    const float* books;      // [m][ksub][es]
    long long es;
    int dsub, ksub, m, d;
    const float* queries;
    const float* cent;       // residual mode: [nlist][cds]
    long long cds;
    int q0;
    long long p0;
    int np;
    const long long* probe;
    const long long* list_off;
    int nlist;
    float* tables;           // [unit][m][ksub]
};

// Workgroup (block of 16 sub-quantisers, unit).  Lane t belongs to sub-quantiser j = 16 blockIdx.x + t / 16 and entry
// c = t % 16: the 16 lanes of a sub-quantiser stage its sub-vector (es floats, zero behind dsub) and then each sums its
// entry as pq_tables_kernel does.  Dynamic LDS: 16 * es floats.
template <bool RES>
static __global__ __launch_bounds__(256) void pq4_tables_kernel(const Pq4Tables a) {
    extern __shared__ __attribute__((aligned(16))) float s_q[];
    const int jj = threadIdx.x >> 4, c = threadIdx.x & 15;
    const int j = blockIdx.x * kPqSmallBlock + jj;
    long long ql = blockIdx.y, l = 0;
    if constexpr (RES) {
        const PqPair pr = pq_pair(a.p0 + blockIdx.y, a.q0, a.np, a.probe, a.list_off, a.nlist, &l);
        if (pr.len <= 0) return;
        ql = pr.ql;
    }
    float* sq = s_q + (long long)jj * a.es;
    if (j < a.m) {
        const float* qv = a.queries + (long long)(a.q0 + ql) * a.d + (long long)j * a.dsub;
        if constexpr (RES) {
            const float* cv = a.cent + l * a.cds + (long long)j * a.dsub;
            for (int i = c; i < a.es; i += 16) sq[i] = i < a.dsub ? __fsub_rn(qv[i], cv[i]) : 0.f;
        } else {
            for (int i = c; i < a.es; i += 16) sq[i] = i < a.dsub ? qv[i] : 0.f;
        }
    }
    __syncthreads();
    if (j >= a.m || c >= a.ksub) return;
    const SqLeafLane w{a.books + ((long long)j * a.ksub + c) * a.es, sq};
    a.tables[((long long)blockIdx.y * a.m + j) * a.ksub + c] = w.sum(a.dsub);
}

static int pq4_tables_launch(bool residual, const Pq4Tables& a, long long units, hipStream_t st) {
    const dim3 grid((unsigned)pq_small_tables_blocks(a.m), (unsigned)units);
    const size_t lds = (size_t)pq_small_tables_lds(a.es);
    if (residual) return launch<pq4_tables_kernel<true>>(grid, dim3(256), lds, st, a);
    return launch<pq4_tables_kernel<false>>(grid, dim3(256), lds, st, a);
}

// ------------------------------------------------------------------ scan
struct Pq4Scan {
    const u32* codes;        // [rows][w] dwords, list-major
    int m, ksub;
    const u32* ids;
    const long long* list_off;
    int nlist;
    const float* tables;     // [unit of the launch][m][ksub]
    int q0;
    long long p0;            // residual mode: first pair of the launch
    const long long* probe;
    const long long* pre;
    int np;
    long long key_stride;
    u64* keys;
};

// A row's W dwords: 16 bytes at a time for W = 4 and 8.
template <int W>
__device__ __forceinline__ void pq4_load_row(const u32* __restrict__ row, u32 (&v)[W]) {
    if constexpr (W % 4 == 0) {
#pragma unroll
        for (int c = 0; c < W; c += 4) {
            const u32x4 x = *reinterpret_cast<const u32x4*>(row + c);
            v[c] = x[0], v[c + 1] = x[1], v[c + 2] = x[2], v[c + 3] = x[3];
        }
    } else {
#pragma unroll
        for (int c = 0; c < W; ++c) v[c] = row[c];
    }
}

// Workgroup (blockIdx.x, unit) walks the chunks blockIdx.x, blockIdx.x + gridDim.x, ... of 256 rows of its unit: in plain
// mode the unit is a query of the slice and a row is a candidate of its concatenated range (pq_scan_kernel's grid and key
// places), in residual mode the unit is a pair and a row is a row of the pair's list (pq_scan_res_kernel's).  W = ceil(m / 8)
// is the row's dwords.  Each wave first loads its unit's tables: register j of lane L holds T[j][min(L & 15, ksub - 1)],
// one dword load per sub-quantiser.  Per row a lane takes nibble j of its dwords for j = 0 .. m-1 in order, fetches the
// entry from the lane that holds it and adds from left to right.  `j < m` is uniform: a padded nibble is never added.
// See the active-lane rule at the top: `live` guards the store and nothing else.
template <int W, bool RES>
static __global__ __launch_bounds__(256) void pq4_scan_kernel(const Pq4Scan a) {
    const int lane = (int)(threadIdx.x & 63u);
    const long long* pq = nullptr;
    long long lo = 0, len;
    int q = 0;
    u64* out;
    if constexpr (RES) {
        const PqPair pr = pq_pair(a.p0 + blockIdx.y, a.q0, a.np, a.probe, a.list_off, a.nlist);
        lo = pr.lo;
        len = pr.len;
        out = a.keys + (long long)pr.ql * a.key_stride + a.pre[(long long)(a.q0 + pr.ql) * (a.np + 1) + pr.jl];
    } else {
        q = a.q0 + (int)blockIdx.y;
        pq = a.pre + (long long)q * (a.np + 1);
        len = pq[a.np];
        out = a.keys + (long long)blockIdx.y * a.key_stride;
    }
    if ((long long)blockIdx.x * kIvfChunk >= len) return;   // the whole workgroup: no lookup is left behind
    const float* tq = a.tables + (long long)blockIdx.y * a.m * a.ksub;
    const int c = (lane & 15) < a.ksub ? (lane & 15) : a.ksub - 1;
    float T[8 * W];
#pragma unroll
    for (int j = 0; j < 8 * W; ++j) T[j] = (j < 8 * (W - 1) || j < a.m) ? tq[j * a.ksub + c] : 0.f;
    // a lookup reads the copy in the reader's own group of 16 lanes, (lane & 48) | code (lanes 0 .. 15 measured the same: DESIGN.md 4.12)
    const u32 group = (u32)(lane & 48) << 2;   // byte address of that group's first lane
    for (long long base = (long long)blockIdx.x * kIvfChunk; base < len; base += (long long)gridDim.x * kIvfChunk) {
        const long long i = base + threadIdx.x;
        const bool live = i < len;
        const long long ic = live ? i : len - 1;   // a lane behind the end stays active on the last valid row
        long long s;
        if constexpr (RES) {
            s = lo + ic;
        } else {
            const int jl = ivf_locate(pq, a.np, ic);
            s = a.list_off[a.probe[(long long)q * a.np + jl]] + (ic - pq[jl]);
        }
        u32 v[W];
        pq4_load_row<W>(a.codes + s * W, v);
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < 8 * W; ++j) {
            if (j < 8 * (W - 1) || j < a.m) {
                const u32 nib = (v[j >> 3] >> (4 * (j & 7))) & 15u;
                const float t = __int_as_float(__builtin_amdgcn_ds_bpermute((int)(group | (nib << 2)), __float_as_int(T[j])));
                acc = j == 0 ? t : __fadd_rn(acc, t);
            }
        }
        const float dist = sqrt_rn_f32(acc);
        if (live) out[i] = ((u64)ordered_f32(dist) << 32) | (u64)a.ids[s];
    }
}

template <bool RES>
static int pq4_scan_launch_w(int w, dim3 grid, hipStream_t st, const Pq4Scan& a) {
    switch (w) {
    case 1: return launch<pq4_scan_kernel<1, RES>>(grid, dim3(256), 0, st, a);
    case 2: return launch<pq4_scan_kernel<2, RES>>(grid, dim3(256), 0, st, a);
    case 3: return launch<pq4_scan_kernel<3, RES>>(grid, dim3(256), 0, st, a);
    case 4: return launch<pq4_scan_kernel<4, RES>>(grid, dim3(256), 0, st, a);
    case 5: return launch<pq4_scan_kernel<5, RES>>(grid, dim3(256), 0, st, a);
    case 6: return launch<pq4_scan_kernel<6, RES>>(grid, dim3(256), 0, st, a);
    case 7: return launch<pq4_scan_kernel<7, RES>>(grid, dim3(256), 0, st, a);
    case 8: return launch<pq4_scan_kernel<8, RES>>(grid, dim3(256), 0, st, a);
    default: return fail(SQ_ERR_INTERNAL, "packed scan: a row of %d dwords", w);
    }
}
static int pq4_scan_launch(bool residual, int w, dim3 grid, hipStream_t st, const Pq4Scan& a) {
    return residual ? pq4_scan_launch_w<true>(w, grid, st, a) : pq4_scan_launch_w<false>(w, grid, st, a);
}

}  // namespace sq
