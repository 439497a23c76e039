// IVF-PQ: inverted lists whose rows are product-quantiser codes (gfx950).
//
// What FaissNearestNeighborsIndex reaches through the factory string "IVFx,PQy" (smqtk_indexing/impls/nn_index/faiss.py:
// 190-192, :385), stated against the oracle in include/smqtk_hip_pq.h: a row belongs to the list of its nearest centroid
// and is stored as m bytes, byte j the nearest entry of codebook j to the row's j-th sub-vector; a query's distance to a
// row is the root of the sum of m table entries T[j][code[j]], T[j][c] = |codebooks[j][c] - q_j|^2.
//
// Everything that must be exact is a call of the certified dense index (sq_dense_search, k = 1: over the centroids and
// over the m codebooks; k = nprobe for the probe) or of sq_ivf_kmeans (training).  The grouping of rows by list, the
// prefix of the probed lists' sizes and the select's post-op are IVF-Flat's (sq_ivf_group.hpp).  New device code is the
// coded storage, pq_tables_kernel and pq_scan_kernel; the host arithmetic is sq_pq_plan.hpp.
//
// Residual mode (sq_pq_create_residual) is the same handle with `residual` set: a row is coded as x - centroids[l(x)]
// (pq_residual_kernel, also behind sq_pq_residuals), a query gets one table set per probed list (pq_tables_res_kernel)
// and pq_scan_res_kernel walks one (query, probed list) pair's rows per workgroup.  Both scans share pq_stage_tables and
// pq_row_sum; a handle made by sq_pq_create takes none of the residual branches.
#include <algorithm>
#include <chrono>
#include <vector>

#include "../../include/smqtk_hip_pq.h"
#include "sq_ivf_group.hpp"
#include "sq_pq_plan.hpp"

namespace sq {

typedef u32 u32x4 __attribute__((ext_vector_type(4)));

struct PqHandle : HandleBase {
    int d = 0, nlist = 0, m = 0, ksub = 0, dsub = 0;
    long long cs = 0, es = 0;            // bytes of a coded row; floats of a codebook entry in `books`
    long long n = 0, id_base = 0;
    sq_handle_t coarse = 0;              // dense index over the centroids: assignment and probing
    std::vector<sq_handle_t> sub;        // dense index over codebook j: the code of a sub-vector
    DevBuf books;                        // [m][ksub][es] float32, zero padded: what the tables kernel reads
    DevBuf codes, ids, list_off;         // [n][cs] bytes list-major, [n] insertion numbers, [nlist + 1]
    std::vector<long long> off_host;     // list_off on the host
    long long add_us = 0;
    // residual mode (sq_pq_create_residual): rows are coded as x - centroids[l(x)], tables are per (query, probed list)
    bool residual = false;
    long long cds = 0;                   // floats of a centroid in `cent`
    DevBuf cent;                         // [nlist][cds] float32, zero padded: what the residual and residual-tables kernels read
    // scratch of a search
    DevBuf q_dev, probe_dist, probe_idx, pre, cnt, tables, keys, out_keys, out_dist, out_idx, sort_tmp;
    HostPinned totals_host;              // [candidates in total, longest candidate list]
    PinnedStage stage;
    ~PqHandle() override {
        if (coarse) (void)sq_dense_destroy(coarse);
        for (sq_handle_t s : sub)
            if (s) (void)sq_dense_destroy(s);
    }
};

// ------------------------------------------------------------------ add
// code byte j of the rows of an add, in insertion order: the entry the codebook's dense index answered
static __global__ __launch_bounds__(256) void pq_pack_kernel(const long long* __restrict__ entry, long long n, int ksub, int j, long long cs,
                                                              unsigned char* __restrict__ codes) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    long long c = entry[i];
    c = c < 0 ? 0 : (c >= ksub ? ksub - 1 : c);
    codes[i * cs + j] = (unsigned char)c;
}
// Both scatters move a coded row as `w` dwords, one lane per dword.
// old row s of list l -> new_off[l] + (s - old_off[l])
static __global__ __launch_bounds__(256) void pq_scatter_old_kernel(const u32* __restrict__ old_codes, const u32* __restrict__ old_ids,
                                                                     const long long* __restrict__ old_off,
                                                                     const long long* __restrict__ new_off, int nlist, long long n_old,
                                                                     int w, u32* __restrict__ new_codes, u32* __restrict__ new_ids) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_old * w) return;
    const long long s = t / w;
    const int c = (int)(t - s * w);
    const int l = ivf_locate(old_off, nlist, s);
    const long long dst = new_off[l] + (s - old_off[l]);
    new_codes[dst * w + c] = old_codes[s * w + c];
    if (c == 0) new_ids[dst] = old_ids[s];
}
// the t-th new row in (list, insertion) order -> add_at[l] + (t - add_pre[l])
static __global__ __launch_bounds__(256) void pq_scatter_new_kernel(const u32* __restrict__ src, const u64* __restrict__ sorted,
                                                                     long long n_add, const long long* __restrict__ add_at,
                                                                     const long long* __restrict__ add_pre, long long n_old, int w,
                                                                     u32* __restrict__ new_codes, u32* __restrict__ new_ids) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= n_add * w) return;
    const long long t = g / w;
    const int c = (int)(g - t * w);
    const u64 key = sorted[t];
    const long long l = (long long)(key >> 32), i = (long long)(key & 0xffffffffull);
    const long long dst = add_at[l] + (t - add_pre[l]);
    new_codes[dst * w + c] = src[i * w + c];
    if (c == 0) new_ids[dst] = (u32)(n_old + i);
}

// Residual mode: out[i][c] = x[i][c] - cent[assign[i]][c], one element per lane and trip.  x and out (row stride d) may
// be the same buffer; cent has row stride cds.
static __global__ __launch_bounds__(256) void pq_residual_kernel(const float* x, long long n, int d, const float* __restrict__ cent,
                                                                  long long cds, const long long* __restrict__ assign, int nlist, float* out) {
    const long long total = n * d;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const long long i = t / d;
        const int c = (int)(t - i * d);
        long long l = assign[i];
        l = l < 0 ? 0 : (l >= nlist ? nlist - 1 : l);
        out[t] = __fsub_rn(x[t], cent[l * cds + c]);
    }
}
static int pq_residual_launch(const float* x, long long n, int d, const float* cent, long long cds, const long long* assign, int nlist,
                              float* out, hipStream_t st) {
    const long long blocks = std::min<long long>((n * d + 255) / 256, pq_residual_blocks_max());
    return launch<pq_residual_kernel>(dim3((unsigned)blocks), dim3(256), 0, st, x, n, d, cent, cds, assign, nlist, out);
}

// One counting sort: assign, code, group, scatter old and new codes into new buffers, swap.  Nothing of the handle
// changes before the swap, so a failed allocation leaves the index as it was.
static int pq_add_part(PqHandle* h, const float* rows, long long n_add, int mem) {
    hipStream_t st = nullptr;
    const int d = h->d, nlist = h->nlist, m = h->m, dsub = h->dsub, w = (int)(h->cs / 4);
    const long long cs = h->cs, n_old = h->n, n_new = n_old + n_add;
    const float* src = rows;
    DevBuf up;
    if (mem != SQ_MEM_DEVICE) {
        SQ_TRY(ivf_alloc(up, (size_t)n_add * d * 4));
        SQ_HIP(hipMemcpy(up.p, rows, (size_t)n_add * d * 4, hipMemcpyHostToDevice));
        src = up.as<float>();
    }
    DevBuf assign, adist, entry, part, fresh;
    SQ_TRY(assign.reserve((size_t)n_add * 8));
    SQ_TRY(adist.reserve((size_t)n_add * 4));
    SQ_TRY(ivf_assign(h->coarse, src, n_add, d, assign.as<long long>(), adist.as<float>(), st));
    DevBuf resid;
    if (h->residual) {   // what is coded is the row's residual against its list's centroid
        SQ_TRY(ivf_alloc(resid, (size_t)n_add * d * 4));
        SQ_TRY(pq_residual_launch(src, n_add, d, h->cent.as<float>(), h->cds, assign.as<long long>(), nlist, resid.as<float>(), st));
        src = resid.as<float>();
    }
    // the codes in insertion order: sub-vector j of every new row as a contiguous matrix (a 2-D copy), its nearest entry
    SQ_TRY(entry.reserve((size_t)n_add * 8));
    SQ_TRY(ivf_alloc(fresh, (size_t)n_add * cs));
    SQ_HIP(hipMemsetAsync(fresh.p, 0, (size_t)n_add * cs, st));
    if (m > 1) SQ_TRY(part.reserve((size_t)n_add * dsub * 4));
    for (int j = 0; j < m; ++j) {
        const float* xj = src;
        if (m > 1) {
            SQ_HIP(hipMemcpy2DAsync(part.p, (size_t)dsub * 4, src + (size_t)j * dsub, (size_t)d * 4, (size_t)dsub * 4, (size_t)n_add,
                                    hipMemcpyDeviceToDevice, st));
            xj = part.as<float>();
        }
        SQ_TRY(ivf_assign(h->sub[(size_t)j], xj, n_add, dsub, entry.as<long long>(), adist.as<float>(), st));
        SQ_TRY(launch<pq_pack_kernel>(dim3((unsigned)((n_add + 255) / 256)), dim3(256), 0, st, entry.as<long long>(), n_add, h->ksub, j, cs,
                                      fresh.as<unsigned char>()));
    }
    SQ_HIP(hipStreamSynchronize(st));
    up.release();
    resid.release();
    part.release();
    entry.release();
    IvfGroup g;
    SQ_TRY(ivf_group(assign.as<long long>(), n_add, nlist, g, st));
    assign.release();
    adist.release();
    g.keys.release();
    g.scratch.release();
    std::vector<long long> add_cnt((size_t)nlist), plan((size_t)3 * nlist + 1);
    for (int l = 0; l < nlist; ++l) add_cnt[(size_t)l] = g.bounds_host[(size_t)l + 1] - g.bounds_host[(size_t)l];
    long long* new_off = plan.data();
    long long* add_at = new_off + nlist + 1;
    long long* add_pre = add_at + nlist;
    if (ivf_merge_offsets(h->off_host.data(), add_cnt.data(), nlist, new_off, add_at, add_pre) != n_new)
        return fail(SQ_ERR_INTERNAL, "sq_pq_add: the counting sort's offsets do not add up");
    DevBuf ncodes, nids, noff, where;
    SQ_TRY(ivf_alloc(ncodes, (size_t)n_new * cs));
    SQ_TRY(ivf_alloc(nids, (size_t)n_new * 4));
    SQ_TRY(ivf_alloc(noff, (size_t)(nlist + 1) * 8));
    SQ_TRY(where.reserve((size_t)2 * nlist * 8));
    SQ_HIP(hipMemcpy(noff.p, new_off, (size_t)(nlist + 1) * 8, hipMemcpyHostToDevice));
    SQ_HIP(hipMemcpy(where.p, add_at, (size_t)2 * nlist * 8, hipMemcpyHostToDevice));
    if (n_old > 0)
        SQ_TRY(launch<pq_scatter_old_kernel>(dim3((unsigned)((n_old * w + 255) / 256)), dim3(256), 0, st, h->codes.as<u32>(), h->ids.as<u32>(),
                                             h->list_off.as<long long>(), noff.as<long long>(), nlist, n_old, w, ncodes.as<u32>(),
                                             nids.as<u32>()));
    SQ_TRY(launch<pq_scatter_new_kernel>(dim3((unsigned)((n_add * w + 255) / 256)), dim3(256), 0, st, fresh.as<u32>(), g.sorted.as<u64>(), n_add,
                                         where.as<long long>(), where.as<long long>() + nlist, n_old, w, ncodes.as<u32>(), nids.as<u32>()));
    SQ_HIP(hipStreamSynchronize(st));
    h->codes = std::move(ncodes);
    h->ids = std::move(nids);
    h->list_off = std::move(noff);
    h->off_host.assign(new_off, new_off + nlist + 1);
    h->n = n_new;
    return SQ_OK;
}

// ------------------------------------------------------------------ search
// The tables of a slice's queries.  Work item (j, query): lane c computes T[j][c] = |codebooks[j][c] - q_j|^2 as the dense
// exact path computes a squared distance (numpy's eight accumulators per leaf, its pairwise tree), the entry read from the
// padded copy `books` ([m][ksub][es]), the query's sub-vector from LDS.  Dynamic LDS: es floats.
static __global__ __launch_bounds__(256) void pq_tables_kernel(const float* __restrict__ books, long long es, int dsub, int ksub, int m,
                                                                const float* __restrict__ queries, int d, float* __restrict__ tables) {
    extern __shared__ __attribute__((aligned(16))) float s_q[];
    const int j = blockIdx.x, ql = blockIdx.y;
    for (int i = threadIdx.x; i < es; i += 256) s_q[i] = i < dsub ? queries[(long long)ql * d + (long long)j * dsub + i] : 0.f;
    __syncthreads();
    const int c = threadIdx.x;
    if (c >= ksub) return;
    const SqLeafLane w{books + ((long long)j * ksub + c) * es, s_q};
    tables[((long long)ql * m + j) * ksub + c] = w.sum(dsub);
}

// What both scans share.  Staging: a pair's or a query's tn table floats into LDS, 16 bytes at a time when tn allows.
__device__ __forceinline__ void pq_stage_tables(float* s_t, const float* __restrict__ tq, int tn) {
    if ((tn & 3) == 0) {
        for (int i = threadIdx.x * 4; i < tn; i += 1024) *reinterpret_cast<f32x4*>(s_t + i) = *reinterpret_cast<const f32x4*>(tq + i);
    } else {
        for (int i = threadIdx.x; i < tn; i += 256) s_t[i] = tq[i];
    }
}
// A row's sum: its code dwords (V16: 16 bytes at a time), m lookups in the staged tables, added from left to right.
template <bool V16>
__device__ __forceinline__ float pq_row_sum(const u32* __restrict__ row, int w, int m, int ksub, const float* s_t) {
    float acc = 0.f;
    if constexpr (V16) {
        for (int c = 0; c < w; c += 4) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(row + c);
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                const int j = c * 4 + b;
                if (j < m) {
                    const float t = s_t[j * ksub + (int)((v[b >> 2] >> (8 * (b & 3))) & 255u)];
                    acc = j == 0 ? t : __fadd_rn(acc, t);
                }
            }
        }
    } else {
        for (int c = 0; c < w; ++c) {
            const u32 v = row[c];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int j = c * 4 + b;
                if (j < m) {
                    const float t = s_t[j * ksub + (int)((v >> (8 * b)) & 255u)];
                    acc = j == 0 ? t : __fadd_rn(acc, t);
                }
            }
        }
    }
    return acc;
}

// The scan.  Workgroup (blockIdx.x, query) stages the query's tables once -- m * ksub floats of dynamic LDS -- and walks
// the chunks blockIdx.x, blockIdx.x + gridDim.x, ... of 256 candidates of the query's concatenated range, one candidate
// per lane.  A lane finds its list in the query's prefix array and reads its row's code dwords (V16: 16 bytes at a time;
// neighbouring lanes read neighbouring rows of a list's contiguous block), looks up m table entries and adds them from
// left to right.  No barrier inside the loop.
template <bool V16>
static __global__ __launch_bounds__(256) void pq_scan_kernel(const u32* __restrict__ codes, int w, int m, int ksub,
                                                              const u32* __restrict__ ids, const long long* __restrict__ list_off,
                                                              const float* __restrict__ tables, int q0,
                                                              const long long* __restrict__ probe, const long long* __restrict__ pre,
                                                              int np, long long key_stride, u64* __restrict__ keys, int stage_only) {
    extern __shared__ __attribute__((aligned(16))) float s_t[];
    const int ql = blockIdx.y, q = q0 + ql;
    const long long* pq = pre + (long long)q * (np + 1);
    const long long total = pq[np];
    if ((long long)blockIdx.x * kIvfChunk >= total) return;
    const int tn = m * ksub;
    pq_stage_tables(s_t, tables + (long long)ql * tn, tn);
    __syncthreads();
    if (stage_only) {   // measurement (option "profile" = 2): what staging alone costs; one store per lane keeps the staging alive
        const long long p = (long long)blockIdx.x * kIvfChunk + threadIdx.x;
        if (p < total) keys[(long long)ql * key_stride + p] = (u64)__float_as_uint(s_t[(int)threadIdx.x % tn]);
        return;
    }
    for (long long base = (long long)blockIdx.x * kIvfChunk; base < total; base += (long long)gridDim.x * kIvfChunk) {
        const long long p = base + threadIdx.x;
        if (p >= total) break;
        const int jl = ivf_locate(pq, np, p);
        const long long l = probe[(long long)q * np + jl];
        const long long s = list_off[l] + (p - pq[jl]);
        const float dist = sqrt_rn_f32(pq_row_sum<V16>(codes + s * w, w, m, ksub, s_t));
        keys[(long long)ql * key_stride + p] = ((u64)ordered_f32(dist) << 32) | (u64)ids[s];
    }
}

// ------------------------------------------------------------------ search, residual mode
// A pair is (query of the slice, probe position), numbered row-major: pair p is query q0 + p / np at position p % np.
// A launch takes the pairs p0 .. p0 + gridDim.y - 1 of the slice; its tables are [pair of the launch][m][ksub].
struct PqPair {
    int ql, jl;          // query inside the slice, probe position
    long long lo, len;   // the pair's list: first row, rows (0: nothing to do)
};
__device__ __forceinline__ PqPair pq_pair(long long p, int q0, int np, const long long* __restrict__ probe,
                                          const long long* __restrict__ list_off, int nlist, long long* list = nullptr) {
    PqPair r;
    r.ql = (int)(p / np);
    r.jl = (int)(p - (long long)r.ql * np);
    const long long l = probe[(long long)(q0 + r.ql) * np + r.jl];
    const bool ok = l >= 0 && l < nlist;
    r.lo = ok ? list_off[l] : 0;
    r.len = ok ? list_off[l + 1] - r.lo : 0;
    if (list) *list = l;
    return r;
}

// The tables of a launch's pairs.  Work item (j, pair): the workgroup stages rq_j = q_j - cent[l]_j in LDS (es floats,
// zero behind dsub), then lane c sums T_l[j][c] = |codebooks[j][c] - rq_j|^2 as pq_tables_kernel does.  A pair whose
// list is empty is skipped: no scan workgroup reads its tables.
static __global__ __launch_bounds__(256) void pq_tables_res_kernel(const float* __restrict__ books, long long es, int dsub, int ksub, int m,
                                                                    const float* __restrict__ queries, int d, const float* __restrict__ cent,
                                                                    long long cds, int q0, long long p0, int np,
                                                                    const long long* __restrict__ probe,
                                                                    const long long* __restrict__ list_off, int nlist,
                                                                    float* __restrict__ tables) {
    extern __shared__ __attribute__((aligned(16))) float s_q[];
    const int j = blockIdx.x;
    long long l = 0;
    const PqPair pr = pq_pair(p0 + blockIdx.y, q0, np, probe, list_off, nlist, &l);
    if (pr.len <= 0) return;
    const float* qv = queries + (long long)(q0 + pr.ql) * d + (long long)j * dsub;
    const float* cv = cent + l * cds + (long long)j * dsub;
    for (int i = threadIdx.x; i < es; i += 256) s_q[i] = i < dsub ? __fsub_rn(qv[i], cv[i]) : 0.f;
    __syncthreads();
    const int c = threadIdx.x;
    if (c >= ksub) return;
    const SqLeafLane w{books + ((long long)j * ksub + c) * es, s_q};
    tables[((long long)blockIdx.y * m + j) * ksub + c] = w.sum(dsub);
}

// The scan.  Workgroup (blockIdx.x, pair) stages its pair's tables and walks the chunks blockIdx.x, blockIdx.x +
// gridDim.x, ... of 256 rows of the pair's list, one row per lane; row i of the list at probe position jl writes its key
// at candidate position pre[jl] + i of its query, where the select expects it.  No search for the list, no barrier in
// the loop; a workgroup whose first chunk lies beyond its list returns before staging.
template <bool V16>
static __global__ __launch_bounds__(256) void pq_scan_res_kernel(const u32* __restrict__ codes, int w, int m, int ksub,
                                                                  const u32* __restrict__ ids, const long long* __restrict__ list_off, int nlist,
                                                                  const float* __restrict__ tables, int q0, long long p0,
                                                                  const long long* __restrict__ probe, const long long* __restrict__ pre,
                                                                  int np, long long key_stride, u64* __restrict__ keys) {
    extern __shared__ __attribute__((aligned(16))) float s_t[];
    const PqPair pr = pq_pair(p0 + blockIdx.y, q0, np, probe, list_off, nlist);
    if ((long long)blockIdx.x * kIvfChunk >= pr.len) return;
    const int tn = m * ksub;
    pq_stage_tables(s_t, tables + (long long)blockIdx.y * tn, tn);
    __syncthreads();
    u64* out = keys + (long long)pr.ql * key_stride + pre[(long long)(q0 + pr.ql) * (np + 1) + pr.jl];
    for (long long base = (long long)blockIdx.x * kIvfChunk; base < pr.len; base += (long long)gridDim.x * kIvfChunk) {
        const long long i = base + threadIdx.x;
        if (i >= pr.len) break;
        const long long s = pr.lo + i;
        const float dist = sqrt_rn_f32(pq_row_sum<V16>(codes + s * w, w, m, ksub, s_t));
        out[i] = ((u64)ordered_f32(dist) << 32) | (u64)ids[s];
    }
}

// The scan of a slice in residual mode: its ns * np pairs in ranges of `ppl`, each range one tables launch and one scan
// launch into the slice's keys.
static int pq_scan_residual(PqHandle* h, const float* q_dev, int q0, int ns, int np, long long ppl, long long mc, hipStream_t st) {
    const int m = h->m, ksub = h->ksub, w = (int)(h->cs / 4);
    const bool prof = h->opt.profile != 0;
    const size_t tb = (size_t)pq_table_bytes(m, ksub);
    const long long pairs = (long long)ns * np, lmax = pq_longest_list(h->off_host.data(), h->nlist);
    for (long long p0 = 0; p0 < pairs; p0 += ppl) {
        const long long pl = pairs - p0 < ppl ? pairs - p0 : ppl;
        if (prof) SQ_HIP(hipEventRecord(h->ev[0], st));
        SQ_TRY(launch<pq_tables_res_kernel>(dim3((unsigned)m, (unsigned)pl), dim3(256), (size_t)h->es * 4, st, h->books.as<float>(), h->es,
                                            h->dsub, ksub, m, q_dev, h->d, h->cent.as<float>(), h->cds, q0, p0, np,
                                            h->probe_idx.as<long long>(), h->list_off.as<long long>(), h->nlist, h->tables.as<float>()));
        if (prof) SQ_HIP(hipEventRecord(h->ev[1], st));
        const dim3 grid((unsigned)pq_scan_groups(ivf_chunks(lmax), pl, cu_count(h->device)), (unsigned)pl);
        const int lds_max = (int)pq_table_bytes(kPqMaxM, kPqMaxKsub);
        if (w % 4 == 0)
            SQ_TRY(launch_lds<pq_scan_res_kernel<true>>(lds_max, grid, dim3(256), tb, st, h->codes.as<u32>(), w, m, ksub, h->ids.as<u32>(),
                                                        h->list_off.as<long long>(), h->nlist, h->tables.as<float>(), q0, p0,
                                                        h->probe_idx.as<long long>(), h->pre.as<long long>(), np, mc, h->keys.as<u64>()));
        else
            SQ_TRY(launch_lds<pq_scan_res_kernel<false>>(lds_max, grid, dim3(256), tb, st, h->codes.as<u32>(), w, m, ksub, h->ids.as<u32>(),
                                                         h->list_off.as<long long>(), h->nlist, h->tables.as<float>(), q0, p0,
                                                         h->probe_idx.as<long long>(), h->pre.as<long long>(), np, mc, h->keys.as<u64>()));
        if (prof) {
            SQ_HIP(hipEventRecord(h->ev[2], st));
            SQ_HIP(hipEventSynchronize(h->ev[2]));
            float ms = 0.f;
            SQ_HIP(hipEventElapsedTime(&ms, h->ev[1], h->ev[2]));
            h->stats.scan_ms += ms;
            SQ_HIP(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
            h->stats.rerank_ms += ms;
        }
        h->stats.scan_launches++;
    }
    return SQ_OK;
}

// The search with queries and outputs in device memory, enqueued on `st`; the last select is not waited for.
static int pq_search_device(PqHandle* h, const float* q_dev, int nq, int k, int nprobe, float* od, long long* oi, hipStream_t st) {
    const int d = h->d, nlist = h->nlist, m = h->m, ksub = h->ksub, np = nprobe < nlist ? nprobe : nlist, w = (int)(h->cs / 4);
    const bool prof = h->opt.profile != 0;
    SQ_TRY(h->probe_dist.reserve((size_t)nq * np * 4));
    SQ_TRY(h->probe_idx.reserve((size_t)nq * np * 8));
    SQ_TRY(sq_dense_search(h->coarse, q_dev, nq, np, h->probe_dist.p, h->probe_idx.as<int64_t>(), SQ_MEM_DEVICE, st));
    SQ_TRY(h->pre.reserve((size_t)nq * (np + 1) * 8));
    SQ_TRY(h->cnt.reserve((size_t)nq * 4));
    SQ_TRY(h->totals_host.reserve(16));
    void* th_dev = nullptr;
    SQ_TRY(h->totals_host.device_ptr(&th_dev));
    SQ_TRY(launch<ivf_probe_sizes_kernel>(dim3(nq), dim3(256), 0, st, h->probe_idx.as<long long>(), np, h->list_off.as<long long>(), nlist,
                                          h->pre.as<long long>(), h->cnt.as<u32>()));
    SQ_TRY(launch<ivf_totals_kernel>(dim3(1), dim3(256), 0, st, h->pre.as<long long>(), np, nq, static_cast<long long*>(th_dev)));
    SQ_HIP(stream_wait(st));
    const long long* th = reinterpret_cast<const long long*>(h->totals_host.p);
    const long long total = th[0], maxc = th[1];
    if (maxc > h->n) return fail(SQ_ERR_INTERNAL, "sq_pq_search: a query has more candidates than the index has rows");
    const long long mc = maxc > 0 ? maxc : 1;
    const int k_sel = (int)ivf_select_k(maxc, k);
    const long long budget = h->opt.ivf_key_budget_mb > 0 ? (long long)h->opt.ivf_key_budget_mb << 20 : kIvfKeyBudget;
    const int slice = (int)pq_slice_queries(nq, maxc, k, m, ksub, budget);
    const size_t tb = (size_t)pq_table_bytes(m, ksub);
    SQ_TRY(h->keys.reserve((size_t)slice * mc * 8));
    SQ_TRY(h->out_keys.reserve((size_t)slice * k_sel * 8));
    // residual mode: one table set per (query, probed list); the slice's pairs go in ranges of `ppl` that the budget holds
    const long long ppl = h->residual ? std::min<long long>(pq_res_pairs_per_launch(slice, maxc, k, m, ksub, budget), (long long)slice * np) : 0;
    if (maxc > 0) SQ_TRY(h->tables.reserve((size_t)(h->residual ? ppl : slice) * tb));
    if (prof)
        for (int i = 0; i < 3; ++i)
            if (!h->ev[i]) SQ_HIP(hipEventCreate(&h->ev[i]));
    for (int q0 = 0; q0 < nq; q0 += slice) {
        const int ns = nq - q0 < slice ? nq - q0 : slice;
        if (maxc > 0 && h->residual) {
            SQ_TRY(pq_scan_residual(h, q_dev, q0, ns, np, ppl, mc, st));
        } else if (maxc > 0) {
            // option "profile": 1 = scan_ms is pq_scan_kernel, rerank_ms is pq_tables_kernel; 2 = scan_ms is a launch of
            // pq_scan_kernel that only stages the tables (the real scan follows it, untimed)
            const int prof_mode = h->opt.profile;
            if (prof) SQ_HIP(hipEventRecord(h->ev[0], st));
            SQ_TRY(launch<pq_tables_kernel>(dim3((unsigned)m, (unsigned)ns), dim3(256), (size_t)h->es * 4, st, h->books.as<float>(), h->es,
                                            h->dsub, ksub, m, q_dev + (size_t)q0 * d, d, h->tables.as<float>()));
            if (prof) SQ_HIP(hipEventRecord(h->ev[1], st));
            const dim3 grid((unsigned)pq_scan_groups(ivf_chunks(maxc), ns, cu_count(h->device)), (unsigned)ns);
            auto scan = [&](int stage_only) {
                const int lds_max = (int)pq_table_bytes(kPqMaxM, kPqMaxKsub);
                if (w % 4 == 0)
                    return launch_lds<pq_scan_kernel<true>>(lds_max, grid, dim3(256), tb, st, h->codes.as<u32>(), w, m, ksub, h->ids.as<u32>(),
                                                            h->list_off.as<long long>(), h->tables.as<float>(), q0, h->probe_idx.as<long long>(),
                                                            h->pre.as<long long>(), np, mc, h->keys.as<u64>(), stage_only);
                return launch_lds<pq_scan_kernel<false>>(lds_max, grid, dim3(256), tb, st, h->codes.as<u32>(), w, m, ksub, h->ids.as<u32>(),
                                                         h->list_off.as<long long>(), h->tables.as<float>(), q0, h->probe_idx.as<long long>(),
                                                         h->pre.as<long long>(), np, mc, h->keys.as<u64>(), stage_only);
            };
            SQ_TRY(scan(prof_mode == 2 ? 1 : 0));
            if (prof) {
                SQ_HIP(hipEventRecord(h->ev[2], st));
                SQ_HIP(hipEventSynchronize(h->ev[2]));
                float ms = 0.f;
                SQ_HIP(hipEventElapsedTime(&ms, h->ev[1], h->ev[2]));
                h->stats.scan_ms += ms;
                SQ_HIP(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
                h->stats.rerank_ms += ms;
            }
            if (prof_mode == 2) SQ_TRY(scan(0));
            h->stats.scan_launches++;
        }
        const IvfFinalize fin{q0, k, h->id_base, od, oi};
        SQ_TRY(select_launch_t<u64>(h->keys.as<u64>(), h->cnt.as<u32>() + q0, (u32)mc, mc, k_sel, ns, h->out_keys.as<u64>(), fin, st, h->sort_tmp));
    }
    h->stats.candidates = total;
    h->stats.bytes_scanned = total * h->cs;
    return SQ_OK;
}

static int pq_shape_check(const char* who, int d, int m, int ksub) {
    switch (pq_shape_error(d, m, ksub)) {
    case 1: return fail(SQ_ERR_INVALID, "%s: d = %d is no multiple of m = %d", who, d, m);
    case 2: return fail(SQ_ERR_INVALID, "%s: m = %d is outside 1 .. %d", who, m, kPqMaxM);
    case 3: return fail(SQ_ERR_INVALID, "%s: ksub = %d is outside 1 .. %d", who, ksub, kPqMaxKsub);
    case 4: return fail(SQ_ERR_UNSUPPORTED, "%s: sub-vectors of d / m = %d floats, more than %d", who, d / m, kPqMaxDsub);
    default: return SQ_OK;
    }
}

}  // namespace sq

using namespace sq;

extern "C" int sq_pq_train(const float* x, int64_t n, int d, int m, int ksub, float* codebooks, int iters, int mem) {
    if (!x || !codebooks || n <= 0 || d <= 0 || iters < 0) return fail(SQ_ERR_INVALID, "sq_pq_train: bad argument");
    SQ_TRY(pq_shape_check("sq_pq_train", d, m, ksub));
    if (n < ksub) return fail(SQ_ERR_INVALID, "sq_pq_train: %lld rows cannot train %d entries", (long long)n, ksub);
    if (n > kIvfGroupMax) return fail(SQ_ERR_UNSUPPORTED, "sq_pq_train: more than 2^26 training rows (train on a sample)");
    if (mem != SQ_MEM_HOST && mem != SQ_MEM_DEVICE) return fail(SQ_ERR_UNSUPPORTED, "sq_pq_train: host or device memory only");
    const int dsub = d / m;
    const size_t cb = (size_t)ksub * dsub * 4;
    const hipMemcpyKind in = mem == SQ_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const hipMemcpyKind back = mem == SQ_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    DevBuf part, book;
    SQ_TRY(ivf_alloc(part, (size_t)n * dsub * 4));
    SQ_TRY(ivf_alloc(book, cb));
    for (int j = 0; j < m; ++j) {
        // the strided gather x[:, j dsub : (j + 1) dsub] is a 2-D copy
        SQ_HIP(hipMemcpy2D(part.p, (size_t)dsub * 4, x + (size_t)j * dsub, (size_t)d * 4, (size_t)dsub * 4, (size_t)n, in));
        SQ_HIP(hipMemcpy(book.p, codebooks + (size_t)j * ksub * dsub, cb, in));
        SQ_TRY(sq_ivf_kmeans(part.as<float>(), n, dsub, book.as<float>(), ksub, iters, SQ_MEM_DEVICE));
        SQ_HIP(hipMemcpy(codebooks + (size_t)j * ksub * dsub, book.p, cb, back));
    }
    return SQ_OK;
}

// [nlist][round_up(d, 4)] float32 on the device, zero padded, from centroids in host memory
static int pq_upload_centroids(const float* centroids, int nlist, int d, DevBuf& cent, long long* cds) {
    *cds = ivf_row_stride(d);
    const size_t bytes = (size_t)nlist * *cds * 4;
    SQ_TRY(ivf_alloc(cent, bytes));
    SQ_HIP(hipMemset(cent.p, 0, bytes));
    SQ_HIP(hipMemcpy2D(cent.p, (size_t)*cds * 4, centroids, (size_t)d * 4, (size_t)d * 4, (size_t)nlist, hipMemcpyHostToDevice));
    return SQ_OK;
}

static int pq_create(const char* who, bool residual, const float* centroids, int nlist, int d, const float* codebooks, int m, int ksub,
                     int64_t id_base, sq_handle_t* out) {
    if (!centroids || !codebooks || !out || nlist <= 0 || d <= 0) return fail(SQ_ERR_INVALID, "%s: bad argument", who);
    SQ_TRY(pq_shape_check(who, d, m, ksub));
    if (nlist > kIvfMaxLists) return fail(SQ_ERR_UNSUPPORTED, "%s: more than %d lists", who, kIvfMaxLists);
    auto h = std::make_unique<PqHandle>();
    h->residual = residual;
    h->kind = H_PQ;
    h->d = d;
    h->nlist = nlist;
    h->m = m;
    h->ksub = ksub;
    h->dsub = d / m;
    h->cs = pq_code_stride(m);
    h->es = pq_entry_stride(h->dsub);
    h->id_base = id_base;
    h->refresh_options();
    if (hipGetDevice(&h->device) != hipSuccess) return fail(SQ_ERR_HIP, "%s: no HIP device", who);
    SQ_TRY(ivf_coarse_create(centroids, nlist, d, SQ_MEM_HOST, &h->coarse));
    if (residual) SQ_TRY(pq_upload_centroids(centroids, nlist, d, h->cent, &h->cds));
    h->sub.assign((size_t)m, 0);
    for (int j = 0; j < m; ++j)
        SQ_TRY(ivf_coarse_create(codebooks + (size_t)j * ksub * h->dsub, ksub, h->dsub, SQ_MEM_HOST, &h->sub[(size_t)j]));
    // the padded copy the tables kernel reads: entry stride es floats
    const size_t entries = (size_t)m * ksub;
    SQ_TRY(ivf_alloc(h->books, entries * h->es * 4));
    SQ_HIP(hipMemset(h->books.p, 0, entries * h->es * 4));
    SQ_HIP(hipMemcpy2D(h->books.p, (size_t)h->es * 4, codebooks, (size_t)h->dsub * 4, (size_t)h->dsub * 4, entries, hipMemcpyHostToDevice));
    h->off_host.assign((size_t)nlist + 1, 0);
    SQ_TRY(ivf_alloc(h->list_off, (size_t)(nlist + 1) * 8));
    SQ_HIP(hipMemset(h->list_off.p, 0, (size_t)(nlist + 1) * 8));
    *out = register_handle(h.release());
    return SQ_OK;
}

extern "C" int sq_pq_create(const float* centroids, int nlist, int d, const float* codebooks, int m, int ksub, int64_t id_base,
                            sq_handle_t* out) {
    return pq_create("sq_pq_create", false, centroids, nlist, d, codebooks, m, ksub, id_base, out);
}

extern "C" int sq_pq_create_residual(const float* centroids, int nlist, int d, const float* codebooks, int m, int ksub, int64_t id_base,
                                     sq_handle_t* out) {
    return pq_create("sq_pq_create_residual", true, centroids, nlist, d, codebooks, m, ksub, id_base, out);
}

extern "C" int sq_pq_residuals(const float* x, int64_t n, int d, const float* centroids, int nlist, float* out, int mem) {
    if (!x || !centroids || !out || n <= 0 || d <= 0 || nlist <= 0) return fail(SQ_ERR_INVALID, "sq_pq_residuals: bad argument");
    if (nlist > kIvfMaxLists) return fail(SQ_ERR_UNSUPPORTED, "sq_pq_residuals: more than %d lists", kIvfMaxLists);
    if (n > kIvfGroupMax) return fail(SQ_ERR_UNSUPPORTED, "sq_pq_residuals: more than 2^26 rows (train on a sample)");
    if (mem != SQ_MEM_HOST && mem != SQ_MEM_DEVICE) return fail(SQ_ERR_UNSUPPORTED, "sq_pq_residuals: host or device memory only");
    struct Coarse {
        sq_handle_t h = 0;
        ~Coarse() {
            if (h) (void)sq_dense_destroy(h);
        }
    } coarse;
    SQ_TRY(ivf_coarse_create(centroids, nlist, d, SQ_MEM_HOST, &coarse.h));
    hipStream_t st = nullptr;
    DevBuf cent, up, assign, adist;
    long long cds = 0;
    SQ_TRY(pq_upload_centroids(centroids, nlist, d, cent, &cds));
    const float* src = x;
    float* dst = out;
    if (mem == SQ_MEM_HOST) {   // the rows go up, are replaced by their residuals in place, and come back
        SQ_TRY(ivf_alloc(up, (size_t)n * d * 4));
        SQ_HIP(hipMemcpy(up.p, x, (size_t)n * d * 4, hipMemcpyHostToDevice));
        src = dst = up.as<float>();
    }
    SQ_TRY(assign.reserve((size_t)n * 8));
    SQ_TRY(adist.reserve((size_t)n * 4));
    SQ_TRY(ivf_assign(coarse.h, src, n, d, assign.as<long long>(), adist.as<float>(), st));
    SQ_TRY(pq_residual_launch(src, n, d, cent.as<float>(), cds, assign.as<long long>(), nlist, dst, st));
    SQ_HIP(hipStreamSynchronize(st));
    if (mem == SQ_MEM_HOST) SQ_HIP(hipMemcpy(out, up.p, (size_t)n * d * 4, hipMemcpyDeviceToHost));
    return SQ_OK;
}

extern "C" int sq_pq_add(sq_handle_t hid, const float* rows, int64_t n_add, int mem) {
    auto* h = static_cast<PqHandle*>(lookup_handle(hid, H_PQ));
    if (!h) return fail(SQ_ERR_INVALID, "sq_pq_add: unknown handle");
    if (!rows || n_add <= 0) return fail(SQ_ERR_INVALID, "sq_pq_add: bad argument");
    if (mem != SQ_MEM_HOST && mem != SQ_MEM_DEVICE) return fail(SQ_ERR_UNSUPPORTED, "sq_pq_add: rows in host or device memory only");
    std::lock_guard<std::mutex> lock(h->mu);
    h->refresh_options();
    if (!ivf_rows_ok(h->n + n_add)) return fail(SQ_ERR_UNSUPPORTED, "sq_pq_add: more than 2^32-1 rows");
    SQ_HIP(hipSetDevice(h->device));
    const auto t0 = std::chrono::steady_clock::now();
    // (an add beyond 2^26 rows is several counting sorts; each leaves a complete index)
    for (long long s = 0; s < n_add; s += kIvfGroupMax)
        SQ_TRY(pq_add_part(h, rows + s * h->d, std::min<long long>(kIvfGroupMax, n_add - s), mem));
    h->add_us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    return SQ_OK;
}

extern "C" int sq_pq_lists(sq_handle_t hid, int64_t* list_off, int64_t* ids, uint8_t* codes) {
    auto* h = static_cast<PqHandle*>(lookup_handle(hid, H_PQ));
    if (!h) return fail(SQ_ERR_INVALID, "sq_pq_lists: unknown handle");
    std::lock_guard<std::mutex> lock(h->mu);
    SQ_HIP(hipSetDevice(h->device));
    if (list_off)
        for (int l = 0; l <= h->nlist; ++l) list_off[l] = h->off_host[(size_t)l];
    if (ids && h->n > 0) {
        std::vector<u32> tmp((size_t)h->n);
        SQ_HIP(hipMemcpy(tmp.data(), h->ids.p, (size_t)h->n * 4, hipMemcpyDeviceToHost));
        for (long long i = 0; i < h->n; ++i) ids[i] = h->id_base + (int64_t)tmp[(size_t)i];
    }
    if (codes && h->n > 0)   // (the 2-D copy drops the padding of a row)
        SQ_HIP(hipMemcpy2D(codes, (size_t)h->m, h->codes.p, (size_t)h->cs, (size_t)h->m, (size_t)h->n, hipMemcpyDeviceToHost));
    return SQ_OK;
}

extern "C" int sq_pq_info(sq_handle_t hid, int64_t* out, int n_out) {
    auto* h = static_cast<PqHandle*>(lookup_handle(hid, H_PQ));
    if (!h) return fail(SQ_ERR_INVALID, "sq_pq_info: unknown handle");
    if (!out || n_out < SQ_PQ_INFO_FIELDS) return fail(SQ_ERR_INVALID, "sq_pq_info: room for %d values needed", SQ_PQ_INFO_FIELDS);
    std::lock_guard<std::mutex> lock(h->mu);
    h->refresh_options();
    int64_t fixed = (int64_t)h->books.cap + (h->residual ? (int64_t)h->cent.cap : 0);
    std::vector<sq_handle_t> dense(h->sub);
    dense.push_back(h->coarse);
    for (sq_handle_t s : dense) {
        int64_t ci[SQ_DENSE_INFO_FIELDS] = {0};
        SQ_TRY(sq_dense_info(s, ci, SQ_DENSE_INFO_FIELDS));
        fixed += ci[2] + ci[4] + ci[5] + ci[6];
    }
    out[0] = h->n;
    out[1] = h->d;
    out[2] = h->nlist;
    out[3] = h->m;
    out[4] = h->ksub;
    out[5] = h->n > 0 ? (int64_t)h->codes.cap : 0;                          // the codes, list-major
    out[6] = (int64_t)((h->n > 0 ? h->ids.cap : 0) + h->list_off.cap);     // insertion numbers and list offsets
    out[7] = fixed;                                                        // codebooks (as m dense indexes and the padded copy) and the coarse index
    out[8] = h->add_us;
    out[9] = h->opt.ivf_key_budget_mb > 0 ? (int64_t)h->opt.ivf_key_budget_mb << 20 : kIvfKeyBudget;
    return SQ_OK;
}

extern "C" int sq_pq_search(sq_handle_t hid, const float* queries, int nq, int k, int nprobe, float* out_dist, int64_t* out_idx, int mem,
                            void* stream) {
    // (the mode is refused first: whatever the handle)
    if (mem != SQ_MEM_HOST && mem != SQ_MEM_DEVICE)
        return fail(SQ_ERR_UNSUPPORTED, "sq_pq_search: blocking calls only (SQ_MEM_HOST or SQ_MEM_DEVICE), not mode %d", mem);
    auto* h = static_cast<PqHandle*>(lookup_handle(hid, H_PQ));
    if (!h) return fail(SQ_ERR_INVALID, "sq_pq_search: unknown handle");
    if (!queries || !out_dist || !out_idx || nq <= 0 || k <= 0 || nprobe < 1) return fail(SQ_ERR_INVALID, "sq_pq_search: bad argument");
    std::lock_guard<std::mutex> lock(h->mu);
    h->refresh_options();
    SQ_HIP(hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const auto t_call = std::chrono::steady_clock::now();
    h->stats = sq_stats_t{};
    if (mem == SQ_MEM_HOST) {
        SQ_TRY(staged_call(h->stage, st, {{h->q_dev, queries, (size_t)nq * h->d * 4}},
                           {{out_dist, h->out_dist, (size_t)nq * k * 4}, {out_idx, h->out_idx, (size_t)nq * k * 8}}, [&] {
                               return pq_search_device(h, h->q_dev.as<float>(), nq, k, nprobe, h->out_dist.as<float>(),
                                                       h->out_idx.as<long long>(), st);
                           }));
    } else {
        SQ_TRY(pq_search_device(h, queries, nq, k, nprobe, out_dist, reinterpret_cast<long long*>(out_idx), st));
        SQ_HIP(stream_wait(st));
    }
    if (h->opt.profile != 0) h->stats.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
    return SQ_OK;
}

extern "C" int sq_pq_destroy(sq_handle_t hid) {
    auto* h = remove_handle(hid, H_PQ);
    if (!h) return fail(SQ_ERR_INVALID, "sq_pq_destroy: unknown handle");
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    delete h;
    return SQ_OK;
}
