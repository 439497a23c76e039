// IVF-SQ: inverted lists whose rows are kept element by element as 8-bit codes or as float16 (gfx950).
//
// What FaissNearestNeighborsIndex reaches through the factory strings "IVFx,SQ8" and "IVFx,SQfp16"
// (smqtk_indexing/impls/nn_index/faiss.py:190-192, :385), stated against the oracle (include/smqtk_hip_isq.h): lists and
// probe are IVF-Flat's over the ORIGINAL rows, a row is stored after one rounding per element, and the distance is
// metrics.euclidean_distance over the decoded row in numpy's order -- so a search returns the bits sq_ivf_search returns
// over the decoded matrix.  The coarse index, the counting sort, the probed lists' prefix and the select's post-op are
// sq_ivf_group.hpp's, the host arithmetic sq_ivf_plan.hpp's, the tree walk sq_pairwise.hpp's.  New device code: the column
// ranges (training), the scatter of code rows, and the decoding scans -- per query here, list-major in sq_isq_shared.hpp;
// the codecs and the encoder are sq_isq_codec.hpp's, the scans' LDS sizes and their route sq_isq_plan.hpp's.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

#include "../../include/smqtk_hip_isq.h"
#include "sq_isq_codec.hpp"
#include "sq_isq_shared.hpp"   // the list-major scan; the LDS sizes and the route: sq_isq_plan.hpp
#include "sq_ivf_group.hpp"

namespace sq {

static_assert(kIsqSq8 == SQ_ISQ_SQ8 && kIsqF16 == SQ_ISQ_F16, "sq_isq_plan.hpp names the kinds of smqtk_hip_isq.h");

struct IsqHandle : HandleBase {
    int d = 0, nlist = 0, code_kind = SQ_ISQ_SQ8;
    long long ld = 0, stride = 0, n = 0, id_base = 0;   // round_up(d, 4); bytes per stored row
    sq_handle_t coarse = 0;              // dense index over the centroids: assignment and probing
    DevBuf codes, ids, list_off, params; // [n][stride] bytes list-major, [n] insertion numbers, [nlist + 1], vmin[ld] then step[ld]
    std::vector<long long> off_host;
    long long add_us = 0;
    // scratch of a search
    DevBuf q_dev, probe_dist, probe_idx, pre, cnt, keys, out_keys, out_dist, out_idx, sort_tmp;
    HostPinned totals_host;              // [candidates in total, longest candidate list, pairs the list-major scan served]
    IvfPairGroups pairs;                 // the list-major scan's groups of a slice
    PinnedStage stage;
    bool list_shape(int* d_out, long long* n_out, long long* id_base_out) const override {
        *d_out = d;
        *n_out = n;
        *id_base_out = id_base;
        return true;
    }
    ~IsqHandle() override {
        if (coarse) (void)sq_dense_destroy(coarse);
    }
};

// ------------------------------------------------------------------ training: the column ranges
// numpy's min / max: a NaN in the column makes the result NaN
__device__ __forceinline__ float isq_min(float m, float v) { return (v < m || v != v) ? v : m; }
__device__ __forceinline__ float isq_max(float m, float v) { return (v > m || v != v) ? v : m; }

// Work item (blockIdx.x, blockIdx.y): columns [64 blockIdx.x, + 64), rows blockIdx.y, + gridDim.y, ... four at a time (one
// per wave, so a wave reads 64 neighbouring floats of a row); part[blockIdx.y][0 / 1][d] = the minimum / maximum it saw.
static __global__ __launch_bounds__(256) void isq_range_part_kernel(const float* __restrict__ x, long long n, int d,
                                                                     float* __restrict__ part) {
    __shared__ float s_min[4][64], s_max[4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, col = blockIdx.x * 64 + lane;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    if (col < d)
        for (long long r = (long long)blockIdx.y * 4 + wv; r < n; r += (long long)gridDim.y * 4) {
            const float v = x[r * d + col];
            mn = isq_min(mn, v);
            mx = isq_max(mx, v);
        }
    s_min[wv][lane] = mn;
    s_max[wv][lane] = mx;
    __syncthreads();
    if (wv == 0 && col < d) {
        for (int w = 1; w < 4; ++w) {
            mn = isq_min(mn, s_min[w][lane]);
            mx = isq_max(mx, s_max[w][lane]);
        }
        part[((long long)blockIdx.y * 2 + 0) * d + col] = mn;
        part[((long long)blockIdx.y * 2 + 1) * d + col] = mx;
    }
}
static __global__ __launch_bounds__(256) void isq_range_final_kernel(const float* __restrict__ part, int parts, int d,
                                                                      float* __restrict__ vmin, float* __restrict__ step) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= d) return;
    float mn = part[col], mx = part[d + col];
    for (int p = 1; p < parts; ++p) {
        mn = isq_min(mn, part[((long long)p * 2 + 0) * d + col]);
        mx = isq_max(mx, part[((long long)p * 2 + 1) * d + col]);
    }
    vmin[col] = mn;
    step[col] = __fdiv_rn(__fsub_rn(mx, mn), 255.f);
}

// ------------------------------------------------------------------ the counting sort's scatter, in 16-byte pieces
// old row s of list l -> new_off[l] + (s - old_off[l]); eight lanes per row
static __global__ __launch_bounds__(256) void isq_scatter_old_kernel(const u32x4* __restrict__ old_codes, const u32* __restrict__ old_ids,
                                                                      const long long* __restrict__ old_off,
                                                                      const long long* __restrict__ new_off, int nlist, long long n_old,
                                                                      long long pcs /* 16-byte pieces per row */,
                                                                      u32x4* __restrict__ new_codes, u32* __restrict__ new_ids) {
    const long long s = (long long)blockIdx.x * 32 + (threadIdx.x >> 3);
    if (s >= n_old) return;
    const int j8 = threadIdx.x & 7;
    const int l = ivf_locate(old_off, nlist, s);
    const long long dst = new_off[l] + (s - old_off[l]);
    for (long long c = j8; c < pcs; c += 8) new_codes[dst * pcs + c] = old_codes[s * pcs + c];
    if (j8 == 0) new_ids[dst] = old_ids[s];
}
// the t-th new row in (list, insertion) order -> add_at[l] + (t - add_pre[l]); `enc`: the encoder's rows in the add's order
static __global__ __launch_bounds__(256) void isq_scatter_new_kernel(const u32x4* __restrict__ enc, long long pcs,
                                                                      const u64* __restrict__ sorted, long long n_add,
                                                                      const long long* __restrict__ add_at,
                                                                      const long long* __restrict__ add_pre, long long n_old,
                                                                      u32x4* __restrict__ new_codes, u32* __restrict__ new_ids) {
    const long long t = (long long)blockIdx.x * 32 + (threadIdx.x >> 3);
    if (t >= n_add) return;
    const int j8 = threadIdx.x & 7;
    const u64 key = sorted[t];
    const long long l = (long long)(key >> 32), i = (long long)(key & 0xffffffffull);
    const long long dst = add_at[l] + (t - add_pre[l]);
    for (long long c = j8; c < pcs; c += 8) new_codes[dst * pcs + c] = enc[i * pcs + c];
    if (j8 == 0) new_ids[dst] = (u32)(n_old + i);
}

static int isq_encode(const IsqHandle* h, const float* src, long long n, u32* out, hipStream_t st) {
    const long long wpr = h->stride / 4, total = n * wpr;
    const dim3 grid((unsigned)std::min<long long>((total + 255) / 256, 1ll << 20));
    const float* vmin = h->params.as<float>();
    if (h->code_kind == SQ_ISQ_SQ8) return launch<isq_encode_kernel<SQ_ISQ_SQ8>>(grid, dim3(256), 0, st, src, h->d, n, vmin, vmin + h->ld, wpr, out);
    return launch<isq_encode_kernel<SQ_ISQ_F16>>(grid, dim3(256), 0, st, src, h->d, n, vmin, vmin, wpr, out);
}

// One counting sort: assign, encode, group, scatter old and new code rows into new buffers, swap.  Nothing of the handle
// changes before the swap, so a failed allocation leaves the index as it was.
static int isq_add_part(IsqHandle* h, const float* rows, long long n_add, int mem) {
    hipStream_t st = nullptr;
    const int d = h->d, nlist = h->nlist;
    const long long pcs = h->stride / 16, n_old = h->n, n_new = n_old + n_add;
    const float* src = rows;
    DevBuf up;
    if (mem != SQ_MEM_DEVICE) {
        SQ_TRY(ivf_alloc(up, (size_t)n_add * d * 4));
        SQ_HIP(hipMemcpy(up.p, rows, (size_t)n_add * d * 4, hipMemcpyHostToDevice));
        src = up.as<float>();
    }
    DevBuf assign, enc;
    SQ_TRY(assign.reserve((size_t)n_add * 8));
    IvfAssignStats as;
    IvfAssignScratch aw;   // (ivf_group below waits for the stream)
    as.timed = h->opt.profile != 0;
    SQ_TRY(ivf_assign(h->coarse, src, n_add, d, assign.as<long long>(), st, h->opt.ivf_assign, aw, &as));
    as.into(h->stats);
    SQ_TRY(ivf_alloc(enc, (size_t)n_add * h->stride));
    SQ_TRY(isq_encode(h, src, n_add, enc.as<u32>(), st));
    IvfGroup g;
    SQ_TRY(ivf_group(assign.as<long long>(), n_add, nlist, g, st));   // (waits for the stream: the float32 rows are done with)
    up.release();
    assign.release();
    g.keys.release();
    g.scratch.release();
    std::vector<long long> add_cnt((size_t)nlist), plan((size_t)3 * nlist + 1);
    for (int l = 0; l < nlist; ++l) add_cnt[(size_t)l] = g.bounds_host[(size_t)l + 1] - g.bounds_host[(size_t)l];
    long long* new_off = plan.data();
    long long* add_at = new_off + nlist + 1;
    long long* add_pre = add_at + nlist;
    if (ivf_merge_offsets(h->off_host.data(), add_cnt.data(), nlist, new_off, add_at, add_pre) != n_new)
        return fail(SQ_ERR_INTERNAL, "sq_isq_add: the counting sort's offsets do not add up");
    DevBuf ncodes, nids, noff;
    SQ_TRY(ivf_alloc(ncodes, (size_t)n_new * h->stride));
    SQ_TRY(ivf_alloc(nids, (size_t)n_new * 4));
    SQ_TRY(ivf_alloc(noff, plan.size() * 8));
    SQ_HIP(hipMemcpy(noff.p, plan.data(), plan.size() * 8, hipMemcpyHostToDevice));
    const long long* noff_d = noff.as<long long>();
    if (n_old > 0)
        SQ_TRY(launch<isq_scatter_old_kernel>(dim3((unsigned)((n_old + 31) / 32)), dim3(256), 0, st, h->codes.as<u32x4>(), h->ids.as<u32>(),
                                              h->list_off.as<long long>(), noff_d, nlist, n_old, pcs, ncodes.as<u32x4>(), nids.as<u32>()));
    SQ_TRY(launch<isq_scatter_new_kernel>(dim3((unsigned)((n_add + 31) / 32)), dim3(256), 0, st, enc.as<u32x4>(), pcs, g.sorted.as<u64>(), n_add,
                                          noff_d + nlist + 1, noff_d + 2 * nlist + 1, n_old, ncodes.as<u32x4>(), nids.as<u32>()));
    SQ_HIP(hipStreamSynchronize(st));
    h->codes = std::move(ncodes);
    h->ids = std::move(nids);
    h->list_off = std::move(noff);   // (its first nlist + 1 words; the rest served the scatter)
    h->off_host.assign(new_off, new_off + nlist + 1);
    h->n = n_new;
    return SQ_OK;
}

// ------------------------------------------------------------------ the scan
// The leaf functor of the decoding scan: SqLeafLane's interface (term, leaf, sum) over a code row, driven by the same
// pw_tree.  One lane per row; numpy's eight interleaved accumulators are eight registers.  Leaf offsets are multiples
// of 8 elements (pw_split, PW_BUFSIZE) and a row starts on a 16-byte boundary, so SQ8 reads 8 codes per 8-byte load and
// 16 per 16-byte load where the offset is a multiple of 16, F16 8 codes per 16-byte load; no load reaches beyond
// off + n <= d, so the padding is never summed.
// LDS, SQ8: for dimensions 4g .. 4g + 3 the twelve floats q[4], vmin[4], step[4] at s[12 g] -- three adjacent 16-byte
// broadcast reads per four dimensions.  F16: the query, s[i] = q[i].
// The accumulators start at zero where numpy's start at the first eight terms: a term is a square, never -0, and
// 0 + t == t bit for bit.
template <int KIND>
struct IsqLeafLane {
    const u8* x;     // the code row
    const float* s;  // LDS
    __device__ __forceinline__ float term(int i) const {
        float xd, q;
        if constexpr (KIND == SQ_ISQ_SQ8) {
            const float* g = s + (i >> 2) * 12 + (i & 3);
            xd = isq_decode_sq8((float)x[i], g[4], g[8]);
            q = g[0];
        } else {
            xd = (float)reinterpret_cast<const _Float16*>(x)[i];
            q = s[i];
        }
        const float t = __fsub_rn(xd, q);
        return __fmul_rn(t, t);
    }
    // four codes of one dword at dimensions 4g .. 4g + 3 into accumulators r[b .. b + 3]
    __device__ __forceinline__ void add4(float (&r)[8], int b, u32 w, const f32x4* g) const {
        const f32x4 q = g[0], vm = g[1], st = g[2];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float c = (float)((w >> (8 * j)) & 0xffu);   // v_cvt_f32_ubyte{j}
            const float t = __fsub_rn(isq_decode_sq8(c, vm[j], st[j]), q[j]);
            r[b + j] = __fadd_rn(r[b + j], __fmul_rn(t, t));
        }
    }
    __device__ __forceinline__ void add8(float (&r)[8], u32 lo, u32 hi, int e) const {
        const f32x4* g = reinterpret_cast<const f32x4*>(s) + (e >> 2) * 3;
        add4(r, 0, lo, g);
        add4(r, 4, hi, g + 3);
    }
    __device__ __forceinline__ float leaf(int off, int n) const {
        if (n < 8) {
            float r = 0.f;
            for (int i = 0; i < n; ++i) r = __fadd_rn(r, term(off + i));
            return r;
        }
        float r[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const int nfull = n - (n % 8);
        int i = 0;
        if constexpr (KIND == SQ_ISQ_SQ8) {
            if (off & 8) {   // up to the next 16-byte boundary
                const u32x2 w = *reinterpret_cast<const u32x2*>(x + off);
                add8(r, w[0], w[1], off);
                i = 8;
            }
            for (; i + 16 <= nfull; i += 16) {
                const u32x4 w = *reinterpret_cast<const u32x4*>(x + off + i);
                add8(r, w[0], w[1], off + i);
                add8(r, w[2], w[3], off + i + 8);
            }
            if (i < nfull) {
                const u32x2 w = *reinterpret_cast<const u32x2*>(x + off + i);
                add8(r, w[0], w[1], off + i);
            }
        } else {
            for (; i < nfull; i += 8) {
                const f16x8 v = *reinterpret_cast<const f16x8*>(x + 2 * (off + i));
                const f32x4 q0 = *reinterpret_cast<const f32x4*>(s + off + i), q1 = *reinterpret_cast<const f32x4*>(s + off + i + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float t0 = __fsub_rn((float)v[j], q0[j]), t1 = __fsub_rn((float)v[4 + j], q1[j]);   // v_cvt_f32_f16
                    r[j] = __fadd_rn(r[j], __fmul_rn(t0, t0));
                    r[4 + j] = __fadd_rn(r[4 + j], __fmul_rn(t1, t1));
                }
            }
        }
        float res = __fadd_rn(__fadd_rn(__fadd_rn(r[0], r[1]), __fadd_rn(r[2], r[3])),
                              __fadd_rn(__fadd_rn(r[4], r[5]), __fadd_rn(r[6], r[7])));
        for (i = nfull; i < n; ++i) res = __fadd_rn(res, term(off + i));
        return res;
    }
    __device__ __forceinline__ float sum(int d) const {
        return pw_tree<float>([this](int off, int n) { return leaf(off, n); }, d);
    }
};

// Work item (blockIdx.x, query): candidates [256 blockIdx.x, + 256) of the query's concatenated range, one per lane, the
// keys written where ivf_scan_kernel writes them.  Dynamic LDS: isq_stage_bytes(d, KIND).
template <int KIND>
static __global__ __launch_bounds__(256) void isq_scan_kernel(const u8* __restrict__ codes, long long stride, int d, long long ld,
                                                               const float* __restrict__ params, const u32* __restrict__ ids,
                                                               const long long* __restrict__ list_off, const float* __restrict__ queries,
                                                               int q0, const long long* __restrict__ probe,
                                                               const long long* __restrict__ pre, int np, long long key_stride,
                                                               u64* __restrict__ keys) {
    extern __shared__ __attribute__((aligned(16))) float s_stage[];
    const int ql = blockIdx.y, q = q0 + ql;
    const long long* pq = pre + (long long)q * (np + 1);
    const long long total = pq[np];
    const long long base = (long long)blockIdx.x * kIvfChunk;
    if (base >= total) return;
    if constexpr (KIND == SQ_ISQ_SQ8) {
        for (int i = threadIdx.x; i < (int)ld; i += 256) {
            float* g = s_stage + (i >> 2) * 12 + (i & 3);
            g[0] = i < d ? queries[(long long)q * d + i] : 0.f;
            g[4] = params[i];
            g[8] = params[ld + i];
        }
    } else {
        for (int i = threadIdx.x; i < d; i += 256) s_stage[i] = queries[(long long)q * d + i];
    }
    __syncthreads();
    const long long p = base + threadIdx.x;
    if (p >= total) return;
    const int j = ivf_locate(pq, np, p);
    const long long l = probe[(long long)q * np + j];
    const long long s = list_off[l] + (p - pq[j]);
    const IsqLeafLane<KIND> w{codes + s * stride, s_stage};
    const float dist = sqrt_rn_f32(w.sum(d));
    keys[(long long)ql * key_stride + p] = ((u64)ordered_f32(dist) << 32) | (u64)ids[s];
}

// The search with queries and outputs in device memory, enqueued on `st`; the last select is not waited for.
// ivf_search_device (sq_ivf.hip) with the decoding scans: the same probe, offsets, slice rule, select and stats.  A slice
// that isq_scan_route takes (option "isq_scan") is grouped by ivf_pair_group and scanned list-major by
// isq_scan_shared_kernel (sq_isq_shared.hpp); every other slice runs isq_scan_kernel.  The keys are the same bits.
static int isq_search_device(IsqHandle* h, const float* q_dev, int nq, int k, int nprobe, float* od, long long* oi, hipStream_t st) {
    const int d = h->d, nlist = h->nlist, np = nprobe < nlist ? nprobe : nlist;
    const bool prof = h->opt.profile != 0;
    SQ_TRY(h->probe_dist.reserve((size_t)nq * np * 4));
    SQ_TRY(h->probe_idx.reserve((size_t)nq * np * 8));
    SQ_TRY(sq_dense_search(h->coarse, q_dev, nq, np, h->probe_dist.p, h->probe_idx.as<int64_t>(), SQ_MEM_DEVICE, st));
    SQ_TRY(h->pre.reserve((size_t)nq * (np + 1) * 8));
    SQ_TRY(h->cnt.reserve((size_t)nq * 4));
    SQ_TRY(h->totals_host.reserve(32));
    void* th_dev = nullptr;
    SQ_TRY(h->totals_host.device_ptr(&th_dev));
    SQ_TRY(launch<ivf_probe_sizes_kernel>(dim3(nq), dim3(256), 0, st, h->probe_idx.as<long long>(), np, h->list_off.as<long long>(), nlist,
                                          h->pre.as<long long>(), h->cnt.as<u32>()));
    SQ_TRY(launch<ivf_totals_kernel>(dim3(1), dim3(256), 0, st, h->pre.as<long long>(), np, nq, static_cast<long long*>(th_dev)));
    SQ_HIP(stream_wait(st));
    const long long* th = reinterpret_cast<const long long*>(h->totals_host.p);
    const long long total = th[0], maxc = th[1];
    long long* served = static_cast<long long*>(th_dev) + 2;   // added to by ivf_pair_groups_kernel, read by sq_isq_search after its wait
    reinterpret_cast<long long*>(h->totals_host.p)[2] = 0;
    if (maxc > kIvfMaxRows) return fail(SQ_ERR_INTERNAL, "sq_isq_search: a query has more candidates than the index has rows");
    const long long mc = maxc > 0 ? maxc : 1;
    const int k_sel = (int)ivf_select_k(maxc, k);
    const long long budget = h->opt.ivf_key_budget_mb > 0 ? (long long)h->opt.ivf_key_budget_mb << 20 : kIvfKeyBudget;
    const int slice = (int)ivf_slice_queries(nq, maxc, k, budget);
    SQ_TRY(h->keys.reserve((size_t)slice * mc * 8));
    SQ_TRY(h->out_keys.reserve((size_t)slice * k_sel * 8));
    if (prof)
        for (int i = 0; i < 2; ++i)
            if (!h->ev[i]) SQ_HIP(hipEventCreate(&h->ev[i]));
    const size_t lds = (size_t)isq_stage_bytes(d, h->code_kind);
    for (int q0 = 0; q0 < nq; q0 += slice) {
        const int m = nq - q0 < slice ? nq - q0 : slice;
        if (maxc > 0) {
            // the slice's candidates: no more than the batch's, nor than m times the longest list of candidates
            const long long cands = std::min(total, (long long)m * maxc), pairs = (long long)m * np;
            const bool shared = isq_scan_route(h->opt.isq_scan, h->code_kind, d, pw_tree_depth(d), m, np, nlist, cands);
            if (shared)
                SQ_TRY(ivf_pair_group<kIvfSharedGroup>(h->probe_idx.as<long long>(), q0, m, np, h->list_off.as<long long>(), nlist, h->pairs, served, st));
            if (prof) SQ_HIP(hipEventRecord(h->ev[0], st));
            const dim3 grid((unsigned)ivf_chunks(maxc), (unsigned)m), items((unsigned)ivf_shared_items_bound(cands, pairs));
            const size_t lds_shared = (size_t)isq_shared_lds_bytes(d, h->code_kind);
            if (shared && h->code_kind == SQ_ISQ_SQ8)
                SQ_TRY(launch_lds<isq_scan_shared_kernel<SQ_ISQ_SQ8, kIvfSharedGroup>>(
                    (int)kIvfSharedLdsBytes, items, dim3(256), lds_shared, st, h->codes.as<u8>(), h->stride, d, h->params.as<float>(), h->ids.as<u32>(),
                    h->list_off.as<long long>(), q_dev, q0, h->pre.as<long long>(), np, h->pairs.sorted.as<u64>(), h->pairs.groups.as<uint2>(),
                    h->pairs.item.as<long long>(), h->pairs.counts.as<long long>(), mc, h->keys.as<u64>()));
            else if (shared)
                SQ_TRY(launch_lds<isq_scan_shared_kernel<SQ_ISQ_F16, kIvfSharedGroup>>(
                    (int)kIvfSharedLdsBytes, items, dim3(256), lds_shared, st, h->codes.as<u8>(), h->stride, d, h->params.as<float>(), h->ids.as<u32>(),
                    h->list_off.as<long long>(), q_dev, q0, h->pre.as<long long>(), np, h->pairs.sorted.as<u64>(), h->pairs.groups.as<uint2>(),
                    h->pairs.item.as<long long>(), h->pairs.counts.as<long long>(), mc, h->keys.as<u64>()));
            else if (h->code_kind == SQ_ISQ_SQ8)
                SQ_TRY(launch_lds<isq_scan_kernel<SQ_ISQ_SQ8>>(kIsqStageMax, grid, dim3(256), lds, st, h->codes.as<u8>(), h->stride, d, h->ld,
                                                               h->params.as<float>(), h->ids.as<u32>(), h->list_off.as<long long>(), q_dev, q0,
                                                               h->probe_idx.as<long long>(), h->pre.as<long long>(), np, mc, h->keys.as<u64>()));
            else
                SQ_TRY(launch_lds<isq_scan_kernel<SQ_ISQ_F16>>(kIsqStageMax, grid, dim3(256), lds, st, h->codes.as<u8>(), h->stride, d, h->ld,
                                                               h->params.as<float>(), h->ids.as<u32>(), h->list_off.as<long long>(), q_dev, q0,
                                                               h->probe_idx.as<long long>(), h->pre.as<long long>(), np, mc, h->keys.as<u64>()));
            if (prof) {
                SQ_HIP(hipEventRecord(h->ev[1], st));
                SQ_HIP(hipEventSynchronize(h->ev[1]));
                float ms = 0.f;
                SQ_HIP(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
                h->stats.scan_ms += ms;
            }
            h->stats.scan_launches++;
        }
        const IvfFinalize fin{q0, k, h->id_base, od, oi};
        SQ_TRY(select_launch_t<u64>(h->keys.as<u64>(), h->cnt.as<u32>() + q0, (u32)mc, mc, k_sel, m, h->out_keys.as<u64>(), fin, st, h->sort_tmp));
    }
    h->stats.candidates = total;
    h->stats.bytes_scanned = total * h->stride;
    return SQ_OK;
}

}  // namespace sq

using namespace sq;

extern "C" int sq_isq_train(const float* x, int64_t n, int d, float* vmin, float* step, int mem) {
    if (!x || !vmin || !step || n <= 0 || d <= 0) return fail(SQ_ERR_INVALID, "sq_isq_train: bad argument");
    if (mem != SQ_MEM_HOST && mem != SQ_MEM_DEVICE) return fail(SQ_ERR_UNSUPPORTED, "sq_isq_train: host or device memory only");
    hipStream_t st = nullptr;
    const float* x_dev = x;
    DevBuf up, part, res;
    if (mem != SQ_MEM_DEVICE) {
        SQ_TRY(ivf_alloc(up, (size_t)n * d * 4));
        SQ_HIP(hipMemcpy(up.p, x, (size_t)n * d * 4, hipMemcpyHostToDevice));
        x_dev = up.as<float>();
    }
    const int parts = (int)std::min<long long>((n + 3) / 4, 256);
    SQ_TRY(part.reserve((size_t)parts * 2 * d * 4));
    SQ_TRY(res.reserve((size_t)2 * d * 4));
    float* vmin_dev = mem == SQ_MEM_DEVICE ? vmin : res.as<float>();
    float* step_dev = mem == SQ_MEM_DEVICE ? step : res.as<float>() + d;
    SQ_TRY(launch<isq_range_part_kernel>(dim3((unsigned)((d + 63) / 64), (unsigned)parts), dim3(256), 0, st, x_dev, (long long)n, d, part.as<float>()));
    SQ_TRY(launch<isq_range_final_kernel>(dim3((unsigned)((d + 255) / 256)), dim3(256), 0, st, part.as<float>(), parts, d, vmin_dev, step_dev));
    SQ_HIP(hipStreamSynchronize(st));
    if (mem != SQ_MEM_DEVICE) {
        SQ_HIP(hipMemcpy(vmin, vmin_dev, (size_t)d * 4, hipMemcpyDeviceToHost));
        SQ_HIP(hipMemcpy(step, step_dev, (size_t)d * 4, hipMemcpyDeviceToHost));
    }
    return SQ_OK;
}

extern "C" int sq_isq_create(const float* centroids, int nlist, int d, int kind, const float* vmin, const float* step, int metric,
                             int64_t id_base, sq_handle_t* out) {
    if (!centroids || !out || nlist <= 0 || d <= 0) return fail(SQ_ERR_INVALID, "sq_isq_create: bad argument");
    if (kind != SQ_ISQ_SQ8 && kind != SQ_ISQ_F16) return fail(SQ_ERR_INVALID, "sq_isq_create: kind %d is neither SQ_ISQ_SQ8 nor SQ_ISQ_F16", kind);
    if (kind == SQ_ISQ_SQ8 && (!vmin || !step)) return fail(SQ_ERR_INVALID, "sq_isq_create: SQ8 needs vmin and step");
    if (kind == SQ_ISQ_F16 && (vmin || step)) return fail(SQ_ERR_INVALID, "sq_isq_create: F16 takes no parameters (vmin and step must be NULL)");
    if (kind == SQ_ISQ_SQ8)
        for (int i = 0; i < d; ++i)
            if (!std::isfinite(vmin[i]) || !std::isfinite(step[i]) || step[i] < 0.f)
                return fail(SQ_ERR_INVALID, "sq_isq_create: vmin / step of dimension %d is not finite, or the step is negative", i);
    if (metric != SQ_METRIC_L2) return fail(SQ_ERR_UNSUPPORTED, "sq_isq_create: the inverted lists are L2 only (metric %d)", metric);
    if (nlist > kIvfMaxLists) return fail(SQ_ERR_UNSUPPORTED, "sq_isq_create: more than %d lists", kIvfMaxLists);
    if (isq_stage_bytes(d, kind) > kIsqStageMax)
        return fail(SQ_ERR_UNSUPPORTED, "sq_isq_create: rows of %d dimensions need %lld bytes of LDS staging, beyond a workgroup's %d", d,
                    isq_stage_bytes(d, kind), kIsqStageMax);
    auto h = std::make_unique<IsqHandle>();
    h->kind = H_ISQ;
    h->code_kind = kind;
    h->d = d;
    h->ld = ivf_row_stride(d);
    h->stride = isq_row_stride(d, kind);
    h->nlist = nlist;
    h->id_base = id_base;
    h->refresh_options();
    if (hipGetDevice(&h->device) != hipSuccess) return fail(SQ_ERR_HIP, "sq_isq_create: no HIP device");
    SQ_TRY(ivf_coarse_create(centroids, nlist, d, SQ_MEM_HOST, &h->coarse));
    h->off_host.assign((size_t)nlist + 1, 0);
    SQ_TRY(ivf_alloc(h->list_off, (size_t)(nlist + 1) * 8));
    SQ_HIP(hipMemset(h->list_off.p, 0, (size_t)(nlist + 1) * 8));
    std::vector<float> par((size_t)2 * h->ld, 0.f);   // F16 keeps the (unused) zeros: one kernel signature
    if (kind == SQ_ISQ_SQ8) {
        std::copy(vmin, vmin + d, par.begin());
        std::copy(step, step + d, par.begin() + h->ld);
    }
    SQ_TRY(ivf_alloc(h->params, par.size() * 4));
    SQ_HIP(hipMemcpy(h->params.p, par.data(), par.size() * 4, hipMemcpyHostToDevice));
    *out = register_handle(h.release());
    return SQ_OK;
}

extern "C" int sq_isq_add(sq_handle_t hid, const float* rows, int64_t n_add, int mem) {
    auto* h = static_cast<IsqHandle*>(lookup_handle(hid, H_ISQ));
    if (!h) return fail(SQ_ERR_INVALID, "sq_isq_add: unknown handle");
    if (!rows || n_add <= 0) return fail(SQ_ERR_INVALID, "sq_isq_add: bad argument");
    if (mem != SQ_MEM_HOST && mem != SQ_MEM_DEVICE) return fail(SQ_ERR_UNSUPPORTED, "sq_isq_add: rows in host or device memory only");
    std::lock_guard<std::mutex> lock(h->mu);
    h->refresh_options();
    if (!ivf_rows_ok(h->n + n_add)) return fail(SQ_ERR_UNSUPPORTED, "sq_isq_add: more than 2^32-1 rows");
    SQ_HIP(hipSetDevice(h->device));
    const auto t0 = std::chrono::steady_clock::now();
    h->stats = sq_stats_t{};   // what the assignment did: launches of ivf_assign_kernel, rows it decided, rows of the exact path
    for (long long s = 0; s < n_add; s += kIvfGroupMax)
        SQ_TRY(isq_add_part(h, rows + s * h->d, std::min<long long>(kIvfGroupMax, n_add - s), mem));
    h->add_us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    return SQ_OK;
}

extern "C" int sq_isq_lists(sq_handle_t hid, int64_t* list_off, int64_t* ids, void* codes) {
    auto* h = static_cast<IsqHandle*>(lookup_handle(hid, H_ISQ));
    if (!h) return fail(SQ_ERR_INVALID, "sq_isq_lists: unknown handle");
    std::lock_guard<std::mutex> lock(h->mu);
    SQ_HIP(hipSetDevice(h->device));
    if (list_off)
        for (int l = 0; l <= h->nlist; ++l) list_off[l] = h->off_host[(size_t)l];
    if (ids && h->n > 0) {
        std::vector<u32> tmp((size_t)h->n);
        SQ_HIP(hipMemcpy(tmp.data(), h->ids.p, (size_t)h->n * 4, hipMemcpyDeviceToHost));
        for (long long i = 0; i < h->n; ++i) ids[i] = h->id_base + (int64_t)tmp[(size_t)i];
    }
    if (codes && h->n > 0) {   // without the padding
        const size_t row = (size_t)h->d * isq_code_bytes(h->code_kind);
        std::vector<u8> tmp((size_t)h->n * h->stride);
        SQ_HIP(hipMemcpy(tmp.data(), h->codes.p, tmp.size(), hipMemcpyDeviceToHost));
        for (long long i = 0; i < h->n; ++i) memcpy(static_cast<u8*>(codes) + (size_t)i * row, tmp.data() + (size_t)i * h->stride, row);
    }
    return SQ_OK;
}

extern "C" int sq_isq_info(sq_handle_t hid, int64_t* out, int n_out) {
    auto* h = static_cast<IsqHandle*>(lookup_handle(hid, H_ISQ));
    if (!h) return fail(SQ_ERR_INVALID, "sq_isq_info: unknown handle");
    if (!out || n_out < SQ_ISQ_INFO_FIELDS) return fail(SQ_ERR_INVALID, "sq_isq_info: room for %d values needed", SQ_ISQ_INFO_FIELDS);
    std::lock_guard<std::mutex> lock(h->mu);
    h->refresh_options();
    long long longest = 0, empty = 0;
    for (int l = 0; l < h->nlist; ++l) {
        const long long c = h->off_host[(size_t)l + 1] - h->off_host[(size_t)l];
        longest = c > longest ? c : longest;
        empty += c == 0;
    }
    int64_t ci[SQ_DENSE_INFO_FIELDS] = {0};
    SQ_TRY(sq_dense_info(h->coarse, ci, SQ_DENSE_INFO_FIELDS));
    out[0] = h->n;
    out[1] = h->d;
    out[2] = h->nlist;
    out[3] = longest;
    out[4] = empty;
    out[5] = h->n > 0 ? (int64_t)h->codes.cap : 0;                         // the code rows, list-major
    out[6] = (int64_t)((h->n > 0 ? h->ids.cap : 0) + h->list_off.cap);     // insertion numbers and list offsets
    out[7] = ci[2] + ci[4] + ci[5] + ci[6] + (int64_t)h->params.cap;       // the coarse index and vmin / step
    out[8] = h->add_us;
    out[9] = h->opt.ivf_key_budget_mb > 0 ? (int64_t)h->opt.ivf_key_budget_mb << 20 : kIvfKeyBudget;
    out[10] = h->code_kind;
    out[11] = h->stride;
    return SQ_OK;
}

extern "C" int sq_isq_search(sq_handle_t hid, const float* queries, int nq, int k, int nprobe, float* out_dist, int64_t* out_idx,
                             int mem, void* stream) {
    if (mem != SQ_MEM_HOST && mem != SQ_MEM_DEVICE)
        return fail(SQ_ERR_UNSUPPORTED, "sq_isq_search: blocking calls only (SQ_MEM_HOST or SQ_MEM_DEVICE), not mode %d", mem);
    auto* h = static_cast<IsqHandle*>(lookup_handle(hid, H_ISQ));
    if (!h) return fail(SQ_ERR_INVALID, "sq_isq_search: unknown handle");
    if (!queries || !out_dist || !out_idx || nq <= 0 || k <= 0 || nprobe < 1) return fail(SQ_ERR_INVALID, "sq_isq_search: bad argument");
    std::lock_guard<std::mutex> lock(h->mu);
    h->refresh_options();
    SQ_HIP(hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const auto t_call = std::chrono::steady_clock::now();
    h->stats = sq_stats_t{};
    if (mem == SQ_MEM_HOST) {
        SQ_TRY(staged_call(h->stage, st, {{h->q_dev, queries, (size_t)nq * h->d * 4}},
                           {{out_dist, h->out_dist, (size_t)nq * k * 4}, {out_idx, h->out_idx, (size_t)nq * k * 8}}, [&] {
                               return isq_search_device(h, h->q_dev.as<float>(), nq, k, nprobe, h->out_dist.as<float>(),
                                                        h->out_idx.as<long long>(), st);
                           }));
    } else {
        SQ_TRY(isq_search_device(h, queries, nq, k, nprobe, out_dist, reinterpret_cast<long long*>(out_idx), st));
        SQ_HIP(stream_wait(st));
    }
    h->stats.mid_tier_queries = reinterpret_cast<const long long*>(h->totals_host.p)[2];   // (query, list) pairs of the list-major scan
    if (h->opt.profile != 0) h->stats.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
    return SQ_OK;
}

extern "C" int sq_isq_destroy(sq_handle_t hid) {
    auto* h = remove_handle(hid, H_ISQ);
    if (!h) return fail(SQ_ERR_INVALID, "sq_isq_destroy: unknown handle");
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    delete h;
    return SQ_OK;
}
