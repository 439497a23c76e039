// IVF-Flat: inverted lists over the float32 rows (gfx950).
//
// What FaissNearestNeighborsIndex reaches through a factory string with an IVF stage and `ivf_nprobe`
// (smqtk_indexing/impls/nn_index/faiss.py:190-192, 230-236, 785, 805-809), stated against the oracle: a row belongs to
// the list of its nearest centroid, a query probes the lists of its nprobe nearest centroids, and the answer is the k
// smallest (distance, id) among the rows of those lists -- distances float32 in metrics.euclidean_distance's own
// arithmetic (utils/metrics.py:73-86), so with every list probed the call returns sq_dense_search's bits.
//
// The two stages that must be exact are calls of the certified dense index over the centroids (sq_dense_search, k = 1
// and k = nprobe: with at most 65536 centroids that is exact keys of every centroid plus the select, ties by list
// number).  New device code is the storage (a stable counting sort into list-major rows), the list scan and the k-means
// update; the host arithmetic is sq_ivf_plan.hpp.
#include <algorithm>
#include <chrono>
#include <vector>

#include "../../include/smqtk_hip_ivf.h"
#include "sq_ivf_group.hpp"   // the coarse index, the counting sort, the probed lists' prefix: shared with sq_pq.hip

namespace sq {

struct IvfHandle : HandleBase {
    int d = 0, nlist = 0;
    long long ld = 0, n = 0, id_base = 0;
    sq_handle_t coarse = 0;              // dense index over the centroids: assignment and probing
    DevBuf rows, ids, list_off;          // [n][ld] float32 list-major, [n] insertion numbers, [nlist + 1]
    std::vector<long long> off_host;     // list_off on the host
    long long add_us = 0;
    // scratch of a search
    DevBuf q_dev, probe_dist, probe_idx, pre, cnt, keys, out_keys, out_dist, out_idx, sort_tmp;
    HostPinned totals_host;              // [candidates in total, longest candidate list]
    PinnedStage stage;
    ~IvfHandle() override {
        if (coarse) (void)sq_dense_destroy(coarse);
    }
};

// ------------------------------------------------------------------ the counting sort (ivf_group: sq_ivf_group.hpp)
// old row s of list l -> new_off[l] + (s - old_off[l]); eight lanes per row, 16 bytes each
static __global__ __launch_bounds__(256) void ivf_scatter_old_kernel(const float* __restrict__ old_rows, const u32* __restrict__ old_ids,
                                                                      const long long* __restrict__ old_off,
                                                                      const long long* __restrict__ new_off, int nlist, long long n_old,
                                                                      long long ld, float* __restrict__ new_rows, u32* __restrict__ new_ids) {
    const long long s = (long long)blockIdx.x * 32 + (threadIdx.x >> 3);
    if (s >= n_old) return;
    const int j8 = threadIdx.x & 7;
    const int l = ivf_locate(old_off, nlist, s);
    const long long dst = new_off[l] + (s - old_off[l]);
    for (long long c = j8 * 4; c < ld; c += 32)
        *reinterpret_cast<f32x4*>(new_rows + dst * ld + c) = *reinterpret_cast<const f32x4*>(old_rows + s * ld + c);
    if (j8 == 0) new_ids[dst] = old_ids[s];
}
// the t-th new row in (list, insertion) order -> add_at[l] + (t - add_pre[l]); rows arrive with stride d and are
// padded with zeros to ld floats (VEC: d == ld and a 16-byte aligned source)
template <bool VEC>
static __global__ __launch_bounds__(256) void ivf_scatter_new_kernel(const float* __restrict__ src, int d, long long ld,
                                                                      const u64* __restrict__ sorted, long long n_add,
                                                                      const long long* __restrict__ add_at,
                                                                      const long long* __restrict__ add_pre, long long n_old,
                                                                      float* __restrict__ new_rows, u32* __restrict__ new_ids) {
    const long long t = (long long)blockIdx.x * 32 + (threadIdx.x >> 3);
    if (t >= n_add) return;
    const int j8 = threadIdx.x & 7;
    const u64 key = sorted[t];
    const long long l = (long long)(key >> 32), i = (long long)(key & 0xffffffffull);
    const long long dst = add_at[l] + (t - add_pre[l]);
    if constexpr (VEC) {
        for (long long c = j8 * 4; c < ld; c += 32)
            *reinterpret_cast<f32x4*>(new_rows + dst * ld + c) = *reinterpret_cast<const f32x4*>(src + i * ld + c);
    } else {
        for (long long c = j8; c < ld; c += 8) new_rows[dst * ld + c] = c < d ? src[i * d + c] : 0.f;
    }
    if (j8 == 0) new_ids[dst] = (u32)(n_old + i);
}

// One counting sort: assign, group, scatter old and new rows into new buffers, swap.  Nothing of the handle changes
// before the swap, so a failed allocation leaves the index as it was.
static int ivf_add_part(IvfHandle* h, const float* rows, long long n_add, int mem) {
    hipStream_t st = nullptr;
    const int d = h->d, nlist = h->nlist;
    const long long ld = h->ld, n_old = h->n, n_new = n_old + n_add;
    const float* src = rows;
    DevBuf up;
    if (mem != SQ_MEM_DEVICE) {
        SQ_TRY(ivf_alloc(up, (size_t)n_add * d * 4));
        SQ_HIP(hipMemcpy(up.p, rows, (size_t)n_add * d * 4, hipMemcpyHostToDevice));
        src = up.as<float>();
    }
    DevBuf assign, adist;
    SQ_TRY(assign.reserve((size_t)n_add * 8));
    SQ_TRY(adist.reserve((size_t)n_add * 4));
    SQ_TRY(ivf_assign(h->coarse, src, n_add, d, assign.as<long long>(), adist.as<float>(), st));
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
        return fail(SQ_ERR_INTERNAL, "sq_ivf_add: the counting sort's offsets do not add up");
    DevBuf nrows, nids, noff;
    SQ_TRY(ivf_alloc(nrows, (size_t)n_new * ld * 4));
    SQ_TRY(ivf_alloc(nids, (size_t)n_new * 4));
    SQ_TRY(ivf_alloc(noff, plan.size() * 8));
    SQ_HIP(hipMemcpy(noff.p, plan.data(), plan.size() * 8, hipMemcpyHostToDevice));
    const long long* noff_d = noff.as<long long>();
    if (n_old > 0)
        SQ_TRY(launch<ivf_scatter_old_kernel>(dim3((unsigned)((n_old + 31) / 32)), dim3(256), 0, st, h->rows.as<float>(), h->ids.as<u32>(),
                                              h->list_off.as<long long>(), noff_d, nlist, n_old, ld, nrows.as<float>(), nids.as<u32>()));
    const dim3 grid((unsigned)((n_add + 31) / 32));
    if (ld == d && (reinterpret_cast<uintptr_t>(src) & 15u) == 0)
        SQ_TRY(launch<ivf_scatter_new_kernel<true>>(grid, dim3(256), 0, st, src, d, ld, g.sorted.as<u64>(), n_add, noff_d + nlist + 1,
                                                    noff_d + 2 * nlist + 1, n_old, nrows.as<float>(), nids.as<u32>()));
    else
        SQ_TRY(launch<ivf_scatter_new_kernel<false>>(grid, dim3(256), 0, st, src, d, ld, g.sorted.as<u64>(), n_add, noff_d + nlist + 1,
                                                     noff_d + 2 * nlist + 1, n_old, nrows.as<float>(), nids.as<u32>()));
    SQ_HIP(hipStreamSynchronize(st));
    h->rows = std::move(nrows);
    h->ids = std::move(nids);
    h->list_off = std::move(noff);   // (its first nlist + 1 words; the rest served the scatter)
    h->off_host.assign(new_off, new_off + nlist + 1);
    h->n = n_new;
    return SQ_OK;
}

// ------------------------------------------------------------------ search
// (1) ivf_probe_sizes_kernel and (2) ivf_totals_kernel: sq_ivf_group.hpp.
// (3) The scan.  Work item (blockIdx.x, query): candidates [256 blockIdx.x, + 256) of the query's concatenated range,
// one per lane.  A lane finds its list in the query's prefix array, reads its row -- neighbouring lanes read
// neighbouring rows of a list's contiguous block -- and computes the distance as dense_exact_l2_kernel does (numpy's
// eight accumulators per leaf, its pairwise tree, a correctly rounded square root).  Dynamic LDS: ld floats.
static __global__ __launch_bounds__(256) void ivf_scan_kernel(const float* __restrict__ rows, long long ld, int d,
                                                               const u32* __restrict__ ids, const long long* __restrict__ list_off,
                                                               const float* __restrict__ queries, int q0,
                                                               const long long* __restrict__ probe, const long long* __restrict__ pre,
                                                               int np, long long key_stride, u64* __restrict__ keys) {
    extern __shared__ __attribute__((aligned(16))) float s_q[];
    const int ql = blockIdx.y, q = q0 + ql;
    const long long* pq = pre + (long long)q * (np + 1);
    const long long total = pq[np];
    const long long base = (long long)blockIdx.x * kIvfChunk;
    if (base >= total) return;
    for (int i = threadIdx.x; i < d; i += 256) s_q[i] = queries[(long long)q * d + i];
    __syncthreads();
    const long long p = base + threadIdx.x;
    if (p >= total) return;
    const int j = ivf_locate(pq, np, p);
    const long long l = probe[(long long)q * np + j];
    const long long s = list_off[l] + (p - pq[j]);
    const SqLeafLane w{rows + s * ld, s_q};
    const float dist = sqrt_rn_f32(w.sum(d));
    keys[(long long)ql * key_stride + p] = ((u64)ordered_f32(dist) << 32) | (u64)ids[s];
}
// (4) the select's post-op, IvfFinalize: sq_ivf_group.hpp.

// ------------------------------------------------------------------ k-means update
// Centroid l, dimensions [64 blockIdx.y, + 64): the float64 sum of the list's rows in insertion order.  Wave w of the
// workgroup adds rows w, w + 4, ... of the list one after the other, the four partial sums are combined as
// (s0 + s1) + (s2 + s3): a fixed tree, no atomics.  Divided by the count, rounded to float32 once.  An empty list
// keeps its centroid.
static __global__ __launch_bounds__(256) void ivf_kmeans_update_kernel(const float* __restrict__ x, int d, const u64* __restrict__ sorted,
                                                                        const long long* __restrict__ bounds,
                                                                        float* __restrict__ centroids) {
    __shared__ double s_part[4][64];
    const int l = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int dim = blockIdx.y * 64 + lane;
    const long long b0 = bounds[l], c = bounds[l + 1] - b0;
    double acc = 0.0;
    if (dim < d)
        for (long long r = wv; r < c; r += 4) {
            const long long i = (long long)(sorted[b0 + r] & 0xffffffffull);
            acc = __dadd_rn(acc, (double)x[i * d + dim]);
        }
    s_part[wv][lane] = acc;
    __syncthreads();
    if (wv == 0 && dim < d && c > 0) {
        const double sum = __dadd_rn(__dadd_rn(s_part[0][lane], s_part[1][lane]), __dadd_rn(s_part[2][lane], s_part[3][lane]));
        centroids[(long long)l * d + dim] = (float)__ddiv_rn(sum, (double)c);
    }
}

// The search with queries and outputs in device memory, enqueued on `st`; the last select is not waited for.
static int ivf_search_device(IvfHandle* h, const float* q_dev, int nq, int k, int nprobe, float* od, long long* oi, hipStream_t st) {
    const int d = h->d, nlist = h->nlist, np = nprobe < nlist ? nprobe : nlist;
    const bool prof = h->opt.profile != 0;
    // probe: the np nearest centroids per query, (distance, list number) order, on the device
    SQ_TRY(h->probe_dist.reserve((size_t)nq * np * 4));
    SQ_TRY(h->probe_idx.reserve((size_t)nq * np * 8));
    SQ_TRY(sq_dense_search(h->coarse, q_dev, nq, np, h->probe_dist.p, h->probe_idx.as<int64_t>(), SQ_MEM_DEVICE, st));
    // candidate offsets; only [total, longest] visit the host
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
    if (maxc > kIvfMaxRows) return fail(SQ_ERR_INTERNAL, "sq_ivf_search: a query has more candidates than the index has rows");
    const long long mc = maxc > 0 ? maxc : 1;
    const int k_sel = (int)ivf_select_k(maxc, k);
    const long long budget = h->opt.ivf_key_budget_mb > 0 ? (long long)h->opt.ivf_key_budget_mb << 20 : kIvfKeyBudget;
    const int slice = (int)ivf_slice_queries(nq, maxc, k, budget);
    SQ_TRY(h->keys.reserve((size_t)slice * mc * 8));
    SQ_TRY(h->out_keys.reserve((size_t)slice * k_sel * 8));
    if (prof)
        for (int i = 0; i < 2; ++i)
            if (!h->ev[i]) SQ_HIP(hipEventCreate(&h->ev[i]));
    for (int q0 = 0; q0 < nq; q0 += slice) {
        const int m = nq - q0 < slice ? nq - q0 : slice;
        if (maxc > 0) {
            if (prof) SQ_HIP(hipEventRecord(h->ev[0], st));
            SQ_TRY(launch<ivf_scan_kernel>(dim3((unsigned)ivf_chunks(maxc), (unsigned)m), dim3(256), (size_t)h->ld * 4, st, h->rows.as<float>(),
                                           h->ld, d, h->ids.as<u32>(), h->list_off.as<long long>(), q_dev, q0, h->probe_idx.as<long long>(),
                                           h->pre.as<long long>(), np, mc, h->keys.as<u64>()));
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
    h->stats.bytes_scanned = total * h->ld * 4;
    return SQ_OK;
}

}  // namespace sq

using namespace sq;

extern "C" int sq_ivf_create(const float* centroids, int nlist, int d, int metric, int64_t id_base, sq_handle_t* out) {
    if (!centroids || !out || nlist <= 0 || d <= 0) return fail(SQ_ERR_INVALID, "sq_ivf_create: bad argument");
    if (metric != SQ_METRIC_L2) return fail(SQ_ERR_UNSUPPORTED, "sq_ivf_create: the inverted lists are L2 only (metric %d)", metric);
    if (nlist > kIvfMaxLists) return fail(SQ_ERR_UNSUPPORTED, "sq_ivf_create: more than %d lists", kIvfMaxLists);
    auto h = std::make_unique<IvfHandle>();
    h->kind = H_IVF;
    h->d = d;
    h->ld = ivf_row_stride(d);
    h->nlist = nlist;
    h->id_base = id_base;
    h->refresh_options();
    if (hipGetDevice(&h->device) != hipSuccess) return fail(SQ_ERR_HIP, "sq_ivf_create: no HIP device");
    SQ_TRY(ivf_coarse_create(centroids, nlist, d, SQ_MEM_HOST, &h->coarse));
    h->off_host.assign((size_t)nlist + 1, 0);
    SQ_TRY(ivf_alloc(h->list_off, (size_t)(nlist + 1) * 8));
    SQ_HIP(hipMemset(h->list_off.p, 0, (size_t)(nlist + 1) * 8));
    *out = register_handle(h.release());
    return SQ_OK;
}

extern "C" int sq_ivf_add(sq_handle_t hid, const float* rows, int64_t n_add, int mem) {
    auto* h = static_cast<IvfHandle*>(lookup_handle(hid, H_IVF));
    if (!h) return fail(SQ_ERR_INVALID, "sq_ivf_add: unknown handle");
    if (!rows || n_add <= 0) return fail(SQ_ERR_INVALID, "sq_ivf_add: bad argument");
    if (mem != SQ_MEM_HOST && mem != SQ_MEM_DEVICE) return fail(SQ_ERR_UNSUPPORTED, "sq_ivf_add: rows in host or device memory only");
    std::lock_guard<std::mutex> lock(h->mu);
    h->refresh_options();
    if (!ivf_rows_ok(h->n + n_add)) return fail(SQ_ERR_UNSUPPORTED, "sq_ivf_add: more than 2^32-1 rows");
    SQ_HIP(hipSetDevice(h->device));
    const auto t0 = std::chrono::steady_clock::now();
    // (an add beyond 2^26 rows is several counting sorts; each leaves a complete index)
    for (long long s = 0; s < n_add; s += kIvfGroupMax)
        SQ_TRY(ivf_add_part(h, rows + s * h->d, std::min<long long>(kIvfGroupMax, n_add - s), mem));
    h->add_us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    return SQ_OK;
}

extern "C" int sq_ivf_lists(sq_handle_t hid, int64_t* list_off, int64_t* ids) {
    auto* h = static_cast<IvfHandle*>(lookup_handle(hid, H_IVF));
    if (!h) return fail(SQ_ERR_INVALID, "sq_ivf_lists: unknown handle");
    std::lock_guard<std::mutex> lock(h->mu);
    SQ_HIP(hipSetDevice(h->device));
    if (list_off)
        for (int l = 0; l <= h->nlist; ++l) list_off[l] = h->off_host[(size_t)l];
    if (ids && h->n > 0) {
        std::vector<u32> tmp((size_t)h->n);
        SQ_HIP(hipMemcpy(tmp.data(), h->ids.p, (size_t)h->n * 4, hipMemcpyDeviceToHost));
        for (long long i = 0; i < h->n; ++i) ids[i] = h->id_base + (int64_t)tmp[(size_t)i];
    }
    return SQ_OK;
}

extern "C" int sq_ivf_info(sq_handle_t hid, int64_t* out, int n_out) {
    auto* h = static_cast<IvfHandle*>(lookup_handle(hid, H_IVF));
    if (!h) return fail(SQ_ERR_INVALID, "sq_ivf_info: unknown handle");
    if (!out || n_out < SQ_IVF_INFO_FIELDS) return fail(SQ_ERR_INVALID, "sq_ivf_info: room for %d values needed", SQ_IVF_INFO_FIELDS);
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
    out[5] = h->n > 0 ? (int64_t)h->rows.cap : 0;                          // the float32 rows, list-major
    out[6] = (int64_t)((h->n > 0 ? h->ids.cap : 0) + h->list_off.cap);     // insertion numbers and list offsets
    out[7] = ci[2] + ci[4] + ci[5] + ci[6];                                // the coarse index: centroids and their statistics
    out[8] = h->add_us;
    out[9] = h->opt.ivf_key_budget_mb > 0 ? (int64_t)h->opt.ivf_key_budget_mb << 20 : kIvfKeyBudget;
    return SQ_OK;
}

extern "C" int sq_ivf_search(sq_handle_t hid, const float* queries, int nq, int k, int nprobe, float* out_dist, int64_t* out_idx,
                             int mem, void* stream) {
    auto* h = static_cast<IvfHandle*>(lookup_handle(hid, H_IVF));
    if (!h) return fail(SQ_ERR_INVALID, "sq_ivf_search: unknown handle");
    if (!queries || !out_dist || !out_idx || nq <= 0 || k <= 0 || nprobe < 1) return fail(SQ_ERR_INVALID, "sq_ivf_search: bad argument");
    if (mem != SQ_MEM_HOST && mem != SQ_MEM_DEVICE)
        return fail(SQ_ERR_UNSUPPORTED, "sq_ivf_search: blocking calls only (SQ_MEM_HOST or SQ_MEM_DEVICE), not mode %d", mem);
    std::lock_guard<std::mutex> lock(h->mu);
    h->refresh_options();
    SQ_HIP(hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const auto t_call = std::chrono::steady_clock::now();
    h->stats = sq_stats_t{};
    if (mem == SQ_MEM_HOST) {
        SQ_TRY(staged_call(h->stage, st, {{h->q_dev, queries, (size_t)nq * h->d * 4}},
                           {{out_dist, h->out_dist, (size_t)nq * k * 4}, {out_idx, h->out_idx, (size_t)nq * k * 8}}, [&] {
                               return ivf_search_device(h, h->q_dev.as<float>(), nq, k, nprobe, h->out_dist.as<float>(),
                                                        h->out_idx.as<long long>(), st);
                           }));
    } else {
        SQ_TRY(ivf_search_device(h, queries, nq, k, nprobe, out_dist, reinterpret_cast<long long*>(out_idx), st));
        SQ_HIP(stream_wait(st));
    }
    if (h->opt.profile != 0) h->stats.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
    return SQ_OK;
}

extern "C" int sq_ivf_destroy(sq_handle_t hid) {
    auto* h = remove_handle(hid, H_IVF);
    if (!h) return fail(SQ_ERR_INVALID, "sq_ivf_destroy: unknown handle");
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    delete h;
    return SQ_OK;
}

extern "C" int sq_ivf_kmeans(const float* x, int64_t n, int d, float* centroids, int nlist, int iters, int mem) {
    if (!x || !centroids || n <= 0 || d <= 0 || nlist <= 0 || iters < 0) return fail(SQ_ERR_INVALID, "sq_ivf_kmeans: bad argument");
    if (n < nlist) return fail(SQ_ERR_INVALID, "sq_ivf_kmeans: %lld rows cannot train %d lists", (long long)n, nlist);
    if (nlist > kIvfMaxLists) return fail(SQ_ERR_UNSUPPORTED, "sq_ivf_kmeans: more than %d lists", kIvfMaxLists);
    if (n > kIvfGroupMax) return fail(SQ_ERR_UNSUPPORTED, "sq_ivf_kmeans: more than 2^26 training rows (train on a sample)");
    if (mem != SQ_MEM_HOST && mem != SQ_MEM_DEVICE) return fail(SQ_ERR_UNSUPPORTED, "sq_ivf_kmeans: host or device memory only");
    hipStream_t st = nullptr;
    const size_t cb = (size_t)nlist * d * 4;
    const hipMemcpyKind in = mem == SQ_MEM_DEVICE ? hipMemcpyDeviceToHost : hipMemcpyHostToHost;
    const hipMemcpyKind back = mem == SQ_MEM_DEVICE ? hipMemcpyHostToDevice : hipMemcpyHostToHost;
    std::vector<float> c_host((size_t)nlist * d);
    SQ_HIP(hipMemcpy(c_host.data(), centroids, cb, in));
    const float* x_dev = x;
    DevBuf up, c_dev, assign, adist;
    if (mem != SQ_MEM_DEVICE) {
        SQ_TRY(ivf_alloc(up, (size_t)n * d * 4));
        SQ_HIP(hipMemcpy(up.p, x, (size_t)n * d * 4, hipMemcpyHostToDevice));
        x_dev = up.as<float>();
    }
    SQ_TRY(c_dev.reserve(cb));
    SQ_TRY(assign.reserve((size_t)n * 8));
    SQ_TRY(adist.reserve((size_t)n * 4));
    IvfGroup g;
    for (int it = 0; it < iters; ++it) {
        // assign: the dense search over a temporary index of this iteration's centroids
        sq_handle_t coarse = 0;
        SQ_TRY(ivf_coarse_create(c_host.data(), nlist, d, SQ_MEM_HOST, &coarse));
        const int rc = ivf_assign(coarse, x_dev, n, d, assign.as<long long>(), adist.as<float>(), st);
        (void)sq_dense_destroy(coarse);
        if (rc != SQ_OK) return rc;
        // update: list-major sums after the same counting sort
        SQ_TRY(ivf_group(assign.as<long long>(), n, nlist, g, st));
        SQ_HIP(hipMemcpyAsync(c_dev.p, c_host.data(), cb, hipMemcpyHostToDevice, st));
        SQ_TRY(launch<ivf_kmeans_update_kernel>(dim3((unsigned)nlist, (unsigned)((d + 63) / 64)), dim3(256), 0, st, x_dev, d, g.sorted.as<u64>(),
                                                g.bounds.as<long long>(), c_dev.as<float>()));
        SQ_HIP(hipMemcpyAsync(c_host.data(), c_dev.p, cb, hipMemcpyDeviceToHost, st));
        SQ_HIP(hipStreamSynchronize(st));
    }
    SQ_HIP(hipMemcpy(centroids, c_host.data(), cb, back));
    return SQ_OK;
}
