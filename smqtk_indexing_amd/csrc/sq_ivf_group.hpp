// What the inverted-list indexes share on the device: IVF-Flat (sq_ivf.hip) and IVF-PQ (sq_pq.hip) include this header.
// The coarse index over the centroids and the assignment by it, the stable counting sort that groups rows by list, the
// per-query prefix of the probed lists' sizes with the two totals the host sizes a scan with, and the select's post-op
// that turns keys into (distance, id).  The host arithmetic is sq_ivf_plan.hpp.
#pragma once
#include <algorithm>
#include <vector>

#include "sq_dense_exact.hpp"
#include "sq_ivf_plan.hpp"
#include "sq_ivf_assign.hpp"   // ivf_assign: the MFMA assignment kernel, its certificate and the exact path behind it

namespace sq {

static constexpr long long kIvfGroupMax = 1ll << 26;   // rows one counting sort takes (its key sort: 1 GB of scratch)

// DevBuf::alloc_exact (these arrays are replaced whole); its failure is reported here, not again by the next launch's check
static int ivf_alloc(DevBuf& b, size_t bytes) { return b.alloc_exact(bytes) == SQ_OK ? SQ_OK : ((void)hipGetLastError(), SQ_ERR_NOMEM); }

// The coarse index: float32 centroids only -- no scan copies, and the candidate cap at its default, so that up to
// 65536 centroids are answered from exact keys of all of them.
static int ivf_coarse_create(const float* centroids, int nlist, int d, int mem, sq_handle_t* out) {
    static const char* const names[] = {"dense_bf16", "dense_int8", "dense_int8_wide", "candidate_cap", "force_fallback", "profile"};
    static const int64_t values[] = {0, 0, 0, 0, 0, 0};
    return sq_dense_create_opts(centroids, nlist, d, SQ_METRIC_L2, mem, 0, names, values, 6, out);
}

// (nearest centroid of n rows: ivf_assign, sq_ivf_assign.hpp)

// ------------------------------------------------------------------ the counting sort
// Rows grouped by list, insertion order inside a list: the keys (list, row) are unique, so their ascending order is
// the stable counting sort's; bounds[l] = rows of lower lists.  No atomics: the same input gives the same order.
static __global__ __launch_bounds__(256) void ivf_group_keys_kernel(const long long* __restrict__ assign, long long n, int nlist,
                                                                     u64* __restrict__ keys) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    long long l = assign[i];
    l = l < 0 ? 0 : (l >= nlist ? nlist - 1 : l);
    keys[i] = ((u64)l << 32) | (u64)(u32)i;
}
static __global__ __launch_bounds__(256) void ivf_bounds_kernel(const u64* __restrict__ sorted, long long n, int nlist,
                                                                 long long* __restrict__ bounds) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l > nlist) return;
    const u64 want = (u64)l << 32;
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (sorted[mid] < want) lo = mid + 1; else hi = mid;
    }
    bounds[l] = lo;
}

struct IvfGroup {
    DevBuf keys, sorted, scratch, bounds, cnt;
    std::vector<long long> bounds_host;   // [nlist + 1]
};
static int ivf_group(const long long* assign, long long n, int nlist, IvfGroup& g, hipStream_t st) {
    SQ_TRY(g.keys.reserve((size_t)n * 8));
    SQ_TRY(g.sorted.reserve((size_t)n * 8));
    SQ_TRY(g.bounds.reserve((size_t)(nlist + 1) * 8));
    SQ_TRY(g.cnt.reserve(64));
    SQ_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(g.cnt.p), (int)(u32)n, 1, st));
    SQ_TRY(launch<ivf_group_keys_kernel>(dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, assign, n, nlist, g.keys.as<u64>()));
    SQ_TRY(sort_select_large<u64, SelectNoPost>(g.keys.as<u64>(), g.cnt.as<u32>(), (u32)n, n, (int)n, 1, g.sorted.as<u64>(), g.scratch,
                                                SelectNoPost(), st));
    SQ_TRY(launch<ivf_bounds_kernel>(dim3((unsigned)(nlist / 256 + 1)), dim3(256), 0, st, g.sorted.as<u64>(), n, nlist, g.bounds.as<long long>()));
    g.bounds_host.resize((size_t)nlist + 1);
    SQ_HIP(hipMemcpyAsync(g.bounds_host.data(), g.bounds.p, (size_t)(nlist + 1) * 8, hipMemcpyDeviceToHost, st));
    SQ_HIP(hipStreamSynchronize(st));
    return SQ_OK;
}

// ------------------------------------------------------------------ search
// (1) per query: the exclusive prefix of its probed lists' sizes, pre[q][0 .. np] (pre[q][np] = its candidates), and
// the candidate count the select reads
static __global__ __launch_bounds__(256) void ivf_probe_sizes_kernel(const long long* __restrict__ probe, int np,
                                                                      const long long* __restrict__ list_off, int nlist,
                                                                      long long* __restrict__ pre, u32* __restrict__ cnt) {
    const int q = blockIdx.x;
    __shared__ long long s_wave[4];
    __shared__ long long s_run;
    if (threadIdx.x == 0) s_run = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    long long* pq = pre + (long long)q * (np + 1);
    for (int j0 = 0; j0 < np; j0 += 256) {
        const int j = j0 + threadIdx.x;
        long long len = 0;
        if (j < np) {
            const long long l = probe[(long long)q * np + j];
            if (l >= 0 && l < nlist) len = list_off[l + 1] - list_off[l];
        }
        long long inc = len;  // inclusive scan inside the wave
        for (int o = 1; o < 64; o <<= 1) {
            const long long t = __shfl_up(inc, o);
            if (lane >= o) inc += t;
        }
        if (lane == 63) s_wave[wv] = inc;
        __syncthreads();
        long long base = s_run;
        for (int w = 0; w < wv; ++w) base += s_wave[w];
        if (j < np) pq[j] = base + inc - len;
        __syncthreads();
        if (threadIdx.x == 0) s_run += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        pq[np] = s_run;
        cnt[q] = (u32)s_run;
    }
}
// (2) the two numbers the host sizes the scan with: [candidates in total, longest candidate list]
static __global__ __launch_bounds__(256) void ivf_totals_kernel(const long long* __restrict__ pre, int np, int nq,
                                                                 long long* __restrict__ totals_host) {
    __shared__ long long s_sum[256], s_max[256];
    long long sum = 0, mx = 0;
    for (int q = threadIdx.x; q < nq; q += 256) {
        const long long t = pre[(long long)q * (np + 1) + np];
        sum += t;
        mx = t > mx ? t : mx;
    }
    s_sum[threadIdx.x] = sum;
    s_max[threadIdx.x] = mx;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            s_sum[threadIdx.x] += s_sum[threadIdx.x + o];
            s_max[threadIdx.x] = s_max[threadIdx.x + o] > s_max[threadIdx.x] ? s_max[threadIdx.x + o] : s_max[threadIdx.x];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        totals_host[0] = s_sum[0];
        totals_host[1] = s_max[0];
    }
}
// ------------------------------------------------------------------ search: pairs grouped by list (the list-major scans)
// A slice of m queries has m * np (query, probe rank) pairs.  ivf_pair_group sorts them by list and cuts every list's run
// into groups of at most G pairs (the arithmetic: sq_ivf_plan.hpp), so that a scan reads a probed list once per group and
// not once per query.  On the device, no atomics, no host visit: the keys (list << 32) | (ql * np + j) are unique, so
// their order, the groups and the numbering of the work items are a function of the probe lists alone.
struct IvfPairGroups {
    DevBuf keys, sorted, scratch, cnt, bounds, groups, item, counts;
    // sorted: [pairs] keys, those of empty and out-of-range lists (all ones) behind the others
    // groups: [<= pairs] (first pair in `sorted`, pairs); item: [groups + 1] exclusive prefix of the groups' row chunks
    // counts: [groups, work items]
};

// pair i = ql * np + j of the slice that starts at query q0 -> its key; cnt[0] = pairs (what the sort reads)
static __global__ __launch_bounds__(256) void ivf_pair_keys_kernel(const long long* __restrict__ probe, int q0, long long pairs, int np,
                                                                    const long long* __restrict__ list_off, int nlist,
                                                                    u64* __restrict__ keys, u32* __restrict__ cnt) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) cnt[0] = (u32)pairs;
    if (i >= pairs) return;
    const long long l = probe[(long long)q0 * np + i];
    const bool live = l >= 0 && l < nlist && list_off[l + 1] > list_off[l];
    keys[i] = live ? ((u64)l << 32) | (u64)(u32)i : ~0ull;
}

// One workgroup walks the lists 1024 at a time: list l is probed by c = bounds[l + 1] - bounds[l] pairs, which makes
// ceil(c / G) groups of ceil(len / 256) work items each; a block-wide exclusive scan numbers both, the list's thread
// writes its groups.  served_host (pinned): the live pairs are added to it -- one thread, in stream order.
template <int G>
static __global__ __launch_bounds__(1024) void ivf_pair_groups_kernel(const long long* __restrict__ bounds,
                                                                       const long long* __restrict__ list_off, int nlist,
                                                                       uint2* __restrict__ groups, long long* __restrict__ item,
                                                                       long long* __restrict__ counts, long long* __restrict__ served_host) {
    __shared__ long long s_g[16], s_i[16];
    __shared__ long long s_run[2];
    if (threadIdx.x == 0) s_run[0] = s_run[1] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int l0 = 0; l0 < nlist; l0 += 1024) {
        const int l = l0 + threadIdx.x;
        long long first = 0, c = 0, chunks = 0;
        if (l < nlist) {
            first = bounds[l];
            c = bounds[l + 1] - first;
            chunks = ivf_row_chunks(list_off[l + 1] - list_off[l]);
        }
        const long long ng = ivf_pair_groups(c, G), ni = ng * chunks;
        long long inc_g = ng, inc_i = ni;   // inclusive scans inside the wave
        for (int o = 1; o < 64; o <<= 1) {
            const long long tg = __shfl_up(inc_g, o), ti = __shfl_up(inc_i, o);
            if (lane >= o) {
                inc_g += tg;
                inc_i += ti;
            }
        }
        if (lane == 63) {
            s_g[wv] = inc_g;
            s_i[wv] = inc_i;
        }
        __syncthreads();
        long long base_g = s_run[0], base_i = s_run[1];
        for (int w = 0; w < wv; ++w) {
            base_g += s_g[w];
            base_i += s_i[w];
        }
        base_g += inc_g - ng;
        base_i += inc_i - ni;
        for (long long g = 0; g < ng; ++g) {
            groups[base_g + g] = make_uint2((u32)(first + g * G), (u32)ivf_pair_group_size(c, g, G));
            item[base_g + g] = base_i + g * chunks;
        }
        __syncthreads();
        if (threadIdx.x == 1023) {
            s_run[0] = base_g + ng;
            s_run[1] = base_i + ni;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        item[s_run[0]] = s_run[1];
        counts[0] = s_run[0];
        counts[1] = s_run[1];
        *served_host += bounds[nlist];
    }
}

// The pairs of queries [q0, q0 + m) grouped for a scan with groups of G, enqueued on `st`.  pairs = m * np fits
// kIvfSharedMaxPairs (ivf_scan_route).
template <int G>
static int ivf_pair_group(const long long* probe, int q0, int m, int np, const long long* list_off, int nlist, IvfPairGroups& g,
                          long long* served_host, hipStream_t st) {
    const long long pairs = (long long)m * np;
    SQ_TRY(g.keys.reserve((size_t)pairs * 8));
    SQ_TRY(g.sorted.reserve((size_t)pairs * 8));
    SQ_TRY(g.cnt.reserve(64));
    SQ_TRY(g.bounds.reserve((size_t)(nlist + 1) * 8));
    SQ_TRY(g.groups.reserve((size_t)pairs * 8));
    SQ_TRY(g.item.reserve((size_t)(pairs + 1) * 8));
    SQ_TRY(g.counts.reserve(64));
    SQ_TRY(launch<ivf_pair_keys_kernel>(dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, st, probe, q0, pairs, np, list_off, nlist,
                                        g.keys.as<u64>(), g.cnt.as<u32>()));
    SQ_TRY(sort_select_large<u64, SelectNoPost>(g.keys.as<u64>(), g.cnt.as<u32>(), (u32)pairs, pairs, (int)pairs, 1, g.sorted.as<u64>(), g.scratch,
                                                SelectNoPost(), st));
    SQ_TRY(launch<ivf_bounds_kernel>(dim3((unsigned)(nlist / 256 + 1)), dim3(256), 0, st, g.sorted.as<u64>(), pairs, nlist, g.bounds.as<long long>()));
    return launch<ivf_pair_groups_kernel<G>>(dim3(1), dim3(1024), 0, st, g.bounds.as<long long>(), list_off, nlist, g.groups.as<uint2>(),
                                             g.item.as<long long>(), g.counts.as<long long>(), served_host);
}

// G squared distances of one row, a leaf (<= 128 elements) of the row in registers at a time: the L2 branch of
// dense_exact_group_kernel (sq_dense_exact.hpp) restated for the list scans -- numpy's eight accumulators per leaf, every
// 16-byte load of a leaf requested before its first use, the queries read from LDS (G rows of dq floats; all lanes read
// the same address).  x: the row, 16-byte aligned.  Only the first `live` slots are scored (a workgroup-wide branch): the
// sums of the others are left at zero and never stored.
template <int G>
struct SqLeafGroup {
    const float* x;
    const float* s_qg;
    int dq, live;
    __device__ __forceinline__ void operator()(int off, int m, float (&v)[G]) const {
        if (m < 8) {
#pragma unroll
            for (int g = 0; g < G; ++g) {
                float r = 0.f;
                for (int i = 0; i < (g < live ? m : 0); ++i) {
                    const float t = __fsub_rn(x[off + i], s_qg[g * dq + off + i]);
                    r = __fadd_rn(r, __fmul_rn(t, t));
                }
                v[g] = r;
            }
            return;
        }
        const int nfull = m - (m % 8);
        const int nv = nfull / 4;   // 2 .. 32 vectors
        f32x4 xr[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) xr[u] = *reinterpret_cast<const f32x4*>(x + off + 4 * (u < nv ? u : 0));
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (g >= live) {
                v[g] = 0.f;
                continue;
            }
            const float* qg = s_qg + g * dq + off;
            float r[8];
            {
                const f32x4 q0 = *reinterpret_cast<const f32x4*>(qg), q1 = *reinterpret_cast<const f32x4*>(qg + 4);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float t0 = __fsub_rn(xr[0][c], q0[c]), t1 = __fsub_rn(xr[1][c], q1[c]);
                    r[c] = __fmul_rn(t0, t0);
                    r[4 + c] = __fmul_rn(t1, t1);
                }
            }
#pragma unroll
            for (int u = 2; u < 32; u += 2) {
                if (u < nv) {
                    const f32x4 q0 = *reinterpret_cast<const f32x4*>(qg + 4 * u);
                    const f32x4 q1 = *reinterpret_cast<const f32x4*>(qg + 4 * u + 4);
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float t0 = __fsub_rn(xr[u][c], q0[c]), t1 = __fsub_rn(xr[u + 1][c], q1[c]);
                        r[c] = __fadd_rn(r[c], __fmul_rn(t0, t0));
                        r[4 + c] = __fadd_rn(r[4 + c], __fmul_rn(t1, t1));
                    }
                }
            }
            float res = __fadd_rn(__fadd_rn(__fadd_rn(r[0], r[1]), __fadd_rn(r[2], r[3])),
                                  __fadd_rn(__fadd_rn(r[4], r[5]), __fadd_rn(r[6], r[7])));
            for (int i = nfull; i < m; ++i) {
                const float t = __fsub_rn(x[off + i], qg[i]);
                res = __fadd_rn(res, __fmul_rn(t, t));
            }
            v[g] = res;
        }
    }
};

// the select's post-op: keys -> (distance, id_base + insertion number), padding behind the candidates
struct IvfFinalize {
    int q0, k;
    long long id_base;
    float* out_dist;
    long long* out_idx;
    __device__ __forceinline__ void operator()(int ql, const u64* sorted, int k_sel) const {
        const long long o = (long long)(q0 + ql) * k;
        for (int j = threadIdx.x; j < k; j += blockDim.x) {
            const u64 key = j < k_sel ? sorted[j] : ~0ull;
            const bool pad = key == ~0ull;
            out_dist[o + j] = pad ? __builtin_inff() : unordered_f32((u32)(key >> 32));
            out_idx[o + j] = pad ? -1ll : id_base + (long long)(key & 0xffffffffull);
        }
    }
};

}  // namespace sq
