// What the inverted-list indexes share on the device: IVF-Flat (sq_ivf.hip) and IVF-PQ (sq_pq.hip) include this header.
// The coarse index over the centroids and the assignment by it, the stable counting sort that groups rows by list, the
// per-query prefix of the probed lists' sizes with the two totals the host sizes a scan with, and the select's post-op
// that turns keys into (distance, id).  The host arithmetic is sq_ivf_plan.hpp.
#pragma once
#include <algorithm>
#include <vector>

#include "sq_dense_exact.hpp"
#include "sq_ivf_plan.hpp"

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

// nearest centroid of n rows (device, row stride d), kIvfAssignSlice rows per call
static int ivf_assign(sq_handle_t coarse, const float* x, long long n, int d, long long* assign, float* dist, hipStream_t st) {
    for (long long s = 0; s < n; s += kIvfAssignSlice) {
        const int m = (int)std::min<long long>(kIvfAssignSlice, n - s);
        SQ_TRY(sq_dense_search(coarse, x + s * d, m, 1, dist + s, reinterpret_cast<int64_t*>(assign + s), SQ_MEM_DEVICE, st));
    }
    return SQ_OK;
}

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
