// Nearest-centroid assignment of a batch of rows on the float32 matrix cores (gfx950): what every inverted-list build
// calls through ivf_assign (sq_ivf_group.hpp).  ivf_assign_kernel scores every (row, centroid) pair as
// s = |c|^2 - 2 x.c with v_mfma_f32_32x32x2_f32, keeps best, best list and runner-up per row in registers, and decides a
// row only when the gap clears the slack of sq_ivf_assign_plan.hpp; the others go to a list and are assigned by the sliced
// exact dense search as before, so the assignment is that search's bits for every input.  DESIGN.md 4.16.
#pragma once
#include <algorithm>

#include "sq_dense_exact.hpp"
#include "sq_ivf_assign_plan.hpp"
#include "sq_ivf_plan.hpp"

namespace sq {

// What an assignment call did: launches of ivf_assign_kernel, rows it decided, rows the exact path assigned.
struct IvfAssignStats {
    long long launches = 0, decided = 0, fallback = 0;
    bool timed = false;       // in: time ivf_assign_kernel with events (option "profile")
    double kernel_ms = 0.0;
    void into(sq_stats_t& s) const {
        s.scan_ms += kernel_ms;
        s.scan_launches += launches;
        s.candidates += decided;
        s.fallback_queries += fallback;
    }
};

// The device scratch of ivf_assign, kept by the caller over its calls (an IVF-PQ add makes m + 1 per block; k-means one per
// iteration): buffers only grow, and the caller waits for the stream before they go.
struct IvfAssignScratch {
    DevBuf nrm, stat, und;     // n_l [centroids padded to the block], {largest n_l, undecided count}, undecided row numbers [n]
    DevBuf rows, got, dist;    // the exact path: gathered rows, their lists, the distances nobody reads
};

// n_l = |c_l|^2: summed in float64 (every product is exact there), rounded to float32 once; +inf behind the last centroid,
// so a padded column never wins.  stat[0]: the largest n_l as float32 bits -- of non-negative floats the unsigned order is
// the numeric one, and a NaN's bits lie above +inf's, so one bad centroid makes every slack of the call NaN.
static __global__ __launch_bounds__(256) void ivf_assign_norm_kernel(const float* __restrict__ c, long long ldc, int d, int nlist, int n_pad,
                                                                      float* __restrict__ nrm, u32* __restrict__ stat) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= n_pad) return;
    if (l >= nlist) {
        nrm[l] = __builtin_inff();
        return;
    }
    double acc = 0.0;
    for (int i = 0; i < d; ++i) {
        const double v = (double)c[(long long)l * ldc + i];
        acc = __dadd_rn(acc, __dmul_rn(v, v));
    }
    const float nl = (float)acc;
    nrm[l] = nl;
    atomicMax(stat, __float_as_uint(nl) & 0x7fffffffu);
}

// Elements k .. k + 3 of the row that starts `off` floats into p; zeros for a missing row and for elements behind d.
// VEC: off % 4 == 0, p 16-byte aligned and the row's stride at least d rounded up to 4, so the 16 bytes are the row's own.
template <bool VEC>
__device__ __forceinline__ f32x4 asg_piece(const float* __restrict__ p, long long off, int k, int d, bool row_ok) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!row_ok || k >= d) return v;
    if constexpr (VEC) {
        v = *reinterpret_cast<const f32x4*>(p + off + k);
#pragma unroll
        for (int e = 1; e < 4; ++e)
            if (k + e >= d) v[e] = 0.f;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k + e < d) v[e] = p[off + k + e];
    }
    return v;
}

// Workgroup b: row tiles b, b + gridDim.x, ... of 128 rows each; wave w owns rows 32 w .. + 31 of the tile for the whole
// centroid loop.  The centroids are the M operand and the rows the N operand of the 32 x 32 x 2 instruction: lane l then
// holds, of row l % 32, the scores of centroids 8 (v / 4) + 4 (l / 32) + v % 4 (v < 16) of each of the block's four
// 32-centroid tiles -- 64 accumulators -- and the running best, its list and the runner-up never leave the lane; lanes l and
// l + 32 are merged once per row tile.
// LDS: the row tile ([128][sx]; RES: whole, staged once per tile; else two k slabs of it), then two slabs [128][sc] of the
// centroid block.  The steps (centroid block, k slab) run as one sequence: step t + 2's global loads are issued into
// registers before step t's MFMAs, stored into the buffer step t + 1 reads at the top of step t, one barrier per step.
// Operand reads and the k slots of the two lane halves: as opq_apply_kernel (sq_opq.hip).
// stat[0]: the norm kernel's largest n_l; stat[1]: the undecided rows' counter; und: their row numbers, any order.
template <bool VEC, bool RES>
static __global__ __launch_bounds__(256) void ivf_assign_kernel(const float* __restrict__ c, long long ldc, int cvec, const float* __restrict__ nrm,
                                                                 int nlist, const float* __restrict__ x, long long n, int d, int sx, int sc,
                                                                 int nslab, int ncb, int x_floats, long long* __restrict__ assign,
                                                                 u32* __restrict__ stat, u32* __restrict__ und) {
    extern __shared__ __attribute__((aligned(16))) float s_asg[];
    float* Xs = s_asg;
    float* Cs = s_asg + x_floats;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, h = lane >> 5;
    const int sr = tid >> 3, sk = (tid & 7) * 4;   // staging of a slab: 8 lanes per row of 32 k, 32 rows per 256 lanes
    const long long tiles = (n + kAsgTileRows - 1) / kAsgTileRows;
    const int total = ncb * nslab;
    const int xbuf = kAsgTileRows * sx, cbuf = kAsgColBlock * sc;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long row0 = tile * kAsgTileRows;
        if constexpr (RES) {   // (the previous tile's last operand reads are behind its last barrier)
            const int pieces = (sx - 4) / 4;   // 16-byte pieces of a staged row: d rounded up to the k step
            for (int idx = tid; idx < kAsgTileRows * pieces; idx += 256) {
                const int r = idx / pieces, p = idx - r * pieces;
                const long long row = row0 + r;
                *reinterpret_cast<f32x4*>(Xs + r * sx + 4 * p) = asg_piece<VEC>(x, row * d, 4 * p, d, row < n);
            }
        }
        f32x4 pc[4], px[4];
        auto fetch = [&](int t) {
            const int cb = t / nslab, k = (t - cb * nslab) * kAsgSlabK + sk;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int l = cb * kAsgColBlock + sr + 32 * u;
                pc[u] = cvec ? asg_piece<true>(c, (long long)l * ldc, k, d, l < nlist) : asg_piece<false>(c, (long long)l * ldc, k, d, l < nlist);
                if constexpr (!RES) {
                    const long long row = row0 + sr + 32 * u;
                    px[u] = asg_piece<VEC>(x, row * d, k, d, row < n);
                }
            }
        };
        auto store = [&](int t) {
            float* cs = Cs + (t & 1) * cbuf;
#pragma unroll
            for (int u = 0; u < 4; ++u) *reinterpret_cast<f32x4*>(cs + (sr + 32 * u) * sc + sk) = pc[u];
            if constexpr (!RES) {
                float* xs = Xs + (t & 1) * xbuf;
#pragma unroll
                for (int u = 0; u < 4; ++u) *reinterpret_cast<f32x4*>(xs + (sr + 32 * u) * sx + sk) = px[u];
            }
        };
        fetch(0);
        store(0);
        if (total > 1) fetch(1);
        __syncthreads();
        f32x16 acc[4];
        float best = __builtin_inff(), second = __builtin_inff(), xn2 = 0.f;
        int best_l = 0;
        for (int t = 0; t < total; ++t) {
            const int cb = t / nslab, s = t - cb * nslab;
            if (t + 1 < total) store(t + 1);   // into the buffer step t - 1 read, behind that step's barrier
            if (t + 2 < total) fetch(t + 2);
            if (s == 0) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int v = 0; v < 16; ++v) acc[j][v] = 0.f;
            }
            const int left_l = nlist - cb * kAsgColBlock;            // centroids from this block on
            const int nj = left_l >= kAsgColBlock ? 4 : (left_l + 31) / 32;   // 32-centroid tiles of the block that hold one
            const int left = d - s * kAsgSlabK;
            const int steps = ((left < kAsgSlabK ? left : kAsgSlabK) + kAsgKStep - 1) / kAsgKStep;   // asg_slab_steps
            const float* xr = Xs + (RES ? s * kAsgSlabK : (t & 1) * xbuf) + (wave * 32 + l32) * sx + 4 * h;
            const float* cr = Cs + (t & 1) * cbuf + l32 * sc + 4 * h;
            for (int kk = 0; kk < steps; ++kk) {
                const f32x4 xv = *reinterpret_cast<const f32x4*>(xr + kk * kAsgKStep);
                if (cb == 0) xn2 += (xv[0] * xv[0] + xv[1] * xv[1]) + (xv[2] * xv[2] + xv[3] * xv[3]);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (j < nj) {
                        const f32x4 cv = *reinterpret_cast<const f32x4*>(cr + j * 32 * sc + kk * kAsgKStep);
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(cv[e], xv[e], acc[j], 0, 0, 0);
                    }
                }
            }
            if (s == nslab - 1) {   // the block's scores, lists ascending: an equal score never replaces the best
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (j < nj) {
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const int l0 = cb * kAsgColBlock + j * 32 + 8 * g + 4 * h;
                            const f32x4 nl = *reinterpret_cast<const f32x4*>(nrm + l0);
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const float sv = __fsub_rn(nl[e], __fmul_rn(2.f, acc[j][4 * g + e]));
                                if (sv < best) {
                                    second = best;
                                    best = sv;
                                    best_l = l0 + e;
                                } else if (sv < second) {
                                    second = sv;
                                }
                            }
                        }
                    }
                }
            }
            __syncthreads();
        }
        // the two halves of a row: the smaller best (equal: the lower list), the runner-up of all the rest
        const float ob = __shfl_xor(best, 32), os = __shfl_xor(second, 32), oxn = __shfl_xor(xn2, 32);
        const int ol = __shfl_xor(best_l, 32);
        const bool take = ob < best || (ob == best && ol < best_l);
        const float loser = take ? best : ob;
        float runner = second < os ? second : os;
        runner = loser < runner ? loser : runner;
        if (take) best = ob, best_l = ol;
        const long long row = row0 + wave * 32 + l32;
        if (h == 0 && row < n) {
            const float T = ivf_assign_slack(d, xn2 + oxn, __uint_as_float(stat[0]));
            // (NaN or +inf anywhere -- the row, a centroid, an overflow -- makes one side of this false)
            if (__fsub_rn(runner, best) > T && fabsf(best) <= 3.0e38f) assign[row] = best_l;
            else und[atomicAdd(&stat[1], 1u)] = (u32)row;
        }
    }
}

// the undecided rows, contiguous (one thread per element), and their lists back to their places
static __global__ __launch_bounds__(256) void ivf_assign_gather_kernel(const float* __restrict__ x, int d, const u32* __restrict__ und, long long cnt,
                                                                        float* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < cnt * d; i += (long long)gridDim.x * 256) {
        const long long j = i / d;
        out[i] = x[(long long)und[j] * d + (i - j * d)];
    }
}
static __global__ __launch_bounds__(256) void ivf_assign_scatter_kernel(const long long* __restrict__ got, const u32* __restrict__ und, long long cnt,
                                                                         long long* __restrict__ assign) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j < cnt) assign[und[j]] = got[j];
}

// the present path: exact keys of every centroid and a select, kIvfAssignSlice rows per call
static int ivf_assign_exact(sq_handle_t coarse, const float* x, long long n, int d, long long* assign, float* dist, hipStream_t st) {
    for (long long s = 0; s < n; s += kIvfAssignSlice) {
        const int m = (int)std::min<long long>(kIvfAssignSlice, n - s);
        SQ_TRY(sq_dense_search(coarse, x + s * d, m, 1, dist + s, reinterpret_cast<int64_t*>(assign + s), SQ_MEM_DEVICE, st));
    }
    return SQ_OK;
}

template <bool VEC, bool RES>
static int ivf_assign_launch(const AsgPlan& p, int device, const float* c, long long ldc, const float* nrm, const float* x, long long n,
                             long long* assign, u32* stat, u32* und, hipStream_t st) {
    const int cvec = ldc % 4 == 0 && reinterpret_cast<uintptr_t>(c) % 16 == 0;
    const dim3 grid(asg_grid(asg_tiles(n), cu_count(device)));
    return launch_lds<ivf_assign_kernel<VEC, RES>>(kAsgLdsMax, grid, dim3(256), (size_t)p.lds_bytes, st, c, ldc, cvec, nrm, p.nlist, x, n, p.d,
                                                   p.sx, p.sc, p.nslab, p.ncb, p.x_floats, assign, stat, und);
}

// Nearest centroid of n rows (device, row stride d) into assign[n].  `mode` is option "ivf_assign": 1 = ivf_assign_kernel
// where ivf_assign_route covers the call, the exact path for the rows it leaves undecided; 0 = the exact path for all.
// Enqueued on `st`; a routed call waits once, for the undecided count.  `w` must outlive the stream's work.
static int ivf_assign(sq_handle_t coarse, const float* x, long long n, int d, long long* assign, hipStream_t st, int mode,
                      IvfAssignScratch& w, IvfAssignStats* stats = nullptr) {
    const float* c = nullptr;
    long long ldc = 0, nlist = 0;
    int cd = 0;
    HandleBase* ch = lookup_handle(coarse, H_DENSE);
    if (!ch) return fail(SQ_ERR_INVALID, "ivf_assign: unknown coarse index");
    const bool routed = mode != 0 && ch->dense_matrix(&c, &ldc, &nlist, &cd) && cd == d && ivf_assign_route(n, d, (int)nlist);
    DevBuf &nrm = w.nrm, &stat = w.stat, &und = w.und, &rows = w.rows, &got = w.got, &dist = w.dist;
    if (!routed) {
        SQ_TRY(dist.reserve((size_t)n * 4));
        SQ_TRY(ivf_assign_exact(coarse, x, n, d, assign, dist.as<float>(), st));
        if (stats) stats->fallback += n;
        return SQ_OK;
    }
    const AsgPlan p = asg_plan(d, (int)nlist);
    const int n_pad = p.ncb * kAsgColBlock;
    SQ_TRY(nrm.reserve((size_t)n_pad * 4));
    SQ_TRY(stat.reserve(64));
    SQ_TRY(und.reserve((size_t)n * 4));
    SQ_HIP(hipMemsetAsync(stat.p, 0, 8, st));
    SQ_TRY(launch<ivf_assign_norm_kernel>(dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, st, c, ldc, d, (int)nlist, n_pad, nrm.as<float>(),
                                          stat.as<u32>()));
    const bool vec = d % 4 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0;
    int device = 0;
    SQ_HIP(hipGetDevice(&device));
    struct Events {
        hipEvent_t e[2] = {nullptr, nullptr};
        ~Events() {
            for (auto& v : e)
                if (v) (void)hipEventDestroy(v);
        }
    } ev;
    const bool timed = stats && stats->timed;
    if (timed) {
        for (auto& v : ev.e) SQ_HIP(hipEventCreate(&v));
        SQ_HIP(hipEventRecord(ev.e[0], st));
    }
    if (vec && p.resident) SQ_TRY((ivf_assign_launch<true, true>(p, device, c, ldc, nrm.as<float>(), x, n, assign, stat.as<u32>(), und.as<u32>(), st)));
    else if (vec) SQ_TRY((ivf_assign_launch<true, false>(p, device, c, ldc, nrm.as<float>(), x, n, assign, stat.as<u32>(), und.as<u32>(), st)));
    else if (p.resident) SQ_TRY((ivf_assign_launch<false, true>(p, device, c, ldc, nrm.as<float>(), x, n, assign, stat.as<u32>(), und.as<u32>(), st)));
    else SQ_TRY((ivf_assign_launch<false, false>(p, device, c, ldc, nrm.as<float>(), x, n, assign, stat.as<u32>(), und.as<u32>(), st)));
    if (timed) SQ_HIP(hipEventRecord(ev.e[1], st));
    u32 host_stat[2] = {0, 0};
    SQ_HIP(hipMemcpyAsync(host_stat, stat.p, 8, hipMemcpyDeviceToHost, st));
    SQ_HIP(hipStreamSynchronize(st));
    if (timed) {
        float ms = 0.f;
        SQ_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        stats->kernel_ms += ms;
    }
    const long long cnt = host_stat[1];
    if (cnt > n) return fail(SQ_ERR_INTERNAL, "ivf_assign: %lld undecided rows of %lld", cnt, n);
    if (stats) stats->launches += 1, stats->decided += n - cnt, stats->fallback += cnt;
    if (cnt == 0) return SQ_OK;
    SQ_TRY(rows.reserve((size_t)cnt * d * 4));
    SQ_TRY(got.reserve((size_t)cnt * 8));
    SQ_TRY(dist.reserve((size_t)cnt * 4));
    const long long blocks = std::min<long long>((cnt * d + 255) / 256, 65536);
    SQ_TRY(launch<ivf_assign_gather_kernel>(dim3((unsigned)blocks), dim3(256), 0, st, x, d, und.as<u32>(), cnt, rows.as<float>()));
    SQ_TRY(ivf_assign_exact(coarse, rows.as<float>(), cnt, d, got.as<long long>(), dist.as<float>(), st));
    SQ_TRY(launch<ivf_assign_scatter_kernel>(dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, got.as<long long>(), und.as<u32>(), cnt, assign));
    return SQ_OK;
}

}  // namespace sq
