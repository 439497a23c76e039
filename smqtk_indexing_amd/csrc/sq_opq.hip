// The OPQ transform (include/smqtk_hip_opq.h): a d x d float32 matrix resident on the device and its product with a
// stream of rows, y = x . A^T, on the float32 matrix cores (gfx950).  The tile and slab arithmetic is sq_opq_plan.hpp's.
#include <chrono>
#include <vector>

#include "../../include/smqtk_hip_opq.h"
#include "sq_common.hpp"
#include "sq_opq_plan.hpp"

namespace sq {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

static_assert(SQ_OPQ_MAX_D == kOpqMaxD, "the header's limit");
static_assert(kOpqTileRows == 64 && kOpqColBlock == 128 && kOpqSlabK == 32 && kOpqKStep == 8, "opq_apply_kernel's wave layout and staging counts");

struct OpqHandle : HandleBase {
    OpqPlan plan;
    DevBuf A;                 // [d][lda] floats, zero padded
    DevBuf x_dev, y_dev;      // a host-memory call's rows and results
    PinnedStage stage;
    long long last_rows = 0, last_us = 0;
};

// Elements k .. k + 3 of the row that starts `off` floats into x; zeros for a row behind n and for elements behind d.
// VEC: d % 4 == 0 and x 16-byte aligned, so a piece is inside the row or wholly behind it.
template <bool VEC>
__device__ __forceinline__ f32x4 opq_row_piece(const float* __restrict__ x, long long off, int k, int d, bool row_ok) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!row_ok) return v;
    if constexpr (VEC) {
        if (k < d) v = *reinterpret_cast<const f32x4*>(x + off + k);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k + e < d) v[e] = x[off + k + e];
    }
    return v;
}

// Workgroup b: row tiles b, b + gridDim.x, ... of 64 rows each; four waves, wave w on rows 32 (w & 1) .. + 31 of the tile and
// columns 64 (w >> 1) .. + 63 of the current block of 128 -- two v_mfma_f32_32x32x2_f32 tiles, 32 accumulators.
// LDS: Xs [64][sx], As [128][sa] (opq_plan); both hold k contiguously, as both A's rows and x's do in memory.
// RES (d <= 512): Xs is the whole tile, staged once per tile; otherwise a 32-k slab of it, staged with every slab of A.
// The steps (column block, k slab) run as one sequence: step t + 1's global loads are issued into registers before step
// t's MFMAs and stored to LDS after them, between two barriers.
// Operand reads: lane l reads 16 bytes, k offsets 8 kk + 4 (l / 32) + 0 .. 3 of row l % 32, from each operand, and feeds
// element e of both to MFMA e: its two k slots are then k = 8 kk + e (lanes 0 .. 31) and 8 kk + 4 + e (32 .. 63) -- the
// same for both operands, and a sum does not care which slot a k sits in.
// Result layout of the instruction: lane l holds column l % 32 and rows 8 (v / 4) + 4 (l / 32) + v % 4, v < 16: a store
// instruction writes two runs of 32 consecutive floats.
template <bool VEC, bool RES>
static __global__ __launch_bounds__(256) void opq_apply_kernel(const float* __restrict__ A, int lda, const float* __restrict__ x,
                                                                float* __restrict__ y, long long n, int d, int sx, int sa, int nslab,
                                                                int ncb) {
    extern __shared__ __attribute__((aligned(16))) float s_opq[];
    float* Xs = s_opq;
    float* As = s_opq + kOpqTileRows * sx;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, h = lane >> 5;
    const int rh = wave & 1, ch = wave >> 1;
    const int sr = tid >> 3, sc = (tid & 7) * 4;   // staging of a slab: 8 lanes per row of 32 k, 32 rows per 256 lanes
    const long long tiles = (n + kOpqTileRows - 1) / kOpqTileRows;
    const int total = ncb * nslab;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long row0 = tile * kOpqTileRows;
        if constexpr (RES) {
            __syncthreads();   // the previous tile's last operand reads
            const int pieces = (sx - 4) / 4;   // 16-byte pieces of a staged row: d rounded up to the k step
            for (int idx = tid; idx < kOpqTileRows * pieces; idx += 256) {
                const int r = idx / pieces, c = idx - r * pieces;
                const long long row = row0 + r;
                *reinterpret_cast<f32x4*>(Xs + r * sx + 4 * c) = opq_row_piece<VEC>(x, row * d, 4 * c, d, row < n);
            }
        }
        f32x4 pa[4], px[2];
        auto fetch = [&](int t) {
            const int cb = t / nslab, k = (t - cb * nslab) * kOpqSlabK + sc;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int col = cb * kOpqColBlock + sr + 32 * u;
                pa[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (col < d && k < lda) pa[u] = *reinterpret_cast<const f32x4*>(A + (long long)col * lda + k);
            }
            if constexpr (!RES) {
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const long long row = row0 + sr + 32 * u;
                    px[u] = opq_row_piece<VEC>(x, row * d, k, d, row < n);
                }
            }
        };
        fetch(0);
        f32x16 acc0, acc1;
        for (int t = 0; t < total; ++t) {
            const int cb = t / nslab, s = t - cb * nslab;
            __syncthreads();   // step t - 1's operand reads
#pragma unroll
            for (int u = 0; u < 4; ++u) *reinterpret_cast<f32x4*>(As + (sr + 32 * u) * sa + sc) = pa[u];
            if constexpr (!RES) {
#pragma unroll
                for (int u = 0; u < 2; ++u) *reinterpret_cast<f32x4*>(Xs + (sr + 32 * u) * sx + sc) = px[u];
            }
            __syncthreads();
            if (t + 1 < total) fetch(t + 1);
            if (s == 0) {
#pragma unroll
                for (int v = 0; v < 16; ++v) acc0[v] = acc1[v] = 0.f;
            }
            const int col_w = cb * kOpqColBlock + ch * 64;   // this wave's first column
            const bool t0 = col_w < d, t1 = col_w + 32 < d;
            if (t0) {
                const int left = d - s * kOpqSlabK;
                const int steps = ((left < kOpqSlabK ? left : kOpqSlabK) + kOpqKStep - 1) / kOpqKStep;   // opq_slab_steps
                const float* xr = Xs + (rh * 32 + l32) * sx + (RES ? s * kOpqSlabK : 0) + 4 * h;
                const float* ar = As + (ch * 64 + l32) * sa + 4 * h;
                for (int kk = 0; kk < steps; ++kk) {
                    const f32x4 xv = *reinterpret_cast<const f32x4*>(xr + kk * kOpqKStep);
                    const f32x4 a0 = *reinterpret_cast<const f32x4*>(ar + kk * kOpqKStep);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[e], a0[e], acc0, 0, 0, 0);
                    if (t1) {
                        const f32x4 a1 = *reinterpret_cast<const f32x4*>(ar + 32 * sa + kk * kOpqKStep);
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[e], a1[e], acc1, 0, 0, 0);
                    }
                }
                if (s == nslab - 1) {
                    const int col = col_w + l32;
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        const long long row = row0 + rh * 32 + 8 * (v / 4) + 4 * h + (v % 4);
                        if (row < n) {
                            if (col < d) y[row * d + col] = acc0[v];
                            if (col + 32 < d) y[row * d + col + 32] = acc1[v];
                        }
                    }
                }
            }
        }
    }
}

template <bool VEC, bool RES>
static int opq_launch(const OpqHandle* h, const float* x, float* y, long long n, hipStream_t st) {
    const OpqPlan& p = h->plan;
    const dim3 grid(opq_grid(opq_tiles(n), cu_count(h->device)));
    return launch_lds<opq_apply_kernel<VEC, RES>>(kOpqLdsMax, grid, dim3(256), (size_t)p.lds_bytes, st, h->A.as<float>(), p.lda, x, y, n, p.d,
                                                  p.sx, p.sa, p.nslab, p.ncb);
}

// x and y in device memory; enqueued on `st`
static int opq_apply_device(OpqHandle* h, const float* x, float* y, long long n, hipStream_t st) {
    const bool prof = h->opt.profile != 0;
    if (prof) {
        for (int i = 0; i < 2; ++i)
            if (!h->ev[i]) SQ_HIP(hipEventCreate(&h->ev[i]));
        SQ_HIP(hipEventRecord(h->ev[0], st));
    }
    const bool vec = h->plan.d % 4 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0;
    if (vec && h->plan.resident) SQ_TRY(opq_launch<true, true>(h, x, y, n, st));
    else if (vec) SQ_TRY(opq_launch<true, false>(h, x, y, n, st));
    else if (h->plan.resident) SQ_TRY(opq_launch<false, true>(h, x, y, n, st));
    else SQ_TRY(opq_launch<false, false>(h, x, y, n, st));
    h->stats.scan_launches++;
    h->stats.bytes_scanned += n * h->plan.d * 4;
    if (prof) {
        SQ_HIP(hipEventRecord(h->ev[1], st));
        SQ_HIP(hipEventSynchronize(h->ev[1]));
        float ms = 0.f;
        SQ_HIP(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
        h->stats.scan_ms += ms;
    }
    return SQ_OK;
}

}  // namespace sq

using namespace sq;

extern "C" int sq_opq_create(const float* A, int d, sq_handle_t* out) {
    if (!out || !A || d < 1) return fail(SQ_ERR_INVALID, "sq_opq_create: bad argument");
    if (d > kOpqMaxD) return fail(SQ_ERR_UNSUPPORTED, "sq_opq_create: d = %d is beyond %d", d, kOpqMaxD);
    auto h = std::make_unique<OpqHandle>();
    h->kind = H_OPQ;
    h->plan = opq_plan(d);
    h->refresh_options();
    if (hipGetDevice(&h->device) != hipSuccess) return fail(SQ_ERR_HIP, "sq_opq_create: no HIP device");
    const int lda = h->plan.lda;
    std::vector<float> pad((size_t)d * lda, 0.f);
    for (int j = 0; j < d; ++j) memcpy(pad.data() + (size_t)j * lda, A + (size_t)j * d, (size_t)d * 4);
    SQ_TRY(h->A.alloc_exact(pad.size() * 4));
    SQ_HIP(hipMemcpy(h->A.p, pad.data(), pad.size() * 4, hipMemcpyHostToDevice));
    *out = register_handle(h.release());
    return SQ_OK;
}

extern "C" int sq_opq_apply(sq_handle_t hid, const float* x, int64_t n, float* y, int mem, void* stream) {
    if (mem != SQ_MEM_HOST && mem != SQ_MEM_DEVICE)
        return fail(SQ_ERR_UNSUPPORTED, "sq_opq_apply: rows in host or device memory only (SQ_MEM_HOST or SQ_MEM_DEVICE), not mode %d", mem);
    if (n < 0 || (n > 0 && (!x || !y))) return fail(SQ_ERR_INVALID, "sq_opq_apply: bad argument");
    if (x && x == y) return fail(SQ_ERR_INVALID, "sq_opq_apply: x and y must not overlap (equal pointers)");
    auto* h = static_cast<OpqHandle*>(lookup_handle(hid, H_OPQ));
    if (!h) return fail(SQ_ERR_INVALID, "sq_opq_apply: unknown handle");
    std::lock_guard<std::mutex> lock(h->mu);
    h->refresh_options();
    const size_t bytes = (size_t)n * h->plan.d * 4;
    const char *xb = reinterpret_cast<const char*>(x), *yb = reinterpret_cast<const char*>(y);
    if (n > 0 && xb < yb + bytes && yb < xb + bytes) return fail(SQ_ERR_INVALID, "sq_opq_apply: x and y must not overlap");
    const auto t_call = std::chrono::steady_clock::now();
    h->stats = sq_stats_t{};
    h->last_rows = n;
    h->last_us = 0;
    if (n == 0) return SQ_OK;
    SQ_HIP(hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (mem == SQ_MEM_HOST) {
        SQ_TRY(staged_call(h->stage, st, {{h->x_dev, x, bytes}}, {{y, h->y_dev, bytes}},
                           [&] { return opq_apply_device(h, h->x_dev.as<float>(), h->y_dev.as<float>(), n, st); }));
    } else {
        SQ_TRY(opq_apply_device(h, x, y, n, st));
    }
    const auto dt = std::chrono::steady_clock::now() - t_call;
    h->last_us = std::chrono::duration_cast<std::chrono::microseconds>(dt).count();
    if (h->opt.profile != 0) h->stats.total_ms = std::chrono::duration<double, std::milli>(dt).count();
    return SQ_OK;
}

extern "C" int sq_opq_info(sq_handle_t hid, int64_t* out, int n_out) {
    auto* h = static_cast<OpqHandle*>(lookup_handle(hid, H_OPQ));
    if (!h) return fail(SQ_ERR_INVALID, "sq_opq_info: unknown handle");
    if (!out || n_out < SQ_OPQ_INFO_FIELDS) return fail(SQ_ERR_INVALID, "sq_opq_info: room for %d values needed", SQ_OPQ_INFO_FIELDS);
    std::lock_guard<std::mutex> lock(h->mu);
    out[0] = h->plan.d;
    out[1] = (int64_t)(h->A.cap + h->x_dev.cap + h->y_dev.cap);
    out[2] = h->last_rows;
    out[3] = h->last_us;
    return SQ_OK;
}

extern "C" int sq_opq_destroy(sq_handle_t hid) {
    auto* h = remove_handle(hid, H_OPQ);
    if (!h) return fail(SQ_ERR_INVALID, "sq_opq_destroy: unknown handle");
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    delete h;
    return SQ_OK;
}
