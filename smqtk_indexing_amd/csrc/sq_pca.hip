// The PCA front stage (include/smqtk_hip_pca.h): the projection y = A (x - mean), d_out <= 512 <= d_in <= 8192, and the
// second moments its training needs, both on the float32 matrix cores (gfx950).  The tile, slab and chunk arithmetic is
// sq_pca_plan.hpp's.
#include <chrono>
#include <vector>

#include "../../include/smqtk_hip_pca.h"
#include "sq_common.hpp"
#include "sq_pca_plan.hpp"

namespace sq {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

static_assert(SQ_PCA_MAX_D_IN == kPcaMaxDin && SQ_PCA_MAX_D_OUT == kPcaMaxDout && SQ_PCA_RUN == kPcaRun, "the header's limits");
static_assert(kPcaSlabK == 32 && kPcaKStep == 8, "pca_apply_kernel's staging counts: 8 lanes x 16 bytes per slab row");
static_assert(kPcaTile == 128 && kPcaSlabRows == 32 && kPcaRun % kPcaSlabRows == 0 && kPcaSlabPitch >= kPcaTile,
              "pca_scatter_kernel's wave layout and staging counts");

struct PcaHandle : HandleBase {
    PcaPlan plan;
    DevBuf A;                 // [d_out][lda] floats, zero padded
    DevBuf mean;              // [lda] floats, zero padded
    DevBuf x_dev, y_dev;      // a host-memory call's rows and results
    PinnedStage stage;
    long long last_rows = 0, last_us = 0;
};

// ------------------------------------------------------------------------------------------------ apply
// Elements k .. k + 3 of the row that starts `off` floats into x, less the mean's; zeros for a row behind n and for
// elements behind d.  VEC: d % 4 == 0 and x 16-byte aligned, so a piece is inside the row or wholly behind it.
template <bool VEC>
__device__ __forceinline__ f32x4 pca_row_piece(const float* __restrict__ x, const float* __restrict__ mean, long long off, int k, int d,
                                               bool row_ok) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!row_ok) return v;
    if constexpr (VEC) {
        if (k < d) v = *reinterpret_cast<const f32x4*>(x + off + k) - *reinterpret_cast<const f32x4*>(mean + k);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k + e < d) v[e] = x[off + k + e] - mean[k + e];
    }
    return v;
}

// Workgroup b: row tiles b, b + gridDim.x, ... of T = 32 RW rows; four waves as RW row groups x CW = 4 / RW column groups,
// wave w on rows 32 (w % RW) .. + 31 of the tile and on the TPW column tiles (32 columns each) from CW-group w / RW on:
// TPW v_mfma_f32_32x32x2_f32 tiles, 16 TPW accumulators, alive from the first k slab to the last -- every output column of
// the tile is an accumulator somewhere in the workgroup, so a row of x is fetched once.
// LDS: Xs [T][36], As [32 CW TPW][36] (pca_plan); both hold k contiguously, as A's rows and x's do in memory.
// Slab s + 1's global loads (A and the centred rows) are issued into registers before slab s's MFMAs and stored to LDS
// after them, between two barriers.
// Operand reads: lane l reads 16 bytes, k offsets 8 kk + 4 (l / 32) + 0 .. 3 of row l % 32, from each operand, and feeds
// element e of both to MFMA e: its two k slots are then k = 8 kk + e (lanes 0 .. 31) and 8 kk + 4 + e (32 .. 63) -- the
// same for both operands, and a sum does not care which slot a k sits in.
// Result layout of the instruction: lane l holds column l % 32 and rows 8 (v / 4) + 4 (l / 32) + v % 4, v < 16.
template <bool VEC, int RW, int TPW>
static __global__ __launch_bounds__(256) void pca_apply_kernel(const float* __restrict__ A, int lda, const float* __restrict__ mean,
                                                                const float* __restrict__ x, float* __restrict__ y, long long n, int d_in,
                                                                int d_out, int nslab) {
    constexpr int CW = 4 / RW, T = 32 * RW, NA = CW * TPW, SX = kPcaSlabK + 4, SA = kPcaSlabK + 4;
    extern __shared__ __attribute__((aligned(16))) float s_pca[];
    float* Xs = s_pca;
    float* As = s_pca + T * SX;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, h = lane >> 5;
    const int rw = wave % RW, cw = wave / RW;
    const int sr = tid >> 3, sc = (tid & 7) * 4;   // staging of a slab: 8 lanes per row of 32 k, 32 rows per 256 lanes
    const long long tiles = (n + T - 1) / T;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long row0 = tile * T;
        f32x4 pa[NA], px[RW];
        auto fetch = [&](int s) {
            const int k = s * kPcaSlabK + sc;
#pragma unroll
            for (int u = 0; u < NA; ++u) {
                const int col = sr + 32 * u;
                pa[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (col < d_out && k < lda) pa[u] = *reinterpret_cast<const f32x4*>(A + (long long)col * lda + k);
            }
#pragma unroll
            for (int u = 0; u < RW; ++u) {
                const long long row = row0 + sr + 32 * u;
                px[u] = pca_row_piece<VEC>(x, mean, row * d_in, k, d_in, row < n);
            }
        };
        fetch(0);
        f32x16 acc[TPW];
#pragma unroll
        for (int t = 0; t < TPW; ++t)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;
        for (int s = 0; s < nslab; ++s) {
            __syncthreads();   // slab s - 1's operand reads (the previous tile's last, at s = 0)
#pragma unroll
            for (int u = 0; u < NA; ++u) *reinterpret_cast<f32x4*>(As + (sr + 32 * u) * SA + sc) = pa[u];
#pragma unroll
            for (int u = 0; u < RW; ++u) *reinterpret_cast<f32x4*>(Xs + (sr + 32 * u) * SX + sc) = px[u];
            __syncthreads();
            if (s + 1 < nslab) fetch(s + 1);
            const int left = d_in - s * kPcaSlabK;
            const int steps = ((left < kPcaSlabK ? left : kPcaSlabK) + kPcaKStep - 1) / kPcaKStep;   // pca_slab_steps
            const float* xr = Xs + (rw * 32 + l32) * SX + 4 * h;
            const float* ar = As + (cw * TPW * 32 + l32) * SA + 4 * h;
            for (int kk = 0; kk < steps; ++kk) {
                const f32x4 xv = *reinterpret_cast<const f32x4*>(xr + kk * kPcaKStep);
#pragma unroll
                for (int t = 0; t < TPW; ++t) {
                    if ((cw * TPW + t) * 32 < d_out) {   // (the same for every lane of the wave)
                        const f32x4 av = *reinterpret_cast<const f32x4*>(ar + t * 32 * SA + kk * kPcaKStep);
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[e], av[e], acc[t], 0, 0, 0);
                    }
                }
            }
        }
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
            const int col = (cw * TPW + t) * 32 + l32;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const long long row = row0 + rw * 32 + 8 * (v / 4) + 4 * h + (v % 4);
                if (row < n && col < d_out) y[row * d_out + col] = acc[t][v];
            }
        }
    }
}

template <bool VEC, int RW, int TPW>
static int pca_launch(const PcaHandle* h, const float* x, float* y, long long n, hipStream_t st) {
    const PcaPlan& p = h->plan;
    const dim3 grid(pca_grid(p, pca_tiles(p, n), cu_count(h->device)));
    return launch_lds<pca_apply_kernel<VEC, RW, TPW>>(kPcaLdsMax, grid, dim3(256), (size_t)p.lds_bytes, st, h->A.as<float>(), p.lda,
                                                      h->mean.as<float>(), x, y, n, p.d_in, p.d_out, p.nslab);
}

template <bool VEC>
static int pca_launch_by_plan(const PcaHandle* h, const float* x, float* y, long long n, hipStream_t st) {
    const PcaPlan& p = h->plan;
    if (p.rw == 4 && p.tpw == 1) return pca_launch<VEC, 4, 1>(h, x, y, n, st);
    if (p.rw == 2 && p.tpw == 1) return pca_launch<VEC, 2, 1>(h, x, y, n, st);
    if (p.rw == 2 && p.tpw == 2) return pca_launch<VEC, 2, 2>(h, x, y, n, st);
    if (p.rw == 2 && p.tpw == 4) return pca_launch<VEC, 2, 4>(h, x, y, n, st);
    if (p.rw == 2 && p.tpw == 8) return pca_launch<VEC, 2, 8>(h, x, y, n, st);
    return fail(SQ_ERR_UNSUPPORTED, "sq_pca_apply: no kernel for the plan (%d row groups, %d tiles per wave)", p.rw, p.tpw);
}

// x and y in device memory; enqueued on `st`
static int pca_apply_device(PcaHandle* h, const float* x, float* y, long long n, hipStream_t st) {
    const bool prof = h->opt.profile != 0;
    if (prof) {
        for (int i = 0; i < 2; ++i)
            if (!h->ev[i]) SQ_HIP(hipEventCreate(&h->ev[i]));
        SQ_HIP(hipEventRecord(h->ev[0], st));
    }
    const bool vec = h->plan.d_in % 4 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0;
    if (vec) SQ_TRY(pca_launch_by_plan<true>(h, x, y, n, st));
    else SQ_TRY(pca_launch_by_plan<false>(h, x, y, n, st));
    h->stats.scan_launches++;
    h->stats.bytes_scanned += n * h->plan.d_in * 4;
    if (prof) {
        SQ_HIP(hipEventRecord(h->ev[1], st));
        SQ_HIP(hipEventSynchronize(h->ev[1]));
        float ms = 0.f;
        SQ_HIP(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
        h->stats.scan_ms += ms;
    }
    return SQ_OK;
}

// ---------------------------------------------------------------------------------------------- moments
// Column sums in float64 by a fixed tree.  Workgroup (bx, chunk): columns 64 bx .. + 63 of rows [chunk rows, ...); lane
// group s = tid / 64 adds rows r0 + s, r0 + s + 4, ... of its column in order, the four groups are added as (0 + 1) + (2 + 3).
static __global__ __launch_bounds__(256) void pca_colsum_kernel(const float* __restrict__ x, long long n, int d, long long chunk_rows,
                                                                 double* __restrict__ part) {
    __shared__ double red[4][kPcaMeanCols];
    const int tid = threadIdx.x, cl = tid & (kPcaMeanCols - 1), s = tid / kPcaMeanCols;
    const int c = blockIdx.x * kPcaMeanCols + cl;
    const long long r0 = (long long)blockIdx.y * chunk_rows;
    const long long r1 = r0 + chunk_rows < n ? r0 + chunk_rows : n;
    double sum = 0.0;
    if (c < d)
        for (long long r = r0 + s; r < r1; r += 4) sum += (double)x[r * d + c];
    red[s][cl] = sum;
    __syncthreads();
    if (s == 0 && c < d) part[(long long)blockIdx.y * d + c] = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
}

// mean[c] = float32((chunk 0 + chunk 1 + ...) / n), c < d; zeros up to dpad
static __global__ __launch_bounds__(256) void pca_mean_kernel(const double* __restrict__ part, int chunks, int d, int dpad, long long n,
                                                               float* __restrict__ mean) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= dpad) return;
    double sum = 0.0;
    if (c < d)
        for (int k = 0; k < chunks; ++k) sum += part[(long long)k * d + c];
    mean[c] = c < d ? (float)(sum / (double)n) : 0.f;
}

// Workgroup (tile, chunk): tile (bi, bj), bi <= bj, of the upper triangle over rows [chunk rows, ...).  The product is
// Xc^T Xc: the MFMA's k runs over ROWS, so both operands are read along rows of the centred slab -- lane l takes column
// l % 32 of slab row 2 kk + l / 32 for the first operand (block bi: the tile's rows) and for the second (block bj: its
// columns).  Four waves, wave w on the 2 x 2 MFMA tiles at rows 64 (w & 1), columns 64 (w >> 1): two reads per operand
// feed four MFMAs.  On a diagonal tile both operands come from the one slab and the wave below the diagonal idles.
// Staging: thread t owns column t % 128 of both blocks (its two means live in registers) and rows t / 128 + 2 u, u < 16,
// of a slab; zeros behind d and behind the chunk.  Slab s + 1's loads are in flight under slab s's MFMAs.
// Every kPcaRun rows (32 slabs) and at the end the 64 float32 accumulators are folded into 64 float64 ones.
// part: [chunk][tile][128][128] float64; rows and columns behind d hold zeros.
static __global__ __launch_bounds__(256) void pca_scatter_kernel(const float* __restrict__ x, const float* __restrict__ mean, long long n,
                                                                  int d, int nb, long long chunk_rows, double* __restrict__ part) {
    __shared__ float Xi[kPcaSlabRows * kPcaSlabPitch];
    __shared__ float Xj[kPcaSlabRows * kPcaSlabPitch];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, h = lane >> 5;
    const int wi = wave & 1, wj = wave >> 1;
    int bi, bj;
    pca_tile_of((int)blockIdx.x, nb, &bi, &bj);
    const bool diag = bi == bj;
    const int c = tid & 127, rr = tid >> 7;
    const int ci = bi * kPcaTile + c, cj = bj * kPcaTile + c;
    const bool oki = ci < d, okj = !diag && cj < d;
    const float mi = oki ? mean[ci] : 0.f, mj = okj ? mean[cj] : 0.f;
    const long long r0 = (long long)blockIdx.y * chunk_rows;
    const long long r1 = r0 + chunk_rows < n ? r0 + chunk_rows : n;
    const int nsl = (int)((r1 - r0 + kPcaSlabRows - 1) / kPcaSlabRows);
    float pi[16], pj[16];
    auto fetch = [&](int sl) {
        const long long base = r0 + (long long)sl * kPcaSlabRows + rr;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const long long row = base + 2 * u;
            pi[u] = (oki && row < r1) ? x[row * d + ci] - mi : 0.f;
            pj[u] = (okj && row < r1) ? x[row * d + cj] - mj : 0.f;
        }
    };
    const float* Bs = diag ? Xi : Xj;
    const bool idle = diag && wi > wj;
    f32x16 acc[2][2];
    double dacc[2][2][16];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                acc[a][b][v] = 0.f;
                dacc[a][b][v] = 0.0;
            }
    if (nsl > 0) fetch(0);
    for (int sl = 0; sl < nsl; ++sl) {
        __syncthreads();   // slab sl - 1's operand reads
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            Xi[(rr + 2 * u) * kPcaSlabPitch + c] = pi[u];
            if (!diag) Xj[(rr + 2 * u) * kPcaSlabPitch + c] = pj[u];
        }
        __syncthreads();
        if (sl + 1 < nsl) fetch(sl + 1);
        if (!idle) {
            const float* ar = Xi + h * kPcaSlabPitch + wi * 64 + l32;
            const float* br = Bs + h * kPcaSlabPitch + wj * 64 + l32;
#pragma unroll 4
            for (int kk = 0; kk < kPcaSlabRows / 2; ++kk) {
                const float a0 = ar[2 * kk * kPcaSlabPitch], a1 = ar[2 * kk * kPcaSlabPitch + 32];
                const float b0 = br[2 * kk * kPcaSlabPitch], b1 = br[2 * kk * kPcaSlabPitch + 32];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
            }
            if ((sl + 1) % (kPcaRun / kPcaSlabRows) == 0 || sl + 1 == nsl) {
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b)
#pragma unroll
                        for (int v = 0; v < 16; ++v) {
                            dacc[a][b][v] += (double)acc[a][b][v];
                            acc[a][b][v] = 0.f;
                        }
            }
        }
    }
    if (idle) return;
    double* out = part + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * (kPcaTile * kPcaTile);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int i = wi * 64 + a * 32 + 8 * (v / 4) + 4 * h + (v % 4);
                const int j = wj * 64 + b * 32 + l32;
                out[i * kPcaTile + j] = dacc[a][b][v];
            }
}

// S[gi][gj] = S[gj][gi] = chunk 0's element + chunk 1's + ..., for the elements of the upper triangle inside d.  (Of a
// diagonal tile only i <= j is read: the part pca_scatter_kernel's idle wave never wrote lies below it.)
static __global__ __launch_bounds__(256) void pca_scatter_reduce_kernel(const double* __restrict__ part, int nchunks, int tiles, int nb, int d,
                                                                         double* __restrict__ S) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)tiles * kPcaTile * kPcaTile) return;
    const int tile = (int)(e / (kPcaTile * kPcaTile)), i = (int)(e / kPcaTile) % kPcaTile, j = (int)(e % kPcaTile);
    int bi, bj;
    pca_tile_of(tile, nb, &bi, &bj);
    const int gi = bi * kPcaTile + i, gj = bj * kPcaTile + j;
    if (gi >= d || gj >= d || (bi == bj && i > j)) return;
    double sum = 0.0;
    for (int k = 0; k < nchunks; ++k) sum += part[((long long)k * tiles + tile) * (kPcaTile * kPcaTile) + i * kPcaTile + j];
    S[(long long)gi * d + gj] = sum;
    S[(long long)gj * d + gi] = sum;
}

// x in device memory -> mean [dpad] float32 and S [d][d] float64 in device memory; blocking
static int pca_moments_device(const float* x, long long n, int d, int device, float* mean, int dpad, double* S) {
    const PcaMomentsPlan p = pca_moments_plan(n, d, cu_count(device));
    DevBuf colpart, part;
    SQ_TRY(colpart.alloc_exact((size_t)p.mean_chunks * d * 8));
    SQ_TRY(part.alloc_exact((size_t)p.nchunks * p.tiles * kPcaTile * kPcaTile * 8));
    hipStream_t st = nullptr;
    SQ_TRY(launch<pca_colsum_kernel>(dim3((d + kPcaMeanCols - 1) / kPcaMeanCols, p.mean_chunks), dim3(256), 0, st, x, n, d,
                                     p.mean_chunk_rows, colpart.as<double>()));
    SQ_TRY(launch<pca_mean_kernel>(dim3((dpad + 255) / 256), dim3(256), 0, st, colpart.as<double>(), p.mean_chunks, d, dpad, n, mean));
    SQ_TRY(launch<pca_scatter_kernel>(dim3(p.tiles, p.nchunks), dim3(256), 0, st, x, mean, n, d, p.nb, p.chunk_rows, part.as<double>()));
    const long long elems = (long long)p.tiles * kPcaTile * kPcaTile;
    SQ_TRY(launch<pca_scatter_reduce_kernel>(dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st, part.as<double>(), p.nchunks, p.tiles,
                                             p.nb, d, S));
    SQ_HIP(hipStreamSynchronize(st));
    return SQ_OK;
}

static bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const char *pa = static_cast<const char*>(a), *pb = static_cast<const char*>(b);
    return pa < pb + nb && pb < pa + na;
}

}  // namespace sq

using namespace sq;

extern "C" int sq_pca_moments(const float* x, int64_t n, int d, float* mean_out, double* scatter_out, int mem) {
    if (mem != SQ_MEM_HOST && mem != SQ_MEM_DEVICE)
        return fail(SQ_ERR_UNSUPPORTED, "sq_pca_moments: rows in host or device memory only (SQ_MEM_HOST or SQ_MEM_DEVICE), not mode %d", mem);
    if (!x || !mean_out || !scatter_out || d < 1) return fail(SQ_ERR_INVALID, "sq_pca_moments: bad argument");
    if (n < 2) return fail(SQ_ERR_INVALID, "sq_pca_moments: at least 2 rows needed, not %lld", (long long)n);
    if (d > kPcaMaxDin) return fail(SQ_ERR_UNSUPPORTED, "sq_pca_moments: d = %d is beyond %d", d, kPcaMaxDin);
    if (n > kPcaMaxN) return fail(SQ_ERR_UNSUPPORTED, "sq_pca_moments: n = %lld is beyond %lld rows; train on a sample", (long long)n, kPcaMaxN);
    const size_t xb = (size_t)n * d * 4, mb = (size_t)d * 4, sb = (size_t)d * d * 8;
    if (ranges_overlap(x, xb, mean_out, mb) || ranges_overlap(x, xb, scatter_out, sb) || ranges_overlap(mean_out, mb, scatter_out, sb))
        return fail(SQ_ERR_INVALID, "sq_pca_moments: x, mean_out and scatter_out must not overlap");
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return fail(SQ_ERR_HIP, "sq_pca_moments: no HIP device");
    const int dpad = (d + 3) / 4 * 4;
    DevBuf mean_dev, x_dev, s_dev;
    SQ_TRY(mean_dev.alloc_exact((size_t)dpad * 4));
    if (mem == SQ_MEM_DEVICE) {
        SQ_TRY(pca_moments_device(x, n, d, device, mean_dev.as<float>(), dpad, scatter_out));
        SQ_HIP(hipMemcpy(mean_out, mean_dev.p, mb, hipMemcpyDeviceToDevice));
        return SQ_OK;
    }
    SQ_TRY(x_dev.alloc_exact(xb));
    SQ_TRY(s_dev.alloc_exact(sb));
    SQ_HIP(hipMemcpy(x_dev.p, x, xb, hipMemcpyHostToDevice));
    SQ_TRY(pca_moments_device(x_dev.as<float>(), n, d, device, mean_dev.as<float>(), dpad, s_dev.as<double>()));
    SQ_HIP(hipMemcpy(mean_out, mean_dev.p, mb, hipMemcpyDeviceToHost));
    SQ_HIP(hipMemcpy(scatter_out, s_dev.p, sb, hipMemcpyDeviceToHost));
    return SQ_OK;
}

extern "C" int sq_pca_create(const float* A, const float* mean, int d_in, int d_out, sq_handle_t* out) {
    if (!out || !A || d_in < 1 || d_out < 1) return fail(SQ_ERR_INVALID, "sq_pca_create: bad argument");
    if (d_in > kPcaMaxDin) return fail(SQ_ERR_UNSUPPORTED, "sq_pca_create: d_in = %d is beyond %d", d_in, kPcaMaxDin);
    if (d_out > kPcaMaxDout) return fail(SQ_ERR_UNSUPPORTED, "sq_pca_create: d_out = %d is beyond %d", d_out, kPcaMaxDout);
    if (d_out > d_in) return fail(SQ_ERR_UNSUPPORTED, "sq_pca_create: d_out = %d is beyond d_in = %d: a projection does not widen", d_out, d_in);
    auto h = std::make_unique<PcaHandle>();
    h->kind = H_PCA;
    h->plan = pca_plan(d_in, d_out);
    h->refresh_options();
    if (hipGetDevice(&h->device) != hipSuccess) return fail(SQ_ERR_HIP, "sq_pca_create: no HIP device");
    const int lda = h->plan.lda;
    std::vector<float> pad((size_t)d_out * lda, 0.f), mpad((size_t)lda, 0.f);
    for (int j = 0; j < d_out; ++j) memcpy(pad.data() + (size_t)j * lda, A + (size_t)j * d_in, (size_t)d_in * 4);
    if (mean) memcpy(mpad.data(), mean, (size_t)d_in * 4);
    SQ_TRY(h->A.alloc_exact(pad.size() * 4));
    SQ_TRY(h->mean.alloc_exact(mpad.size() * 4));
    SQ_HIP(hipMemcpy(h->A.p, pad.data(), pad.size() * 4, hipMemcpyHostToDevice));
    SQ_HIP(hipMemcpy(h->mean.p, mpad.data(), mpad.size() * 4, hipMemcpyHostToDevice));
    *out = register_handle(h.release());
    return SQ_OK;
}

extern "C" int sq_pca_apply(sq_handle_t hid, const float* x, int64_t n, float* y, int mem, void* stream) {
    if (mem != SQ_MEM_HOST && mem != SQ_MEM_DEVICE)
        return fail(SQ_ERR_UNSUPPORTED, "sq_pca_apply: rows in host or device memory only (SQ_MEM_HOST or SQ_MEM_DEVICE), not mode %d", mem);
    if (n < 0 || (n > 0 && (!x || !y))) return fail(SQ_ERR_INVALID, "sq_pca_apply: bad argument");
    if (x && x == y) return fail(SQ_ERR_INVALID, "sq_pca_apply: x and y must not overlap (equal pointers)");
    auto* h = static_cast<PcaHandle*>(lookup_handle(hid, H_PCA));
    if (!h) return fail(SQ_ERR_INVALID, "sq_pca_apply: unknown handle");
    std::lock_guard<std::mutex> lock(h->mu);
    h->refresh_options();
    const size_t xbytes = (size_t)n * h->plan.d_in * 4, ybytes = (size_t)n * h->plan.d_out * 4;
    if (n > 0 && ranges_overlap(x, xbytes, y, ybytes)) return fail(SQ_ERR_INVALID, "sq_pca_apply: x and y must not overlap");
    const auto t_call = std::chrono::steady_clock::now();
    h->stats = sq_stats_t{};
    h->last_rows = n;
    h->last_us = 0;
    if (n == 0) return SQ_OK;
    SQ_HIP(hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (mem == SQ_MEM_HOST) {
        SQ_TRY(staged_call(h->stage, st, {{h->x_dev, x, xbytes}}, {{y, h->y_dev, ybytes}},
                           [&] { return pca_apply_device(h, h->x_dev.as<float>(), h->y_dev.as<float>(), n, st); }));
    } else {
        SQ_TRY(pca_apply_device(h, x, y, n, st));
    }
    const auto dt = std::chrono::steady_clock::now() - t_call;
    h->last_us = std::chrono::duration_cast<std::chrono::microseconds>(dt).count();
    if (h->opt.profile != 0) h->stats.total_ms = std::chrono::duration<double, std::milli>(dt).count();
    return SQ_OK;
}

extern "C" int sq_pca_info(sq_handle_t hid, int64_t* out, int n_out) {
    auto* h = static_cast<PcaHandle*>(lookup_handle(hid, H_PCA));
    if (!h) return fail(SQ_ERR_INVALID, "sq_pca_info: unknown handle");
    if (!out || n_out < SQ_PCA_INFO_FIELDS) return fail(SQ_ERR_INVALID, "sq_pca_info: room for %d values needed", SQ_PCA_INFO_FIELDS);
    std::lock_guard<std::mutex> lock(h->mu);
    out[0] = h->plan.d_in;
    out[1] = h->plan.d_out;
    out[2] = (int64_t)(h->A.cap + h->mean.cap + h->x_dev.cap + h->y_dev.cap);
    out[3] = h->last_rows;
    out[4] = h->last_us;
    out[5] = h->plan.tile_rows;
    out[6] = h->plan.blocks_per_cu;
    return SQ_OK;
}

extern "C" int sq_pca_destroy(sq_handle_t hid) {
    auto* h = remove_handle(hid, H_PCA);
    if (!h) return fail(SQ_ERR_INVALID, "sq_pca_destroy: unknown handle");
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    delete h;
    return SQ_OK;
}
