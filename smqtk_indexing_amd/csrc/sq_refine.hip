// The refine stage behind the inverted-list indexes: a store of all rows in id order, in a wider code than the lists',
// and the gather-decode-rerank of a coded index's candidates against it (gfx950).
//
// What FaissNearestNeighborsIndex reaches through the factory strings "IVFx,PQy,RFlat", "IVFx,PQy,Refine(SQfp16)" and
// "IVFx,PQy,Refine(SQ8)", stated against the oracle (include/smqtk_hip_refine.h): the base answers kb candidates, the
// store ranks them by metrics.euclidean_distance over the decoded row in numpy's order.  The codecs and the encoder are
// sq_isq_codec.hpp's, the tree walk sq_pairwise.hpp's, the select and its post-op sq_select.hpp's and sq_ivf_group.hpp's.
// New device code: the filter of a candidate list and the re-rank kernel in its two variants.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

#include "../../include/smqtk_hip_refine.h"
#include "sq_isq_codec.hpp"
#include "sq_ivf_group.hpp"

namespace sq {

typedef u32 u32x4 __attribute__((ext_vector_type(4)));

static_assert(SQ_REFINE_SQ8 == kCodecSq8 && SQ_REFINE_F16 == kCodecF16 && SQ_REFINE_F32 == kCodecF32, "the codec's kinds");

// ------------------------------------------------------------------ the plan of a re-rank workgroup
static constexpr int kRefineLdsMax = 160 * 1024;   // dynamic LDS a re-rank workgroup may ask for
static constexpr int kRefineTile = 32;             // candidates per workgroup: eight lanes each
static constexpr int kRefineSlabPieces = 64;       // 16-byte pieces of a row the tile holds at a time (1024 bytes)
static constexpr int kRefineLoads = kRefineTile * kRefineSlabPieces / 256;   // pieces a lane gathers per slab, at the most

// pieces of a row in LDS at a time: the whole row, or a slab of it
inline int refine_slab_pieces(long long stride) { return (int)std::min<long long>(stride / 16, kRefineSlabPieces); }
// The LDS pitch of a tile row, in bytes: the slab rounded up to 32 bytes, and 32 more when that is an even number of
// 32-byte units.  Bank arithmetic: in the sum phase the eight lanes of a candidate read 8 consecutive elements of one row
// -- 32, 16 or 8 contiguous bytes, at most 8 dwords from an address that is a multiple of their span -- and a wave holds 8
// candidates, rows r .. r + 7 of the tile, at the same column.  Row r starts (pitch / 4) * r dwords into the tile; with
// pitch / 32 odd that is 8 * odd * r, so the 8 rows start at the 8 distinct multiples of 8 modulo 64: their 8-dword
// spans cover the 64 banks once and no two lanes of a wave meet on a bank with different addresses.  (A pitch of 512 or
// 1024 bytes -- a d = 128 row of float32, or any full slab -- would put all 8 rows on the same 8 banks: eight-way.)
inline int refine_pitch(int slab_pieces) {
    const int p = (slab_pieces * 16 + 31) / 32 * 32;
    return (p / 32) % 2 ? p : p + 32;
}
// dynamic LDS: the tile's row numbers, the staged query (SQ8: with vmin and step), the tile
inline long long refine_stage_bytes(int d, int kind) { return (kind == SQ_REFINE_SQ8 ? 3 : 1) * ivf_row_stride(d) * 4; }
inline long long refine_lds_bytes(int d, int kind) {
    return kRefineTile * 4 + refine_stage_bytes(d, kind) + (long long)kRefineTile * refine_pitch(refine_slab_pieces(isq_row_stride(d, kind)));
}

struct RefineHandle : HandleBase {
    int d = 0, code_kind = SQ_REFINE_F32;
    long long ld = 0, stride = 0, n = 0, id_base = 0;   // round_up(d, 4); bytes per stored row
    DevBuf codes, params;                // [n][stride] bytes in id order; vmin[ld] then step[ld]
    long long add_us = 0;
    // scratch of a call
    DevBuf q_dev, cand_dev, cand_dist, rows, cnt, keys, out_keys, out_dist, out_idx, sort_tmp;
    std::vector<u32> cnt_host;
    PinnedStage stage;
};

// ------------------------------------------------------------------ the filter of the candidate lists
// Query q = blockIdx.x: the entries of cand[q][0 .. kb) inside [id_base, id_base + n) in their order, as row numbers, and
// how many they are.  No atomics: the same list gives the same order.
static __global__ __launch_bounds__(256) void refine_valid_kernel(const long long* __restrict__ cand, int kb, long long id_base,
                                                                   long long n, u32* __restrict__ rows, u32* __restrict__ cnt) {
    const int q = blockIdx.x;
    __shared__ u32 s_wave[4];
    __shared__ u32 s_run;
    if (threadIdx.x == 0) s_run = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int j0 = 0; j0 < kb; j0 += 256) {
        const int j = j0 + threadIdx.x;
        long long row = -1;
        if (j < kb) row = cand[(long long)q * kb + j] - id_base;   // (an id far below id_base wraps to a negative or huge row: invalid either way)
        const bool ok = j < kb && row >= 0 && row < n && cand[(long long)q * kb + j] >= id_base;
        u32 inc = ok ? 1u : 0u;  // inclusive scan inside the wave
        for (int o = 1; o < 64; o <<= 1) {
            const u32 t = __shfl_up(inc, o);
            if (lane >= o) inc += t;
        }
        if (lane == 63) s_wave[wv] = inc;
        __syncthreads();
        u32 base = s_run;
        for (int w = 0; w < wv; ++w) base += s_wave[w];
        if (ok) rows[(long long)q * kb + base + inc - 1] = (u32)row;
        __syncthreads();
        if (threadIdx.x == 0) s_run += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) cnt[q] = s_run;
}

// ------------------------------------------------------------------ the re-rank
// Element i of a code row whose byte 0 is at x, decoded, against the staged query: one term of the sum.
// LDS staging, SQ8: for dimensions 4g .. 4g + 3 the twelve floats q[4], vmin[4], step[4] at s[12 g] (isq_scan_kernel's
// layout); F16 / F32: the query, s[i] = q[i].
template <int KIND>
__device__ __forceinline__ float refine_term(const u8* x, const float* s, int i) {
    float xd, q;
    if constexpr (KIND == SQ_REFINE_SQ8) {
        const float* g = s + (i >> 2) * 12 + (i & 3);
        xd = isq_decode_sq8((float)x[i], g[4], g[8]);   // v_cvt_f32_ubyte0
        q = g[0];
    } else if constexpr (KIND == SQ_REFINE_F16) {
        xd = (float)reinterpret_cast<const _Float16*>(x)[i];   // v_cvt_f32_f16
        q = s[i];
    } else {
        xd = reinterpret_cast<const float*>(x)[i];
        q = s[i];
    }
    const float t = __fsub_rn(xd, q);
    return __fmul_rn(t, t);
}

// Work item (blockIdx.x, query): candidates [32 blockIdx.x, + 32) of the query's filtered list, eight lanes each.
// DIRECT = false: the tile's code rows are gathered into LDS first (refine_pitch: the layout), slab by slab where a row
// is wider than a slab; DIRECT = true: every lane reads its elements from global memory (rows_rerank_keys_kernel's shape).
// Both sum with pw_leaf under pw_tree -- lane j of a candidate is accumulator j of numpy's leaf -- so the bits agree.
// The walk over the tree depends on d alone: every lane of the workgroup asks for the same leaves in the same order, and
// the barriers around a slab's gather sit in uniform control flow.  Candidates behind the list's end repeat its last one
// for the loads and the sums and are dropped where the key is stored, so no cross-lane or LDS read depends on a lane
// that is switched off.
// Dynamic LDS: refine_lds_bytes(d, KIND).
template <int KIND, bool DIRECT>
static __global__ __launch_bounds__(256) void refine_rerank_kernel(const u8* __restrict__ codes, long long stride, int d, long long ld,
                                                                    const float* __restrict__ params, const float* __restrict__ queries,
                                                                    const u32* __restrict__ rows, const u32* __restrict__ cnt, int kb,
                                                                    int slab_pieces, int pitch, u64* __restrict__ keys) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    u32* s_rows = reinterpret_cast<u32*>(s_raw);
    float* s_stage = reinterpret_cast<float*>(s_raw + kRefineTile * 4);
    const int q = blockIdx.y;
    const int c = (int)cnt[q];
    const int base = blockIdx.x * kRefineTile;
    if (base >= c) return;
    if (threadIdx.x < kRefineTile) {
        const int p = base + threadIdx.x;
        s_rows[threadIdx.x] = rows[(long long)q * kb + (p < c ? p : c - 1)];
    }
    if constexpr (KIND == SQ_REFINE_SQ8) {
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
    const int g = threadIdx.x >> 3, j8 = threadIdx.x & 7;
    const long long row = s_rows[g];
    float sum;
    if constexpr (DIRECT) {
        const u8* x = codes + row * stride;
        auto term = [x, s_stage](int i) { return refine_term<KIND>(x, s_stage, i); };
        sum = np_pairwise_sum<float>(term, d, j8);
    } else {
        constexpr int CB = KIND == SQ_REFINE_F32 ? 4 : KIND == SQ_REFINE_F16 ? 2 : 1;
        unsigned char* s_tile = s_raw + kRefineTile * 4 + (KIND == SQ_REFINE_SQ8 ? 3 : 1) * ld * 4;
        const u32x4* src = reinterpret_cast<const u32x4*>(codes);
        const int pcs = (int)(stride / 16);
        int w0 = 0, wp = 0;   // the slab in LDS: pieces [w0, w0 + wp) of every row of the tile
        // the gather: piece t, t + 256, ... of the tile's slab; consecutive lanes take consecutive pieces of one row, and
        // a lane's loads are all issued before the first is stored
        auto gather = [&](int first) {
            w0 = first;
            wp = pcs - first < slab_pieces ? pcs - first : slab_pieces;
            const int total = kRefineTile * wp;
            u32x4 r[kRefineLoads];
#pragma unroll
            for (int u = 0; u < kRefineLoads; ++u) {
                const int idx = threadIdx.x + u * 256;
                if (idx < total) {
                    const int tr = idx / wp, tc = idx - tr * wp;
                    r[u] = __builtin_nontemporal_load(src + (long long)s_rows[tr] * pcs + w0 + tc);
                }
            }
#pragma unroll
            for (int u = 0; u < kRefineLoads; ++u) {
                const int idx = threadIdx.x + u * 256;
                if (idx < total) {
                    const int tr = idx / wp, tc = idx - tr * wp;
                    *reinterpret_cast<u32x4*>(s_tile + tr * pitch + tc * 16) = r[u];
                }
            }
        };
        gather(0);
        __syncthreads();
        const unsigned char* xrow = s_tile + g * pitch;
        auto leaf = [&](int off, int m) {
            if ((long long)(off + m) * CB > (long long)(w0 + wp) * 16) {   // the leaf reaches beyond the slab: the next slab starts at its first piece
                __syncthreads();
                gather(off * CB / 16);
                __syncthreads();
            }
            const u8* x = xrow - (long long)w0 * 16;   // byte 0 of the row, were all of it in LDS
            auto term = [x, s_stage](int i) { return refine_term<KIND>(x, s_stage, i); };
            return pw_leaf<float>(term, off, m, j8);
        };
        sum = pw_tree<float>(leaf, d);
    }
    const int p = base + g;
    if (j8 == 0 && p < c) keys[(long long)q * kb + p] = ((u64)ordered_f32(sqrt_rn_f32(sum)) << 32) | (u64)(u32)row;
}

template <int KIND, bool DIRECT>
static int refine_launch(RefineHandle* h, const float* q_dev, int nq, int kb, hipStream_t st) {
    const int sp = refine_slab_pieces(h->stride);
    const dim3 grid((unsigned)((kb + kRefineTile - 1) / kRefineTile), (unsigned)nq);
    const size_t lds = DIRECT ? (size_t)(kRefineTile * 4 + refine_stage_bytes(h->d, KIND)) : (size_t)refine_lds_bytes(h->d, KIND);
    return launch_lds<refine_rerank_kernel<KIND, DIRECT>>(kRefineLdsMax, grid, dim3(256), lds, st, h->codes.as<u8>(), h->stride, h->d, h->ld,
                                                          h->params.as<float>(), q_dev, h->rows.as<u32>(), h->cnt.as<u32>(), kb, sp,
                                                          refine_pitch(sp), h->keys.as<u64>());
}

// The re-rank with queries, candidates and outputs in device memory, enqueued on `st`; the select is not waited for.
static int refine_rerank_device(RefineHandle* h, const float* q_dev, int nq, const long long* cand, int kb, int k, float* od,
                                long long* oi, hipStream_t st) {
    const bool prof = h->opt.profile != 0;
    SQ_TRY(h->rows.reserve((size_t)nq * kb * 4));
    SQ_TRY(h->cnt.reserve((size_t)nq * 4));
    SQ_TRY(h->keys.reserve((size_t)nq * kb * 8));
    SQ_TRY(h->out_keys.reserve((size_t)nq * k * 8));
    SQ_TRY(launch<refine_valid_kernel>(dim3(nq), dim3(256), 0, st, cand, kb, h->id_base, h->n, h->rows.as<u32>(), h->cnt.as<u32>()));
    if (prof) {
        for (int i = 0; i < 2; ++i)
            if (!h->ev[i]) SQ_HIP(hipEventCreate(&h->ev[i]));
        SQ_HIP(hipEventRecord(h->ev[0], st));
    }
    const bool direct = h->opt.refine_direct < 0 ? h->code_kind == SQ_REFINE_SQ8 : h->opt.refine_direct != 0;   // (automatic: sq_common.hpp)
    switch (h->code_kind * 2 + (direct ? 1 : 0)) {
        case 0: SQ_TRY(refine_launch<SQ_REFINE_SQ8, false>(h, q_dev, nq, kb, st)); break;
        case 1: SQ_TRY(refine_launch<SQ_REFINE_SQ8, true>(h, q_dev, nq, kb, st)); break;
        case 2: SQ_TRY(refine_launch<SQ_REFINE_F16, false>(h, q_dev, nq, kb, st)); break;
        case 3: SQ_TRY(refine_launch<SQ_REFINE_F16, true>(h, q_dev, nq, kb, st)); break;
        case 4: SQ_TRY(refine_launch<SQ_REFINE_F32, false>(h, q_dev, nq, kb, st)); break;
        default: SQ_TRY(refine_launch<SQ_REFINE_F32, true>(h, q_dev, nq, kb, st)); break;
    }
    if (prof) {
        SQ_HIP(hipEventRecord(h->ev[1], st));
        SQ_HIP(hipEventSynchronize(h->ev[1]));
        float ms = 0.f;
        SQ_HIP(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
        h->stats.scan_ms += ms;
    }
    h->stats.scan_launches++;
    // keys (ordered distance, row number): ascending is (distance, id) order whatever the candidates' order was
    const IvfFinalize fin{0, k, h->id_base, od, oi};
    return select_launch_t<u64>(h->keys.as<u64>(), h->cnt.as<u32>(), (u32)kb, kb, k, nq, h->out_keys.as<u64>(), fin, st, h->sort_tmp);
}

// Queries a call takes at a time: the scratch of a slice -- candidate ids and distances, row numbers and keys, 24 kb bytes
// per query -- stays under the IVF searches' key budget (option "ivf_key_budget_mb", 256 MB), and a launch's grid.y under
// its limit.  Every slice is a complete call: filter, re-rank, select, its outputs at their place.
static int refine_slice_queries(const RefineHandle* h, int nq, int kb) {
    const long long budget = h->opt.ivf_key_budget_mb > 0 ? (long long)h->opt.ivf_key_budget_mb << 20 : kIvfKeyBudget;
    const long long fit = budget / (24ll * kb);
    return (int)std::max<long long>(1, std::min<long long>({(long long)nq, fit, 32768ll}));
}

// after the stream has drained: the valid candidates of the slice, added to the call's
static int refine_count(RefineHandle* h, int nq) {
    h->cnt_host.resize((size_t)nq);
    SQ_HIP(hipMemcpy(h->cnt_host.data(), h->cnt.p, (size_t)nq * 4, hipMemcpyDeviceToHost));
    long long total = 0;
    for (u32 c : h->cnt_host) total += c;
    h->stats.candidates += total;
    h->stats.bytes_scanned += total * h->stride;
    return SQ_OK;
}

static int refine_check_call(const char* who, const void* queries, const void* od, const void* oi, int nq, int k, int kb, int mem) {
    if (mem != SQ_MEM_HOST && mem != SQ_MEM_DEVICE)
        return fail(SQ_ERR_UNSUPPORTED, "%s: blocking calls only (SQ_MEM_HOST or SQ_MEM_DEVICE), not mode %d", who, mem);
    if (!queries || !od || !oi || nq <= 0 || k <= 0 || kb <= 0) return fail(SQ_ERR_INVALID, "%s: bad argument", who);
    if (kb < k) return fail(SQ_ERR_INVALID, "%s: %d candidates cannot answer k = %d", who, kb, k);
    return SQ_OK;
}

}  // namespace sq

using namespace sq;

extern "C" int sq_refine_create(int d, int kind, const float* vmin, const float* step, int64_t id_base, sq_handle_t* out) {
    if (!out || d <= 0) return fail(SQ_ERR_INVALID, "sq_refine_create: bad argument");
    if (kind != SQ_REFINE_SQ8 && kind != SQ_REFINE_F16 && kind != SQ_REFINE_F32)
        return fail(SQ_ERR_INVALID, "sq_refine_create: kind %d is none of SQ_REFINE_SQ8, SQ_REFINE_F16, SQ_REFINE_F32", kind);
    if (kind == SQ_REFINE_SQ8 && (!vmin || !step)) return fail(SQ_ERR_INVALID, "sq_refine_create: SQ8 needs vmin and step");
    if (kind != SQ_REFINE_SQ8 && (vmin || step)) return fail(SQ_ERR_INVALID, "sq_refine_create: F16 and F32 take no parameters (vmin and step must be NULL)");
    if (kind == SQ_REFINE_SQ8)
        for (int i = 0; i < d; ++i)
            if (!std::isfinite(vmin[i]) || !std::isfinite(step[i]) || step[i] < 0.f)
                return fail(SQ_ERR_INVALID, "sq_refine_create: vmin / step of dimension %d is not finite, or the step is negative", i);
    if (refine_lds_bytes(d, kind) > kRefineLdsMax)
        return fail(SQ_ERR_UNSUPPORTED, "sq_refine_create: rows of %d dimensions need %lld bytes of LDS, beyond a workgroup's %d", d,
                    refine_lds_bytes(d, kind), kRefineLdsMax);
    auto h = std::make_unique<RefineHandle>();
    h->kind = H_REFINE;
    h->code_kind = kind;
    h->d = d;
    h->ld = ivf_row_stride(d);
    h->stride = isq_row_stride(d, kind);
    h->id_base = id_base;
    h->refresh_options();
    if (hipGetDevice(&h->device) != hipSuccess) return fail(SQ_ERR_HIP, "sq_refine_create: no HIP device");
    std::vector<float> par((size_t)2 * h->ld, 0.f);   // F16 / F32 keep the (unused) zeros: one kernel signature
    if (kind == SQ_REFINE_SQ8) {
        std::copy(vmin, vmin + d, par.begin());
        std::copy(step, step + d, par.begin() + h->ld);
    }
    SQ_TRY(ivf_alloc(h->params, par.size() * 4));
    SQ_HIP(hipMemcpy(h->params.p, par.data(), par.size() * 4, hipMemcpyHostToDevice));
    *out = register_handle(h.release());
    return SQ_OK;
}

extern "C" int sq_refine_add(sq_handle_t hid, const float* rows, int64_t n_add, int mem) {
    if (mem != SQ_MEM_HOST && mem != SQ_MEM_DEVICE) return fail(SQ_ERR_UNSUPPORTED, "sq_refine_add: rows in host or device memory only");
    auto* h = static_cast<RefineHandle*>(lookup_handle(hid, H_REFINE));
    if (!h) return fail(SQ_ERR_INVALID, "sq_refine_add: unknown handle");
    if (!rows || n_add <= 0) return fail(SQ_ERR_INVALID, "sq_refine_add: bad argument");
    std::lock_guard<std::mutex> lock(h->mu);
    h->refresh_options();
    if (!ivf_rows_ok(h->n + n_add)) return fail(SQ_ERR_UNSUPPORTED, "sq_refine_add: more than 2^32-1 rows");
    SQ_HIP(hipSetDevice(h->device));
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t st = nullptr;
    const float* src = rows;
    DevBuf up;
    if (mem != SQ_MEM_DEVICE) {
        SQ_TRY(ivf_alloc(up, (size_t)n_add * h->d * 4));
        SQ_HIP(hipMemcpy(up.p, rows, (size_t)n_add * h->d * 4, hipMemcpyHostToDevice));
        src = up.as<float>();
    }
    // nothing of the handle changes before the buffer has grown, so a failed allocation leaves the store as it was
    const size_t used = (size_t)h->n * h->stride, need = (size_t)(h->n + n_add) * h->stride;
    if (const int rc = grow_keep(h->codes, used, need); rc != SQ_OK) {   // (its own message and code stand)
        (void)hipGetLastError();
        return rc;
    }
    const long long wpr = h->stride / 4, total = n_add * wpr;
    const dim3 grid((unsigned)std::min<long long>((total + 255) / 256, 1ll << 20));
    u32* dst = reinterpret_cast<u32*>(h->codes.as<u8>() + used);
    const float* vmin = h->params.as<float>();
    if (h->code_kind == SQ_REFINE_SQ8) SQ_TRY(launch<isq_encode_kernel<kCodecSq8>>(grid, dim3(256), 0, st, src, h->d, (long long)n_add, vmin, vmin + h->ld, wpr, dst));
    else if (h->code_kind == SQ_REFINE_F16) SQ_TRY(launch<isq_encode_kernel<kCodecF16>>(grid, dim3(256), 0, st, src, h->d, (long long)n_add, vmin, vmin, wpr, dst));
    else SQ_TRY(launch<isq_encode_kernel<kCodecF32>>(grid, dim3(256), 0, st, src, h->d, (long long)n_add, vmin, vmin, wpr, dst));
    SQ_HIP(hipStreamSynchronize(st));
    h->n += n_add;
    h->add_us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    return SQ_OK;
}

extern "C" int sq_refine_rows(sq_handle_t hid, int64_t first, int64_t n, void* codes) {
    auto* h = static_cast<RefineHandle*>(lookup_handle(hid, H_REFINE));
    if (!h) return fail(SQ_ERR_INVALID, "sq_refine_rows: unknown handle");
    std::lock_guard<std::mutex> lock(h->mu);
    if (first < 0 || n < 0 || first + n > h->n || (n > 0 && !codes)) return fail(SQ_ERR_INVALID, "sq_refine_rows: rows [%lld, + %lld) of %lld", (long long)first, (long long)n, h->n);
    if (n == 0) return SQ_OK;
    SQ_HIP(hipSetDevice(h->device));
    const size_t row = (size_t)h->d * isq_code_bytes(h->code_kind);
    std::vector<u8> tmp((size_t)n * h->stride);
    SQ_HIP(hipMemcpy(tmp.data(), h->codes.as<u8>() + (size_t)first * h->stride, tmp.size(), hipMemcpyDeviceToHost));
    for (long long i = 0; i < n; ++i) memcpy(static_cast<u8*>(codes) + (size_t)i * row, tmp.data() + (size_t)i * h->stride, row);
    return SQ_OK;
}

extern "C" int sq_refine_info(sq_handle_t hid, int64_t* out, int n_out) {
    auto* h = static_cast<RefineHandle*>(lookup_handle(hid, H_REFINE));
    if (!h) return fail(SQ_ERR_INVALID, "sq_refine_info: unknown handle");
    if (!out || n_out < SQ_REFINE_INFO_FIELDS) return fail(SQ_ERR_INVALID, "sq_refine_info: room for %d values needed", SQ_REFINE_INFO_FIELDS);
    std::lock_guard<std::mutex> lock(h->mu);
    out[0] = h->n;
    out[1] = h->d;
    out[2] = h->code_kind;
    out[3] = h->stride;
    out[4] = h->n * h->stride;          // the code rows in use (the buffer grows ahead of them)
    out[5] = (int64_t)h->params.cap;
    out[6] = h->add_us;
    return SQ_OK;
}

extern "C" int sq_refine_rerank(sq_handle_t hid, const float* queries, int nq, const int64_t* cand, int kb, int k, float* out_dist,
                                int64_t* out_idx, int mem, void* stream) {
    SQ_TRY(refine_check_call("sq_refine_rerank", queries, out_dist, out_idx, nq, k, kb, mem));
    if (!cand) return fail(SQ_ERR_INVALID, "sq_refine_rerank: bad argument");
    auto* h = static_cast<RefineHandle*>(lookup_handle(hid, H_REFINE));
    if (!h) return fail(SQ_ERR_INVALID, "sq_refine_rerank: unknown handle");
    std::lock_guard<std::mutex> lock(h->mu);
    h->refresh_options();
    SQ_HIP(hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const auto t_call = std::chrono::steady_clock::now();
    h->stats = sq_stats_t{};
    const int slice = refine_slice_queries(h, nq, kb);
    for (int q0 = 0; q0 < nq; q0 += slice) {
        const int m = nq - q0 < slice ? nq - q0 : slice;
        const float* qs = queries + (size_t)q0 * h->d;
        const int64_t* cs = cand + (size_t)q0 * kb;
        float* od = out_dist + (size_t)q0 * k;
        int64_t* oi = out_idx + (size_t)q0 * k;
        if (mem == SQ_MEM_HOST) {
            SQ_TRY(staged_call(h->stage, st, {{h->q_dev, qs, (size_t)m * h->d * 4}, {h->cand_dev, cs, (size_t)m * kb * 8}},
                               {{od, h->out_dist, (size_t)m * k * 4}, {oi, h->out_idx, (size_t)m * k * 8}}, [&] {
                                   return refine_rerank_device(h, h->q_dev.as<float>(), m, h->cand_dev.as<long long>(), kb, k,
                                                               h->out_dist.as<float>(), h->out_idx.as<long long>(), st);
                               }));
        } else {
            SQ_TRY(refine_rerank_device(h, qs, m, reinterpret_cast<const long long*>(cs), kb, k, od, reinterpret_cast<long long*>(oi), st));
            SQ_HIP(stream_wait(st));
        }
        SQ_TRY(refine_count(h, m));
    }
    if (h->opt.profile != 0) h->stats.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
    return SQ_OK;
}

extern "C" int sq_refine_search(sq_handle_t hid, sq_handle_t base, const float* queries, int nq, int k, int kb, int nprobe,
                                float* out_dist, int64_t* out_idx, int mem, void* stream) {
    SQ_TRY(refine_check_call("sq_refine_search", queries, out_dist, out_idx, nq, k, kb, mem));
    if (nprobe < 1) return fail(SQ_ERR_INVALID, "sq_refine_search: bad argument");
    auto* h = static_cast<RefineHandle*>(lookup_handle(hid, H_REFINE));
    if (!h) return fail(SQ_ERR_INVALID, "sq_refine_search: unknown handle");
    int base_kind = 0;
    HandleBase* b = nullptr;
    for (int kind : {H_IVF, H_PQ, H_ISQ})
        if (!b && (b = lookup_handle(base, kind))) base_kind = kind;
    int bd = 0;
    long long bn = 0, bid = 0;
    if (!b || !b->list_shape(&bd, &bn, &bid))
        return fail(SQ_ERR_UNSUPPORTED, "sq_refine_search: the base must be an IVF-Flat, IVF-PQ or IVF-SQ handle");
    std::lock_guard<std::mutex> lock(h->mu);
    h->refresh_options();
    if (bd != h->d || bn != h->n || bid != h->id_base)
        return fail(SQ_ERR_INVALID, "sq_refine_search: the base holds %lld rows of %d dimensions from id %lld, the store %lld of %d from %lld", bn,
                    bd, bid, h->n, h->d, h->id_base);
    SQ_HIP(hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const auto t_call = std::chrono::steady_clock::now();
    h->stats = sq_stats_t{};
    // the base's blocking device call leaves its kb candidates in this handle's scratch; the re-rank follows on the stream
    auto run = [&](const float* q_dev, int nq, float* od, long long* oi) -> int {   // (nq: the slice's)
        SQ_TRY(h->cand_dist.reserve((size_t)nq * kb * 4));
        SQ_TRY(h->cand_dev.reserve((size_t)nq * kb * 8));
        float* cd = h->cand_dist.as<float>();
        int64_t* ci = h->cand_dev.as<int64_t>();
        if (base_kind == H_IVF) SQ_TRY(sq_ivf_search(base, q_dev, nq, kb, nprobe, cd, ci, SQ_MEM_DEVICE, st));
        else if (base_kind == H_PQ) SQ_TRY(sq_pq_search(base, q_dev, nq, kb, nprobe, cd, ci, SQ_MEM_DEVICE, st));
        else SQ_TRY(sq_isq_search(base, q_dev, nq, kb, nprobe, cd, ci, SQ_MEM_DEVICE, st));
        // the base may have been added to since the check above (its lock is its own search's): what it answered is
        // re-ranked only if it still is the index the store mirrors.  Ids beyond the store are skipped in any case.
        if (!b->list_shape(&bd, &bn, &bid) || bd != h->d || bn != h->n || bid != h->id_base)
            return fail(SQ_ERR_INVALID, "sq_refine_search: the base changed during the call");
        return refine_rerank_device(h, q_dev, nq, h->cand_dev.as<long long>(), kb, k, od, oi, st);
    };
    const int slice = refine_slice_queries(h, nq, kb);
    for (int q0 = 0; q0 < nq; q0 += slice) {
        const int m = nq - q0 < slice ? nq - q0 : slice;
        const float* qs = queries + (size_t)q0 * h->d;
        float* od = out_dist + (size_t)q0 * k;
        int64_t* oi = out_idx + (size_t)q0 * k;
        if (mem == SQ_MEM_HOST) {
            SQ_TRY(staged_call(h->stage, st, {{h->q_dev, qs, (size_t)m * h->d * 4}},
                               {{od, h->out_dist, (size_t)m * k * 4}, {oi, h->out_idx, (size_t)m * k * 8}},
                               [&] { return run(h->q_dev.as<float>(), m, h->out_dist.as<float>(), h->out_idx.as<long long>()); }));
        } else {
            SQ_TRY(run(qs, m, od, reinterpret_cast<long long*>(oi)));
            SQ_HIP(stream_wait(st));
        }
        SQ_TRY(refine_count(h, m));
    }
    if (h->opt.profile != 0) h->stats.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
    return SQ_OK;
}

extern "C" int sq_refine_destroy(sq_handle_t hid) {
    auto* h = remove_handle(hid, H_REFINE);
    if (!h) return fail(SQ_ERR_INVALID, "sq_refine_destroy: unknown handle");
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    delete h;
    return SQ_OK;
}
