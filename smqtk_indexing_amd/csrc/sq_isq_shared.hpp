// IVF-SQ: the list-major scan (option "isq_scan"; included by sq_isq.hip).  ivf_scan_shared_kernel's work split
// (sq_ivf.hip) over code rows: a work item is one group of ivf_pair_group -- one list and up to G of the slice's queries
// that probe it -- x one chunk of 256 rows of that list, one row per lane.  A lane requests every 16-byte load of a leaf
// (<= 128 elements) of its code row before the first use, decodes the leaf ONCE into 128 float registers and adds it into
// the sums of the group's live queries, so per element and query only subtract, multiply and add remain.  The order of
// the sums is IsqLeafLane's (numpy's eight interleaved accumulators per leaf, the tail and leaves below 8 element by
// element, the pairwise tree, a correctly rounded root, no contraction), so a key carries the bits the per-query scan
// writes, and it is stored in the slot the per-query scan fills: nothing downstream changes, and there are no atomics.
#pragma once
#include "sq_isq_codec.hpp"
#include "sq_isq_plan.hpp"
#include "sq_ivf_group.hpp"

namespace sq {

typedef u32 u32x2 __attribute__((ext_vector_type(2)));
typedef u32 u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

static_assert(kIsqSq8 == kCodecSq8 && kIsqF16 == kCodecF16, "sq_isq_plan.hpp names the codecs of sq_isq_codec.hpp");

// The leaf functor of pw_tree_multi: G leaf sums of one code row.
// LDS, SQ8: for dimensions 4b .. 4b + 3 the (2 + G) * 4 adjacent floats vmin[4], step[4], q_0[4] .. q_{G-1}[4] at
// s[(2 + G) * 4 * b] -- the per-query scan's twelve-float groups with the ranges first and G queries behind them; every
// lane reads the same address, so each read is a 16-byte broadcast.  F16: G queries of dq floats, s[g * dq + i].
// Only the first `live` slots are scored (a workgroup-wide branch); the sums of the others stay zero and are never stored.
template <int KIND, int G>
struct IsqLeafGroup {
    static constexpr int BLK = (2 + G) * 4;
    const u8* x;      // the code row, 16-byte aligned
    const float* s;   // LDS
    int dq, live;

    // slot g's query at dimensions e .. e + 3, e a multiple of 4
    __device__ __forceinline__ const float* q4(int g, int e) const {
        if constexpr (KIND == kIsqSq8) return s + (e >> 2) * BLK + 8 + 4 * g;
        else return s + g * dq + e;
    }
    // element i added into every live sum: the tail of a leaf, and leaves below 8
    __device__ __forceinline__ void add_one(int i, float (&v)[G]) const {
        float xd;
        if constexpr (KIND == kIsqSq8) {
            const float* b = s + (i >> 2) * BLK + (i & 3);
            xd = isq_decode_sq8((float)x[i], b[0], b[4]);
        } else {
            xd = (float)reinterpret_cast<const _Float16*>(x)[i];
        }
#pragma unroll
        for (int g = 0; g < G; ++g)
            if (g < live) {
                const float t = __fsub_rn(xd, q4(g, i & ~3)[i & 3]);
                v[g] = __fadd_rn(v[g], __fmul_rn(t, t));
            }
    }
    // elements [off, off + nfull) decoded into xd, nfull a multiple of 8 in 8 .. 128; off is a multiple of 8 (pw_split).
    // SQ8: eight 16-byte loads where off is a multiple of 16; where it is not, an 8-byte load up to the boundary and
    // the 16-byte loads behind it.  A load that would start at or beyond off + nfull is pointed at the aligned 16 bytes
    // that hold (or precede) element off instead, so none leaves the row: a load starts below off + nfull <= d on a
    // 16-byte boundary, and the row's stride is a whole number of 16-byte pieces.
    __device__ __forceinline__ void decode(int off, int nfull, float (&xd)[128]) const {
        if constexpr (KIND == kIsqSq8) {
            u32 w[34];   // dword u = elements 4u .. 4u + 3 of the leaf
            if (off & 8) {
                const u32x2 h = *reinterpret_cast<const u32x2*>(x + off);
                w[0] = h[0];
                w[1] = h[1];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const u32x4 t = *reinterpret_cast<const u32x4*>(x + off + (8 + 16 * j < nfull ? 8 + 16 * j : -8));
#pragma unroll
                    for (int c = 0; c < 4; ++c) w[2 + 4 * j + c] = t[c];
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const u32x4 t = *reinterpret_cast<const u32x4*>(x + off + (16 * j < nfull ? 16 * j : 0));
#pragma unroll
                    for (int c = 0; c < 4; ++c) w[4 * j + c] = t[c];
                }
            }
            const f32x4* par = reinterpret_cast<const f32x4*>(s + (off >> 2) * BLK);
#pragma unroll
            for (int u = 0; u < 32; ++u)
                if (4 * u < nfull) {
                    const f32x4 vm = par[u * (BLK / 4)], st = par[u * (BLK / 4) + 1];
#pragma unroll
                    for (int c = 0; c < 4; ++c) xd[4 * u + c] = isq_decode_sq8((float)((w[u] >> (8 * c)) & 0xffu), vm[c], st[c]);   // v_cvt_f32_ubyte{c}
                }
        } else {
            f16x8 h[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) h[j] = *reinterpret_cast<const f16x8*>(x + 2 * (off + (8 * j < nfull ? 8 * j : 0)));
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (8 * j < nfull) {
#pragma unroll
                    for (int c = 0; c < 8; ++c) xd[8 * j + c] = (float)h[j][c];   // v_cvt_f32_f16
                }
        }
    }
    __device__ __forceinline__ void operator()(int off, int m, float (&v)[G]) const {
#pragma unroll
        for (int g = 0; g < G; ++g) v[g] = 0.f;   // (a term is a square, never -0: 0 + t == t bit for bit)
        const int nfull = m < 8 ? 0 : m - (m % 8);
        if (nfull > 0) {
            float xd[128];
            decode(off, nfull, xd);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (g >= live) continue;
                float r[8];
                {
                    const f32x4 q0 = *reinterpret_cast<const f32x4*>(q4(g, off)), q1 = *reinterpret_cast<const f32x4*>(q4(g, off + 4));
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float t0 = __fsub_rn(xd[c], q0[c]), t1 = __fsub_rn(xd[4 + c], q1[c]);
                        r[c] = __fmul_rn(t0, t0);
                        r[4 + c] = __fmul_rn(t1, t1);
                    }
                }
#pragma unroll
                for (int u = 2; u < 32; u += 2)
                    if (4 * u < nfull) {
                        const f32x4 q0 = *reinterpret_cast<const f32x4*>(q4(g, off + 4 * u));
                        const f32x4 q1 = *reinterpret_cast<const f32x4*>(q4(g, off + 4 * u + 4));
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const float t0 = __fsub_rn(xd[4 * u + c], q0[c]), t1 = __fsub_rn(xd[4 * u + 4 + c], q1[c]);
                            r[c] = __fadd_rn(r[c], __fmul_rn(t0, t0));
                            r[4 + c] = __fadd_rn(r[4 + c], __fmul_rn(t1, t1));
                        }
                    }
                v[g] = __fadd_rn(__fadd_rn(__fadd_rn(r[0], r[1]), __fadd_rn(r[2], r[3])),
                                 __fadd_rn(__fadd_rn(r[4], r[5]), __fadd_rn(r[6], r[7])));
            }
        }
        for (int i = nfull; i < m; ++i) add_one(off + i, v);
    }
};

// Work item blockIdx.x: found in the groups' prefix of chunks with the walk the per-query scan makes (ivf_locate); blocks
// beyond the device-side count of work items return at once.  An unused slot of a group repeats the first query and
// stores nothing.  The key of row r of the list of pair (q, j) goes to keys[ql * key_stride + pre[q][j] + r].
// params: vmin[dq] then step[dq], dq = round_up(d, 4).  Dynamic LDS: isq_shared_lds_bytes(d, KIND).
template <int KIND, int G>
static __global__ __launch_bounds__(256) void isq_scan_shared_kernel(const u8* __restrict__ codes, long long stride, int d,
                                                                      const float* __restrict__ params, const u32* __restrict__ ids,
                                                                      const long long* __restrict__ list_off, const float* __restrict__ queries,
                                                                      int q0, const long long* __restrict__ pre, int np,
                                                                      const u64* __restrict__ sorted, const uint2* __restrict__ groups,
                                                                      const long long* __restrict__ item, const long long* __restrict__ counts,
                                                                      long long key_stride, u64* __restrict__ keys) {
    extern __shared__ __attribute__((aligned(16))) float s_stage[];
    __shared__ long long s_key[G];   // where a slot's keys of this list start
    __shared__ int s_query[G];
    const long long b = blockIdx.x;
    if (b >= counts[1]) return;
    const int grp = ivf_locate(item, (int)counts[0], b);
    const long long chunk = b - item[grp];
    const uint2 gd = groups[grp];   // (first pair in `sorted`, pairs)
    const int live = (int)gd.y;
    const long long l = (long long)(sorted[gd.x] >> 32);
    const long long lo = list_off[l], len = list_off[l + 1] - lo;
    if (threadIdx.x < G) {
        const int slot = threadIdx.x;
        const long long pi = (long long)(sorted[gd.x + (slot < live ? slot : 0)] & 0xffffffffull);
        const long long ql = pi / np, j = pi - ql * np;
        s_query[slot] = q0 + (int)ql;
        s_key[slot] = ql * key_stride + pre[(q0 + ql) * (np + 1) + j];
    }
    __syncthreads();
    const int dq = (d + 3) / 4 * 4;
    for (int i = threadIdx.x; i < dq; i += 256) {
        if constexpr (KIND == kIsqSq8) {
            float* blk = s_stage + (i >> 2) * IsqLeafGroup<KIND, G>::BLK + (i & 3);
            blk[0] = params[i];
            blk[4] = params[dq + i];
#pragma unroll
            for (int g = 0; g < G; ++g) blk[8 + 4 * g] = i < d ? queries[(long long)s_query[g] * d + i] : 0.f;
        } else {
#pragma unroll
            for (int g = 0; g < G; ++g) s_stage[g * dq + i] = i < d ? queries[(long long)s_query[g] * d + i] : 0.f;
        }
    }
    __syncthreads();
    const long long r = chunk * kIvfChunk + threadIdx.x;
    if (r >= len) return;
    const long long row = lo + r;
    float acc[G];
    pw_tree_multi<float, G, kIvfSharedDepth>(IsqLeafGroup<KIND, G>{codes + row * stride, s_stage, dq, live}, d, acc);
    const u64 id = (u64)ids[row];
#pragma unroll
    for (int g = 0; g < G; ++g)
        if (g < live) keys[s_key[g] + r] = ((u64)ordered_f32(sqrt_rn_f32(acc[g])) << 32) | id;
}

}  // namespace sq
