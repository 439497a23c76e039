// The certified float16 filter of ItqFunctor.get_hash for descriptors of 513 .. 8192 elements (the reference's own
// examples hash 2048-d and 4096-d CNN descriptors) and for every width of 1 .. 512 that is no multiple of 64 (100-,
// 200-, 300-d descriptors: itq_filter_route, sq_itq.hip), codes up to 256 bits in one pass over the rows -- and for
// every width up to 8192 at 257 .. 1024 bits, one pass per 256 bits ("Codes beyond 256 bits" below) --, float32 or
// float64 rows of whole 16-byte pieces, normalize None / 2.
// sq_itq_wide.hpp keeps a 32-row tile's fragments resident (d/2 registers per lane: 256 at d = 512) and streams R past
// them; that does not stretch.  Here BOTH operands are blocked over k, in slabs of 64:
//
//   * a wave owns a 32-row tile and the accumulators of ALL column tiles (CT <= 8 tiles of 32 hash bits), so a row is
//     read from HBM exactly once -- at 4096 -> 256 bits the three products are 6.3 MFLOP against 16 KB of row bytes,
//     the pass is bound by the matrix cores and by nothing else only if the rows are not read once per column group;
//   * the rows come straight from global memory into registers (lane = row, 32 consecutive bytes per k-step: the two
//     halves of the lanes consume whole 64-byte pieces, the four k-steps of a slab a row's whole 256 bytes), one slab
//     ahead of the MFMAs, and are split into float16 planes exactly as in sq_itq_wide.hpp;
//   * R streams through a double buffer in LDS that the four waves of a workgroup share (128 rows use every byte
//     fetched from L2): the image is stored slab by slab in the order the MFMA fragments are read -- [slab][column
//     tile][plane][k-step][lane] x 16 bytes -- so one LDS-DMA instruction moves one fragment (1 KB, contiguous in
//     global memory and in LDS) and a fragment read is lane * 16: no bank conflict, no swizzle.  One s_barrier per
//     slab (12 CT MFMAs per wave).
//   * a d that is no multiple of 64 (1000, 2000, 4100; 4, 36, 100, 300, 500): a 16-byte piece is inside its row or
//     beyond it (load_x), a piece beyond it is not read -- the last row of the caller's buffer ends the last access --
//     and stands as zeros in the fragments, in |x|^2 and in max |x_k|; the image is zero there (the caller clears it),
//     so the k-steps past d add exact zeros to the accumulators.  Nothing in the kernel depends on d >= 513: a row
//     shorter than one slab (d < 64) is one slab with most pieces absent.
//
// Error bound.  As in sq_itq_fast.hpp, relative to |x||R_b| (Cauchy-Schwarz):
//   2^-20 (x: two truncated float16 planes) + 2^-21 (the dropped x_lo R_lo) + 2^-20 (the reference's float32 x/|x|,
//   the float32 scale / subtract here) [+ 2^-18, normalize=2: |x|^2 is summed per slab and lane in float32 -- 32
//   products, 2^-19 -- and across slabs in float64; numpy's own pairwise float32 norm is within 2^-20].
//   float32 accumulation: summing d products into one accumulator would cost 1.5 d 2^-24 = 7.3e-4 at d = 8192 -- 3 % of
//   the bits undecided.  So the MFMA accumulator is FLUSHED per slab: it takes the 3 x 64 products of one slab
//   (x_hi R_hi, x_lo R_hi, x_hi R_lo: 1.5 (192 + 8) 2^-24 of the slab's sum of |x_k R_kb| (1 + 2^-9), and the slabs'
//   bounds add up to |x||R_b|) and is then added to the tile's running float32 sum on the vector unit:
//   ceil(d / 64) additions, 1.5 (d / 64 + 1) 2^-24.  At d = 4096: 2.6e-5 in all, about 0.13 % of the bits undecided
//   on normal data (z_b is spread over |x||R_b| / sqrt(d)); at d = 8192: 3.2e-5; at d <= 512 (at most 8 slabs): at most
//   2.1e-5 (the per-slab term dominates).  Zero-padded k is on neither side of the bound: the padded products are 0 * 0 with
//   no rounding, |x| and |R_b| (itq_fast_prep_kernel sums k < d only) do not see them, and the slab count is ceil(d / 64).
//   c_b = mean . R_b is subtracted last, once, in float32 (it does not ride through the accumulation); its rounding
//   and float64 summation error are itq_fast_prep_kernel's cberr, R's own residual its colnorm, the float16
//   subnormal part of the split its cabs: those coefficients carry over unchanged.
// Range: a tile with an element not below 60000 in magnitude, or a non-finite |x|^2, sends all its bits to float64.
//
// The undecided bits -- (row, column tile, mask) entries as in sq_itq_wide.hpp -- are evaluated by
// itq_fix_bits_xwide_kernel on v_mfma_f64_16x16x4_f64 with the operand order of itq_hash_kernel (sq_itq_exact.hpp): 16
// entries per wave, entry i's row as row i of A and its column of R as column i of B, the diagonal of the product kept.
// An element of an MFMA result depends on its own row of A and column of B only, so each such z_b is the float64
// kernel's z_b to the last bit, whatever cancels in it (rows that lie in the span of a few rotation columns leave
// z_b of the order of the rounding error of the sum: a different summation order would flip those signs).
//
// Codes beyond 256 bits (5 .. 16 words).  A wave cannot own more than 8 column tiles of accumulators (256 registers),
// so the columns run in groups of ITQX_GROUP_CT tiles: group g is words 4 g .. 4 g + 3 of the code, the last group the
// remaining 1 .. 4 words (the CT = 2 / 4 / 6 / 8 instantiations).  One launch per group (itq_xwide_path, sq_itq.hip):
// the kernel is the one above, handed the group's slice of the slab image (each slice is laid out
// [slab][column tile][plane][k-step][lane] by itself) and of colnorm / cb32 / cberr / cabs, `word0` = 4 g as the word of
// out[n][words] its first column tile belongs to, and the right-alignment pad in group 0 only (pad < 64).  The error
// terms are per column, so the bound above holds unchanged.  The undecided entries keep their format -- the 3-bit tile
// field is local to the group, n < 2^29 stays the limit --: each group's entries are evaluated by a launch of
// itq_fix_bits_xwide_kernel with the group's first column (`col0`) before the next group's pass overwrites the
// segments.  The rows are read once per group: see DESIGN.md for where that binds (many bits over narrow rows).
#pragma once
#include "sq_itq_fast.hpp"

namespace sq {

static constexpr int ITQX_WAVES = 4;
static constexpr int ITQX_SLAB_K = 64;          // k per slab: 4 MFMA k-steps, one 256-byte unit of a float32 row
static constexpr int ITQX_MAX_D = 8192;   // (no lower limit: sq_itq.hip routes d <= 512, d % 64 != 0 here too)
static constexpr int ITQX_GROUP_CT = 8;   // column tiles of one pass over the rows: 256 bits, 4 code words
static constexpr int ITQX_MAX_WORDS = 16; // 1024 bits: four such passes

struct ItqXwideArgs {
    const void* x;         // [n][d] rows of T, 16-byte aligned rows
    long long n;
    int d;
    const uint4* ximage;   // [slab][column tile][plane][k-step][lane] x 16 bytes (itq_xwide_relayout_kernel)
    const float* colnorm;  // [pc] per-column error coefficients (itq_fast_prep_kernel)
    const float* cabs;
    const float* cb32;
    const float* cberr;
    u64* out;              // [n][words]
    int words, pad, bits;  // words: of the whole code (the row stride of out); pad: leading zero columns of THIS launch's columns
    int word0;             // first code word of this launch's column group (4 g: see "Codes beyond 256 bits" above)
    u64* seg;              // [waves of the launch][seg_cap] undecided entries: (row | column tile << 29) << 32 | 32-column mask
    u32* seg_cnt;
    long long seg_cap;
    long long n_tiles;
    int nslab;             // ceil(d / 64)
};

// itq_fast_prep_kernel's image ([pc][2 planes][dp], 16-byte chunks swizzled by column inside 256-byte segments) ->
// the slab order above.  One thread per 16-byte chunk.  The source is zero beyond d (the caller clears it).
static __global__ __launch_bounds__(256) void itq_xwide_relayout_kernel(const uint4* __restrict__ img, uint4* __restrict__ ximg,
                                                                         int dp, int ct_n, long long total) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int lane = (int)(t & 63);
    long long r = t >> 6;
    const int s = (int)(r & 3);
    r >>= 2;
    const int p = (int)(r & 1);
    r >>= 1;
    const int ct = (int)(r % ct_n);
    const int slab = (int)(r / ct_n);
    const int pc = ct * 32 + (lane & 31), h = lane >> 5;
    const int k = slab * ITQX_SLAB_K + 16 * s + 8 * h;     // first of the chunk's 8 elements
    const int chunk = ((k & 127) >> 3) ^ (pc & 15);
    const long long src16 = (((long long)pc * 2 + p) * dp + (long long)(k >> 7) * 128) / 8 + chunk;   // in 16-byte units
    ximg[t] = img[src16];
}

template <class T, bool NORMED, int CT>
__global__ __launch_bounds__(ITQX_WAVES * 64, CT <= 2 ? 2 : 1) void itq_xwide_kernel(ItqXwideArgs a) {
    constexpr u32 SLAB_BYTES = (u32)CT * 8192u;          // CT tiles x 2 planes x 4 k-steps x 1 KB
    constexpr int PC = CT * 32;
    constexpr int NP = sizeof(T) == 4 ? 2 : 4;           // 16-byte pieces of a lane's 8 elements of a k-step
    typedef typename std::conditional<sizeof(T) == 4, itq_f32x4, double __attribute__((ext_vector_type(2)))>::type piece_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // LDS: [2 slab buffers][column constants 3 x PC floats]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r31 = lane & 31, h = lane >> 5;
    const int D = a.d;
    const u32 lds_base = (u32)(uintptr_t)smem;
    float* lconst = reinterpret_cast<float*>(smem + 2u * SLAB_BYTES);   // c_b, epsA, epsB: eps(column) = epsA U + epsB
    for (int i = threadIdx.x; i < PC; i += ITQX_WAVES * 64) {
        const float cn = a.colnorm[i], cb = a.cb32[i], ce = a.cberr[i], ca = a.cabs[i];
        lconst[i] = cb;
        if constexpr (NORMED) {
            // z~ = (x . R_b) / |x| - c_b: eps = colnorm + cberr + cabs U, U = the largest 1/|x| of the tile
            lconst[PC + i] = ca;
            lconst[2 * PC + i] = cn + ce;
        } else {
            // z~ = x . R_b - c_b: eps = colnorm U + cberr + cabs, U = the largest |x| of the tile
            lconst[PC + i] = cn;
            lconst[2 * PC + i] = ce + ca;
        }
    }
    __syncthreads();

    const long long wave_id = (long long)blockIdx.x * ITQX_WAVES + wave;
    const long long nwaves = (long long)gridDim.x * ITQX_WAVES;
    const long long rounds = (a.n_tiles + nwaves - 1) / nwaves;   // every wave runs the same rounds (barriers)
    u64* myseg = a.seg + wave_id * a.seg_cap;
    u32 wcount = 0;
    const unsigned char* img = reinterpret_cast<const unsigned char*>(a.ximage);
    const int nslab = a.nslab;
    // slab DMA: the CT * 8 fragments of a slab, dealt round-robin to the four waves
    auto issue_slab = [&](int slab, int buf) __attribute__((always_inline)) {
        const unsigned char* src = img + (size_t)slab * SLAB_BYTES;
#pragma unroll
        for (int j = 0; j < CT * 2; ++j) {
            const int piece = j * ITQX_WAVES + wave;
            glds16<false>(src + (size_t)piece * 1024, (u32)lane * 16u, lds_base + (u32)buf * SLAB_BYTES + (u32)piece * 1024u);
        }
    };

    for (long long round = 0; round < rounds; ++round) {
        long long tile = wave_id + round * nwaves;
        const bool active = tile < a.n_tiles;
        if (!active) tile = a.n_tiles - 1;          // keeps the barriers and the R stream; nothing is stored
        long long row0 = tile * 32;
        const long long shift = row0 + 32 > a.n ? row0 + 32 - a.n : 0;   // the last tile: the window moves back (n >= 32)
        row0 -= shift;
        const T* xrow = reinterpret_cast<const T*>(a.x) + (row0 + r31) * (long long)D;
        // this lane's 8 elements of each of a slab's 4 k-steps: k = k0 + 16 s + 8 h + (0..7); rows are 16-byte
        // aligned and d is a whole number of 16-byte pieces, so a piece is inside the row or beyond it
        auto load_x = [&](int k0, piece_t (&raw)[4][NP]) __attribute__((always_inline)) {
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int e = 0; e < NP; ++e) {
                    const int k = k0 + 16 * s + 8 * h + e * (8 / NP);
                    piece_t v;
#pragma unroll
                    for (int j = 0; j < 8 / NP; ++j) v[j] = 0;
                    if (k < D) v = *reinterpret_cast<const piece_t*>(xrow + k);
                    raw[s][e] = v;
                }
        };
        itq_f32x16 accS[CT], accM[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                accS[ct][i] = 0.f;
                accM[ct][i] = 0.f;
            }
        double sumsq = 0.0;
        float amax = 0.f;
        piece_t nxt[4][NP];
        issue_slab(0, 0);
        load_x(0, nxt);
        for (int sl = 0; sl < nslab; ++sl) {
            piece_t cur[4][NP];
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int e = 0; e < NP; ++e) cur[s][e] = nxt[s][e];
            // slab sl: own pieces (vmcnt) and the other waves' (barrier) have landed, and every wave has finished
            // reading the buffer slab sl + 1 is about to overwrite
            wait_vmcnt<0>();
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if (sl + 1 < nslab) {
                issue_slab(sl + 1, (sl + 1) & 1);
                load_x((sl + 1) * ITQX_SLAB_K, nxt);
            }
            // split into float16 planes: B fragments of the 4 k-steps (lane = row)
            itq_f16x8 xh[4], xl[4];
            float part = 0.f;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                itq_u32x4 hw, lw;
                if constexpr (sizeof(T) == 4) {
#pragma unroll
                    for (int j = 0; j < 8; j += 2) {
                        const float u0 = cur[s][j >> 2][j & 3], u1 = cur[s][j >> 2][(j & 3) + 1];
                        part = __fmaf_rn(u0, u0, part);
                        part = __fmaf_rn(u1, u1, part);
                        amax = fmaxf(amax, fmaxf(fabsf(u0), fabsf(u1)));
                        u32 hh, ll;
                        split_f16_pair(u0, u1, hh, ll);
                        hw[j >> 1] = hh;
                        lw[j >> 1] = ll;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const double d0 = cur[s][e][0], d1 = cur[s][e][1];
                        const float f0 = (float)d0, f1 = (float)d1;
                        part = __fmaf_rn(f0, f0, part);
                        part = __fmaf_rn(f1, f1, part);
                        amax = fmaxf(amax, fmaxf(fabsf(f0), fabsf(f1)));
                        const auto hv = __builtin_amdgcn_cvt_pkrtz(f0, f1);   // two float16, round toward zero
                        // the residual is formed in float64 (x - hi is exact there), rounded to float32, truncated to float16
                        const float l0 = (float)(d0 - (double)(float)hv[0]), l1 = (float)(d1 - (double)(float)hv[1]);
                        hw[e] = __builtin_bit_cast(u32, hv);
                        lw[e] = __builtin_bit_cast(u32, __builtin_amdgcn_cvt_pkrtz(l0, l1));
                    }
                }
                xh[s] = __builtin_bit_cast(itq_f16x8, hw);
                xl[s] = __builtin_bit_cast(itq_f16x8, lw);
            }
            sumsq += (double)part;
            // A = R's fragment (M = column), B = the row fragment (N = row): D[column][row], lane = row
            const unsigned char* buf = smem + (size_t)(sl & 1) * SLAB_BYTES + lane * 16;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    const itq_f16x8 bh = *reinterpret_cast<const itq_f16x8*>(buf + ((ct * 2 + 0) * 4 + s) * 1024);
                    const itq_f16x8 bl = *reinterpret_cast<const itq_f16x8*>(buf + ((ct * 2 + 1) * 4 + s) * 1024);
                    accM[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh, xh[s], accM[ct], 0, 0, 0);
                    accM[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh, xl[s], accM[ct], 0, 0, 0);
                    accM[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bl, xh[s], accM[ct], 0, 0, 0);
                }
            }
            // flush: the slab's sum joins the tile's running sum (the float32 accumulation bound scales with 192, not 3 d)
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    accS[ct][i] = __fadd_rn(accS[ct][i], accM[ct][i]);
                    accM[ct][i] = 0.f;
                }
        }
        // row norms: lane L < 32 and its twin L + 32 end with |x|^2 and max |x_k| of row r31
        sumsq += __shfl_xor(sumsq, 32);
        amax = fmaxf(amax, __shfl_xor(amax, 32));
        const float sumsq_f = (float)sumsq;
        float rowscale = 1.f, U;
        if constexpr (NORMED) {
            rowscale = sumsq > 0.0 ? (float)(1.0 / sqrt(sumsq)) : 0.f;   // zero row: z~ = -mean . R_b
            float rsmax = rowscale;
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) rsmax = fmaxf(rsmax, __shfl_xor(rsmax, o));
            U = rsmax * 1.0001f;   // the absolute part of the split's error meets the largest 1/|x| of the tile
        } else {
            float g = sumsq_f;
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) g = fmaxf(g, __shfl_xor(g, o));
            U = sqrtf(g) * 1.0001f;
        }
        // a float16 plane saturates from |x_k| = 65504 on; a NaN hides from fmaxf but not from the sum
        const bool bad_rows = __ballot(!(amax < 60000.f) || !(sumsq_f < 3.0e38f)) != 0ull;

        u32 word_hi = 0;   // sign bits of the even column tile of the current output word (this lane's row)
        const long long row = row0 + r31;
        const bool mine = active && lane < 32 && r31 >= (int)shift && row < a.n;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            // lane = row r31, register i = column (i & 3) + 8 (i >> 2) + 4 h of the tile
            u32 bits = 0, unc = 0;
            itq_f32x4 cbv[4], eav[4], ebv[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                cbv[g] = *reinterpret_cast<const itq_f32x4*>(lconst + ct * 32 + 8 * g + 4 * h);
                eav[g] = *reinterpret_cast<const itq_f32x4*>(lconst + PC + ct * 32 + 8 * g + 4 * h);
                ebv[g] = *reinterpret_cast<const itq_f32x4*>(lconst + 2 * PC + ct * 32 + 8 * g + 4 * h);
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int col = (i & 3) + 8 * (i >> 2) + 4 * h;
                const float raw = accS[ct][i];
                float z;
                if constexpr (NORMED)
                    z = __fmaf_rn(raw, rowscale, -cbv[i >> 2][i & 3]);
                else
                    z = __fsub_rn(raw, cbv[i >> 2][i & 3]);
                // (the 1.0001: the rounding of z~ itself and of this multiply-add)
                const float eps = __fmaf_rn(eav[i >> 2][i & 3], U, ebv[i >> 2][i & 3]) * 1.0001f;
                bits |= (z >= 0.f ? 1u : 0u) << (31 - col);       // column 0 -> most significant
                unc |= (!(fabsf(z) > eps) ? 1u : 0u) << col;      // true for a NaN; bit c = column c of the tile
            }
            bits |= __shfl_xor(bits, 32);   // the other half of the lanes holds the other 16 columns of the same row
            unc |= __shfl_xor(unc, 32);
            {
                const int lo = a.pad - ct * 32;   // columns below `pad` are padding: never undecided
                const u32 valid = lo <= 0 ? ~0u : (lo >= 32 ? 0u : (~0u << lo));
                unc = bad_rows ? valid : (unc & valid);
            }
            if ((ct & 1) == 0) {
                word_hi = bits;
            } else if (mine) {
                u64 v = ((u64)word_hi << 32) | (u64)bits;
                if ((ct >> 1) == 0 && a.pad > 0) v &= (~0ull) >> a.pad;
                a.out[row * a.words + a.word0 + (ct >> 1)] = v;
            }
            {
                const bool need = mine && unc != 0;
                const u64 nb = __ballot(need);
                const u32 p = wcount + __builtin_amdgcn_mbcnt_hi((u32)(nb >> 32), __builtin_amdgcn_mbcnt_lo((u32)nb, 0u));
                if (need && (long long)p < a.seg_cap) myseg[p] = ((u64)((u32)row | ((u32)ct << 29)) << 32) | (u64)unc;
                wcount += (u32)__popcll(nb);
            }
        }
        // every wave is done with the slab buffers before the next round's slab 0 lands in buffer 0
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    }
    if (lane == 0) a.seg_cnt[wave_id] = wcount;
}

// The undecided bits in float64, bit-identical to itq_hash_kernel (see the header).  16 entries per wave and pass:
// lane (i = lane & 15, g = lane >> 4) feeds entry i's v[c + 4 g + j] as A and R[c + 4 g + j][column of entry i] as B
// to the j-th v_mfma_f64_16x16x4_f64 of 16-k step c, in itq_hash_kernel's order; element (i, i) of the result is
// register i >> 2 of lane (i, g = i & 3).  v = x / |x| (x's dtype, numpy's norm) minus the mean in the promoted dtype.
// col0: the first padded column of the column group the entries come from (0 for codes up to 256 bits).
template <class T>
static __global__ __launch_bounds__(256) void itq_fix_bits_xwide_kernel(ItqArgs a, const u64* __restrict__ seg,
                                                                         const u32* __restrict__ seg_cnt, long long seg_cap,
                                                                         const double* __restrict__ rt64, int col0) {
    const long long w = blockIdx.x;
    const long long cnt_raw = seg_cnt[w];
    const u32 cnt = (u32)(cnt_raw < seg_cap ? cnt_raw : seg_cap);
    const int lane = threadIdx.x & 63, l15 = lane & 15, g = lane >> 4;
    const u32 group = (u32)(threadIdx.x >> 6) + 4u * blockIdx.y, ngroups = 4u * gridDim.y;
    const T* X = reinterpret_cast<const T*>(a.x);
    const bool vec4 = a.d % 4 == 0;   // (rows are 16-byte aligned; float64 rows of d % 4 == 2 take scalar loads)
    for (u32 e0 = group * 16u; e0 < cnt; e0 += ngroups * 16u) {   // wave-uniform
        const bool have = e0 + (u32)l15 < cnt;
        const u64 ent = have ? seg[w * seg_cap + e0 + l15] : 0ull;   // (no entry: row 0, nothing undecided)
        const long long row = (long long)((u32)(ent >> 32) & 0x1fffffffu);
        const int ct = (int)((ent >> 61) & 7u);
        u32 mask = (u32)ent;
        const T* xr = X + row * a.d;
        T nrm = (T)1;
        if (a.norm == SQ_NORM_L2) {
            // numpy's pairwise order: eight cooperating lanes per row (np_pairwise_sum), entries q and q + 8 of group q
            T got[2];
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const long long rq = __shfl(row, (lane >> 3) + 8 * p);   // lane q < 16 holds entry q's row
                const T* xq = X + rq * a.d;
                auto term = [xq](int i) { return mul_rn(xq[i], xq[i]); };
                T v = sqrt_rn(np_pairwise_sum<T>(term, a.d, lane & 7));
                got[p] = v == (T)0 ? (T)1 : v;
            }
            const T n0 = __shfl(got[0], 8 * (l15 & 7)), n1 = __shfl(got[1], 8 * (l15 & 7));
            nrm = l15 < 8 ? n0 : n1;
        }
        while (__ballot(mask != 0u) != 0ull) {   // nearly always one pass
            const bool live = mask != 0u;
            const int pc = col0 + ct * 32 + (live ? __ffs((int)mask) - 1 : 0);   // padded column of the whole code (col0: the entries' column group); the filter only flags pc >= pad
            mask &= mask - 1u;
            const double* rcol = rt64 + (long long)pc * a.d;   // column pc of R, contiguous (itq_fast_prep_kernel)
            f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
            for (int c = 0; c < a.d16; c += 16) {
                const int kb = c + 4 * g;
                T xq[4];
                double bv[4];
                if (vec4 && kb < a.d) {
                    const typename Vec4<T>::type v4 = *reinterpret_cast<const typename Vec4<T>::type*>(xr + kb);
                    const f64x4 r4 = *reinterpret_cast<const f64x4*>(rcol + kb);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        xq[j] = v4[j];
                        bv[j] = r4[j];
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        xq[j] = kb + j < a.d ? xr[kb + j] : (T)0;
                        bv[j] = kb + j < a.d ? rcol[kb + j] : 0.0;
                    }
                }
                double av[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int k = kb + j;
                    double v = 0.0;
                    if (k < a.d) {
                        T xv = xq[j];
                        if (a.norm == SQ_NORM_L2) xv = div_rn(xv, nrm);
                        if constexpr (sizeof(T) == 4) {
                            if (a.sub32)
                                v = (double)__fsub_rn(xv, (float)a.mean[k]);
                            else
                                v = __dsub_rn((double)xv, a.mean[k]);
                        } else {
                            v = __dsub_rn((double)xv, a.mean[k]);
                        }
                    }
                    av[j] = v;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[j], bv[j], acc, 0, 0, 0);
            }
            const int reg = l15 >> 2;
            const double z = reg == 0 ? acc[0] : reg == 1 ? acc[1] : reg == 2 ? acc[2] : acc[3];
            if (live && g == (l15 & 3)) {   // set the bit to the float64 sign in place
                unsigned long long* word = reinterpret_cast<unsigned long long*>(a.out + row * a.words + (pc >> 6));
                const unsigned long long bit = 1ull << (63 - (pc & 63));
                if (z >= 0.0)
                    atomicOr(word, bit);
                else
                    atomicAnd(word, ~bit);
            }
        }
    }
}

}  // namespace sq
