// The int8 first-stage filter for rows of 513 to 8192 dimensions (gfx950).        (included by sq_dense.hip)
//
// sq_dense_i8.hpp stops at 512-byte rows: its kernels keep the query planes in registers and join the two planes'
// integer sums by a shift.  Wider rows -- the 2048- and 4096-dimensional descriptors of the reference's own examples
// (docs/examples/caffe_build_index.rst:35) -- only had dense_wide_scan_kernel over the bfloat16 copy, 2 d_pad + 4 bytes per
// row of a pass that is HBM bound.  Here the same walk runs over an int8 copy of d_pad8 + 4 bytes per row.
//
// The copy and its certificate are sq_dense_i8.hpp's, unchanged: x8 = clamp(rint(x' / Dx), +-127) with ONE scale per
// matrix (x' = x - c for L2, x / |x| for cosine), the residual r_row = |x' - Dx x8| measured per row in float64, rows far
// above the rest flagged as always-candidates (N_row = -inf), data no clamp suits declined.  None of that depends on d:
//     e(row, q) <= 2 r_row |q''| + |Dx x8| rq + rounding        (Cauchy-Schwarz on the two measured residuals)
// so the sampled threshold T' = T_s + 2 e_q, the second-level threshold (sq_dense_tighten.hpp), the exact re-rank from
// the ORIGINAL float32 rows, the select and the per-query certificate s > T' - e_q follow as they do for narrow rows.
//
// Layout.  Rows are plain row-major int8, padded with zeros to whole 128 bytes (row_bytes = 128 ceil(d / 128)); the row
// terms N_row sit in an array of their own.  A lane's operand of v_mfma_i32_32x32x32_i8 is 16 consecutive k of one row:
// lane (r, h) of k-step s reads bytes 32 s + 16 h .. + 15 of row r, so the row loads are plain 16-byte global loads
// straight into the MFMA's A registers (no LDS ring), as in sq_dense_wide.hpp.  The kernel walks k-units of 256 bytes
// (eight k-steps, sixteen MFMAs for the two query planes -- the bfloat16 kernel's loads and MFMAs per unit).  A row of
// an odd number of 128-byte pieces ends in the middle of its last unit: the second half of that unit's loads then
// reads the first 128 bytes of the NEXT row (256 spare bytes behind the copy keep the last row's inside the allocation)
// against query-plane bytes that are zero there -- integer products: exactly zero, whatever the bytes.  The query
// planes are therefore padded to whole units (qw = 256 ceil(row_bytes / 256) bytes per query and plane).
//
// The accumulators.  With |x8|, |Q8| <= 127 the joined sum 256 sum + sum' of the narrow kernel leaves an i32 at d ~ 520.
// Here each plane keeps an i32 accumulator of its own for the whole row:
//     |sum|, |sum'| <= 127 * 127 * 8192 = 132 128 768 < 2^27 < 2^31        (d_pad8 <= 8192 = MAX_DPAD)
// so neither can wrap for ANY bytes, and they are joined once per tile in float64:
//     w = 256 sum + sum'   (|w| < 2^35: exact),      s~ = float32(N_row + (Dx Dq / 256) w)
// The float64 product and sum carry a relative 2^-52 each; what is left are the roundings the narrow kernel's bound
// already pays for with its term 4 * 2^-24 ((X + R)(|w_q| + rq) + X^2): the float32 value of the unit Dx Dq (2^-24 of
// |unit w| <= (X + R)(|w_q| + rq)), the final conversion to float32 (2^-24 of |N| + |unit w|) and N_row's own rounding
// (2^-24 X^2) -- three of the four 2^-24 the term holds, the float64 steps far inside the fourth.  e_q is computed by
// the same expression (dense8_wide_prep_queries_kernel); nothing is added to it and nothing is missing from it.
#pragma once
#include "sq_dense_i8.hpp"
#include "sq_dense_wide.hpp"

namespace sq {

static constexpr int I8W_ROW_ALIGN = 128;    // rows of the copy are padded to whole 128 bytes
static constexpr int I8W_UNIT = 256;         // bytes of a row the kernel takes per step (eight k-steps of the int8 MFMA)
static constexpr int I8W_SPARE = 256;        // bytes behind the copy (the last row's half unit, see above)
__host__ __device__ constexpr int i8w_row_bytes(int d) { return (d + I8W_ROW_ALIGN - 1) / I8W_ROW_ALIGN * I8W_ROW_ALIGN; }
__host__ __device__ constexpr int i8w_units(int row_bytes) { return (row_bytes + I8W_UNIT - 1) / I8W_UNIT; }
static_assert(127ll * 127 * MAX_DPAD < (1ll << 31), "a plane's i32 accumulator holds the widest row");

// ---------------------------------------------------------------- per call
// sum of one float64 per thread over a 256-thread workgroup, the same bits in every thread
__device__ __forceinline__ double i8w_block_sum(double v, double* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();   // (red may still be read from the sum before)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// Query prep, one 256-thread workgroup per query of the padded tile: what dense8_prep_queries_kernel does, for any row
// width -- the planes Q8 = rint(w / Dq) and Q8' = rint(256 (w / Dq - Q8)) of w = -2 (q - c) (cosine: -q / |q|) with the
// query's own scale Dq = max |w| / 127, the residual rq measured in float64 against what is stored, |q''|^2, {unit, e_q},
// the threshold / counter / flag state of the call and the aligned float32 copy the re-rank reads.
//   qs8: [2][32][qw] (plane, query), zero behind d
static __global__ __launch_bounds__(256) void dense8_wide_prep_queries_kernel(const float* __restrict__ q, int nq, int d,
                                                                              const float* __restrict__ center, double dx, double r_max,
                                                                              double x_max, signed char* __restrict__ qs8, int qw,
                                                                              float2* __restrict__ par, double* __restrict__ qn2,
                                                                              float* __restrict__ thr, u32* __restrict__ cnt,
                                                                              u32* __restrict__ oflag, float* __restrict__ q_al, int ldq,
                                                                              int cosine) {
    __shared__ double red[4];
    __shared__ float redm[4];
    const int qi = blockIdx.x, t = threadIdx.x;
    const bool real = qi < nq;
    if (t == 0) {
        // padding queries of the tile: a NaN threshold -- no comparison passes, not even an always-candidate row's -inf
        thr[qi] = real ? -__builtin_inff() : __builtin_nanf("");
        cnt[qi] = 0u;
        if (qi == 0) *oflag = 0u;
    }
    const float* qrow = q + (long long)(real ? qi : 0) * d;
    if (real)
        for (int i = t; i < ldq; i += 256) q_al[(long long)qi * ldq + i] = i < d ? qrow[i] : 0.f;
    auto value = [&](int k) -> float {   // q'' before the cosine scaling
        if (!real || k >= d) return 0.f;
        return center ? __fsub_rn(qrow[k], center[k]) : qrow[k];
    };
    double rn = 1.0;
    if (cosine) {
        double nn = 0.0;
        for (int k = t; k < d; k += 256) {
            const double v = (double)value(k);
            nn += v * v;
        }
        rn = sqrt(i8w_block_sum(nn, red));   // (a zero query: NaN planes -- no scale, the exact path answers it as the reference does)
    }
    auto scaled = [&](int k) -> float { return cosine ? (float)((double)value(k) / rn) : value(k); };
    const float sc = cosine ? -1.f : -2.f;
    double Qs = 0.0;
    float mx = 0.f;
    for (int k = t; k < d; k += 256) {
        const float v = scaled(k);
        Qs += (double)v * (double)v;
        float m = fabsf(sc * v);
        if (!(m == m)) m = __builtin_inff();
        mx = fmaxf(mx, m);
    }
    const double Q = i8w_block_sum(Qs, red);
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((t & 63) == 0) redm[t >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(redm[0], redm[1]), fmaxf(redm[2], redm[3]));
    const bool ok = real && mx < 3.0e38f && mx > 0.f;   // zero / non-finite / padding queries: all-zero planes, nothing certified by them
    const double dq = ok ? (double)mx / 127.0 : 1.0;
    const double inv_dq = 1.0 / dq;
    signed char* p0 = qs8 + (long long)qi * qw;
    signed char* p1 = qs8 + (long long)(TILE_ROWS + qi) * qw;
    double r2 = 0.0;
    for (int k = t; k < qw; k += 256) {
        float qt8 = 0.f, ql8 = 0.f;
        if (ok && k < d) {
            const double w = (double)(sc * scaled(k));
            const double ws = w * inv_dq;
            qt8 = fminf(fmaxf(rintf((float)ws), -127.f), 127.f);
            ql8 = fminf(fmaxf(rintf((float)((ws - (double)qt8) * 256.0)), -127.f), 127.f);
            const double res = w - ((double)qt8 + (double)ql8 * 0.00390625) * dq;
            r2 += res * res;
        }
        p0[k] = (signed char)(int)qt8;
        p1[k] = (signed char)(int)ql8;
    }
    const double r2s = i8w_block_sum(r2, red);
    if (t == 0) {
        // e_q exactly as dense8_prep_query_row forms it (the derivation of its rounding term for this kernel: file header)
        const double rq = sqrt(r2s) * (1.0 + 1e-9);
        const double unit = dx * dq;
        const double xr = x_max + r_max, qn = sqrt(Q), wn = (cosine ? 1.0 : 2.0) * qn;
        double e = r_max * wn + xr * rq + 4.0 * 5.9604644775390625e-08 * (xr * (wn + rq) + x_max * x_max);
        e *= 1.0 + 1e-6;
        float ef = (float)e;
        if ((double)ef < e) ef = __uint_as_float(__float_as_uint(ef) + 1u);
        if (!ok && real) ef = __builtin_inff();   // (Dense8ThrPost gives such a query a NaN threshold: it takes the next tier)
        par[qi] = make_float2((float)unit, real ? ef : 0.f);
        qn2[qi] = real ? Q : 0.0;
    }
}

// Dense8ThrPost that also hands the threshold before the slack to the second-level threshold (sq_dense_tighten.hpp sizes
// its histogram bins with it)
struct Dense8WideThrPost {
    Dense8ThrPost base;
    float* traw_out;
    __device__ __forceinline__ void prologue(int, double*) const {}
    __device__ __forceinline__ float operator()(int q, float t) const {
        if (traw_out) traw_out[q] = t;
        return base(q, t);
    }
};

struct Dense8WideArgs {
    const signed char* scan8;   // [n_pad][row_bytes] (+ I8W_SPARE)
    const float* nrow;          // [n_pad] N_row (+inf: padding and removed rows, -inf: always-candidate rows)
    int row_bytes;
    int ku;                     // k-units of 256 bytes per row (the last one may be half a unit of this row)
    long long n;
    long long n_tiles;          // ceil(n / 32)
    const signed char* qs8;     // [2][32][256 ku]: plane, query
    const float2* par;          // [32] {unit, e_q}
    const float* thr;           // [32]
    uint2* wave_out;            // per-wave segments of (first row, mask << 16 | query), as dense_wide_scan_kernel writes them
    u32* wave_cnt;
    u32 wave_cap;
    float* wave_score;          // parallel to wave_out: each entry's smallest score (-inf: it holds an always-candidate row)
    float* sample_out;          // [32][ns] (SAMPLE)
    long long ns;
    long long tile_step;        // SAMPLE: every tile_step-th tile; EMIT: 1
    long long n_sel;            // tiles this launch visits
    int nrb;                    // workgroups
};

// dense_wide_scan_kernel<2, 1, SAMPLE> over the int8 copy: a wave owns a 32-row tile and walks its k-units, the next unit's
// row loads requested before this unit's sixteen MFMAs; the query tile's fragments of a unit reach the workgroup's eight
// waves through a double-buffered LDS copy ([plane][query][16 chunks, chunk c at c ^ (query & 15)]), one barrier per
// unit; the planes themselves stay in L2.
// (four waves per SIMD, i.e. 128 registers: two eight-wave workgroups per CU -- twice the row bytes in flight)
template <bool SAMPLE>
__global__ __launch_bounds__(WIDE_WAVES * 64, 4) void dense8_wide_scan_kernel(Dense8WideArgs a) {
    constexpr int PLANE_BYTES = TILE_ROWS * I8W_UNIT;   // one plane's fragments of a k-unit
    __shared__ __attribute__((aligned(16))) unsigned char qbuf[2][2 * PLANE_BYTES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r31 = lane & 31, h = lane >> 5;
    const long long gw = (long long)blockIdx.x * WIDE_WAVES + wave;   // unique per wave of the launch
    const long long nwaves = (long long)a.nrb * WIDE_WAVES;
    uint2* wout = a.wave_out + gw * a.wave_cap;
    const int ku = a.ku;
    const size_t qw = (size_t)ku * I8W_UNIT;
    const float thr_l = SAMPLE ? 0.f : a.thr[r31];
    const double unit_lo = (double)a.par[r31].x * 0.00390625;   // Dx Dq / 256
    // thread t brings chunk (t & 15) of query (t >> 4) of both planes: 16 threads read 256 contiguous bytes
    const int lq = tid >> 4, lc = tid & 15;
    const unsigned char* qsrc = reinterpret_cast<const unsigned char*>(a.qs8) + (size_t)lq * qw + (size_t)lc * 16;
    const size_t plane_stride = (size_t)TILE_ROWS * qw;
    const u32 qdst = (u32)(lq * I8W_UNIT + ((lc ^ (lq & 15)) * 16));
    u32 tail_mask = 0;   // rows of the last, partial tile that exist (bit i <-> accumulator register i of this lane)
    {
        const int nvalid = (int)(a.n - (a.n_tiles - 1) * TILE_ROWS);
#pragma unroll
        for (int i = 0; i < 16; ++i) tail_mask |= ((i & 3) + 8 * (i >> 2) + 4 * h < nvalid ? 1u : 0u) << i;
    }
    // rounds of the WORKGROUP (its first wave has the most tiles): every wave walks them all -- the barriers are the
    // workgroup's -- and skips the arithmetic of a round it has no tile in
    const long long wg_first = (long long)blockIdx.x * WIDE_WAVES;
    const long long rounds = wg_first < a.n_sel ? (a.n_sel - wg_first + nwaves - 1) / nwaves : 0;
    if (rounds > 0) {   // unit 0 of the query tile
        *reinterpret_cast<i32x4*>(qbuf[0] + qdst) = *reinterpret_cast<const i32x4*>(qsrc);
        *reinterpret_cast<i32x4*>(qbuf[0] + PLANE_BYTES + qdst) = *reinterpret_cast<const i32x4*>(qsrc + plane_stride);
    }
    u32 wcount = 0;
    int step = 0;   // (round, k-unit) steps so far: buffer step & 1 holds this step's query fragments
    for (long long it = 0; it < rounds; ++it) {
        const long long sel = gw + it * nwaves;
        const bool active = sel < a.n_sel;
        const long long row0 = (active ? sel : 0) * a.tile_step * TILE_ROWS;
        const unsigned char* arow = reinterpret_cast<const unsigned char*>(a.scan8) + (size_t)(row0 + r31) * a.row_bytes + (size_t)h * 16;
        i32x4 av[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) av[s] = *reinterpret_cast<const i32x4*>(arow + s * 32);
        i32x16 acc, acl;   // one i32 accumulator per query plane for the whole row: |sum| <= 127 * 127 * 8192 < 2^27 (file header)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = acl[i] = 0;
        for (int kc = 0; kc < ku; ++kc, ++step) {
            // requests of the NEXT step: the row fragments of this tile's next unit (the last unit re-requests itself: no
            // branch around the loads) and the workgroup's share of the next query unit (the next round starts at unit 0)
            i32x4 an[8];
            const int kn = kc + 1 < ku ? kc + 1 : kc;
            const int kq = kc + 1 < ku ? kc + 1 : 0;
#pragma unroll
            for (int s = 0; s < 8; ++s) an[s] = *reinterpret_cast<const i32x4*>(arow + (size_t)kn * I8W_UNIT + s * 32);
            const i32x4 nq0 = *reinterpret_cast<const i32x4*>(qsrc + (size_t)kq * I8W_UNIT);
            const i32x4 nq1 = *reinterpret_cast<const i32x4*>(qsrc + plane_stride + (size_t)kq * I8W_UNIT);
            __syncthreads();   // this step's buffer is complete; nobody still reads the other one
            const unsigned char* qb = qbuf[step & 1];
            i32x4 bq[8], bl[8];
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const u32 at = (u32)(r31 * I8W_UNIT + (((2 * s + h) ^ (r31 & 15)) * 16));
                bq[s] = *reinterpret_cast<const i32x4*>(qb + at);
                bl[s] = *reinterpret_cast<const i32x4*>(qb + PLANE_BYTES + at);
            }
            if (active) {
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    acl = __builtin_amdgcn_mfma_i32_32x32x32_i8(av[s], bl[s], acl, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(av[s], bq[s], acc, 0, 0, 0);
                }
            }
            unsigned char* qn = qbuf[(step + 1) & 1];
            *reinterpret_cast<i32x4*>(qn + qdst) = nq0;
            *reinterpret_cast<i32x4*>(qn + PLANE_BYTES + qdst) = nq1;
#pragma unroll
            for (int s = 0; s < 8; ++s) av[s] = an[s];
        }
        if (!active) continue;
        // ---- tile complete: scores of 32 rows x 32 queries (lane = query, register i = row (i & 3) + 8 (i >> 2) + 4 h)
        const bool is_tail = row0 + TILE_ROWS > a.n;   // wave-uniform: the last, partial tile
        f32x16 sc;
        float m = __builtin_inff();
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const f32x4 nv4 = *reinterpret_cast<const f32x4*>(a.nrow + row0 + 8 * c + 4 * h);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = 4 * c + j;
                float nv = nv4[j];
                if constexpr (SAMPLE) nv = nv == -__builtin_inff() ? __builtin_inff() : nv;   // an always-candidate row is no sample
                // 256 sum + sum' in float64: exact (|.| < 2^35); one rounding, to float32, at the end
                const double w = __fma_rn((double)acc[i], 256.0, (double)acl[i]);
                sc[i] = (float)__fma_rn(w, unit_lo, (double)nv);
                if (!is_tail || ((tail_mask >> i) & 1u)) m = fminf(m, sc[i]);   // (the rows that exist)
            }
        }
        if constexpr (SAMPLE) {
            a.sample_out[(long long)r31 * a.ns + sel * 2 + h] = m;
        } else {
            const u64 hit = __ballot(m <= thr_l);
            if (hit != 0) {
                u32 mask = le_mask16(sc, thr_l);
                if (is_tail) mask &= tail_mask;
                const u64 bal = __ballot(mask != 0);
                if (mask) {
                    const u32 pos = wcount + __builtin_amdgcn_mbcnt_hi((u32)(bal >> 32), __builtin_amdgcn_mbcnt_lo((u32)bal, 0u));
                    if (pos < a.wave_cap) {
                        wout[pos] = make_uint2((u32)(row0 + 4 * h), (mask << 16) | (u32)r31);
                        if (a.wave_score) a.wave_score[gw * a.wave_cap + pos] = m;   // (second-level threshold: sq_dense_tighten.hpp)
                    }
                }
                wcount += (u32)__popcll(bal);
            }
        }
    }
    if constexpr (!SAMPLE) {
        if (lane == 0) {
            a.wave_cnt[2 * gw] = wcount;   // entries written (beyond wave_cap: overflow)
            a.wave_cnt[2 * gw + 1] = 0u;   // first query tile of this wave's group
        }
    }
}

}  // namespace sq
