// ITQ hash codes in the reference's own arithmetic: the float64 kernels of sq_itq.hip.
//
// ItqArgs (what every ITQ kernel of a call is handed), numpy's correctly rounded element operations and row norms
// (itq_norms_kernel), and itq_hash_kernel: z = (v - mean) . R on v_mfma_f64_16x16x4_f64, sign bits packed MSB first
// (see sq_itq.hip for the contract).  The certified filters (sq_itq_fast.hpp, sq_itq_wide.hpp, sq_itq_xwide.hpp) leave
// their undecided bits to float64 evaluations that follow this arithmetic, and include this header for it.
#pragma once
#include "sq_common.hpp"
#include "sq_pairwise.hpp"

namespace sq {


typedef double f64x4 __attribute__((ext_vector_type(4)));

struct ItqArgs {
    const void* x;
    long long n;
    int d;
    const double* mean;
    const double* rot;  // [d][bits]
    int bits;
    int words;          // W = ceil(bits/64)
    int pad;            // W*64 - bits leading zero columns
    int norm;           // SQ_NORM_NONE / SQ_NORM_L2 / _L1 / _L0 / _INF / _NEG_INF
    u64* out;           // [n][W]
    int dk;             // k rows of R staged per chunk (multiple of 16)
    int nchunks;
    int d16;            // d rounded up to 16
    const void* nrm;    // [n] row L2 norms in x's dtype (normalize=2), from itq_norms_kernel
    int vec4;           // rows are 4-element aligned (d % 4 == 0, base aligned): vector loads of x
    int sub32;              // x - mean in float32 (float32 rows and a float32 model mean: numpy's promotion)
    const u32* list;        // optional: only these rows (the filter's uncertain rows, sq_itq_fast.hpp)
    const u32* list_total;  // device count of `list`
    int exact;              // option "itq_exact" of the call (the model handle's override, or the process-wide value)
    int debug;              // option "dense_debug" of the call (ablation bits)
};

template <class T>
struct Vec4;
template <>
struct Vec4<float> {
    typedef float type __attribute__((ext_vector_type(4)));
};
template <>
struct Vec4<double> {
    typedef double type __attribute__((ext_vector_type(4)));
};

__device__ __forceinline__ float div_rn(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ double div_rn(double a, double b) { return __ddiv_rn(a, b); }
__device__ __forceinline__ float mul_rn(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ double mul_rn(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ float sqrt_rn(float a) { return (float)sqrt((double)a); }
__device__ __forceinline__ double sqrt_rn(double a) { return sqrt(a); }

// Row norms in numpy's arithmetic (itq.py:185: np.linalg.norm(v, ord, axis, keepdims), numpy/linalg/linalg.py):
//   ord 2:    sqrt(add.reduce(x * x))      pairwise float sum in x's dtype, correctly rounded sqrt
//   ord 1:    add.reduce(abs(x))           the same pairwise sum of |x|
//   ord 0:    (x != 0).astype(dtype).sum() (exact: small integers)
//   ord inf:  abs(x).max()     ord -inf: abs(x).min()      (a NaN wins, as in numpy's maximum / minimum)
// and 0 -> 1 (itq.py:187).  8 lanes per row.  Kept out of the MFMA kernel so that one stays within 256
// VGPRs (two workgroups per CU) without spilling.
__device__ __forceinline__ float abs_t(float v) { return fabsf(v); }
__device__ __forceinline__ double abs_t(double v) { return fabs(v); }
template <class T>
__global__ __launch_bounds__(256) void itq_norms_kernel(const T* __restrict__ X, long long n_all, int d, T* __restrict__ nrm,
                                                        const u32* __restrict__ list, const u32* __restrict__ list_total,
                                                        int ord) {
    const int j8 = threadIdx.x & 7;
    const long long stride = (long long)gridDim.x * 32;
    const long long n = list ? (long long)*list_total : n_all;  // listed rows only (sq_itq_fast.hpp), or all
    for (long long row0 = (long long)blockIdx.x * 32; row0 < n; row0 += stride) {
        long long row = row0 + (threadIdx.x >> 3);
        const bool live = row < n;
        row = live ? row : n - 1;
        if (list) row = (long long)list[row];
        const T* xr = X + row * d;
        T nv;
        if (ord == SQ_NORM_INF || ord == SQ_NORM_NEG_INF) {
            const bool mx = ord == SQ_NORM_INF;
            T m = abs_t(xr[j8 < d ? j8 : 0]);
            bool nan = m != m;
            for (int i = j8 + 8; i < d; i += 8) {
                const T v = abs_t(xr[i]);
                nan |= v != v;
                m = mx ? (v > m ? v : m) : (v < m ? v : m);
            }
            for (int o = 1; o < 8; o <<= 1) {
                const T v = __shfl_xor(m, o);
                nan |= (bool)__shfl_xor((int)nan, o);
                m = mx ? (v > m ? v : m) : (v < m ? v : m);
            }
            nv = nan ? (T)__builtin_nanf("") : m;
        } else if (ord == SQ_NORM_L1) {
            auto term = [xr](int i) { return abs_t(xr[i]); };
            nv = np_pairwise_sum<T>(term, d, j8);
        } else if (ord == SQ_NORM_L0) {
            auto term = [xr](int i) { return xr[i] != (T)0 ? (T)1 : (T)0; };
            nv = np_pairwise_sum<T>(term, d, j8);
        } else {
            auto term = [xr](int i) { return mul_rn(xr[i], xr[i]); };
            nv = sqrt_rn(np_pairwise_sum<T>(term, d, j8));
        }
        if (nv == (T)0) nv = (T)1;
        if (live && j8 == 0) nrm[row] = nv;
    }
}

// CT column tiles of 16 hash bits per pass (CT*16 padded columns), RT = 16/CT
// row tiles of 16 rows per wave.  grid.y walks groups of CT*16 columns.
template <class T, int CT>
__global__ __launch_bounds__(256, 2) void itq_hash_kernel(ItqArgs a) {
    constexpr int RT = 16 / CT;
    constexpr int NCOL = CT * 16;
    constexpr int RSTRIDE = NCOL + 4;        // f64 per staged R row (+32 B: lanes l and l+16 hit different bank halves)
    constexpr int ROWS_PER_WAVE = RT * 16;
    constexpr int ROWS_PER_BLOCK = 4 * ROWS_PER_WAVE;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* s_mean = reinterpret_cast<double*>(smem);                 // [d16]
    double* s_rot = s_mean + a.d16;                                    // [dk][RSTRIDE]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const T* X = reinterpret_cast<const T*>(a.x);
    const int col0 = blockIdx.y * NCOL;      // first padded column of this group

    for (int i = threadIdx.x; i < a.d16; i += 256) s_mean[i] = i < a.d ? a.mean[i] : 0.0;

    auto stage_rot = [&](int chunk) {
        const int k0 = chunk * a.dk;
        for (int e = threadIdx.x; e < a.dk * NCOL; e += 256) {
            const int kr = e / NCOL, pc = e - kr * NCOL;
            const int k = k0 + kr;
            const int b = col0 + pc - a.pad;
            double v = 0.0;
            if (k < a.d && b >= 0 && b < a.bits) v = a.rot[(long long)k * a.bits + b];
            s_rot[kr * RSTRIDE + pc] = v;
        }
    };
    if (a.nchunks == 1) stage_rot(0);
    __syncthreads();

    // rows to do: all n, or the listed ones (virtual row v -> list[v])
    const long long nrows = a.list ? (long long)*a.list_total : a.n;
    const long long nblocks = (nrows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    for (long long blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const long long wrow0 = blk * ROWS_PER_BLOCK + (long long)wave * ROWS_PER_WAVE;
        f64x4 acc[RT][CT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = f64x4{0.0, 0.0, 0.0, 0.0};
        T nrm_l[RT];
        const T* xrow[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            long long row = wrow0 + rt * 16 + l15;
            row = row < nrows ? row : nrows - 1;
            if (a.list) row = (long long)a.list[row];
            xrow[rt] = X + row * a.d;
            nrm_l[rt] = a.nrm ? reinterpret_cast<const T*>(a.nrm)[row] : (T)1;
        }
        for (int chunk = 0; chunk < a.nchunks; ++chunk) {
            if (a.nchunks > 1) {
                __syncthreads();
                stage_rot(chunk);
                __syncthreads();
            }
            const int k0 = chunk * a.dk;
            for (int c = 0; c < a.dk; c += 16) {
                const int kb = k0 + c + 4 * g;  // this lane's 4 consecutive k
                if (k0 + c >= a.d16) break;
                double av[RT][4];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    T xq[4];
                    if (a.vec4 && kb < a.d) {  // d % 4 == 0 and 16-byte aligned rows: one vector load
                        const typename Vec4<T>::type v4 = *reinterpret_cast<const typename Vec4<T>::type*>(xrow[rt] + kb);
#pragma unroll
                        for (int j = 0; j < 4; ++j) xq[j] = v4[j];
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) xq[j] = (kb + j < a.d) ? xrow[rt][kb + j] : (T)0;
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int k = kb + j;
                        double v = 0.0;
                        if (k < a.d) {
                            T xv = xq[j];
                            if (a.nrm) xv = div_rn(xv, nrm_l[rt]);
                            if constexpr (sizeof(T) == 4) {
                                if (a.sub32)
                                    v = (double)__fsub_rn(xv, (float)s_mean[k]);  // s_mean[k] is a float32 value
                                else
                                    v = __dsub_rn((double)xv, s_mean[k]);
                            } else {
                                v = __dsub_rn((double)xv, s_mean[k]);
                            }
                        }
                        av[rt][j] = v;
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double* brow = s_rot + (size_t)(c + 4 * g + j) * RSTRIDE + l15;
                    double bv[CT];
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct) bv[ct] = brow[ct * 16];
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                        for (int ct = 0; ct < CT; ++ct)
                            acc[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[rt][j], bv[ct], acc[rt][ct], 0, 0, 0);
                }
            }
        }
        // ---- sign bits -> packed words.  D layout: col = lane&15, row = (lane>>4) + 4*reg
        constexpr int WPG = (CT + 3) / 4;  // words per column group
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            u64 cw[4][WPG];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int w = 0; w < WPG; ++w) cw[r][w] = 0ull;
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const u64 m = __ballot(acc[rt][ct][r] >= 0.0);
                    const u32 m16 = (u32)(m >> (16 * g)) & 0xffffu;
                    const u64 rev = (u64)(__brev(m16) >> 16);  // column 0 -> most significant of the 16
                    cw[r][ct / 4] |= rev << (48 - 16 * (ct % 4));
                }
            }
            if (l15 == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    long long row = wrow0 + rt * 16 + g + 4 * r;
                    if (row < nrows) {
                        if (a.list) row = (long long)a.list[row];
#pragma unroll
                        for (int w = 0; w < WPG; ++w) {
                            const int gw = blockIdx.y * (NCOL / 64) + w;
                            if (gw < a.words) {
                                u64 v = cw[r][w];
                                if (gw == 0 && a.pad > 0) v &= (~0ull) >> a.pad;
                                a.out[row * a.words + gw] = v;
                            }
                        }
                    }
                }
            }
        }
    }
}

template <class T, int CT>
static int itq_launch_t(const ItqArgs& a0, hipStream_t st, int device) {
    ItqArgs a = a0;
    constexpr int NCOL = CT * 16, RSTRIDE = NCOL + 4, RT = 16 / CT;
    const size_t fixed = (size_t)a.d16 * 8;
    size_t budget = 76 * 1024;  // two workgroups per CU: one hides the other's load + conversion phase
    // (8192-d rows with 256-bit codes: the mean alone is 64 KB -- one workgroup per CU rather than a refusal; the
    // chunking does not touch the order of a sum)
    if (fixed + (size_t)16 * RSTRIDE * 8 > budget) budget = 156 * 1024;
    if (fixed + (size_t)16 * RSTRIDE * 8 > budget)
        return fail(SQ_ERR_UNSUPPORTED, "sq_itq_hash: d=%d too large for the LDS mean vector", a.d);
    int dk = (int)((budget - fixed) / ((size_t)RSTRIDE * 8));
    dk = dk / 16 * 16;
    if (dk > a.d16) dk = a.d16;
    a.dk = dk;
    a.nchunks = (a.d16 + dk - 1) / dk;
    a.vec4 = (a.d % 4 == 0) && (reinterpret_cast<uintptr_t>(a.x) % (4 * sizeof(T)) == 0);
    const size_t lds = fixed + (size_t)dk * RSTRIDE * 8;
    const long long rows_per_block = 4ll * RT * 16;
    const long long nblocks = (a.n + rows_per_block - 1) / rows_per_block;
    long long gx = 2ll * cu_count(device);
    if (gx > nblocks) gx = nblocks;
    const int groups = (a.words * 64 + NCOL - 1) / NCOL;
    return launch_lds<itq_hash_kernel<T, CT>>(160 * 1024, dim3((unsigned)gx, (unsigned)groups), dim3(256), lds, st, a);
}

}  // namespace sq
