// The scalar codecs of include/smqtk_hip_isq.h -- 8-bit codes with trained ranges, float16 -- and the kernel that codes
// float32 rows with them: one piece of code for the IVF-SQ lists (sq_isq.hip) and the refine store (sq_refine.hip), whose
// third kind keeps the float32 row itself.
#pragma once
#include "sq_common.hpp"

namespace sq {

typedef unsigned char u8;
typedef unsigned short u16;

static constexpr int kCodecSq8 = 0, kCodecF16 = 1, kCodecF32 = 2;   // SQ_ISQ_SQ8 / SQ_ISQ_F16, SQ_REFINE_SQ8 / _F16 / _F32

// bytes of one code and of a stored row (whole 16-byte pieces, zero padded)
inline int isq_code_bytes(int kind) { return kind == kCodecF32 ? 4 : kind == kCodecF16 ? 2 : 1; }
inline long long isq_row_stride(int d, int kind) { return ((long long)d * isq_code_bytes(kind) + 15) / 16 * 16; }

__device__ __forceinline__ u32 isq_encode_sq8(float x, float vmin, float step) {
    const float t = __fdiv_rn(__fsub_rn(x, vmin), step);
    return (step != 0.f && t > 0.f) ? (u32)fminf(rintf(t), 255.f) : 0u;   // NaN compares false: code 0
}
__device__ __forceinline__ float isq_decode_sq8(float code, float vmin, float step) { return __fadd_rn(vmin, __fmul_rn(step, code)); }
__device__ __forceinline__ u32 isq_encode_f16(float x) {
    const _Float16 h = (_Float16)x;   // v_cvt_f16_f32: nearest even, subnormal halves kept, overflow to inf
    return (u32)__builtin_bit_cast(u16, h);
}

// Float32 rows (stride d, any alignment) -> padded code rows in the order of the add.  A lane writes one dword of a
// code row -- four 8-bit codes, two halves or one float -- so a wave's stores are contiguous; the padding behind d is zero.
template <int KIND>
static __global__ __launch_bounds__(256) void isq_encode_kernel(const float* __restrict__ src, int d, long long n,
                                                                 const float* __restrict__ vmin, const float* __restrict__ step,
                                                                 long long wpr /* dwords per code row */, u32* __restrict__ out) {
    constexpr int PER = KIND == kCodecSq8 ? 4 : KIND == kCodecF16 ? 2 : 1;
    const long long total = n * wpr;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const long long r = idx / wpr;
        const int i0 = (int)(idx - r * wpr) * PER;
        u32 word = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = i0 + j;
            if (i < d) {
                const float v = src[r * d + i];
                if constexpr (KIND == kCodecSq8) word |= isq_encode_sq8(v, vmin[i], step[i]) << (8 * j);
                else if constexpr (KIND == kCodecF16) word |= isq_encode_f16(v) << (16 * j);
                else word = __float_as_uint(v);
            }
        }
        out[idx] = word;
    }
}

}  // namespace sq
