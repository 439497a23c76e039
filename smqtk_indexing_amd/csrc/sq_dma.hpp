// LDS-DMA helpers shared by the streaming kernels (dense scan, ITQ filter):
// per-wave HBM -> LDS copies that bypass registers, and the counted waits that
// order a wave's own ring without a workgroup barrier.
#pragma once
#include "sq_common.hpp"

namespace sq {

// (readfirstlane: a no-op where hipcc has the wave-uniform value in scalar registers anyway; where it has moved a
// uniform computation to the vector unit, the "s" constraint alone would be handed a VGPR)
__device__ __forceinline__ const void* uniform_ptr(const void* p) {
    const u64 v = (u64)(uintptr_t)p;
    const u32 lo = __builtin_amdgcn_readfirstlane((u32)v), hi = __builtin_amdgcn_readfirstlane((u32)(v >> 32));
    return (const void*)(uintptr_t)(((u64)hi << 32) | lo);
}
// LDS-DMA: 64 lanes x 16 bytes land at lds_dst + lane*16 (wave-uniform base in
// M0); the global source is a wave-uniform 64-bit base (SGPR pair) plus a
// per-lane 32-bit byte offset.  Issued from inline asm so that hipcc does not
// fence every later ds_read with vmcnt(0); completion is tracked by the counted
// waits below (cdna_hip_programming.md section 5.7).
// NT: non-temporal cache policy for bytes that are read once (a whole-matrix stream): they do not displace what
// other kernels keep in L2 / MALL and land sooner (MI355X_MICROARCH.md, "nt-weights").  Never for data that several
// workgroups re-read from L2.
template <bool NT = false>
__device__ __forceinline__ void glds16(const void* gbase_uniform, u32 voff, u32 lds_dst) {
    u32 keep;
    if constexpr (NT)
        asm volatile(
            "s_mov_b32 %0, m0\n\t"
            "s_mov_b32 m0, %3\n\t"
            "s_nop 0\n\t"
            "global_load_lds_dwordx4 %1, %2 nt\n\t"
            "s_mov_b32 m0, %0"
            : "=&s"(keep)
            : "v"(voff), "s"(uniform_ptr(gbase_uniform)), "s"(__builtin_amdgcn_readfirstlane(lds_dst))
            : "memory");
    else
        asm volatile(
            "s_mov_b32 %0, m0\n\t"
            "s_mov_b32 m0, %3\n\t"
            "s_nop 0\n\t"
            "global_load_lds_dwordx4 %1, %2\n\t"
            "s_mov_b32 m0, %0"
            : "=&s"(keep)
            : "v"(voff), "s"(uniform_ptr(gbase_uniform)), "s"(__builtin_amdgcn_readfirstlane(lds_dst))
            : "memory");
}
__device__ __forceinline__ void glds4(const void* gbase_uniform, u32 voff, u32 lds_dst) {
    u32 keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dword %1, %2\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(uniform_ptr(gbase_uniform)), "s"(__builtin_amdgcn_readfirstlane(lds_dst))
        : "memory");
}

// The same copies with M0 written once for several pieces: the instruction offset OFF (-4096 .. 4095) moves the LDS
// destination AND the global address, so a caller that wants the global address unshifted takes OFF off its per-lane
// offset.  Used where one wave per SIMD makes scalar issue slots count (five scalar instructions per piece in the
// self-contained form above).  Nothing else in those kernels touches M0 (gfx9 LDS instructions do not need it).
__device__ __forceinline__ void glds_set_m0(u32 lds_dst) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0" ::"s"(__builtin_amdgcn_readfirstlane(lds_dst)) : "memory");
}
template <int OFF, bool NT = false>
__device__ __forceinline__ void glds16_m0(const void* gbase_uniform, u32 voff) {
    static_assert(OFF >= -4096 && OFF <= 4095, "13-bit signed instruction offset");
    if constexpr (NT)
        asm volatile("global_load_lds_dwordx4 %0, %1 offset:%2 nt" ::"v"(voff), "s"(uniform_ptr(gbase_uniform)), "n"(OFF) : "memory");
    else
        asm volatile("global_load_lds_dwordx4 %0, %1 offset:%2" ::"v"(voff), "s"(uniform_ptr(gbase_uniform)), "n"(OFF) : "memory");
}
template <int OFF>
__device__ __forceinline__ void glds4_m0(const void* gbase_uniform, u32 voff) {
    static_assert(OFF >= -4096 && OFF <= 4095, "13-bit signed instruction offset");
    asm volatile("global_load_lds_dword %0, %1 offset:%2" ::"v"(voff), "s"(uniform_ptr(gbase_uniform)), "n"(OFF) : "memory");
}
// A whole ring unit in one statement (the int8 stream, sq_dense_i8.hpp): eight 1 KiB pieces behind ONE write of M0
// (= lds_dst + 4096: the instruction offsets -4096 .. 3072 reach the eight pieces, and `voff_s[j]` is the lane's source
// offset of piece j plus 4096 - 1024 j, so that the global address stays where it was), then -- TERMS -- the 256 bytes of
// row terms behind a second write.  Straight-line: no M0 save / restore (nothing else in these kernels reads M0, and
// hipcc keeps nothing in it across a statement), one wait state after each M0 write (SALU write of M0 -> LDS-DMA), no
// branch.  The "s" operands must come from scalar arithmetic, never straight from a v_readfirstlane (VALU write of an
// SGPR -> VMEM read of it: five wait states nobody would insert here).
#define SQ_GLDS16X8(NT_)                                              \
    "s_mov_b32 m0, %9\n\t"                                            \
    "s_nop 0\n\t"                                                     \
    "global_load_lds_dwordx4 %0, %8 offset:-4096" NT_ "\n\t"          \
    "global_load_lds_dwordx4 %1, %8 offset:-3072" NT_ "\n\t"          \
    "global_load_lds_dwordx4 %2, %8 offset:-2048" NT_ "\n\t"          \
    "global_load_lds_dwordx4 %3, %8 offset:-1024" NT_ "\n\t"          \
    "global_load_lds_dwordx4 %4, %8" NT_ "\n\t"                       \
    "global_load_lds_dwordx4 %5, %8 offset:1024" NT_ "\n\t"           \
    "global_load_lds_dwordx4 %6, %8 offset:2048" NT_ "\n\t"           \
    "global_load_lds_dwordx4 %7, %8 offset:3072" NT_
#define SQ_GLDS4_TERMS           \
    "\n\ts_mov_b32 m0, %10\n\t"  \
    "s_nop 0\n\t"                \
    "global_load_lds_dword %11, %12"
template <bool NT, bool TERMS>
__device__ __forceinline__ void glds_unit8(const void* gbase_uniform, const u32* voff_s, u32 lds_dst, const void* terms_uniform = nullptr,
                                           u32 voff_terms = 0, u32 lds_terms = 0) {
    const u32 m0a = __builtin_amdgcn_readfirstlane(lds_dst + 4096u), m0b = __builtin_amdgcn_readfirstlane(lds_terms);
    const void* gb = uniform_ptr(gbase_uniform);
    if constexpr (TERMS) {
        const void* tb = uniform_ptr(terms_uniform);
        if constexpr (NT)
            asm volatile(SQ_GLDS16X8(" nt") SQ_GLDS4_TERMS ::"v"(voff_s[0]), "v"(voff_s[1]), "v"(voff_s[2]), "v"(voff_s[3]), "v"(voff_s[4]),
                         "v"(voff_s[5]), "v"(voff_s[6]), "v"(voff_s[7]), "s"(gb), "s"(m0a), "s"(m0b), "v"(voff_terms), "s"(tb)
                         : "memory");
        else
            asm volatile(SQ_GLDS16X8("") SQ_GLDS4_TERMS ::"v"(voff_s[0]), "v"(voff_s[1]), "v"(voff_s[2]), "v"(voff_s[3]), "v"(voff_s[4]),
                         "v"(voff_s[5]), "v"(voff_s[6]), "v"(voff_s[7]), "s"(gb), "s"(m0a), "s"(m0b), "v"(voff_terms), "s"(tb)
                         : "memory");
    } else {
        if constexpr (NT)
            asm volatile(SQ_GLDS16X8(" nt")::"v"(voff_s[0]), "v"(voff_s[1]), "v"(voff_s[2]), "v"(voff_s[3]), "v"(voff_s[4]), "v"(voff_s[5]),
                         "v"(voff_s[6]), "v"(voff_s[7]), "s"(gb), "s"(m0a)
                         : "memory");
        else
            asm volatile(SQ_GLDS16X8("")::"v"(voff_s[0]), "v"(voff_s[1]), "v"(voff_s[2]), "v"(voff_s[3]), "v"(voff_s[4]), "v"(voff_s[5]),
                         "v"(voff_s[6]), "v"(voff_s[7]), "s"(gb), "s"(m0a)
                         : "memory");
    }
}
#undef SQ_GLDS16X8
#undef SQ_GLDS4_TERMS

// A ticket of a workgroup's LDS counter: lane 0 alone adds one (the statement narrows exec itself: every lane of the wave
// must be active) and the old value comes back wave-uniform.  One statement with its own wait, so nothing reads the
// register before the value has landed; hipcc's own sequence for `if (lane == 0) atomicAdd` is three times as long.
__device__ __forceinline__ u32 lds_ticket_take(u32 lds_addr) {
    u32 tv;
    u64 keep;
    asm volatile(
        "s_mov_b64 %1, exec\n\t"
        "s_mov_b64 exec, 1\n\t"
        "ds_add_rtn_u32 %0, %2, %3\n\t"
        "s_mov_b64 exec, %1\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(tv), "=&s"(keep)
        : "v"(lds_addr), "v"(1u)
        : "memory");
    return (u32)__builtin_amdgcn_readfirstlane((int)tv);
}

// call f(integral_constant<int, j>) for the one j in [0, N) that equals the (compile-time foldable) argument
template <int N, int J = 0, class F>
__device__ __forceinline__ void static_for_one(int j, F&& f) {
    if constexpr (J < N) {
        if (j == J)
            f(std::integral_constant<int, J>{});
        else
            static_for_one<N, J + 1>(j, f);
    }
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// Allow `units` younger units to stay outstanding.  PER = DMA instructions per
// unit: 8, or 9 when every unit also carries its tile's norms (KU == 1, L2).
// With KU > 1 only a tile's first unit has the norm load: counting 8 is then
// merely conservative.
template <int NSTAGE, int PER>
__device__ __forceinline__ void wait_units_in_flight(int units) {
    if constexpr (NSTAGE >= 4) {
        if (units >= 3) {
            wait_vmcnt<3 * PER>();
            return;
        }
    }
    if constexpr (NSTAGE >= 3) {
        if (units == 2) {
            wait_vmcnt<2 * PER>();
            return;
        }
    }
    if (units == 1)
        wait_vmcnt<PER>();
    else
        wait_vmcnt<0>();
}

// A store the counted waits know about: exactly one VMEM instruction under the current exec mask.
__device__ __forceinline__ void store_u64_counted(u64* p, u64 v) {
    asm volatile("global_store_dwordx2 %0, %1, off" ::"v"(p), "v"(v) : "memory");
}

// Allow `units` younger DMA units (PER instructions each) and the stores of `epis` younger tile epilogues
// (S store instructions each) to stay outstanding: vmcnt is one in-order queue for a wave's loads and stores.
template <int PER, int S, int EMAX, int U, int E>
__device__ __forceinline__ void wait_ops_rec(int units, int epis) {
    if (units == U && epis == E) {
        wait_vmcnt<(U * PER + E * S < 63 ? U * PER + E * S : 63)>();
        return;
    }
    if constexpr (E > 0)
        wait_ops_rec<PER, S, EMAX, U, E - 1>(units, epis);
    else if constexpr (U > 0)
        wait_ops_rec<PER, S, EMAX, U - 1, EMAX>(units, epis);
    else
        wait_vmcnt<0>();  // anything unexpected: drain
}
template <int NSTAGE, int PER, int S>
__device__ __forceinline__ void wait_ops_in_flight(int units, int epis) {
    wait_ops_rec<PER, S, NSTAGE, NSTAGE - 1, NSTAGE>(units, epis);
}

}  // namespace sq
