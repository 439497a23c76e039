// The tile and slab arithmetic of opq_apply_kernel (sq_opq.hip), plain C++: what a workgroup holds in LDS for a row width,
// which of the two staging paths a width takes, and how many workgroups a call launches.  tests/host/opq_plan_main.cpp walks
// every width under the host sanitizers.
#pragma once

namespace sq {

static constexpr int kOpqMaxD = 4096;          // widest row sq_opq_create takes
static constexpr int kOpqTileRows = 64;        // rows a workgroup owns at a time: two 32-row MFMA tiles
static constexpr int kOpqColBlock = 128;       // output columns per pass over k: 2 x 2 waves of 32 rows x 64 columns each
static constexpr int kOpqSlabK = 32;           // k elements of A (and, past kOpqResidentMaxD, of the rows) in LDS at a time
static constexpr int kOpqKStep = 8;            // k elements per 16-byte operand read: four MFMAs of k = 2, both lane halves
static constexpr int kOpqResidentMaxD = 512;   // up to here the whole row tile stays in LDS across the column blocks
static constexpr int kOpqLdsMax = 160 * 1024;  // dynamic LDS a workgroup may ask for
static constexpr int kOpqBlocksPerCu = 8;      // workgroups a call launches per compute unit at the most; they loop over the tiles

// LDS pitch of an operand row of `k` elements, in floats: k rounded up to the k step, and four more.  Bank arithmetic: an
// MFMA operand read is one 16-byte read per lane, lane l at row l % 32 and k offset 4 (l / 32); a pitch of 8 m + 4 floats
// is 4 (2 m + 1) dwords, an odd multiple of four, so 16 consecutive rows start at the 16 distinct multiples of four modulo
// 64 and their 4-dword reads cover the 64 banks once.  (A pitch of 32 or 512 floats would put every row on the same four.)
inline int opq_pitch(int k) { return (k + kOpqKStep - 1) / kOpqKStep * kOpqKStep + 4; }

struct OpqPlan {
    int d = 0;
    int lda = 0;        // floats per row of the device copy of A: d rounded up to 4, zero padded, so A is always read in 16-byte pieces
    int resident = 0;   // 1: the row tile is staged once, whole; 0: a k slab of it beside every slab of A
    int sx = 0, sa = 0; // LDS pitches of the row tile and of the slab of A
    int nslab = 0;      // k slabs per column block
    int ncb = 0;        // column blocks
    int lds_bytes = 0;  // dynamic LDS: [kOpqTileRows][sx] then [kOpqColBlock][sa] floats
};

inline OpqPlan opq_plan(int d) {
    OpqPlan p;
    p.d = d;
    p.lda = (d + 3) / 4 * 4;
    p.resident = d <= kOpqResidentMaxD ? 1 : 0;
    p.sx = opq_pitch(p.resident ? d : kOpqSlabK);
    p.sa = opq_pitch(kOpqSlabK);
    p.nslab = (d + kOpqSlabK - 1) / kOpqSlabK;
    p.ncb = (d + kOpqColBlock - 1) / kOpqColBlock;
    p.lds_bytes = (kOpqTileRows * p.sx + kOpqColBlock * p.sa) * 4;
    return p;
}

// k steps of slab s that hold an element of the row: the steps behind them are never read (the last one is zero padded)
inline int opq_slab_steps(int d, int s) {
    const int left = d - s * kOpqSlabK;
    return ((left < kOpqSlabK ? left : kOpqSlabK) + kOpqKStep - 1) / kOpqKStep;
}

inline long long opq_tiles(long long n) { return (n + kOpqTileRows - 1) / kOpqTileRows; }
// workgroups of a call over `tiles` row tiles on `cus` compute units: workgroup b takes tiles b, b + grid, ...
inline unsigned opq_grid(long long tiles, int cus) {
    const long long cap = (long long)(cus > 0 ? cus : 1) * kOpqBlocksPerCu;
    return (unsigned)(tiles < cap ? (tiles > 0 ? tiles : 1) : cap);
}

}  // namespace sq
