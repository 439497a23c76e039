// The host arithmetic of ivf_assign_kernel (sq_ivf_assign.hpp), plain C++: which calls the kernel takes, what a workgroup
// holds in LDS for a row width, how many workgroups a call launches, and the slack of its certificate.
#pragma once
#include <cmath>

#ifdef __HIPCC__
#define SQ_ASG_HD __host__ __device__
#else
#define SQ_ASG_HD
#endif

namespace sq {

static constexpr int kAsgMaxD = 1024;          // widest row the kernel takes: the slack's gamma bounds are stated up to here
static constexpr int kAsgMaxLists = 65536;     // as the coarse index (kIvfMaxLists)
static constexpr int kAsgTileRows = 128;       // rows a workgroup owns at a time: 32 per wave, the N operand of its MFMAs
static constexpr int kAsgColBlock = 128;       // centroids per pass over k: four 32 x 32 tiles per wave, 64 accumulators
static constexpr int kAsgSlabK = 32;           // k elements of the centroids (and, past kAsgResidentMaxD, of the rows) per LDS buffer
static constexpr int kAsgKStep = 8;            // k elements per 16-byte operand read: four MFMAs of k = 2, both lane halves
static constexpr int kAsgResidentMaxD = 240;   // up to here the whole row tile stays in LDS over the centroid loop
static constexpr int kAsgLdsMax = 160 * 1024;  // dynamic LDS a workgroup may ask for
static constexpr int kAsgBlocksPerCu = 4;      // workgroups a call launches per compute unit at the most; they loop over the tiles

// LDS pitch of an operand row of `k` elements, in floats: k rounded up to the k step, and four more -- an odd multiple of
// four dwords, so the 16-byte operand reads of 16 consecutive rows cover the 64 banks once (sq_opq_plan.hpp: opq_pitch).
inline int asg_pitch(int k) { return (k + kAsgKStep - 1) / kAsgKStep * kAsgKStep + 4; }

struct AsgPlan {
    int d = 0, nlist = 0;
    int resident = 0;   // 1: the row tile is staged once, whole; 0: a k slab of it beside every slab of the centroids
    int sx = 0, sc = 0; // LDS pitches of the row tile and of a centroid slab
    int nslab = 0;      // k slabs per centroid block
    int ncb = 0;        // centroid blocks
    int x_floats = 0;   // floats of the row tile's part of LDS (resident: one tile; else two slab buffers)
    int lds_bytes = 0;  // dynamic LDS: the row part, then two centroid slab buffers of [kAsgColBlock][sc] floats
};

inline AsgPlan asg_plan(int d, int nlist) {
    AsgPlan p;
    p.d = d;
    p.nlist = nlist;
    p.resident = d <= kAsgResidentMaxD ? 1 : 0;
    p.sx = asg_pitch(p.resident ? d : kAsgSlabK);
    p.sc = asg_pitch(kAsgSlabK);
    p.nslab = (d + kAsgSlabK - 1) / kAsgSlabK;
    p.ncb = (nlist + kAsgColBlock - 1) / kAsgColBlock;
    p.x_floats = kAsgTileRows * p.sx * (p.resident ? 1 : 2);
    p.lds_bytes = (p.x_floats + 2 * kAsgColBlock * p.sc) * 4;
    return p;
}

// k steps of slab s that hold an element of the row: the steps behind them are never read (the last one is zero padded)
inline int asg_slab_steps(int d, int s) {
    const int left = d - s * kAsgSlabK;
    return ((left < kAsgSlabK ? left : kAsgSlabK) + kAsgKStep - 1) / kAsgKStep;
}

inline long long asg_tiles(long long n) { return (n + kAsgTileRows - 1) / kAsgTileRows; }
inline unsigned asg_grid(long long tiles, int cus) {
    const long long cap = (long long)(cus > 0 ? cus : 1) * kAsgBlocksPerCu;
    return (unsigned)(tiles < cap ? (tiles > 0 ? tiles : 1) : cap);
}

// The calls the kernel takes: float32 rows of 1 .. kAsgMaxD elements, up to 65536 centroids, as many rows as one counting
// sort takes (row numbers are 32-bit in the undecided list).  Everything else is the sliced dense search.
inline bool ivf_assign_route(long long n, int d, int nlist) {
    return n >= 1 && n <= (1ll << 26) && d >= 1 && d <= kAsgMaxD && nlist >= 1 && nlist <= kAsgMaxLists;
}

// The slack T of a row: the row is decided when second - best > T (DESIGN.md 4.16 derives every term).
//   xn2:   the kernel's float32 sum of the row's squares (any order); cmax2: the largest float32 |c_l|^2.
//   u = 2^-24.  With X >= |x| and C >= max |c_l|:
//     8 (d + 8) u X C                  twice the MFMA dot product's error doubled by the factor 2 of the score, rounding
//                                      unit 2 u (any faithful rounding), d + 8 terms (zero padding), any order
//     + 5 u (X C + C^2)                twice: n_l rounded once from float64, the score's subtraction rounded once
//     + 2 (d + 7) u (X + C)^2          the exact path: gamma_{d+2} on each of two squared sums, and the factor
//                                      1 + 5 u that separates two floats whose square roots round apart
//   all of it times 1.001 (gamma_k <= 1.0001 k u for k <= 1640, X and C from rounded sums, this function's own roundings)
//   plus 2^-60 (1 + X + C)^2 for everything that underflows.
// Beyond (X + C)^2 = 1e37 a sum may overflow: the slack is +inf.  NaN in, NaN out; the caller compares with `>`.
SQ_ASG_HD inline float ivf_assign_slack(int d, float xn2, float cmax2) {
    const float u = 5.9604644775390625e-8f;   // 2^-24
    const float X = sqrtf(xn2), C = sqrtf(cmax2);
    const float P = (X + C) * (X + C);
    const float fd = (float)d;
    const float rel = (8.f * fd + 64.f) * (X * C) + 5.f * (X * C + C * C) + (2.f * fd + 14.f) * P;
    const float T = 1.001f * u * rel + 8.673617379884035e-19f * ((1.f + X + C) * (1.f + X + C));   // 2^-60
    return P < 1e37f ? T : (P != P ? P : __builtin_inff());
}

}  // namespace sq
