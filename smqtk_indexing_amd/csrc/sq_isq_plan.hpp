// The host's arithmetic around the IVF-SQ scans (sq_isq.hip): the LDS a scan workgroup stages and which of the two scans
// a slice of queries runs.  Everything else -- row chunks, key slices, the pair groups and their work items -- is
// sq_ivf_plan.hpp's.  Plain C++, no runtime header: tests/host/isq_shared_plan_main.cpp runs it on the CPU.
#pragma once
#include "sq_ivf_plan.hpp"

namespace sq {

static constexpr int kIsqSq8 = 0, kIsqF16 = 1;    // SQ_ISQ_SQ8 / SQ_ISQ_F16 (include/smqtk_hip_isq.h; sq_isq.hip asserts the two)
static constexpr int kIsqStageMax = 160 * 1024;   // dynamic LDS a per-query scan workgroup may ask for

// bytes of the per-query scan's LDS staging: the query, for SQ8 interleaved with vmin and step
inline long long isq_stage_bytes(int d, int kind) { return (kind == kIsqSq8 ? 3 : 1) * ivf_row_stride(d) * 4; }

// ------------------------------------------------------------------ the list-major scan (isq_scan_shared_kernel)
// Bytes of its LDS staging for groups of G = kIvfSharedGroup queries.  SQ8: per four dimensions vmin[4], step[4] and the
// G queries' four floats, (2 + G) * 4 adjacent floats -- the ranges are staged once for the group.  F16: the G queries,
// round_up(d, 4) floats each.
inline long long isq_shared_lds_bytes(int d, int kind) {
    return ((kind == kIsqSq8 ? 2 : 0) + kIvfSharedGroup) * ivf_row_stride(d) * 4;
}

// Option "isq_scan" = -1: pairs per list of the index from which a slice takes the list-major scan, per kind
// (profiles/ivf_sq_shared_scan.txt: the smallest of 1, 2, 4, 8 at which the list-major call is no slower than the
// per-query call on every measured batch the rule takes: at 1 pair per list both kinds still lose, 0.87 x and 0.91 x; at 4
// and 16 both gain; nothing was measured between 1 and 4).  0 would mean: never.
static constexpr long long kIsqSharedAutoRatioSq8 = 2;
static constexpr long long kIsqSharedAutoRatioF16 = 2;
inline long long isq_shared_auto_ratio(int kind) { return kind == kIsqSq8 ? kIsqSharedAutoRatioSq8 : kIsqSharedAutoRatioF16; }

// Which scan a slice of m queries x np probes runs: true = the list-major scan.  `mode` is option "isq_scan" (0 = the
// per-query scan, 1 = list-major wherever the kernel can run, -1 = list-major where the slice additionally has
// isq_shared_auto_ratio(kind) pairs per list of the index); `tree_depth` is pw_tree_depth(d).  The limits on pairs and
// work items are ivf_scan_route's: one sort, a one-dimensional grid.
inline bool isq_scan_route(int mode, int kind, int d, int tree_depth, long long m, long long np, long long nlist, long long cands) {
    if (mode == 0) return false;
    if (isq_shared_lds_bytes(d, kind) > kIvfSharedLdsBytes || tree_depth > kIvfSharedDepth) return false;
    const long long pairs = m * np;
    if (pairs < 1 || pairs > kIvfSharedMaxPairs || ivf_shared_items_bound(cands, pairs) > kIvfSharedMaxItems) return false;
    if (mode > 0) return true;
    const long long ratio = isq_shared_auto_ratio(kind);
    return ratio > 0 && pairs >= ratio * nlist;
}

}  // namespace sq
