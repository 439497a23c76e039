// Exact brute-force L2 / cosine top-k over a float32 descriptor matrix (gfx950).
//
// What it replaces: the per-candidate python distance calls + stable sort of
// LSHNearestNeighborIndex._nn (smqtk_indexing/impls/nn_index/lsh.py:505-519)
// and the faiss "IDMap,Flat" search + recompute of
// FaissNearestNeighborsIndex._nn (impls/nn_index/faiss.py:751-831), both of
// which evaluate metrics.euclidean_distance / cosine_distance
// (utils/metrics.py:73-86, 89-137) for every row and keep the n smallest.
//
// Structure:
//   1. dense_scan_kernel (sq_dense_scan.hpp) streams a bfloat16 copy of the
//      matrix (L2: of the rows minus their column means) once per group of 1, 2
//      or 4 32-query tiles: LDS-DMA ring per wave, bf16 MFMA (x_hi*q_hi
//      [+ x_hi*q_lo]), scores s = |x|^2 - 2 x.q (cosine: -x^.q^) compared with a
//      per-query threshold; survivors leave as per-wave lists of (first row,
//      mask, query) entries.  The threshold comes from the same kernel in SAMPLE
//      mode over every S-th tile + kth_threshold_f32_kernel.
//   1b. calls of up to 32 queries over rows of up to 512 dimensions stream an int8 copy instead (dense8_scan_kernel,
//      sq_dense_i8.hpp: one scale per matrix, residuals measured per row at build): half the bytes, same downstream.
//   2. dense_rerank_*_kernel (sq_dense_exact.hpp) recomputes the distance of every
//      survivor from the ORIGINAL float32 rows in the REFERENCE arithmetic
//      (float32 subtract, square, numpy pairwise order, correctly rounded sqrt;
//      cosine in float64, scipy's order) and forms (distance, row) keys.
//   3. select_topk_kernel sorts the keys; its post-op (DenseFinalize*) converts and
//      CERTIFIES each query against the filter's error bound.  Queries that fail
//      (or overflow their list) are redone on the exact full-keys path.
//
// Host driver: dense_enqueue chooses the stage that takes a call (dense_small_ / dense8_wide_ / dense8_ / dense_bf16_enqueue);
// the chains end in dense_survivor_tail.  dense_resolve: dense_resolve_wait, dense_mid_tier, dense_exact_path.  Slots: sq_pipeline.hpp.
#include <algorithm>
#include <type_traits>
#include <vector>
#include <cmath>

#include "sq_dense_exact.hpp"
#include "sq_dense_scan.hpp"
#include "sq_dense_mid.hpp"
#include "sq_dense_i8.hpp"
#include "sq_dense_wide.hpp"
#include "sq_dense_i8_wide.hpp"
#include "sq_dense_tighten.hpp"
#include "sq_dense_remove.hpp"

namespace sq {

// Per-call workspace: the slots of the handle's CallRing (sq_pipeline.hpp has the rotation).  The kernels of call i + 1 are enqueued --
// and, with the slots' own streams, partly run -- while call i is still on the device; dense_resolve reads a call's status words.
struct DenseCall {
    bool pending = false;
    const float* q = nullptr;
    int nq = 0, k = 0, nq_pad = 0;
    void* out_dist = nullptr;
    long long* out_idx = nullptr;
    hipStream_t st = nullptr;     // the stream the call's kernels were enqueued on
    bool small = false, all_fallback = false, prof = false, use_event = false, int8 = false;
    bool mid_direct = false;    // no first filter ran (it is suspended: DenseHandle::first_suspended): every query starts at the middle tier
    u32 cap = 0;                  // candidate-list length the call was enqueued with
    sq_stats_t stats{};
};
struct DenseSlot {
    DevBuf q_scaled, q_al, qn2, thr, wave_out, wave_cnt, cnt, keys, sample, out_keys, cos_nq, oflag;
    DevBuf q8, par8;              // int8 filter: the query tile's plane and {score unit, e_q}
    DevBuf clk8;                  // measurement ("dense_debug" & 8192): the body kernel's per-workgroup clocks
    int clk8_wgs = 0;
    DevBuf wave_score, hist8;     // ... the fused call's tightened threshold: an entry's smallest score, the per-query histograms
    DevBuf tg;                    // the wide-row path's second-level threshold (sq_dense_tighten.hpp): [hist | raw thresholds | T'' | keys of T'']
    void* tg_zeroed = nullptr;    // the allocation of tg that has been wiped once (its histogram is zero between calls)
    DevBuf sort_tmp;              // scratch of the any-k sorted select (k beyond the one-workgroup select): one per call in flight
    HostPinned status_host;
    // captured call graph of the int8 path ("dense_graph"): one hipGraphLaunch instead of six kernel launches per call
    HostPinned call_ptrs;         // DenseCallPtrs of the call in flight
    hipGraphExec_t gexec = nullptr;
    u64 gkey = 0, seen_key = 0;   // what gexec was captured for / the key of the slot's last eager call
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // call start, scan start, scan end, call end, re-rank end
    SlotSync sync;                // the slot's internal stream (asynchronous calls with "dense_async_streams" = 2) and its ordering events (sq_pipeline.hpp)
    DenseCall call;
    void drop_graph() {   // (a captured call graph holds the index's shape and buffers: sq_dense_compact)
        if (gexec) (void)hipGraphExecDestroy(gexec), gexec = nullptr;
        gkey = seen_key = 0;
    }
    ~DenseSlot() {   // (the buffers and `sync` free themselves, after this body)
        drop_graph();
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

// The int8 first-stage filter's copy (sq_dense_i8.hpp): the copy, its row terms, what the build measured and how the
// filter has fared since.  A handle keeps the two buffers exactly while `use` is set (dense8_build, dense8_append).
struct Int8Copy {
    DevBuf scan, nrow;          // int8 rows [n_alloc][row_bytes] (wide rows: + I8W_SPARE), float32 row terms [n_alloc + 64]
    bool use = false;           // the copy exists (and follows appends)
    bool suspended = false;     // ... but automatic mode (dense_int8 = -1) leaves it alone: its lists overflowed three calls in a row.  dense_int8 = 1 re-arms it, a rebuild (the index doubled) too
    int overflow = 0;           // calls in a row in which the filter's lists overflowed (data it does not suit)
    int row_bytes = 0;          // 128, 256 or 512; rows beyond 512 dimensions (sq_dense_i8_wide.hpp): a multiple of 128
    long long n_pass = 0;       // rows a pass covers (what sq_stats_t.bytes_scanned prices): whole 64-row units, wide rows whole 32-row tiles
    long long n_alloc = 0;      // rows the copy is allocated and padded for: a multiple of 128 (the largest ring unit)
    float dx = 0.f, cut = 0.f;  // the build's step and residual cut (R^2 rounded down): rows appended later are quantised and flagged with them
    double rmax = 0.0, xmax = 0.0;   // R and X of the filter's error bound: the largest residual and the largest |x'| of the rows under the cut
    long long flagged = 0;      // always-candidate rows (beyond the cut)
    long long n8_built = 0;     // rows the clamp was last chosen from, accepted or not (an index twice that size chooses again)
    void drop() { scan.release(), nrow.release(), use = false; }   // (n8_built stays: the attempt counts)
    // a call may take the int8 stage / what sq_dense_info reports as "in use" and as the copy's bytes
    bool active(const Options& o) const { return use && o.dense_int8 != 0 && !(suspended && o.dense_int8 < 0); }
    bool in_use() const { return use && !suspended; }
    size_t bytes() const {
        // (rows beyond 512 dimensions: the bytes the copy occupies, not its allocations -- it follows every append)
        if (use && row_bytes > I8_MAX_ROW_BYTES) return (size_t)n_alloc * row_bytes + I8W_SPARE + (size_t)(n_alloc + 64) * 4;
        return scan.cap + nrow.cap;
    }
    // an int8 stage takes a call although automatic mode had suspended it (dense_int8 = 1 on the handle): the filter is
    // armed again (and judged again from the next calls: three heavy ones in a row suspend it)
    void rearm() { if (suspended) suspended = false, overflow = 0; }
    void note_overflow(bool heavy, const Options& o) {
        overflow = heavy ? overflow + 1 : 0;
        if (overflow >= 3 && o.dense_int8 < 0) suspended = true;
    }
};

struct DenseHandle : HandleBase {
    const float* db = nullptr;  // device [n][ld], the caller's float32 rows (borrowed or owned)
    DevBuf owned;
    DevBuf scan;                // bfloat16 scan copy [n_pad][d_pad*2 bytes]
    DevBuf norms;               // float32 |x - c|^2 [n_pad] (cosine: of the rows themselves)
    DevBuf center;              // float32 c [d_pad]: column means (L2), the filter's origin
    DevBuf cos_nx;              // float64 |x|^2 [n] in the reference order (cosine re-rank)
    long long n = 0, n_pad = 0;
    int d = 0, d_pad = 0;
    long long ld = 0;
    int metric = SQ_METRIC_L2;
    long long id_base = 0;
    double xn2_max = 0.0;       // max squared row norm (error bound of the L2 filter)
    Int8Copy i8;                // the int8 first-stage filter
    bool graph_broken = false;  // a call-graph capture failed on this handle: eager launches from then on
    long long build_us = 0, build8_us = 0;   // sq_dense_info: wall time of sq_dense_create / of its int8 part
    DevBuf norms1;  // L2: |x|^2 (1 - alpha) for one query plane (`norms`: two planes)
    // rows taken out by sq_dense_remove (sq_dense_remove.hpp): a bitmap over the n rows, allocated at the first removal
    // (null until then: every kernel that takes it does exactly what it did).  Ids stay stable: removed rows keep their
    // place until sq_dense_compact.
    DevBuf dead;
    long long dead_words = 0;   // 32-bit words of `dead` in use (zero behind the rows)
    long long n_live = 0;       // rows not removed: what k is clamped to
    const u32* deadp() const { return dead.as<u32>(); }
    DevBuf zeros;   // cosine: the 32 zero "norms" every tile of an AGPR-configuration scan starts from (norm_step 0)
    static constexpr int kMaxDepth = 6;
    CallRing<DenseSlot, kMaxDepth> ring;   // the call slots (option dense_async_depth: 2 .. kMaxDepth in flight)
    // workspace shared by all calls: host-memory staging, the exact path (runs synchronously), index build
    DevBuf q_dev, out_dist_dev, out_idx_dev, big_keys, fb_sample, fb_keys, fb_out, scratch, fb_cnt, fb_sort;
    DevBuf mid_q, mid_planes, mid_small, mid_qal, mid_wave_out, mid_wave_cnt, mid_keys, mid_out, mid_sample;  // the middle tier (synchronous)
    DevBuf mid_cos_center, mid_cos_rows;   // cosine tier: column means c [d_pad], [2][mid_cos_ld] float32 1/|x| and x.c/|x| (built at first use)
    long long mid_cos_n = -1, mid_cos_ld = 0;   // rows mid_cos_rows covers (an append makes it stale)
    // The first filters' candidate lists overflowed for most queries of three calls in a row (descriptors sharing a large
    // offset under cosine, one tight cluster: every row inside the slack): calls go straight to the middle tier -- the
    // overflowing pass, its re-rank of `cap` rows per query and its select bought nothing (2 M x 128 cosine, 32 queries:
    // 5.6 of a 5.8 ms call).  The first filter is tried again after 16 such calls, then 32, 64 ... 1024 while it keeps
    // overflowing (a burst of atypical queries costs sixteen slower calls, data of that geometry a probe in a thousand);
    // the first probe that does not overflow re-arms it.
    int overflow16 = 0;
    bool first_suspended = false;
    unsigned direct_calls = 0, probe_interval = 16;
    // what sq_dense_create starts from, for an index whose rows have changed under it (sq_dense_compact): the statistics
    // and the first filters' record are of the old rows, the captured call graphs hold the old shape and the old buffers
    void reset_filter_state() {
        xn2_max = 0.0, mid_cos_n = -1;
        overflow16 = 0, first_suspended = false, direct_calls = 0, probe_interval = 16;
        for (auto& sl : ring.slot) sl.drop_graph();
    }
    PinnedStage stage;
    hipEvent_t ev_ref = nullptr;   // SQ_TRACE (measurement aid): the origin of the printed call timelines
    ~DenseHandle() override {
        if (ev_ref) (void)hipEventDestroy(ev_ref);
    }
};

// SQ_HOSTPROF=1 (measurement aid): host nanoseconds of an asynchronous sq_dense_search by section, printed by sq_dense_sync
struct HostProf {
    bool on = getenv("SQ_HOSTPROF") != nullptr;
    long long ns[6] = {0, 0, 0, 0, 0, 0};   // entry (lookup, lock, options, device), resolve of the slot, stream / event setup, enqueue, wait-resolve, calls
    std::chrono::steady_clock::time_point t;
    void start() { if (on) t = std::chrono::steady_clock::now(); }
    void lap(int i) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        ns[i] += std::chrono::duration_cast<std::chrono::nanoseconds>(now - t).count();
        t = now;
    }
};
static HostProf g_hostprof;

// -------------------------------------------------------------- host driver
// the int8 kernels of a row width of 128, 256 or 512 bytes: f(KS), KS = row bytes / 32 (sq_dense_i8.hpp I8Geom<KS>; the
// prep and build kernels take EPL = KS / 2; `chunks`: wide rows go in chunks of 512 bytes) -- the Hamming driver's with_width
template <class F>
static int with_row8(int row8, F&& f, bool chunks = false) {
    switch (chunks && row8 > 512 ? 512 : row8) {
        case 128: return f(std::integral_constant<int, 4>{});
        case 256: return f(std::integral_constant<int, 8>{});
        case 512: return f(std::integral_constant<int, 16>{});
    }
    return fail(SQ_ERR_INVALID, "int8: no kernel for rows of %d bytes", row8);
}

// What the stages of a call (dense_enqueue) and its later tiers (dense_resolve) share beside DenseCall.
struct DenseCtx {
    int kk;
    bool cosine;
    u32 cap;
    int qt, qp, nqt, group_q;   // first stage: query tiles per wave, query planes, groups of qt tiles, queries per scan workgroup
    long long key_stride;
    size_t key_bytes;
    long long id_base;
    void* out_dist;
    long long* out_idx;
    u32* cnt;
    float* thr;
    double* qn2;
    u32* oflag;
    const double* cnq;
    // per-query candidate counts and status words land in pinned host memory straight from the finalisation (no copy
    // launch): [cnt (nq_pad) | status (nq)], by their host and by their device address
    u32 *hs_cnt, *hs, *hs_cnt_dev, *hs_dev;
    int bind(const DenseHandle* h, DenseSlot& s) {   // (s.call is filled, the slot's buffers are reserved)
        const DenseCall& c = s.call;
        kk = (int)(c.k < h->n_live ? c.k : h->n_live);   // (removed rows are no neighbours: sq_dense_remove)
        cosine = h->metric == SQ_METRIC_COSINE;
        key_bytes = cosine ? sizeof(K128) : sizeof(u64);
        cap = c.cap;
        id_base = h->id_base;
        out_dist = c.out_dist;
        out_idx = c.out_idx;
        cnt = s.cnt.as<u32>();
        thr = s.thr.as<float>();
        qn2 = s.qn2.as<double>();
        oflag = s.oflag.as<u32>();
        cnq = s.cos_nq.as<double>();
        hs_cnt = reinterpret_cast<u32*>(s.status_host.p);
        hs = hs_cnt + c.nq_pad;
        SQ_TRY(s.status_host.device_ptr(reinterpret_cast<void**>(&hs_cnt_dev)));
        hs_dev = hs_cnt_dev + c.nq_pad;
        return SQ_OK;
    }
    // the finalisation of a filter stage: counts and the filter bound certified, the counts copied out
    template <class M>
    typename M::Fin filter_fin(double slack = 0.0) const {
        auto f = M::finalize(*this, cnt, cap, 1, slack);
        f.cnt_out = hs_cnt_dev;
        f.overflow = oflag;
        return f;
    }
};

// What the two metrics do not share on the host: key and distance types and the select's finalisation (sq_dense_exact.hpp).
// finalize() fills what the structs take by position; the members after q0 have the same names in both and are set by name.
template <bool COSINE>
struct DenseMetric {
    static constexpr bool cosine = COSINE;
    using Key = std::conditional_t<COSINE, K128, u64>;
    using Dist = std::conditional_t<COSINE, double, float>;
    using Fin = std::conditional_t<COSINE, DenseFinalizeCos, DenseFinalizeL2>;
    // slack: FilterBound::beta (L2), eps of the filter's similarity (cosine)
    static Fin finalize(const DenseCtx& e, const u32* cnt, u32 cap, int certify, double slack = 0.0) {
        Dist* dist = static_cast<Dist*>(e.out_dist);
        if constexpr (COSINE)
            return Fin{cnt, cap, e.kk, e.id_base, e.thr, slack, certify, dist, e.out_idx, e.hs_dev, nullptr, nullptr, 0};
        else
            return Fin{cnt, cap, e.kk, e.id_base, e.thr, e.qn2, slack, certify, dist, e.out_idx, e.hs_dev, nullptr, nullptr, 0};
    }
};
template <class F>
static int by_metric(bool cosine, F&& f) {
    return cosine ? f(DenseMetric<true>{}) : f(DenseMetric<false>{});
}

// The per-row terms of the handle's copies that say "never emitted" (sq_dense_remove.hpp)
static DenseDeadTerms dense_dead_terms(const DenseHandle* h) {
    const bool cosine = h->metric == SQ_METRIC_COSINE;
    DenseDeadTerms t{};
    if (!cosine) {
        t.norms = h->norms.as<float>();
        t.norms1 = h->norms1.as<float>();
    }
    t.nrow8 = h->i8.nrow.as<float>();   // (null without a copy)
    if (cosine && h->scan.p) {
        t.scan = h->scan.as<uint4>();
        t.scan_cpr = h->d_pad / 8;
    }
    if (cosine && h->mid_cos_rows.p && h->mid_cos_n == h->n) {
        t.mid_cos = h->mid_cos_rows.as<float>();
        t.mid_cos_ld = h->mid_cos_ld;
    }
    return t;
}
// ... written again for the removed rows from `row_from` on, after a build kernel has rewritten the terms there
static int dense_dead_reapply(DenseHandle* h, long long row_from, hipStream_t st) {
    if (!h->dead.p || row_from >= h->n) return SQ_OK;
    return launch<dense_dead_reapply_kernel>(dim3((unsigned)((h->n - row_from + 255) / 256)), dim3(256), 0, st, h->deadp(), row_from, h->n,
                                             dense_dead_terms(h));
}
template <int WAVES, int NSTAGE, int KU, int QT, int QP, bool AB, bool SAMPLE, bool NT = false>
static int scan_launch_t(const DenseScanArgs& a, size_t lds, hipStream_t st) {
    return launch_lds<dense_scan_kernel<WAVES, NSTAGE, KU, QT, QP, AB, SAMPLE, NT>>(160 * 1024, dim3((unsigned)(a.nrb * a.nqt)),
                                                                                   dim3(WAVES * 64), lds, st, a);
}

static constexpr int SCAN_LDS_TAIL = 8 * 16;  // per-wave survivor counters

// Launch geometry of the scan for a padded dimension and `qt` query tiles per wave:
// waves per workgroup and ring depth.
struct ScanGeom {
    int waves, stages;
    size_t lds;
};
static ScanGeom scan_geometry(const Options& o, int d_pad, int qt, int qp) {
    const int ku = d_pad / KT;
    const bool ab = qt > 1 || qp == 1;   // query fragments in AGPRs (multi-tile batches)
    const bool qreg = ab || ku <= 1;     // not re-read from an LDS copy
    const int qb = qreg ? 0 : TILE_ROWS * d_pad * 4;
    ScanGeom g{};
    // eight waves (two per SIMD) whenever the query fragments leave room: one tile, or two tiles of one plane
    g.waves = (ku <= 1 && (qt == 1 || (qt == 2 && qp == 1))) ? 8 : 4;
    if (ku <= 1 && o.dense_waves == 4) g.waves = 4;
    int ns = (160 * 1024 - qb - SCAN_LDS_TAIL) / (g.waves * SLOT_BYTES);
    const int ns_max = g.waves == 8 ? 2 : 4;
    if (ns > ns_max) ns = ns_max;
    if (qt == 1 && !ab && o.dense_stages >= 2 && o.dense_stages <= ns) ns = o.dense_stages;
    g.stages = ns;
    g.lds = (size_t)qb + (size_t)g.waves * ns * SLOT_BYTES + SCAN_LDS_TAIL;
    // staging the query tiles through the ring needs the ring to be at least as large
    if (qreg && (size_t)qt * TILE_ROWS * d_pad * 4 > (size_t)g.waves * ns * SLOT_BYTES) g.stages = 0;
    return g;
}

template <int KU, bool SAMPLE>
static int scan_launch_ku(const DenseScanArgs& a, const ScanGeom& g, int qt, int qp, hipStream_t st) {
    if constexpr (KU <= 1) {
        // one group of query tiles over a copy far beyond the MALL: the non-temporal build of the two kernels that serve
        // 33 .. 128 queries
        const bool nt = a.nt && a.nqt == 1;
        if (qt == 4 && qp == 1 && nt) return scan_launch_t<4, 4, KU, 4, 1, true, SAMPLE, true>(a, g.lds, st);
        if (qt == 4) return qp == 1 ? scan_launch_t<4, 4, KU, 4, 1, true, SAMPLE>(a, g.lds, st) : scan_launch_t<4, 4, KU, 4, 2, true, SAMPLE>(a, g.lds, st);
        if (qt == 2 && qp == 1 && g.waves == 8 && nt) return scan_launch_t<8, 2, KU, 2, 1, true, SAMPLE, true>(a, g.lds, st);
        if (qt == 2 && qp == 1 && g.waves == 8) return scan_launch_t<8, 2, KU, 2, 1, true, SAMPLE>(a, g.lds, st);
        if (qt == 2) return qp == 1 ? scan_launch_t<4, 4, KU, 2, 1, true, SAMPLE>(a, g.lds, st) : scan_launch_t<4, 4, KU, 2, 2, true, SAMPLE>(a, g.lds, st);
        if (g.waves == 8) return scan_launch_t<8, 2, KU, 1, 2, false, SAMPLE>(a, g.lds, st);
    } else if (qp == 1) {
        // d_pad > 128, several query tiles in the batch: all k-units' q_hi fragments in AGPRs (KU * QT * 32 <= 256)
        if (qt == 2) return scan_launch_t<4, 4, KU, 2, 1, true, SAMPLE>(a, g.lds, st);
        return fail(SQ_ERR_UNSUPPORTED, "dense scan: no kernel for d_pad=%d qt=%d", KU * KT, qt);
    }
    switch (g.stages) {
        case 4: return scan_launch_t<4, 4, KU, 1, 2, false, SAMPLE>(a, g.lds, st);
        case 3: return scan_launch_t<4, 3, KU, 1, 2, false, SAMPLE>(a, g.lds, st);
        default: return scan_launch_t<4, 2, KU, 1, 2, false, SAMPLE>(a, g.lds, st);
    }
}

template <bool SAMPLE>
static int scan_launch(const Options& o, const DenseScanArgs& a, int d_pad, int qt, int qp, hipStream_t st) {
    if (d_pad > RING_MAX_DPAD) {   // rows beyond the ring kernels: one query tile per wave, fragments straight from global memory
        if (qt != 1 && qt != 2 && qt != 4) return fail(SQ_ERR_UNSUPPORTED, "dense scan: d_pad=%d takes one, two or four query tiles per wave", d_pad);
        auto go = [&](auto t) {
            constexpr int QT = decltype(t)::value;
            const dim3 grid((unsigned)(a.nrb * a.nqt)), block(WIDE_WAVES * 64);
            return qp == 2 ? launch<dense_wide_scan_kernel<2, QT, SAMPLE>>(grid, block, 0, st, a, d_pad / KT)
                           : launch<dense_wide_scan_kernel<1, QT, SAMPLE>>(grid, block, 0, st, a, d_pad / KT);
        };
        return qt == 4 ? go(std::integral_constant<int, 4>{}) : qt == 2 ? go(std::integral_constant<int, 2>{}) : go(std::integral_constant<int, 1>{});
    }
    const ScanGeom g = scan_geometry(o, d_pad, qt, qp);
    if (g.stages < 2 || ((qt > 1 || qp == 1) && g.waves == 4 && g.stages != 4))
        return fail(SQ_ERR_UNSUPPORTED, "dense scan: d_pad=%d qt=%d leaves no room for the LDS ring", d_pad, qt);
    switch (d_pad / KT) {
        case 1: return scan_launch_ku<1, SAMPLE>(a, g, qt, qp, st);
        case 2: return scan_launch_ku<2, SAMPLE>(a, g, qt, qp, st);
        case 3: return scan_launch_ku<3, SAMPLE>(a, g, qt, qp, st);
        case 4: return scan_launch_ku<4, SAMPLE>(a, g, qt, qp, st);
        default: return fail(SQ_ERR_UNSUPPORTED, "dense scan: d_pad=%d", d_pad);
    }
}

// Error coefficients of the filter score (derivation at their use in dense_bf16_enqueue); the index build
// needs them too: the L2 scan starts from row norms shrunk by the row's share of the bound.
static constexpr double kEpsA2 = 0.0078125 + 6.103515625e-05;   // two query planes: 2^-7 + 2^-14
static constexpr double kEpsA1 = 0.015625 + 1.220703125e-04;    // one query plane:  2^-6 + 2^-13
static double dense_eps_b(int d_pad) { return (3.0 * d_pad + 8.0) * 1.1920928955078125e-07; }

// Query tiles per wave for a batch of `nqt` 32-query tiles (sq_dense_scan.hpp): one tile keeps the
// HBM-bound configuration; larger batches reuse each streamed row tile for 2 or 4 query tiles, as
// many as the register budget allows (four at d_pad = 128, two beyond).
static int scan_query_tiles(const Options& o, int d_pad, int nqt) {
    const int ku = d_pad / KT;
    if (nqt <= 1) return 1;
    if (d_pad > RING_MAX_DPAD) {   // (sq_dense_wide.hpp: two tiles per wave for batches beyond 32 queries, four beyond 64)
        if (o.dense_qt == 1 || o.dense_qt == 2 || o.dense_qt == 4) return o.dense_qt;
        return nqt >= 3 ? 4 : 2;
    }
    int want = nqt >= 3 ? 4 : 2;
    if (o.dense_qt == 1 || o.dense_qt == 2 || o.dense_qt == 4) want = o.dense_qt;
    if (ku >= 2 && want > 2) want = 2;  // four tiles of a 256-wide row spill past 512 registers
    if (ku > 1 && want == 1) return 1;  // forced: the LDS-copy kernel
    return want;
}

// Launch of an int8 ring kernel for the row width KS (sq_dense_i8.hpp I8Geom<KS>) on `nrb` workgroups.  (The kernels have a
// few bytes of static LDS of their own: the attribute every instantiation needs once is the ring, not the CU's 160 KiB.)
template <int KS, auto Kernel, class... A>
static int i8_ring_launch(int nrb, hipStream_t st, const A&... a) {
    using G = I8Geom<KS>;
    constexpr int ring = G::WAVES * G::NSTAGE * G::SLOT_BYTES;
    return launch_lds<Kernel>(ring, dim3((unsigned)nrb), dim3(G::WAVES * 64), ring, st, a...);
}
template <bool SAMPLE>
static int dense8_scan_launch(int row_bytes, const Dense8ScanArgs& a, hipStream_t st) {
    return with_row8(row_bytes, [&](auto ks) { return i8_ring_launch<ks(), dense8_scan_kernel<ks(), SAMPLE>>(a.nrb, st, a); });
}
// one query tile per wave: dense8_scan_kernel for the row width; 2 or 4 tiles (128-byte rows): dense8_scan_mt_kernel
template <bool SAMPLE>
static int dense8_scan_any(int row_bytes, int qt, const Dense8ScanArgs& a, hipStream_t st) {
    using G = I8Geom<4>;
    const dim3 grid((unsigned)(a.nrb * a.nqt)), block(G::WAVES * 64);
    const size_t ring = (size_t)G::WAVES * G::NSTAGE * G::SLOT_BYTES;
    if (qt == 1) return dense8_scan_launch<SAMPLE>(row_bytes, a, st);
    if (row_bytes == 128 && qt == 2) return launch_lds<dense8_scan_mt_kernel<2, SAMPLE>>(160 * 1024, grid, block, ring, st, a);
    if (row_bytes == 128 && qt == 4) return launch_lds<dense8_scan_mt_kernel<4, SAMPLE>>(160 * 1024, grid, block, ring, st, a);
    return fail(SQ_ERR_INVALID, "int8 scan: %d query tiles per wave over %d-byte rows", qt, row_bytes);
}
// the three-launch form of a one-tile int8 call (sq_dense_i8.hpp): head and body per row width / metric
static int dense8_head_launch(int row_bytes, const Dense8HeadArgs& a, hipStream_t st) {
    return with_row8(row_bytes, [&](auto ks) { return i8_ring_launch<ks(), dense8_head_kernel<ks()>>(a.s.nrb, st, a); });
}
static int dense8_body_launch(int row_bytes, bool cosine, const Dense8ScanArgs& a, const Dense8TailArgs& t, hipStream_t st) {
    return with_row8(row_bytes, [&](auto ks) {
        return cosine ? i8_ring_launch<ks(), dense8_body_kernel<ks(), true>>(a.nrb, st, a, t)
                      : i8_ring_launch<ks(), dense8_body_kernel<ks(), false>>(a.nrb, st, a, t);
    });
}
static int i8_waves(int row_bytes) { return row_bytes == 512 ? I8Geom<16>::WAVES : I8Geom<4>::WAVES; }

// Shapes the middle tier covers (sq_dense_mid.hpp)
static bool dense_mid_shape_ok(const DenseHandle* h) {
    const bool cosine = h->metric == SQ_METRIC_COSINE;
    return h->d <= 512 && (reinterpret_cast<uintptr_t>(h->db) & 15u) == 0 && (h->ld & 3) == 0 && h->ld >= (h->d + 3) / 4 * 4 && h->n >= 32 &&
           (cosine ? h->cos_nx.p != nullptr : h->norms.p != nullptr);
}

// ---- rules the first-stage chains share
// Every stride-th 32-row tile is sampled (the bfloat16 chain and the wide int8 chain).  The sample pass costs
// ~ n * groups / stride, the re-rank + select ~ nq * stride * k (candidates per query ~ stride * k * slack); with
// groups ~ nq / (32 qt) the balance is stride ~ sqrt(n / (qt k)), independent of the batch: 20 at 10 M rows, k = 100,
// one query tile per wave (measured optimum 16-24; 8-12 with four tiles; 4 on a 1.25 M-row shard).
static long long dense_tile_stride(const Options& o, long long n, long long n_tiles, int kk, int qt, bool cosine, u32 cap) {
    long long stride = o.sample_stride;
    if (stride <= 0) {
        // (the float64 cosine re-rank costs ~3.6x the float32 L2 one per candidate: sqrt of that off the stride)
        stride = (long long)(20.0 * sqrt((double)n / 1e7 * 100.0 / (double)kk / (double)qt) / (cosine ? 1.9 : 1.0) + 0.5);
        if (stride > 24) stride = 24;
        if (stride < 2) stride = 2;
        if (stride > (long long)cap / (8ll * kk)) stride = (long long)cap / (8ll * kk);  // room in the key lists
    }
    if (stride > 64) stride = 64;
    if (stride < 1) stride = 1;
    while (stride > 1 && (n_tiles / stride) * 2 < 8ll * kk) stride >>= 1;
    return stride;
}
// Non-temporal row stream ("dense_nt"): automatic mode turns it on for a copy far beyond the MALL (`auto_ok`: the int8
// chain only with one query group -- several groups re-read the rows from L2) and leaves a head of `keep_mb_default` MB
// ("dense_nt_keep_mb") on the default cache policy.
static void dense_nt_policy(const Options& o, size_t copy_bytes, long long row_bytes, long long keep_mb_default, bool auto_ok, int& nt,
                            long long& nt_from_row) {
    const long long keep_mb = o.dense_nt_keep_mb > 0 ? o.dense_nt_keep_mb : keep_mb_default;
    nt = o.dense_nt >= 0 ? o.dense_nt : (copy_bytes > ((size_t)512 << 20) && auto_ok ? 1 : 0);
    nt_from_row = o.dense_nt == 0 ? 0x7fffffffffffffffll : o.dense_nt == 1 ? 0ll : (keep_mb << 20) / row_bytes;
}
// Workgroups of the full pass (returned) and of the sample pass.  One scan workgroup per CU fills the chip -- and
// leaves nothing for the other call slot's short kernels (re-rank, select of the previous call; query prep, sample pass,
// threshold of the next), whose workgroups need LDS of their own.  When the two slots run on their own streams the scan
// takes three quarters of the CUs: alone it is as fast (HBM bound: 0.433 ms on 160 workgroups against 0.439 on 256 at
// 10 M x 128), and the pipelined step drops from 0.50 to 0.46 ms (tools/step_sweep.py dense_blocks=...).
// (one query tile group only: the multi-tile configurations are MFMA bound and want every CU; `own` > 0: the kernel's own
// count where option dense_blocks leaves the choice)
// Pipelined one-group calls: the sample pass is a scan kernel too (one workgroup wants most of a CU's LDS), so on
// as many workgroups as the full pass it cannot run BESIDE the neighbouring call's full pass (192 of the 256
// CUs) -- its tail queues behind that pass and the two scans of a step serialise (a 1.25 M-row shard: 16 + 63 us
// of an 83 us step).  On the spare quarter of the CUs it runs wholly under the neighbour's full pass.
static int dense_pass_blocks(const Options& o, bool use_event, int nqt, int cus, int own, int& nrb_sample) {
    const bool pipelined = use_event && o.dense_async_streams == 2 && nqt == 1;
    const int nrb = ((o.dense_blocks > 0 ? o.dense_blocks : own > 0 ? own : pipelined ? cus * 3 / 4 : cus) + 7) / 8 * 8;
    nrb_sample = nrb;
    if (pipelined && o.dense_blocks <= 0) {
        const int sb = ((o.dense_sample_blocks > 0 ? o.dense_sample_blocks : (o.dense_sample_blocks < 0 ? nrb : cus - nrb)) + 7) / 8 * 8;
        if (sb >= 8 && sb < nrb) nrb_sample = sb;
    }
    return nrb;
}
// The second-level threshold's scratch in the slot (sq_dense_tighten.hpp): [hist | raw thresholds | T'' | keys of T''],
// a fixed layout (the histogram region never meets old thresholds).  A new allocation is wiped once;
// dense_tighten_thr_kernel leaves the histogram clean.
struct DenseTighten {
    u32 *hist = nullptr, *thr2k = nullptr;
    float *traw = nullptr, *thr2 = nullptr;
};
static int dense_tighten_scratch(DenseSlot& s, size_t entries, hipStream_t st, DenseTighten& t) {
    SQ_TRY(s.wave_score.reserve(entries * 4));
    SQ_TRY(s.tg.reserve((size_t)TG_CAP_Q * (TG_BINS + 3) * 4));
    if (s.tg_zeroed != s.tg.p) {
        SQ_HIP(hipMemsetAsync(s.tg.p, 0, s.tg.cap, st));
        s.tg_zeroed = s.tg.p;
    }
    t.hist = s.tg.as<u32>();
    t.traw = reinterpret_cast<float*>(t.hist + (size_t)TG_CAP_Q * TG_BINS);
    t.thr2 = t.traw + TG_CAP_Q;
    t.thr2k = reinterpret_cast<u32*>(t.thr2 + TG_CAP_Q);
    return SQ_OK;
}
static constexpr u32 kWaveCap = 2048;   // entries of a wave's survivor segment

// The survivors of a pass -- per-wave segments of (first row, mask, query) entries -- and where their keys go: exact
// re-rank from the float32 rows (wave segments -> per-query keys), select, certify.
// A re-rank workgroup takes `wpb` survivor segments of one scan workgroup (its waves share the query
// group), 128 threads per segment (512 at most).  Many small workgroups win: the kernel is a chain of dependent
// memory round trips per workgroup, not the per-query atomics (2 vs 8 segments: 37 vs 50 us at 10 M rows).
struct DenseSurvivors {
    const uint2* wave_out;
    const u32* wave_cnt;
    long long n_waves;
    int wpb;
    const float* q_al;   // the queries, [nq][ldq] float32
    int ldq, nq;
    void *keys, *out_keys;   // [nq][cap], [nq][k]
    DevBuf* sort_tmp;
    int debug = 0;
    long long expect = 0;               // the select's hint: candidates per query
    const float *wave_score = nullptr, *thr2 = nullptr;   // a second-level threshold (sq_dense_tighten.hpp): the entries' scores, T'' ...
    const u32* thr2k = nullptr;                           // ... and its keys
    hipEvent_t ev_rerank = nullptr;     // profiling: recorded between the re-rank and the select
};
// (e: the counters, thresholds, overflow flag and query norms the lists belong to, and the queries per scan workgroup)
template <class M>
static int dense_survivor_tail(const DenseHandle* h, const DenseCtx& e, const DenseSurvivors& v, int k, typename M::Fin fin, hipStream_t st) {
    using K = typename M::Key;
    const dim3 grid((unsigned)((v.n_waves + v.wpb - 1) / v.wpb)), block((unsigned)std::min(512, 128 * v.wpb));
    const size_t lds = (e.group_q == TILE_ROWS && v.ldq <= 156) ? (size_t)32 * (v.ldq + 4) * 4 : 0;  // the query tile in LDS (rerank_block)
    K* keys = static_cast<K*>(v.keys);
    const double* cnx = M::cosine ? h->cos_nx.as<double>() : nullptr;
    const double* cnq = M::cosine ? e.cnq : nullptr;
    if (v.thr2)
        SQ_TRY(launch<dense_rerank_filtered_kernel<K, M::cosine>>(grid, block, lds, st, h->db, h->ld, h->d, v.q_al, v.ldq, v.wave_out, v.wave_cnt,
                                                                  kWaveCap, v.n_waves, v.wpb, v.nq, e.group_q, keys, e.cnt, e.cap, e.oflag, cnx, cnq,
                                                                  v.debug, v.wave_score, v.thr2));
    else if constexpr (M::cosine)
        SQ_TRY(launch<dense_rerank_cos_kernel>(grid, block, lds, st, h->db, h->ld, h->d, v.q_al, v.ldq, v.wave_out, v.wave_cnt, kWaveCap, v.n_waves,
                                               v.wpb, v.nq, e.group_q, keys, e.cnt, e.cap, e.oflag, cnx, cnq, v.debug));
    else
        SQ_TRY(launch<dense_rerank_l2_kernel>(grid, block, lds, st, h->db, h->ld, h->d, v.q_al, v.ldq, v.wave_out, v.wave_cnt, kWaveCap, v.n_waves,
                                              v.wpb, v.nq, e.group_q, keys, e.cnt, e.cap, e.oflag, v.debug));
    if (v.ev_rerank) SQ_HIP(hipEventRecord(v.ev_rerank, st));
    fin.thr2k = v.thr2k;
    return select_launch_t<K>(keys, e.cnt, e.cap, (long long)e.cap, k, v.nq, static_cast<K*>(v.out_keys), fin, st, *v.sort_tmp, v.expect);
}
static DenseSurvivors dense_survivors(const DevBuf& wave_out, const DevBuf& wave_cnt, const DevBuf& q_al, const DevBuf& keys, const DevBuf& out_keys,
                                      DevBuf& sort_tmp, long long n_waves, int wpb, int ldq, int nq, const DenseTighten& tg = DenseTighten{}) {
    DenseSurvivors v{};
    v.wave_out = wave_out.as<uint2>();
    v.wave_cnt = wave_cnt.as<u32>();
    v.n_waves = n_waves;
    v.wpb = wpb;
    v.q_al = q_al.as<float>();
    v.ldq = ldq;
    v.nq = nq;
    v.keys = keys.p;
    v.out_keys = out_keys.p;
    v.sort_tmp = &sort_tmp;
    v.thr2 = tg.thr2;
    v.thr2k = tg.thr2k;
    return v;
}
// ... of a first-stage chain: the slot's lists (with a second-level threshold: its entries' scores), the call's queries
static DenseSurvivors dense_slot_survivors(const DenseHandle* h, DenseSlot& s, long long n_waves, int wpb, int ldq, const DenseTighten& tg = DenseTighten{}) {
    DenseSurvivors v = dense_survivors(s.wave_out, s.wave_cnt, s.q_al, s.keys, s.out_keys, s.sort_tmp, n_waves, wpb, ldq, s.call.nq, tg);
    v.wave_score = tg.thr2 ? s.wave_score.as<float>() : nullptr;
    v.debug = h->opt.dense_debug;
    if (s.call.prof) v.ev_rerank = s.ev[4];
    return v;
}

// Exact L2 keys of all n rows for the queries of grid.y (dense_exact_l2_kernel: the query staged in LDS; rows too wide for
// that: dense_exact_l2_pieces_kernel, one row per lane)
static int dense_exact_l2_keys(dim3 grid, hipStream_t st, const float* db, long long ld, int d, const float* q, const u32* cnt, long long n, u64* keys,
                               long long key_stride, float* sample, int sample_stride, const u32* dead) {
    if (dense_exact_stages_whole(d))
        return launch<dense_exact_l2_kernel>(grid, dim3(256), (size_t)((d + 3) / 4 * 4) * 4, st, db, ld, d, q, nullptr, cnt, (u32)n, n, 0ll, keys, key_stride,
                                             sample, sample_stride, dead);
    return launch<dense_exact_l2_pieces_kernel>(dim3((unsigned)((n + 255) / 256), grid.y), dim3(256), (size_t)kExactPiece * 4, st, db, ld, d, q, nullptr, cnt,
                                                (u32)n, n, 0ll, keys, key_stride, sample, sample_stride, dead);
}

// ---- every row is a candidate (n <= cap): exact keys for all rows, no scan
static int dense_small_enqueue(DenseHandle* h, DenseSlot& s, const DenseCtx& e) {
    const long long n = h->n;
    const int d = h->d;
    DenseCall& c = s.call;
    hipStream_t st = c.st;
    SQ_TRY(s.keys.reserve((size_t)c.nq * e.key_stride * e.key_bytes));
    SQ_TRY(launch<fill_u32_kernel>(dim3((c.nq_pad + 255) / 256), dim3(256), 0, st, e.cnt, (long long)c.nq_pad, (u32)n));
    const dim3 grid((unsigned)((n + 255) / 256), c.nq);
    if (c.prof) SQ_HIP(hipEventRecord(s.ev[1], st));
    c.stats.scan_launches = 1;
    c.stats.bytes_scanned = n * (long long)d * 4;
    return by_metric(e.cosine, [&](auto m) {
        using M = decltype(m);
        using K = typename M::Key;
        K* keys = s.keys.as<K>();
        if constexpr (M::cosine)
            SQ_TRY(launch<dense_exact_cos_kernel>(grid, dim3(256), 0, st, h->db, h->ld, d, c.q, nullptr, e.cnt, (u32)n, n, 0ll, keys, e.key_stride,
                                                  h->cos_nx.as<double>(), e.cnq, nullptr, 0, h->deadp()));
        else
            SQ_TRY(dense_exact_l2_keys(grid, st, h->db, h->ld, d, c.q, e.cnt, n, keys, e.key_stride, nullptr, 0, h->deadp()));
        if (c.prof) SQ_HIP(hipEventRecord(s.ev[2], st));
        auto fin = M::finalize(e, e.cnt, (u32)n, 0);
        fin.cnt_out = e.hs_cnt_dev;
        fin.dead = h->deadp();   // (the keys hold removed rows)
        return select_launch_t<K>(keys, e.cnt, (u32)n, e.key_stride, c.k, c.nq, s.out_keys.as<K>(), fin, st, s.sort_tmp);
    });
}

// The int8 first stage of a call of up to 32 queries over rows of 513 to 8192 dimensions (sq_dense_i8_wide.hpp): query
// prep, sample pass, threshold, full pass, second-level threshold, re-rank, select -- the wide bfloat16 chain with the
// int8 kernels in the places of its prep and its two passes, and the int8 certificate (Dense8ThrPost, DenseFinalize*::lin)
// in the place of the bfloat16 bound.
// (filter_ok: kk is inside the one-workgroup select; larger batches take the bfloat16 chain)
static int dense8_wide_enqueue(DenseHandle* h, DenseSlot& s, const DenseCtx& e) {
    const long long n = h->n;
    DenseCall& c = s.call;
    const int d = h->d, row8 = h->i8.row_bytes, ku = i8w_units(row8), qw = ku * I8W_UNIT;
    hipStream_t st = c.st;
    c.int8 = true;
    h->i8.rearm();
    c.stats.scan_launches = 2;
    c.stats.bytes_scanned = h->i8.n_pass * ((long long)row8 + 4);
    const long long n_tiles = (n + TILE_ROWS - 1) / TILE_ROWS;
    const long long stride = dense_tile_stride(h->opt, n, n_tiles, e.kk, 1, e.cosine, e.cap);
    const long long ns_tiles = (n_tiles + stride - 1) / stride;
    const long long ns = ns_tiles * 2;   // one sample (a 16-row group minimum) per lane half and tile
    const int cus = cu_count(h->device);
    int nrb = h->opt.dense_blocks > 0 ? h->opt.dense_blocks : 2 * cus;   // (32 KB of LDS: two eight-wave workgroups per CU)
    nrb = (nrb + 7) / 8 * 8;
    const long long n_waves = (long long)nrb * WIDE_WAVES;
    const int ldq = (d + 3) / 4 * 4;
    const bool tighten = h->opt.dense_tighten != 0;
    SQ_TRY(s.sample.reserve((size_t)TILE_ROWS * ns * 4));
    SQ_TRY(s.keys.reserve((size_t)c.nq * e.key_stride * e.key_bytes));
    SQ_TRY(s.q8.reserve((size_t)2 * TILE_ROWS * qw));
    SQ_TRY(s.par8.reserve((size_t)TILE_ROWS * 8));
    SQ_TRY(s.wave_out.reserve((size_t)n_waves * kWaveCap * 8));
    SQ_TRY(s.wave_cnt.reserve((size_t)n_waves * 8));
    SQ_TRY(s.q_al.reserve((size_t)c.nq * ldq * 4));
    DenseTighten tg;
    if (tighten) SQ_TRY(dense_tighten_scratch(s, (size_t)n_waves * kWaveCap, st, tg));
    const float* centerp = (!e.cosine && h->center.p) ? h->center.as<float>() : nullptr;
    SQ_TRY(launch<dense8_wide_prep_queries_kernel>(dim3(TILE_ROWS), dim3(256), 0, st, c.q, c.nq, d, centerp, (double)h->i8.dx, h->i8.rmax, h->i8.xmax,
                                                   s.q8.as<signed char>(), qw, s.par8.as<float2>(), e.qn2, e.thr, e.cnt, e.oflag, s.q_al.as<float>(), ldq,
                                                   e.cosine ? 1 : 0));
    Dense8WideArgs a{};
    a.scan8 = h->i8.scan.as<signed char>();
    a.nrow = h->i8.nrow.as<float>();
    a.row_bytes = row8;
    a.ku = ku;
    a.n = n;
    a.n_tiles = n_tiles;
    a.qs8 = s.q8.as<signed char>();
    a.par = s.par8.as<float2>();
    a.thr = e.thr;
    a.wave_out = s.wave_out.as<uint2>();
    a.wave_cnt = s.wave_cnt.as<u32>();
    a.wave_cap = kWaveCap;
    a.sample_out = s.sample.as<float>();
    a.ns = ns;
    // sample pass
    a.tile_step = stride;
    a.n_sel = ns_tiles;
    a.nrb = nrb;
    if (ns_tiles < (long long)nrb * WIDE_WAVES) a.nrb = (int)(((ns_tiles + WIDE_WAVES - 1) / WIDE_WAVES + 7) / 8 * 8);
    SQ_TRY(launch<dense8_wide_scan_kernel<true>>(dim3((unsigned)a.nrb), dim3(WIDE_WAVES * 64), 0, st, a));
    const Dense8WideThrPost tp{Dense8ThrPost{s.par8.as<float2>(), e.qn2}, tg.traw};
    SQ_TRY(launch<kth_threshold_f32_kernel<Dense8WideThrPost>>(dim3(c.nq), dim3(1024), 0, st, a.sample_out, ns, e.kk, e.thr, tp));
    // full pass
    a.tile_step = 1;
    a.n_sel = n_tiles;
    a.nrb = nrb;
    a.wave_score = tighten ? s.wave_score.as<float>() : nullptr;
    if (c.prof) SQ_HIP(hipEventRecord(s.ev[1], st));
    SQ_TRY(launch<dense8_wide_scan_kernel<false>>(dim3((unsigned)nrb), dim3(WIDE_WAVES * 64), 0, st, a));
    if (c.prof) SQ_HIP(hipEventRecord(s.ev[2], st));
    if (tighten) {
        const Dense8WideThrPost tp2{tp.base, nullptr};   // (the same slack rule, nothing else)
        SQ_TRY(launch<dense_tighten_hist_kernel>(dim3(64, 1), dim3(256), 0, st, a.wave_out, a.wave_score, a.wave_cnt, kWaveCap, n_waves,
                                                 (const float*)e.thr, (const float*)tg.traw, TILE_ROWS, tg.hist));
        SQ_TRY(launch<dense_tighten_thr_kernel<Dense8WideThrPost>>(dim3(1), dim3(64), 0, st, tg.hist, (const float*)e.thr, (const float*)tg.traw, c.nq,
                                                                   TILE_ROWS, e.kk, tp2, tg.thr2, tg.thr2k));
    }
    // exact re-rank of the survivors from the float32 rows, select, certify: the bfloat16 chain's kernels
    DenseSurvivors v = dense_slot_survivors(h, s, n_waves, 2, ldq, tg);
    return by_metric(e.cosine, [&](auto m) {
        using M = decltype(m);
        auto fin = e.filter_fin<M>();
        fin.lin = s.par8.as<float2>();
        v.expect = M::cosine ? 0 : 4 * stride * e.kk;
        return dense_survivor_tail<M>(h, e, v, c.k, fin, st);
    });
}

// The int8 chain eagerly or as a captured graph.  A launch costs ~2.8 us of host time
// (tools/micro/launch_cost.hip: 19.3 us for a chain of seven, 5.6-6.3 us for one hipGraphLaunch of the same chain; in
// this call 20 against 9.5 us, tools/host_sections.py).  It does not shorten a 1.25 M-row shard's ~55 us step -- that
// is the latency of the chain itself, three deep -- but frees the host thread for the gather / merge work of a
// sharded search.  The slot's first call of a shape runs eagerly (it sizes the workspace and sets the kernels'
// attributes), the second captures, later ones launch the graph; the caller's pointers travel through a pinned
// block (DenseCallPtrs), which `chain(stream, ind)` hands to its first and last kernel.
// `by_value`: everything the captured launches were given by value (shapes, the slot's and the handle's buffers).
template <class Chain>
static int dense8_launch_chain(DenseHandle* h, DenseSlot& s, std::initializer_list<u64> by_value, Chain&& chain) {
    const DenseCall& c = s.call;
    hipStream_t st = c.st;
    if (c.use_event && !c.prof && h->opt.dense_graph != 0 && !h->graph_broken && st != nullptr && st == s.sync.own) {   // (never a capture on the caller's stream)
        u64 key = 0xcbf29ce484222325ull;
        for (u64 v : by_value) key = (key ^ v) * 0x100000001b3ull;
        if (key == 0) key = 1;
        if (s.gexec && s.gkey != key) {
            (void)hipGraphExecDestroy(s.gexec);
            s.gexec = nullptr;
        }
        if (!s.gexec && s.seen_key == key) {   // second call of this shape on this slot: capture
            SQ_TRY(s.call_ptrs.reserve(sizeof(DenseCallPtrs)));
            void* ind_dev = nullptr;
            SQ_TRY(s.call_ptrs.device_ptr(&ind_dev));
            // (a capture that fails is no reason to fail the search: the handle goes back to eager launches for good)
            hipGraph_t g = nullptr;
            bool ok = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess;
            if (ok) {
                const int rc = chain(st, static_cast<const DenseCallPtrs*>(ind_dev));
                const hipError_t ec = hipStreamEndCapture(st, &g);
                ok = rc == SQ_OK && ec == hipSuccess && g != nullptr;
            }
            if (ok) ok = hipGraphInstantiate(&s.gexec, g, nullptr, nullptr, 0) == hipSuccess;
            if (g) (void)hipGraphDestroy(g);
            if (!ok) {
                (void)hipGetLastError();
                s.gexec = nullptr;
                h->graph_broken = true;
            } else {
                s.gkey = key;
                if (getenv("SQ_INT8_REPORT")) fprintf(stderr, "[smqtk_hip] call graph captured (%d queries, k = %d)\n", c.nq, c.k);
            }
        }
        s.seen_key = key;
        if (s.gexec) {
            *static_cast<DenseCallPtrs*>(s.call_ptrs.p) = DenseCallPtrs{c.q, c.out_dist, c.out_idx};
            SQ_HIP(hipGraphLaunch(s.gexec, st));
            return SQ_OK;
        }
    }
    return chain(st, nullptr);
}

// ---- the int8 first-stage filter (sq_dense_i8.hpp): half the bytes per row, measured error bound
static int dense8_enqueue(DenseHandle* h, DenseSlot& s, const DenseCtx& e) {
    const long long n = h->n;
    DenseCall& c = s.call;
    const int d = h->d;
    c.int8 = true;
    h->i8.rearm();
    // (128-byte rows stream in ring units of 64 rows on eight waves.  Two other geometries were built and measured --
    // commit 5048766: 128-row units on four waves 0.197 against 0.204 ms per pass alone but 0.244-0.251 against 0.223-0.226 ms
    // per pipelined step; 32-row units on sixteen waves 0.236 -- and removed again.)
    const int row8 = h->i8.row_bytes, unit_rows = i8_unit_rows(row8), spu = 2 * (unit_rows / 32), waves8 = i8_waves(row8);   // samples per unit
    const long long n_units = (n + unit_rows - 1) / unit_rows;
    long long stride = h->opt.sample_stride;
    if (stride <= 0) {
        // units of 64 rows, four samples per unit: the bf16 path's cost model in units of two tiles
        // (measured at 10 M x 128, k = 100: 0.293 / 0.269 / 0.262 / 0.258 / 0.257 / 0.257 / 0.263 ms per step at 6 / 8 / 10 / 12 / 16 / 20 / 24)
        // 256- and 512-byte rows: flat from 8 to 14, best at 10 (0.471 / 0.988 ms per step at 10 M x 256 / 512); the float64 cosine
        // re-rank costs ~3.6x the float32 one per candidate: sqrt of that off the stride, as in the bf16 path
        stride = (long long)((row8 == 128 ? 14.0 : 10.0) * sqrt((double)n / 1e7 * 100.0 / (double)e.kk / (double)e.qt) / (e.cosine ? 1.9 : 1.0) + 0.5);
        if (stride > 16) stride = 16;
        // The fused call with the tightened threshold (sq_dense_i8.hpp): the sample only has to keep the first-level
        // entries inside the wave segments -- what is re-ranked no longer depends on it -- so it is several times sparser
        const bool will_tighten = h->opt.dense_fused != 0 && h->opt.dense_tighten != 0 && e.qt == 1 && e.nqt == 1;
        if (will_tighten) {
            stride = (long long)(40.0 * sqrt((double)n / 1e7 * 100.0 / (double)e.kk) + 0.5);
            if (stride > 64) stride = 64;
        }
        if (stride < 1) stride = 1;
        if (stride > (long long)e.cap / (16ll * e.kk)) stride = std::max<long long>(1, (long long)e.cap / (16ll * e.kk));
    }
    while (stride > 1 && (n_units / stride) * spu < 8ll * e.kk) stride >>= 1;
    const long long ns_units = (n_units + stride - 1) / stride;
    const long long ns = ns_units * spu;
    SQ_TRY(s.keys.reserve((size_t)c.nq * e.key_stride * e.key_bytes));
    SQ_TRY(s.q8.reserve((size_t)2 * c.nq_pad * row8));
    SQ_TRY(s.par8.reserve((size_t)c.nq_pad * 8));
    const int cus = cu_count(h->device);
    int nrb_sample = 0;
    const int nrb = dense_pass_blocks(h->opt, c.use_event, e.nqt, cus, 0, nrb_sample);
    const long long n_waves = (long long)nrb * e.nqt * waves8;
    const int ldq = (d + 3) / 4 * 4;
    SQ_TRY(s.wave_out.reserve((size_t)n_waves * kWaveCap * 8));
    SQ_TRY(s.wave_cnt.reserve((size_t)n_waves * 8));
    SQ_TRY(s.q_al.reserve((size_t)c.nq * ldq * 4));
    const float* centerp = (!e.cosine && h->center.p) ? h->center.as<float>() : nullptr;
    Dense8ScanArgs a{};
    a.scan8 = h->i8.scan.as<signed char>();
    a.nrow = h->i8.nrow.as<float>();
    a.n = n;
    a.n_units = n_units;
    a.qs8 = s.q8.as<signed char>();
    a.par = s.par8.as<float2>();
    a.thr = e.thr;
    a.wave_out = s.wave_out.as<uint2>();
    a.wave_cnt = s.wave_cnt.as<u32>();
    a.wave_cap = kWaveCap;
    a.sample_out = s.sample.as<float>();
    a.ns = ns;
    a.nqt = e.nqt;
    a.plane_rows = c.nq_pad;
    a.debug = h->opt.dense_debug;
    // (cacheable head: 32-64 MB measured best here -- 0.244 ms per step at 10 M rows against 0.250 at the bf16 copy's 192 MB)
    dense_nt_policy(h->opt, (size_t)h->i8.n_pass * row8, row8, 64, e.nqt == 1, a.nt, a.nt_from_row);
    if (ns_units < (long long)nrb_sample * waves8) nrb_sample = (int)(((ns_units + waves8 - 1) / waves8 + 7) / 8 * 8);
    // Three launches instead of six (sq_dense_i8.hpp, "a call in three launches"): one query tile, and a head grid whose
    // M = workgroups x waves x 2 lane minima per query number at least 4 k (the threshold is then within a few per cent of
    // the k-th smallest sample) and at most 2048 (what the last workgroup's waves hold in registers).
    bool fused = h->opt.dense_fused != 0 && e.qt == 1 && e.nqt == 1 && ns_units >= 2ll * e.kk;
    const bool tighten = fused && h->opt.dense_tighten != 0;
    if (fused) {
        const int lanes_per_wg = waves8 * 2;
        const int wg_min = ((4 * e.kk + lanes_per_wg - 1) / lanes_per_wg + 7) / 8 * 8, wg_max = 2048 / lanes_per_wg;
        if (wg_min > wg_max || wg_min > cus)
            fused = false;
        else
            nrb_sample = std::min(std::max(nrb_sample, wg_min), std::min(wg_max, (cus + 7) / 8 * 8));
    }
    // minima a head workgroup hands over per query: the k best of a call fall on a workgroup k / workgroups at a time
    int keep8 = waves8 * 2;
    if (fused) {
        const double per_wg = (double)e.kk / nrb_sample;
        if (per_wg <= 1.7 && keep8 > 4) keep8 = 4;
        else if (per_wg <= 4.5 && keep8 > 8) keep8 = 8;
    }
    const long long lane_m = (long long)nrb_sample * keep8;
    SQ_TRY(s.sample.reserve(fused ? (size_t)TILE_ROWS * lane_m * 4 : (size_t)c.nq_pad * ns * 4));
    a.sample_out = s.sample.as<float>();
    if (fused) {
        SQ_TRY(s.wave_score.reserve((size_t)n_waves * kWaveCap * 4));
        SQ_TRY(s.hist8.reserve((size_t)I8_HIST_WORDS * 4));
        a.wave_score = s.wave_score.as<float>();
        a.hist = s.hist8.as<u32>();
    }
    int wpb = 2;   // survivor segments per re-rank workgroup: four at the most here
    if (!e.cosine && h->opt.dense_rerank_segments > 0 && waves8 % h->opt.dense_rerank_segments == 0 && h->opt.dense_rerank_segments <= 4)
        wpb = h->opt.dense_rerank_segments;
    const double* cnx = h->cos_nx.as<double>();
    // the chain of three or six launches
    auto chain = [&](hipStream_t cs, const DenseCallPtrs* ind) -> int {
        if (fused) {
            // head: query prep + sample pass (lane minima) + thresholds by the last workgroup
            Dense8HeadArgs ha{};
            ha.s = a;
            ha.s.unit_step = stride;
            ha.s.n_sel = ns_units;
            ha.s.nrb = nrb_sample;
            ha.q = c.q;
            ha.nq = c.nq;
            ha.d = d;
            ha.center = centerp;
            ha.dx = (double)h->i8.dx;
            ha.r_max = h->i8.rmax;
            ha.x_max = h->i8.xmax;
            ha.cosine = e.cosine ? 1 : 0;
            ha.qn2 = e.qn2;
            ha.cnt = e.cnt;
            ha.oflag = e.oflag;
            ha.q_al = s.q_al.as<float>();
            ha.ldq = ldq;
            ha.ind = ind;
            ha.lane_min = s.sample.as<float>();
            ha.keep = keep8;
            ha.kk = e.kk;
            SQ_TRY(dense8_head_launch(row8, ha, cs));
            // body: the full pass; its workgroups re-rank their own survivors when the stream has drained
            Dense8ScanArgs b = a;
            b.unit_step = 1;
            b.n_sel = n_units;
            b.nrb = nrb;
            Dense8TailArgs ta{h->db, h->ld, d, s.q_al.as<float>(), ldq, c.nq, s.keys.p, e.cnt, e.cap, e.oflag, cnx, e.cnq, h->opt.dense_debug, e.qn2, e.kk,
                              tighten ? 1 : 0, nullptr};
            s.clk8_wgs = 0;
            if ((h->opt.dense_debug & 8192) && !c.use_event) {   // (blocking calls only: read and printed by dense_body_clocks)
                SQ_TRY(s.clk8.reserve((size_t)nrb * 64));
                SQ_HIP(hipMemsetAsync(s.clk8.p, 0, (size_t)nrb * 64, cs));
                ta.clk = s.clk8.as<long long>();
                s.clk8_wgs = nrb;
            }
            if (c.prof) SQ_HIP(hipEventRecord(s.ev[1], cs));
            SQ_TRY(dense8_body_launch(row8, e.cosine, b, ta, cs));
            if (c.prof) {
                SQ_HIP(hipEventRecord(s.ev[2], cs));
                SQ_HIP(hipEventRecord(s.ev[4], cs));
            }
            return by_metric(e.cosine, [&](auto m) {
                using M = decltype(m);
                using K = typename M::Key;
                auto fin = e.filter_fin<M>();
                fin.lin = s.par8.as<float2>();
                fin.ind = ind;
                if (tighten) fin.thr2k = a.hist + TILE_ROWS * I8_HIST_BINS;
                fin.cnt_shift = I8_CNT_SHIFT;
                return select_launch_t<K>(s.keys.as<K>(), e.cnt, e.cap, e.key_stride, c.k, c.nq, s.out_keys.as<K>(), fin, cs, s.sort_tmp, 8 * stride * e.kk,
                                          I8_CNT_SHIFT);
            });
        }
        SQ_TRY(with_row8(row8, [&](auto ks) {
            return launch<dense8_prep_queries_kernel<decltype(ks)::value / 2>>(dim3(c.nq_pad / 4), dim3(64), 0, cs, c.q, c.nq, d, centerp, (double)h->i8.dx, h->i8.rmax,
                                                                               h->i8.xmax, s.q8.as<signed char>(), s.par8.as<float2>(), e.qn2, e.thr, e.cnt,
                                                                               e.oflag, s.q_al.as<float>(), ldq, ind, e.cosine ? 1 : 0, c.nq_pad);
        }));
        Dense8ScanArgs b = a;
        b.unit_step = stride;   // sample pass (on the CUs the pipelined full pass leaves free)
        b.n_sel = ns_units;
        b.nrb = nrb_sample;
        SQ_TRY(dense8_scan_any<true>(row8, e.qt, b, cs));
        SQ_TRY(launch<kth_threshold_f32_kernel<Dense8ThrPost>>(dim3(c.nq), dim3(1024), 0, cs, a.sample_out, ns, e.kk, e.thr,
                                                               Dense8ThrPost{s.par8.as<float2>(), e.qn2}));
        b.unit_step = 1;        // full pass
        b.n_sel = n_units;
        b.nrb = nrb;
        if (c.prof) SQ_HIP(hipEventRecord(s.ev[1], cs));
        SQ_TRY(dense8_scan_any<false>(row8, e.qt, b, cs));
        if (c.prof) SQ_HIP(hipEventRecord(s.ev[2], cs));
        DenseSurvivors v = dense_slot_survivors(h, s, n_waves, wpb, ldq);
        v.expect = 8 * stride * e.kk;
        return by_metric(e.cosine, [&](auto m) {
            using M = decltype(m);
            auto fin = e.filter_fin<M>();
            fin.lin = s.par8.as<float2>();
            fin.ind = ind;
            return dense_survivor_tail<M>(h, e, v, c.k, fin, cs);
        });
    };
    c.stats.scan_launches = 2;
    c.stats.bytes_scanned = h->i8.n_pass * ((long long)row8 + 4) * e.nqt;
    return dense8_launch_chain(
        h, s,
        {(u64)(fused ? 1 : 0), (u64)(tighten ? 1 : 0), (u64)(uintptr_t)s.wave_score.p, (u64)(uintptr_t)s.hist8.p, (u64)lane_m, (u64)c.nq, (u64)c.k, (u64)row8,
         (u64)e.qt, (u64)e.nqt, (u64)wpb, (u64)stride, (u64)nrb, (u64)nrb_sample, (u64)ns, (u64)a.nt, (u64)a.nt_from_row, (u64)n, (u64)h->n_live, (u64)e.cap,
         (u64)h->opt.dense_debug, (u64)h->id_base, (u64)(uintptr_t)c.st, (u64)(uintptr_t)h->db, (u64)(uintptr_t)centerp, (u64)(uintptr_t)h->i8.scan.p,
         (u64)(uintptr_t)h->i8.nrow.p, (u64)(uintptr_t)s.q8.p, (u64)(uintptr_t)s.par8.p, (u64)(uintptr_t)s.sample.p, (u64)(uintptr_t)s.keys.p,
         (u64)(uintptr_t)s.wave_out.p, (u64)(uintptr_t)s.wave_cnt.p, (u64)(uintptr_t)s.q_al.p, (u64)(uintptr_t)e.cnt, (u64)(uintptr_t)e.thr,
         (u64)(uintptr_t)e.qn2, (u64)(uintptr_t)e.oflag, (u64)(uintptr_t)s.out_keys.p, (u64)(uintptr_t)e.hs_cnt_dev, (u64)(uintptr_t)cnx,
         (u64)(uintptr_t)e.cnq, (u64)(e.cosine ? 1 : 0)},
        chain);
}

// ---- the bfloat16 chain: sample pass, threshold, full pass, [second-level threshold,] re-rank, select
static int dense_bf16_enqueue(DenseHandle* h, DenseSlot& s, const DenseCtx& e) {
    const long long n = h->n;
    DenseCall& c = s.call;
    const int d = h->d, d_pad = h->d_pad;
    hipStream_t st = c.st;
    uint4* qs = s.q_scaled.as<uint4>();
    // error bound of the bf16 filter score (sq_dense_exact.hpp filter_eps):
    //   products: |x q' - x_hi (q'_hi + q'_lo)| <= (2^-8 + 2^-15) |x||q'|, q' = -2q  ->  eps_a = 2^-7 + 2^-14 (times X|q|)
    //             (cosine: unit vectors and q' = -q^ without the factor 2: half of that)
    //   float32 accumulation of 2d+1 terms and the float32 norm                     ->  eps_b = (3d+8) 2^-23
    //   one query plane: |x q' - x_hi q'_hi| <= (2^-8 + 2^-8 + 2^-16) |x||q'|                 ->  eps_a = 2^-6 + 2^-13
    const double eps_a = (e.qp == 2 ? kEpsA2 : kEpsA1) * (e.cosine ? 0.5 : 1.0);
    const double eps_b = dense_eps_b(d_pad);
    const long long n_tiles = (n + TILE_ROWS - 1) / TILE_ROWS;
    const long long stride = dense_tile_stride(h->opt, n, n_tiles, e.kk, e.qt, e.cosine, e.cap);
    const long long ns_tiles = (n_tiles + stride - 1) / stride;
    // one sample (a 16-row group minimum) per lane half per tile; the four-tile sample pass writes runs of four
    // tiles ([query][half][tiles rounded up to 4], +inf in the padding: dense_scan_kernel CHUNK)
    const bool sample_runs = e.qt == 4 && e.qp == 1 && d_pad == KT;
    const long long ns = (sample_runs ? (ns_tiles + 3) / 4 * 4 : ns_tiles) * 2;
    SQ_TRY(s.sample.reserve((size_t)c.nq_pad * ns * 4));
    SQ_TRY(s.keys.reserve((size_t)c.nq * e.key_stride * e.key_bytes));
    const int cus = cu_count(h->device);
    // (the wide kernel, 122 registers and 32 KB of LDS: two eight-wave workgroups per CU -- twice the row bytes in flight;
    // two tiles per wave: one workgroup per CU)
    int nrb_sample = 0;
    const int nrb = dense_pass_blocks(h->opt, c.use_event, e.nqt, cus, d_pad <= RING_MAX_DPAD ? 0 : e.qt == 1 ? 2 * cus : cus, nrb_sample);
    const int wv = d_pad > RING_MAX_DPAD ? WIDE_WAVES : scan_geometry(h->opt, d_pad, e.qt, e.qp).waves;
    // survivors leave the scan as per-wave segments; the re-rank kernel turns them into per-query key lists
    const long long n_waves = (long long)nrb * e.nqt * wv;
    const int ldq = (d + 3) / 4 * 4;
    SQ_TRY(s.wave_out.reserve((size_t)n_waves * kWaveCap * 8));
    SQ_TRY(s.wave_cnt.reserve((size_t)n_waves * 8));
    SQ_TRY(s.q_al.reserve((size_t)c.nq * ldq * 4));
    // rows beyond the ring kernels: a second-level threshold between the pass and the re-rank (sq_dense_tighten.hpp).
    // (The ring kernels do not store their entries' scores: the few instructions that would in dense_scan_kernel's
    // emission path changed the answers of its hand-scheduled multi-tile builds -- one query of a hundred lost the
    // survivors of its last row tiles -- and were taken out again; tools/tighten_debug.py.  In the compiler-scheduled
    // one-tile builds alone they were correct but not worth it: 10 M x 128 without the int8 copy, 3.3 k -> 2.1 k rows
    // re-ranked per query, 0.424 -> 0.451 ms per step: two more launches against 512-byte gathers.)
    const bool wide_tighten = h->opt.dense_tighten != 0 && d_pad > RING_MAX_DPAD && e.group_q <= TG_MAX_GROUP && c.nq_pad <= TG_CAP_Q;
    DenseTighten tg;
    if (wide_tighten) SQ_TRY(dense_tighten_scratch(s, (size_t)n_waves * kWaveCap, st, tg));
    // L2, one query tile per wave (the HBM-bound configuration a pipelined step runs): no prep launch -- the scan
    // kernels build the planes of their query tile themselves and the threshold kernel's prologue does the rest
    // (DenseScanArgs::raw_q, DenseThrPost).  The head of a call is then sample pass -> threshold: on a 1.25 M-row
    // shard the three-launch head (prep 6-27 us beside the neighbours' kernels, sample, threshold) no longer
    // fitted under the previous call's 59 us scan, and the scans did not run back to back.
    const bool fused_prep = !e.cosine && e.qt == 1 && e.qp == 2 && h->opt.dense_fused_prep != 0 && d_pad <= RING_MAX_DPAD;
    const float* centerp = h->center.p ? h->center.as<float>() : nullptr;
    if (!fused_prep)
        SQ_TRY(launch<dense_prep_queries_kernel>(dim3(c.nq_pad), dim3(256), 0, st, c.q, c.nq, d, d_pad, h->metric, qs, e.qn2, e.thr, e.cnt, e.oflag,
                                                 s.q_al.as<float>(), ldq, centerp));
    DenseScanArgs a{};
    if (fused_prep) {
        a.raw_q = c.q;
        a.raw_nq = c.nq;
        a.raw_d = d;
        a.center = centerp;
    }
    a.scan = h->scan.as<uint4>();
    a.norms = e.cosine ? nullptr : (e.qp == 1 ? h->norms1.as<float>() : h->norms.as<float>());  // n' of this plane count
    a.norm_step = 1;
    // non-temporal stream (32 queries, pipelined step): 10 M rows 0.456 -> 0.401 ms, 5 M 0.251 -> 0.227, 2.5 M 0.147 ->
    // 0.139.  One-tile kernel: everything behind a cacheable head of 192 MB ("dense_nt_keep_mb"); multi-tile kernels
    // with one query group: their non-temporal build when the copy is far beyond the MALL.
    dense_nt_policy(h->opt, (size_t)h->n_pad * d_pad * 2, (long long)d_pad * 2, 192, true, a.nt, a.nt_from_row);
    if (e.cosine && (e.qt > 1 || e.qp == 1)) {  // the AGPR configurations always stream a norm piece
        a.norms = h->zeros.as<float>();
        a.norm_step = 0;
    }
    a.n = n;
    a.n_tiles = n_tiles;
    a.qs = qs;
    a.thr = e.thr;
    a.wave_out = s.wave_out.as<uint2>();
    a.wave_cnt = s.wave_cnt.as<u32>();
    a.wave_cap = kWaveCap;
    a.sample_out = s.sample.as<float>();
    a.ns = ns;
    a.nqt = e.nqt;
    a.debug = h->opt.dense_debug;
    // sample pass
    a.tile_step = stride;
    a.n_sel = ns_tiles;
    a.nrb = nrb_sample;
    {
        const long long work = sample_runs ? (ns_tiles + 3) / 4 : ns_tiles;  // runs / tiles a wave takes at a time
        if (work < (long long)nrb * wv) a.nrb = (int)(((work + wv - 1) / wv + 7) / 8 * 8);
    }
    SQ_TRY(scan_launch<true>(h->opt, a, d_pad, e.qt, e.qp, st));
    DenseThrPost tp{e.qn2, e.cosine ? 1 : 0, filter_bound(e.cosine ? 1 : 0, eps_a, eps_b, h->xn2_max)};
    tp.traw_out = tg.traw;
    if (fused_prep) {
        tp.raw_q = c.q;
        tp.nq = c.nq;
        tp.nq_pad = c.nq_pad;
        tp.d = d;
        tp.ldq = ldq;
        tp.center = centerp;
        tp.qn2_out = e.qn2;
        tp.thr_out = e.thr;
        tp.cnt = e.cnt;
        tp.oflag = e.oflag;
        tp.q_al = s.q_al.as<float>();
    }
    SQ_TRY(launch<kth_threshold_f32_kernel<DenseThrPost>>(dim3(c.nq), dim3(1024), 0, st, a.sample_out, ns, e.kk, e.thr, tp));
    // full pass
    a.tile_step = 1;
    a.n_sel = n_tiles;
    a.nrb = nrb;
    if (c.prof) SQ_HIP(hipEventRecord(s.ev[1], st));
    a.wave_score = wide_tighten ? s.wave_score.as<float>() : nullptr;
    SQ_TRY(scan_launch<false>(h->opt, a, d_pad, e.qt, e.qp, st));
    if (c.prof) SQ_HIP(hipEventRecord(s.ev[2], st));
    if (wide_tighten) {
        DenseThrPost tp2 = tp;   // (the same slack rule, nothing else)
        tp2.traw_out = nullptr;
        tp2.raw_q = nullptr;
        SQ_TRY(launch<dense_tighten_hist_kernel>(dim3(e.nqt > 4 ? 16 : 64, e.nqt), dim3(256), 0, st, a.wave_out, a.wave_score, a.wave_cnt, kWaveCap, n_waves,
                                                 (const float*)e.thr, (const float*)tg.traw, e.group_q, tg.hist));
        SQ_TRY(launch<dense_tighten_thr_kernel<DenseThrPost>>(dim3((c.nq_pad + 63) / 64), dim3(64), 0, st, tg.hist, (const float*)e.thr, (const float*)tg.traw,
                                                              c.nq, c.nq_pad, e.kk, tp2, tg.thr2, tg.thr2k));
    }
    c.stats.scan_launches = 2;
    c.stats.bytes_scanned = h->n_pad * ((long long)d_pad * 2 + (e.cosine ? 0 : 4));
    // (L2, four-wave scan workgroups, i.e. multi-tile batches: 4 segments per re-rank workgroup measured 2 % faster than 2;
    // the cosine kernel's row stage is sized for 256 threads)
    int wpb = (wv == 4 && !e.cosine) ? 4 : 2;
    if (h->opt.dense_rerank_segments > 0 && wv % h->opt.dense_rerank_segments == 0) wpb = h->opt.dense_rerank_segments;
    DenseSurvivors v = dense_slot_survivors(h, s, n_waves, wpb, ldq, tg);
    return by_metric(e.cosine, [&](auto m) {
        using M = decltype(m);
        v.expect = M::cosine ? 0 : 4 * stride * e.kk;   // ~2.7 stride k candidates per query on N(0,1) data
        return dense_survivor_tail<M>(h, e, v, c.k, e.filter_fin<M>(M::cosine ? eps_a + eps_b : 0.5 * eps_a + eps_b), st);
    });
}

static int dense_bf16_materialize(DenseHandle* h);   // (option "dense_bf16": the scan copy built by the first call that streams it)

// Enqueue one search (nq <= kDenseQueryChunk queries) on `st` with the workspace of slot `s`; nothing is
// waited for.  dense_resolve() finishes the call: it waits for the kernels, reads the status words and
// sends uncertified queries down the exact path.  This function chooses the stage that takes the call and fills
// DenseCall; the stages are dense_small_enqueue, dense8_wide_enqueue, dense8_enqueue and dense_bf16_enqueue.
static int dense_enqueue(DenseHandle* h, DenseSlot& s, const float* q, int nq, int k, void* out_dist, long long* out_idx,
                         hipStream_t st, bool use_event) {
    const long long n = h->n;
    const int d = h->d, d_pad = h->d_pad;
    const int kk = (int)(k < h->n_live ? k : h->n_live);   // (removed rows are no neighbours: sq_dense_remove)
    const bool cosine = h->metric == SQ_METRIC_COSINE;
    // (profile = N > 1: every N-th asynchronous call only -- four event records per call weigh on a small shard's step)
    const bool prof = h->opt.profile == 1 || (h->opt.profile > 1 && (!use_event || h->ring.calls % (unsigned)h->opt.profile == 0));
    const size_t key_bytes = cosine ? sizeof(K128) : sizeof(u64);
    u32 cap = h->opt.candidate_cap > 0 ? (u32)h->opt.candidate_cap : 65536u;
    if (cap < (u32)(4 * kk)) cap = (u32)(4 * kk);
    const bool small = n <= (long long)cap;
    DenseCtx e{};
    e.key_stride = small ? n : (long long)cap;
    // k beyond the one-workgroup select (16384; cosine 7168): every query takes the exact path, whose select sorts
    // (the reference has no limit on n: lsh.py:513-518)
    // filter_ok: the shape allows a first-stage filter at all (rows wider than MAX_DPAD have no scan copy of any kind)
    const bool filter_ok = !small && kk <= (cosine ? kSelectLdsKeys128 : kSelectLdsKeys64) && d_pad <= MAX_DPAD;
    const int qt = e.qt = scan_query_tiles(h->opt, d_pad, (nq + TILE_ROWS - 1) / TILE_ROWS);  // query tiles per wave
    // query planes: the multi-tile configuration is MFMA bound, so it drops q_lo (half the MFMAs, twice the
    // product bound: ~1.4x more rows pass the filter) unless asked otherwise
    // (rows beyond the ring kernels, sq_dense_wide.hpp: two planes unless option dense_qplanes = 1 -- half the query bytes read from L2 per row tile, twice the slack)
    e.qp = d_pad > RING_MAX_DPAD ? (h->opt.dense_qplanes == 1 ? 1 : 2) : ((qt > 1 && (h->opt.dense_qplanes != 2 || d_pad > KT)) ? 1 : 2);
    e.group_q = qt * TILE_ROWS;                                    // queries per scan workgroup
    e.nqt = (nq + e.group_q - 1) / e.group_q;                      // groups of qt query tiles
    const int nq_pad = e.nqt * e.group_q;
    // Which first stage takes the call.  The shortcut past a suspended filter and the two int8 stages need no bfloat16
    // copy; the bfloat16 chain does, and builds it here when option "dense_bf16" left it for the first call that wants it.
    const bool int8_on = filter_ok && h->i8.active(h->opt);
    const bool take_mid = filter_ok && h->first_suspended && h->opt.dense_mid_tier != 0 && !h->opt.force_fallback && dense_mid_shape_ok(h) &&
                          ++h->direct_calls % h->probe_interval != 0;
    const bool take_i8_wide = !take_mid && int8_on && h->i8.row_bytes > I8_MAX_ROW_BYTES && nq <= TILE_ROWS;
    const bool take_i8 = !take_mid && int8_on && h->i8.row_bytes <= I8_MAX_ROW_BYTES &&
                         (nq <= TILE_ROWS || (h->i8.row_bytes == 128 && (qt == 2 || qt == 4) && nq <= h->opt.dense_int8_batch));
    bool take_bf16 = filter_ok && !take_mid && !take_i8_wide && !take_i8 && h->opt.dense_bf16 != 0;
    if (take_bf16 && !h->scan.p) {
        SQ_TRY(dense_bf16_materialize(h));   // (finishes the calls in flight first; no memory for the copy is no error)
        take_bf16 = h->scan.p != nullptr;
    }
    DenseCall& c = s.call;
    c = DenseCall{};
    c.q = q;
    c.nq = nq;
    c.k = k;
    c.nq_pad = nq_pad;
    c.out_dist = out_dist;
    c.out_idx = out_idx;
    c.st = st;
    c.prof = prof;
    c.small = small;
    c.cap = cap;
    c.use_event = use_event;
    if (prof) {
        for (auto& ev : s.ev)
            if (!ev) SQ_HIP(hipEventCreate(&ev));
        if (!h->ev_ref && getenv("SQ_TRACE")) {
            SQ_HIP(hipEventCreate(&h->ev_ref));
            SQ_HIP(hipEventRecord(h->ev_ref, st));
        }
        SQ_HIP(hipEventRecord(s.ev[0], st));
    }
    SQ_TRY(s.cnt.reserve((size_t)nq_pad * 4 * 32));   // (the fused int8 call keeps its counters a cache line apart: I8_CNT_SHIFT)
    SQ_TRY(s.thr.reserve((size_t)nq_pad * 4));
    SQ_TRY(s.qn2.reserve((size_t)nq_pad * 8));
    SQ_TRY(s.q_scaled.reserve((size_t)nq_pad * d_pad * 4));
    SQ_TRY(s.out_keys.reserve((size_t)nq * k * key_bytes));
    SQ_TRY(s.status_host.reserve((size_t)(nq_pad + nq) * 4));
    if (!s.oflag.p) {   // [0] overflow flag of a call, [1] ticket counter of the fused head (self-cleaning: zero between calls)
        SQ_TRY(s.oflag.reserve(64));
        SQ_HIP(hipMemsetAsync(s.oflag.p, 0, 64, st));
    }
    if (cosine) {
        SQ_TRY(s.cos_nq.reserve((size_t)nq * 8));
        SQ_TRY(launch<dense_cos_qnorm_kernel>(dim3((nq + 63) / 64), dim3(64), 0, st, q, nq, d, s.cos_nq.as<double>()));
    }
    SQ_TRY(e.bind(h, s));
    if (small) {
        SQ_TRY(dense_small_enqueue(h, s, e));
    } else if (take_mid) {
        c.all_fallback = true;   // (nothing enqueued: dense_resolve starts every query at the middle tier)
        c.mid_direct = true;
    } else if (take_i8_wide) {
        SQ_TRY(dense8_wide_enqueue(h, s, e));
    } else if (take_i8) {
        SQ_TRY(dense8_enqueue(h, s, e));
    } else if (take_bf16) {
        SQ_TRY(dense_bf16_enqueue(h, s, e));
    } else {
        c.all_fallback = true;  // rows wider than the MFMA scan covers: exact path for every query
        // no bfloat16 copy to stream ("dense_bf16" = 0, or no memory for it): the middle tier first where its shape rule allows
        c.mid_direct = filter_ok && h->opt.dense_mid_tier != 0 && !h->opt.force_fallback && dense_mid_shape_ok(h);
    }
    if (prof) SQ_HIP(hipEventRecord(s.ev[3], st));
    if (use_event) SQ_TRY(s.sync.mark_done(st));
    c.pending = true;
    return SQ_OK;
}

// Measurement ("dense_debug" & 8192): where the fused int8 body kernel's workgroups spent their time (100 MHz clock;
// + 16384: printed).  Returns the kernel's own split for sq_stats_t in ms: the part after the last wave of any workgroup
// has left the stream is the tail (thresholds + re-rank).
static int dense_body_clocks(DenseHandle* h, DenseSlot& s, double& clk_tail_ms) {
    std::vector<long long> ck((size_t)s.clk8_wgs * 8);
    SQ_HIP(hipMemcpy(ck.data(), s.clk8.p, ck.size() * 8, hipMemcpyDeviceToHost));
    long long t0 = ck[0], tend = 0;
    for (int w = 0; w < s.clk8_wgs; ++w) t0 = std::min(t0, ck[(size_t)w * 8]), tend = std::max(tend, ck[(size_t)w * 8 + 4]);
    double sum[5] = {0, 0, 0, 0, 0}, mx[5] = {0, 0, 0, 0, 0}, mn[5] = {1e30, 1e30, 1e30, 1e30, 1e30};
    for (int w = 0; w < s.clk8_wgs; ++w) {
        const long long* e = &ck[(size_t)w * 8];
        const double v[5] = {(e[0] - t0) * 0.01, (e[1] - e[0]) * 0.01, (e[2] - e[1]) * 0.01, (e[3] - e[2]) * 0.01, (e[4] - e[3]) * 0.01};
        for (int j = 0; j < 5; ++j) sum[j] += v[j], mx[j] = std::max(mx[j], v[j]), mn[j] = std::min(mn[j], v[j]);
    }
    const char* names[5] = {"start offset", "stream (first wave out)", "wave skew (all waves out)", "thresholds", "re-rank"};
    if (h->opt.dense_debug & 16384) {
        fprintf(stderr, "[body clocks] %d workgroups, kernel span %.1f us\n", s.clk8_wgs, (tend - t0) * 0.01);
        for (int j = 0; j < 5; ++j) fprintf(stderr, "   %-28s min %8.1f  mean %8.1f  max %8.1f us\n", names[j], mn[j], sum[j] / s.clk8_wgs, mx[j]);
    }
    long long stream_end = 0;
    for (int w = 0; w < s.clk8_wgs; ++w) stream_end = std::max(stream_end, ck[(size_t)w * 8 + 2]);
    clk_tail_ms = (double)(tend - stream_end) * 1e-5;
    s.clk8_wgs = 0;
    return SQ_OK;
}

// dense_resolve, first phase: wait for the call's kernels, then timing, statistics and the bookkeeping that suspends a
// first filter whose lists overflow call after call.
static int dense_resolve_wait(DenseHandle* h, DenseSlot& s, const DenseCtx& e) {
    const DenseCall& c = s.call;
    const long long n = h->n;
    const int nq = c.nq;
    SQ_TRY(s.sync.wait(c.use_event, c.st));  // counts and status words are in e.hs_cnt / e.hs now
    SQ_HIP(hipGetLastError());
    double clk_tail_ms = -1.0;
    if (s.clk8_wgs > 0 && (h->opt.dense_debug & 8192)) SQ_TRY(dense_body_clocks(h, s, clk_tail_ms));
    if (c.prof) {
        float t1 = 0, t2 = 0;
        SQ_HIP(hipEventElapsedTime(&t1, s.ev[1], s.ev[2]));
        SQ_HIP(hipEventElapsedTime(&t2, s.ev[0], s.ev[3]));
        h->stats.scan_ms = t1;
        h->stats.total_ms = t2;
        if (h->ev_ref) {   // when the call's head / scan / re-rank / select ended, on the clock of the first traced call
            float at[5] = {0, 0, 0, 0, 0};
            const int order[5] = {0, 1, 2, 4, 3};
            for (int j = 0; j < 5; ++j) (void)hipEventElapsedTime(&at[j], h->ev_ref, s.ev[order[j]]);
            fprintf(stderr, "[smqtk_hip] trace slot %d: start %.1f | head-> %.1f | scan-> %.1f | rerank-> %.1f | select-> %.1f us\n",
                    (int)(&s - h->ring.slot), at[0] * 1e3f, at[1] * 1e3f, at[2] * 1e3f, at[3] * 1e3f, at[4] * 1e3f);
        }
        if (c.stats.scan_launches == 2) {  // (the filter path: a re-rank kernel followed the scan)
            float t3 = 0;
            SQ_HIP(hipEventElapsedTime(&t3, s.ev[2], s.ev[4]));
            h->stats.rerank_ms = t3;
            // the fused int8 call re-ranks inside the full-pass kernel: with its clocks recorded (dense_debug & 8192) the
            // tail's share of scan_ms is reported as rerank_ms
            if (clk_tail_ms >= 0.0) h->stats.rerank_ms = clk_tail_ms;
        }
    }
    for (int qi = 0; qi < nq; ++qi) h->stats.candidates += e.hs_cnt[qi];
    int over = 0;   // queries whose lists overflowed
    for (int qi = 0; qi < nq; ++qi) over += (e.hs[qi] & 1u) ? 1 : 0;
    if (c.int8) {
        // data the measured bound does not suit (every row of a tight cluster inside the slack): the lists overflow call
        // after call and each query pays a second tier -- after three such calls in a row the handle goes back to bf16
        const long long cands = h->stats.candidates;   // (of this call: summed above)
        // (... or pass so many rows that the re-rank outweighs the bytes saved: the bf16 filter passes ~50 k of 10 M)
        const bool heavy = 2 * over > nq || cands > (long long)nq * std::max<long long>(24ll * 1024, n / 128);
        h->i8.note_overflow(heavy, h->opt);
    }
    if (!c.small && (!c.int8 || h->opt.dense_int8 > 0)) {   // (an int8 stage in automatic mode suspends itself first, above)
        const bool heavy = 2 * over > nq;
        if (h->first_suspended) {          // this call was a probe
            if (heavy) {
                h->probe_interval = std::min(1024u, 2u * h->probe_interval);
                h->direct_calls = 0;   // (the next probe a whole interval from here)
            } else {
                h->first_suspended = false;
                h->overflow16 = 0;
                h->probe_interval = 16u;
            }
        } else {
            h->overflow16 = heavy ? h->overflow16 + 1 : 0;
            if (h->overflow16 >= 3) {
                h->first_suspended = true;
                h->direct_calls = 0;
            }
        }
    }
    return SQ_OK;
}

// Column means of the float32 rows into out[d_pad] (float64 sums over row blocks), finished on return: the L2 filter's
// origin (rows appended later keep it) and the cosine middle tier's
static int dense_column_means(const DenseHandle* h, DevBuf& out, hipStream_t st) {
    const long long n = h->n, rpb = 512;
    const int d = h->d, d_pad = h->d_pad;
    SQ_TRY(out.reserve((size_t)d_pad * 4));
    DevBuf colsum;
    int rc = colsum.reserve((size_t)d * 8);
    if (rc == SQ_OK && hipMemsetAsync(colsum.p, 0, (size_t)d * 8, st) != hipSuccess) rc = fail(SQ_ERR_HIP, "column means: memset failed");
    if (rc == SQ_OK) rc = launch<dense_colsum_kernel>(dim3((unsigned)((n + rpb - 1) / rpb)), dim3(256), 0, st, h->db, n, h->ld, d, rpb, colsum.as<double>());
    if (rc == SQ_OK) rc = launch<dense_center_kernel>(dim3((d_pad + 255) / 256), dim3(256), 0, st, colsum.as<double>(), n, d, d_pad, out.as<float>());
    if (rc == SQ_OK && stream_wait(st) != hipSuccess) rc = fail(SQ_ERR_HIP, "column means failed: %s", hipGetErrorString(hipGetLastError()));
    return rc;
}
// the cosine tier's origin and per-row terms (sq_dense_mid.hpp), once per index and again after an append
static int dense_mid_cos_terms(DenseHandle* h, hipStream_t st) {
    const long long n = h->n;
    const int d = h->d;
    if (!h->mid_cos_center.p) SQ_TRY(dense_column_means(h, h->mid_cos_center, st));
    h->mid_cos_ld = (n + 63) / 64 * 64;
    SQ_TRY(h->mid_cos_rows.reserve((size_t)h->mid_cos_ld * 2 * 4));
    SQ_TRY(launch<dense_mid_cos_rows_kernel>(dim3((unsigned)((n + 31) / 32)), dim3(256), 0, st, h->db, n, h->ld, d,
                                             (const float*)h->mid_cos_center.as<float>(), (const double*)h->cos_nx.as<double>(),
                                             h->mid_cos_rows.as<float>(), h->mid_cos_ld));
    h->mid_cos_n = n;
    return dense_dead_reapply(h, 0, st);   // (the terms just built are those of every row: removed ones leave again)
}

// dense_resolve, second phase -- the middle tier (sq_dense_mid.hpp): the uncertified queries of a filtered call, 32 per
// pass over the float32 rows, scored with 64 times less slack; whatever it certifies is final, the rest stays in `todo`
// and goes on to the exact path.
static int dense_mid_tier(DenseHandle* h, DenseSlot& s, const DenseCtx& e, std::vector<int>& todo) {
    const DenseCall& c = s.call;
    const long long n = h->n;
    const int d = h->d, d_pad = h->d_pad;
    const u32* deadp = h->deadp();
    hipStream_t st = c.st;
    const int ldq = (d + 3) / 4 * 4;
    const double eps_b_mid = (4.0 * d_pad + 8.0) * 1.1920928955078125e-07;
    const FilterBound fb_mid = filter_bound(0, kEpsAMid, eps_b_mid, h->xn2_max);
    const double alpha1 = filter_bound(0, kEpsA2, dense_eps_b(d_pad), 0.0).alpha;
    float c1 = (float)((1.0 - fb_mid.alpha) / (1.0 - alpha1) * (1.0 - 4.8e-7));
    const int waves = (size_t)TILE_ROWS * d_pad * 4 + (size_t)d_pad * 4 + (size_t)8 * MID_NSTAGE * MID_SLOT_BYTES <= 160 * 1024 - 64 ? 8 : 4;
    const size_t mid_lds = (size_t)TILE_ROWS * d_pad * 4 + (size_t)d_pad * 4 + (size_t)waves * MID_NSTAGE * MID_SLOT_BYTES;
    const int cus = cu_count(h->device);
    const long long n_tiles = (n + 31) / 32;
    int nrb = cus;
    if ((long long)nrb * waves > n_tiles) nrb = (int)((n_tiles + waves - 1) / waves);
    const long long n_waves = (long long)nrb * waves;
    SQ_TRY(h->mid_q.reserve((size_t)MID_MAX_Q * d * 4));
    SQ_TRY(h->mid_planes.reserve((size_t)MID_MAX_Q * d_pad * 4));
    // [qn2 f64 x32][thr f32 x32][cnt u32 x32][oflag u32 x16][qmap i32 x32]
    // cosine adds [cnq f64 x32][qw f32 x32][lin float2 x32]
    SQ_TRY(h->mid_small.reserve(32 * 8 + 32 * 4 + 32 * 4 + 64 + 32 * 4 + 32 * 8 + 32 * 4 + 32 * 8));
    SQ_TRY(h->mid_qal.reserve((size_t)MID_MAX_Q * ldq * 4));
    SQ_TRY(h->mid_wave_out.reserve((size_t)n_waves * kWaveCap * 8));
    SQ_TRY(h->mid_wave_cnt.reserve((size_t)n_waves * 8));
    SQ_TRY(h->mid_keys.reserve((size_t)MID_MAX_Q * e.cap * e.key_bytes));
    SQ_TRY(h->mid_out.reserve((size_t)MID_MAX_Q * c.k * e.key_bytes));
    DenseCtx me = e;   // the tier's own counters, thresholds and norms; its launches take 32 queries; no counts are copied out
    me.group_q = TILE_ROWS;
    me.hs_cnt_dev = nullptr;
    me.qn2 = h->mid_small.as<double>();
    me.thr = reinterpret_cast<float*>(me.qn2 + 32);
    me.cnt = reinterpret_cast<u32*>(me.thr + 32);
    me.oflag = me.cnt + 32;
    int* m_map = reinterpret_cast<int*>(me.oflag + 16);
    double* m_cnq = reinterpret_cast<double*>(m_map + 32);
    me.cnq = m_cnq;
    float* m_qw = reinterpret_cast<float*>(m_cnq + 32);
    float2* m_lin = reinterpret_cast<float2*>(m_qw + 32);
    if (e.cosine && h->mid_cos_n != n) SQ_TRY(dense_mid_cos_terms(h, st));
    // sample of true scores: every mid_stride-th row (about 64 k candidates per query pass the bound it gives)
    long long mid_stride = std::min<long long>(64, std::min<long long>((long long)e.cap / (8ll * e.kk), n / (8ll * e.kk)));
    if (mid_stride < 1) mid_stride = 1;
    const long long mid_ns = (n + mid_stride - 1) / mid_stride;
    const size_t mid_sample_lds = (size_t)d * 33 * 4;
    const dim3 sample_grid((unsigned)((mid_ns + 7) / 8));
    SQ_TRY(h->mid_sample.reserve((size_t)MID_MAX_Q * mid_ns * 4));
    const float* mq = h->mid_q.as<float>();
    const float* centerp = h->center.p ? h->center.as<float>() : nullptr;
    std::vector<int> left;
    for (size_t t0 = 0; t0 < todo.size(); t0 += MID_MAX_Q) {
        MidSelection sel{};
        sel.count = (int)std::min<size_t>(MID_MAX_Q, todo.size() - t0);
        for (int j = 0; j < MID_MAX_Q; ++j) sel.idx[j] = todo[t0 + (size_t)(j < sel.count ? j : 0)];
        SQ_TRY(launch<dense_mid_gather_kernel>(dim3(MID_MAX_Q), dim3(128), 0, st, c.q, d, sel, h->mid_q.as<float>(), m_map));
        DenseMidArgs a{};
        a.x = h->db;
        a.n = n;
        a.ld = h->ld;
        a.d = d;
        a.center = centerp;
        a.norms = h->norms.as<float>();
        a.norm_scale = c1;
        a.qs = h->mid_planes.as<uint4>();
        a.d_pad = d_pad;
        a.thr = me.thr;
        a.wave_out = h->mid_wave_out.as<uint2>();
        a.wave_cnt = h->mid_wave_cnt.as<u32>();
        a.wave_cap = kWaveCap;
        a.n_tiles = n_tiles;
        a.nrb = nrb;
        a.rowstat = e.cosine ? h->mid_cos_rows.as<float>() : nullptr;
        a.rowstat_ld = h->mid_cos_ld;
        a.qw = m_qw;
        const DenseSurvivors v = dense_survivors(h->mid_wave_out, h->mid_wave_cnt, h->mid_qal, h->mid_keys, h->mid_out, h->fb_sort, n_waves, 2, ldq,
                                                 sel.count);
        SQ_TRY(by_metric(e.cosine, [&](auto m) {
            using M = decltype(m);
            // query planes, a sample of true scores, the threshold from it
            if constexpr (M::cosine) {
                SQ_TRY(launch<dense_mid_cos_queries_kernel>(dim3(MID_MAX_Q), dim3(256), 0, st, h->mid_q.as<float>(), sel.count, d, d_pad,
                                                            (const float*)h->mid_cos_center.as<float>(), eps_b_mid, h->mid_planes.as<uint4>(), me.qn2, me.thr,
                                                            me.cnt, me.oflag, h->mid_qal.as<float>(), ldq, m_qw, m_lin));
                SQ_TRY(launch<dense_cos_qnorm_kernel>(dim3(1), dim3(64), 0, st, mq, sel.count, d, m_cnq));
                SQ_TRY(launch<dense_mid_cos_sample_kernel>(sample_grid, dim3(256), mid_sample_lds, st, h->db, h->ld, d, n, mid_stride, mid_ns, mq,
                                                           (const double*)me.qn2, (const double*)h->cos_nx.as<double>(), h->mid_sample.as<float>(), deadp));
                SQ_TRY(launch<kth_threshold_f32_kernel<DenseMidCosThrPost>>(
                    dim3(sel.count), dim3(1024), 0, st, h->mid_sample.as<float>(), mid_ns, e.kk, me.thr,
                    DenseMidCosThrPost{m_map, (const double*)c.out_dist, (const u32*)e.hs_dev, c.k, e.kk, (const float2*)m_lin}));
            } else {
                SQ_TRY(launch<dense_prep_queries_kernel>(dim3(MID_MAX_Q), dim3(256), 0, st, h->mid_q.as<float>(), sel.count, d, d_pad, h->metric,
                                                         h->mid_planes.as<uint4>(), me.qn2, me.thr, me.cnt, me.oflag, h->mid_qal.as<float>(), ldq, centerp));
                SQ_TRY(launch_lds<dense_mid_sample_kernel>(512 * 33 * 4, sample_grid, dim3(256), mid_sample_lds, st, h->db, h->ld, d, n, mid_stride, mid_ns,
                                                           mq, (const double*)me.qn2, h->mid_sample.as<float>(), deadp));
                SQ_TRY(launch<kth_threshold_f32_kernel<DenseMidThrPost>>(
                    dim3(sel.count), dim3(1024), 0, st, h->mid_sample.as<float>(), mid_ns, e.kk, me.thr,
                    DenseMidThrPost{m_map, (const float*)c.out_dist, (const u32*)e.hs_dev, c.k, e.kk, me.qn2, fb_mid.beta}));
            }
            SQ_TRY(waves == 8 ? launch_lds<dense_mid_scan_kernel<8, M::cosine>>(160 * 1024, dim3(nrb), dim3(512), mid_lds, st, a)
                              : launch_lds<dense_mid_scan_kernel<4, M::cosine>>(160 * 1024, dim3(nrb), dim3(256), mid_lds, st, a));
            auto fin = me.filter_fin<M>(M::cosine ? 0.0 : fb_mid.beta);
            fin.qmap = m_map;
            if constexpr (M::cosine) fin.lin = m_lin;
            return dense_survivor_tail<M>(h, me, v, c.k, fin, st);
        }));
        h->stats.scan_launches++;
        h->stats.bytes_scanned += n * (long long)d * 4;
        h->stats.mid_tier_queries += sel.count;
        SQ_HIP(stream_wait(st));  // the status words of these queries are in e.hs now
        SQ_HIP(hipGetLastError());
        for (int j = 0; j < sel.count; ++j)
            if (e.hs[sel.idx[j]] != 0) left.push_back(sel.idx[j]);
    }
    todo.swap(left);
    return SQ_OK;
}

// dense_resolve, third phase -- the exact full-keys path, a group of up to 8 queries per pass over the matrix
// (dense_exact_group_kernel): exact keys for all n rows, then a two-level select -- the k-th smallest of every
// fb_stride-th exact distance bounds the k-th of all, the keys at or below it (~2 k fb_stride of them) are compacted by
// the whole device and the one-workgroup select runs on those.  (That select over all n keys directly: 13 ms
// per query at 10 M rows against 1.2 ms for the keys.)  Ties that overflow the compacted list, or too few
// finite distances, go on to the select over all keys.
static int dense_exact_path(DenseHandle* h, DenseSlot& s, const DenseCtx& e, const std::vector<int>& todo) {
    const DenseCall& c = s.call;
    const long long n = h->n;
    const int d = h->d;
    const u32* deadp = h->deadp();
    hipStream_t st = c.st;
    const double* cnx = h->cos_nx.as<double>();
    long long fb_stride = std::min<long long>(64, std::min<long long>((long long)e.cap / (4ll * e.kk), n / (8ll * e.kk)));
    if (n < 65536 || fb_stride < 2 || (h->opt.dense_debug & 128)) fb_stride = 0;  // debug 128: measurement, full select
    const long long fb_ns = fb_stride ? (n + fb_stride - 1) / fb_stride : 0;
    // The group kernel takes a row width when its eight staged queries fit the LDS (round_up(d, 4) <= 5112) and the
    // row's summation tree fits the kernel's fixed depth (every width the LDS admits does; the rule is the tree's depth,
    // not d <= 128 << depth: 8191 elements need 7 levels).  Every other width goes one query per pass.
    const size_t grp_lds = (size_t)EXACT_GROUP * ((d + 3) / 4 * 4) * 4;
    constexpr int grp_lds_max = 160 * 1024 - 256;   // (the attribute is set once per device: the largest group any index asks for)
    const bool grp_ok = grp_lds <= (size_t)grp_lds_max && pw_tree_depth(d) <= EXACT_GROUP_DEPTH;
    // group size: the key arrays of a group stay under 4 GB; debug 256: measurement, one query per pass
    int gmax = 1;
    if (grp_ok && !(h->opt.dense_debug & 256))
        gmax = (int)std::min<long long>(EXACT_GROUP, std::max<long long>(1, (4ll << 30) / (n * (long long)e.key_bytes)));
    // the exact path keeps its own per-query counters: the slot's belong to a call that may still be in flight
    // when another asynchronous call's queries are redone
    SQ_TRY(h->fb_cnt.reserve((size_t)(c.nq + 64) * 4));
    u32* full_cnt = h->fb_cnt.as<u32>();
    for (size_t t0 = 0; t0 < todo.size(); t0 += (size_t)gmax) {
        const int gn = (int)std::min<size_t>((size_t)gmax, todo.size() - t0);
        ExactGroup grp{};
        for (int g = 0; g < EXACT_GROUP; ++g) grp.idx[g] = todo[t0 + (size_t)(g < gn ? g : 0)];
        grp.count = gn;
        h->stats.fallback_queries += gn;
        SQ_TRY(h->big_keys.reserve((size_t)gn * n * e.key_bytes));
        float* fb_sample = nullptr;
        float* fb_thr = nullptr;
        u32* fb_cnt = nullptr;
        if (fb_stride) {
            SQ_TRY(h->fb_sample.reserve((size_t)gn * fb_ns * 4 + 256));
            SQ_TRY(h->fb_keys.reserve((size_t)gn * e.cap * e.key_bytes));
            fb_thr = h->fb_sample.as<float>();               // [8] thresholds | [8] counts | samples
            fb_cnt = reinterpret_cast<u32*>(fb_thr + 8);
            fb_sample = fb_thr + 64;
        }
        unsigned gx = (unsigned)((n + 255) / 256);
        if (gx > 8192) gx = 8192;
        h->stats.scan_launches++;
        h->stats.bytes_scanned += n * (long long)d * 4;
        bool done[EXACT_GROUP] = {false, false, false, false, false, false, false, false};
        SQ_TRY(by_metric(e.cosine, [&](auto m) {
            using M = decltype(m);
            using K = typename M::Key;
            K* big = h->big_keys.as<K>();
            if (grp_ok) {
                SQ_TRY(launch_lds<dense_exact_group_kernel<M::cosine, K>>(grp_lds_max, dim3(gx), dim3(256), grp_lds, st, h->db, h->ld, d, c.q, grp, n, big,
                                                                          fb_sample, fb_ns, (int)fb_stride, M::cosine ? cnx : nullptr,
                                                                          M::cosine ? e.cnq : nullptr, deadp));
            } else {  // one query per pass (!grp_ok makes gmax 1: gn == 1)
                const int qi = grp.idx[0];
                if constexpr (M::cosine)
                    SQ_TRY(launch<dense_exact_cos_kernel>(dim3(gx, 1), dim3(256), 0, st, h->db, h->ld, d, c.q + (long long)qi * d, nullptr, full_cnt + qi,
                                                          (u32)n, n, 0ll, big, n, cnx, e.cnq + qi, fb_sample, (int)fb_stride, deadp));
                else
                    SQ_TRY(dense_exact_l2_keys(dim3(gx, 1), st, h->db, h->ld, d, c.q + (long long)qi * d, full_cnt + qi, n, big, n, fb_sample,
                                               (int)fb_stride, deadp));
            }
            if (fb_stride) {
                SQ_TRY(launch<kth_threshold_f32_kernel<KthIdentity>>(dim3(gn), dim3(1024), 0, st, fb_sample, fb_ns, e.kk, fb_thr, KthIdentity{}));
                SQ_TRY(launch<fill_u32_kernel>(dim3(1), dim3(64), 0, st, fb_cnt, (long long)gn, 0u));
                const unsigned gc = (unsigned)std::min<long long>((n + 1023) / 1024, 512);
                SQ_TRY(launch<dense_compact_keys_kernel<K>>(dim3(gc, gn), dim3(256), 0, st, big, n, fb_thr, h->fb_keys.as<K>(), e.cap, fb_cnt));
                SQ_TRY(h->fb_out.reserve((size_t)gn * c.k * e.key_bytes));
                auto fin = M::finalize(e, fb_cnt, e.cap, 2);
                fin.sel = grp;
                fin.dead = deadp;   // (the keys hold removed rows)
                SQ_TRY(select_launch_t<K>(h->fb_keys.as<K>(), fb_cnt, e.cap, (long long)e.cap, c.k, gn, h->fb_out.as<K>(), fin, st, h->fb_sort));
                SQ_HIP(stream_wait(st));  // the status words of the group are in e.hs now
                SQ_HIP(hipGetLastError());
                for (int g = 0; g < gn; ++g) done[g] = e.hs[grp.idx[g]] == 0;
            }
            for (int g = 0; g < gn; ++g) {
                if (done[g]) continue;
                const int qi = grp.idx[g];
                SQ_TRY(launch<fill_u32_kernel>(dim3(1), dim3(64), 0, st, full_cnt + qi, 1ll, (u32)n));
                SQ_TRY(h->fb_out.reserve((size_t)c.k * e.key_bytes));
                auto fin = M::finalize(e, full_cnt, (u32)n, 0);
                fin.q0 = qi;
                fin.dead = deadp;
                SQ_TRY(select_launch_t<K>(big + (long long)g * n, full_cnt + qi, (u32)n, n, c.k, 1, h->fb_out.as<K>(), fin, st, h->fb_sort));
            }
            return SQ_OK;
        }));
    }
    SQ_HIP(hipStreamSynchronize(st));
    SQ_HIP(hipGetLastError());
    return SQ_OK;
}

// Finish the call enqueued on slot `s`: wait for its kernels, collect the statistics, and redo every query the
// filter could not certify -- middle tier, then exact path (synchronously, on the call's stream).  h->stats = this call's.
static int dense_resolve(DenseHandle* h, DenseSlot& s) {
    DenseCall& c = s.call;
    if (!c.pending) return SQ_OK;
    c.pending = false;
    DenseCtx e{};
    SQ_TRY(e.bind(h, s));
    h->stats = c.stats;
    if (!c.all_fallback) SQ_TRY(dense_resolve_wait(h, s, e));
    const bool force_fb = h->opt.force_fallback != 0;
    std::vector<int> todo;
    for (int qi = 0; qi < c.nq; ++qi)
        if (c.all_fallback || (!c.small && (e.hs[qi] != 0 || force_fb))) todo.push_back(qi);
    if (todo.empty()) return SQ_OK;
    if (c.mid_direct)
        for (int qi = 0; qi < c.nq; ++qi) e.hs[qi] = 1u;   // (no first-filter result to take a bound from: DenseMid*ThrPost)
    if ((!c.all_fallback || c.mid_direct) && !c.small && !force_fb && h->opt.dense_mid_tier != 0 && dense_mid_shape_ok(h)) {
        SQ_TRY(dense_mid_tier(h, s, e, todo));
        if (todo.empty()) return SQ_OK;
    }
    return dense_exact_path(h, s, e, todo);
}

// Finish every asynchronous call still in flight, oldest first.
static int dense_sync_all(DenseHandle* h) {
    return h->ring.drain([h](DenseSlot& s) { return dense_resolve(h, s); });
}

static int dense_search_device(DenseHandle* h, const float* q, int nq, int k, void* out_dist, long long* out_idx,
                               hipStream_t st) {
    SQ_TRY(dense_enqueue(h, h->ring.slot[0], q, nq, k, out_dist, out_idx, st, false));
    return dense_resolve(h, h->ring.slot[0]);
}

// Large batches run in chunks so that the per-query workspace (candidate key lists of `cap` keys, the
// sample scores) stays bounded: 4096 queries need ~2.4 GB at the default list size.
static constexpr int kDenseQueryChunk = 4096;

static int dense_search_chunked(DenseHandle* h, const float* q, int nq, int k, void* out_dist, long long* out_idx,
                                hipStream_t st) {
    if (nq <= kDenseQueryChunk) return dense_search_device(h, q, nq, k, out_dist, out_idx, st);
    const size_t dsz = h->metric == SQ_METRIC_COSINE ? 8 : 4;
    sq_stats_t total{};
    for (int q0 = 0; q0 < nq; q0 += kDenseQueryChunk) {
        const int m = nq - q0 < kDenseQueryChunk ? nq - q0 : kDenseQueryChunk;
        SQ_TRY(dense_search_device(h, q + (long long)q0 * h->d, m, k, static_cast<char*>(out_dist) + (size_t)q0 * k * dsz,
                                   out_idx + (long long)q0 * k, st));
        total.scan_ms += h->stats.scan_ms;
        total.rerank_ms += h->stats.rerank_ms;
        total.total_ms += h->stats.total_ms;
        total.scan_launches += h->stats.scan_launches;
        total.candidates += h->stats.candidates;
        total.fallback_queries += h->stats.fallback_queries;
        total.bytes_scanned += h->stats.bytes_scanned;
    }
    h->stats = total;
    return SQ_OK;
}

// Row statistics and the bfloat16 scan copy of rows [row_base, n) -- row_base a multiple of 32 -- plus the padding
// rows of the last tile: the whole matrix at create (row_base = 0), the new rows on append.  The buffers are
// already large enough (dense_grow); the largest squared norm accumulates across calls.
// `parts`: the statistics, the copy, or both.  The copy part runs only where the handle keeps a copy (h->scan: option
// "dense_bf16"); on its own (dense_bf16_materialize) it leaves the statistics as they are -- cosine recomputes the rows'
// 1/|x| with the kernel that made them at create (it writes the same `norms` again), L2 reads the origin chosen at create.
enum : int { ROWS_STATS = 1, ROWS_COPY = 2 };
static int dense_build_rows(DenseHandle* h, long long row_base, int parts = ROWS_STATS | ROWS_COPY) {
    const long long n = h->n, n_pad = h->n_pad;
    const int d = h->d, d_pad = h->d_pad;
    const bool cosine = h->metric == SQ_METRIC_COSINE;
    const bool stats = (parts & ROWS_STATS) != 0;
    const bool copy = (parts & ROWS_COPY) != 0 && h->scan.p != nullptr && d_pad <= MAX_DPAD;
    SQ_TRY(h->scratch.reserve(256));
    float prev = (float)h->xn2_max;
    SQ_HIP(hipMemset(h->scratch.p, 0, 256));
    SQ_HIP(hipMemcpy(h->scratch.p, &prev, 4, hipMemcpyHostToDevice));  // non-negative floats order like their bits
    DevBuf inv;  // cosine: 1/|x| of the rows being built, indexed by row - row_base
    float* invp = nullptr;
    if (cosine) {
        SQ_TRY(inv.reserve((size_t)(n_pad - row_base) * 4));
        invp = inv.as<float>() - row_base;
    }
    int rc = SQ_OK;
    if (cosine && stats)
        rc = launch<dense_cos_norm_kernel>(dim3((unsigned)((n - row_base + 255) / 256)), dim3(256), 0, nullptr, h->db, n, h->ld, d,
                                           h->cos_nx.as<double>(), row_base);
    float* centerp = h->center.p ? h->center.as<float>() : nullptr;
    float* norms1p = nullptr;
    double shrink2 = 1.0, shrink1 = 1.0;
    if (!cosine) {
        // the row's share alpha |x|^2 of the filter's error bound comes off the stored norm (FilterBound)
        norms1p = h->norms1.as<float>();
        shrink2 = 1.0 - filter_bound(0, kEpsA2, dense_eps_b(d_pad), 0.0).alpha;
        shrink1 = 1.0 - filter_bound(0, kEpsA1, dense_eps_b(d_pad), 0.0).alpha;
    }
    if (rc == SQ_OK && (stats || (copy && cosine)))
        rc = launch<dense_rowstats_kernel>(dim3((unsigned)((n_pad - row_base) / 32)), dim3(256), 0, nullptr, h->db, n, h->ld, d, n_pad,
                                           h->scratch.as<u32>(), h->norms.as<float>(), invp, centerp, norms1p, shrink2, shrink1, row_base);
    const long long chunks = (n_pad - row_base) * (long long)(d_pad / 8);
    if (rc == SQ_OK && copy)
        rc = launch<dense_build_scan_kernel>(dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, nullptr, h->db, n, h->ld, d, d_pad, n_pad, invp,
                                             centerp, h->scan.as<uint4>(), row_base);
    u32 bits = 0;
    hipError_t e = hipMemcpy(&bits, h->scratch.p, 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (rc != SQ_OK) return rc;
    if (e != hipSuccess) return fail(SQ_ERR_HIP, "dense index build failed: %s", hipGetErrorString(e));
    float f;
    memcpy(&f, &bits, 4);
    h->xn2_max = (double)f;
    return SQ_OK;
}

// Option "dense_bf16" = -1 (or a handle whose option went from 0 to non-zero): the bfloat16 scan copy, built from the
// resident float32 rows by the first search that takes the bfloat16 chain -- the bytes sq_dense_create would have written
// (the same kernels, the origin and the statistics of the handle), with the removed rows' terms on top.  Called under the
// handle's lock before the call is enqueued: the calls in flight are finished first, as sq_dense_append does.  No memory
// for the copy is not an error: h->scan stays null, the call is answered by the later tiers and a later call tries again.
static int dense_bf16_materialize(DenseHandle* h) {
    if (h->scan.p || h->d_pad > MAX_DPAD) return SQ_OK;
    SQ_TRY(dense_sync_all(h));
    if (h->scan.reserve((size_t)h->n_pad * h->d_pad * 2) != SQ_OK) {
        (void)hipGetLastError();
        return SQ_OK;
    }
    int rc = dense_build_rows(h, 0, ROWS_COPY);
    if (rc == SQ_OK) rc = dense_dead_reapply(h, 0, nullptr);
    if (rc == SQ_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(SQ_ERR_HIP, "dense index: building the bfloat16 copy failed");
    if (rc != SQ_OK) h->scan.release();
    return rc;
}

// The int8 first-stage copy (sq_dense_i8.hpp), built at create for L2 matrices of up to 128 dimensions: the clamp and the
// residual bound R chosen from the measured residuals of twelve candidate clamps (the pair with the least R that leaves
// no more than 256 rows, or 20 per million, beyond it: those become always-candidates), the copy, its float64 residuals.  Data
// no clamp suits (heavy tails: too many rows beyond every bound) keeps the bf16 filter alone, and so does a failure to
// allocate: neither is an error.
// (rows of 513 to 8192 dimensions, sq_dense_i8_wide.hpp: only where option "dense_int8_wide" asks for it)
static bool dense8_is_wide(const DenseHandle* h) { return h->d > I8_MAX_ROW_BYTES; }
static bool dense8_wide_wanted(const DenseHandle* h) { return h->opt.dense_int8_wide != 0 && h->d_pad <= MAX_DPAD; }
// the build kernels for a row width: EPL = row bytes / 64, wide rows in chunks of 512 bytes (EPL = 8)
template <class F>
static int with_epl8(int row8, F&& f) {
    return with_row8(row8, [&](auto ks) { return f(std::integral_constant<int, decltype(ks)::value / 2>{}); }, true);
}
// rows a pass over the copy covers: whole ring units of 64 rows, wide rows whole 32-row tiles
static long long dense8_pass_rows(const DenseHandle* h, long long n) { return dense8_is_wide(h) ? (n + 31) / 32 * 32 : (n + 63) / 64 * 64; }

static size_t dense8_spare(const DenseHandle* h) { return dense8_is_wide(h) ? I8W_SPARE : 0; }   // (the wide kernel's last half unit: sq_dense_i8_wide.hpp)
// On every way out of dense8_build and dense8_append: a handle that does not use the copy keeps no memory for one (the
// build declined, an allocation failed, an append stopped half-way: a copy that lacks the new rows is not kept either).
struct Dense8DropUnused {
    Int8Copy& c;
    ~Dense8DropUnused() { if (!c.use) c.drop(); }
};
struct Dense8Stats {   // what dense8_quantise reads back (the kernels keep the maxima as the bits of non-negative floats)
    double energy, sum_r2;
    float max_r2, max_n;
    u32 flagged, pad;
};
// What the build's kernels share: the rows they quantise -- cosine the unit-length rows (nx64: their float64 |x|^2), L2 the
// rows minus the filter's origin -- and their scratch.
struct Dense8Work {
    const double* nx64;
    const float* center;
    DevBuf tmp, r2row;   // 64 bytes [Dense8Stats], the rows' squared residuals [n_alloc]
    explicit Dense8Work(const DenseHandle* h)
        : nx64(h->metric == SQ_METRIC_COSINE ? h->cos_nx.as<double>() : nullptr), center(h->metric != SQ_METRIC_COSINE ? h->center.as<float>() : nullptr) {}
};

// The element rms of the rows the copy would hold, from three passes of dense8_energy_kernel: no cap, then 16 x the mean
// of the pass before.  0: half the rows are non-finite or beyond 16 x the mean -- not this filter's data.
static int dense8_measure_rms(const DenseHandle* h, Dense8Work& w, int blocks, double* rms) {
    double cap_e = (double)__builtin_inff();
    for (int pass = 0; pass < 3; ++pass) {
        double er[2] = {0.0, 0.0};
        SQ_HIP(hipMemset(w.tmp.p, 0, 64));
        SQ_TRY(with_epl8(h->i8.row_bytes, [&](auto epl) {
            return launch<dense8_energy_kernel<decltype(epl)::value>>(dim3(blocks), dim3(256), 0, nullptr, h->db, h->n, h->ld, h->d, w.center, w.nx64, cap_e, w.tmp.as<double>());
        }));
        SQ_HIP(hipMemcpy(er, w.tmp.p, 16, hipMemcpyDeviceToHost));
        if (!(er[1] >= 0.5 * (double)h->n)) return *rms = 0.0, SQ_OK;
        *rms = sqrt(er[0] / (er[1] * h->d));
        cap_e = 16.0 * er[0] / er[1];
    }
    return SQ_OK;
}

// The clamp and R from the measured residuals of the candidate clamps (dense8_clip_stats_kernel, i8_choose_clamp);
// `best` stays empty where no clamp suits the data (or there is no memory for the counts).
static int dense8_choose(const DenseHandle* h, const Dense8Work& w, const Dense8ClipArgs& ca, int blocks, I8Clamp* best) {
    DevBuf clipbuf;   // counts u32 [NCLIP][NCUT] (freed on return: the copy is built next)
    const size_t clip_bytes = I8_NCLIP * I8_NCUT * 4;
    if (clipbuf.reserve(clip_bytes) != SQ_OK) return SQ_OK;
    SQ_HIP(hipMemset(clipbuf.p, 0, clip_bytes));
    // large matrices choose from every 8th row (the kernel evaluates twelve clamps per element: 16 ms of a 40 ms build at
    // 10 M x 128 when it reads every row; the choice needs the shape of the residuals' tail, not every row)
    const int clip_step = h->n >= 2000000 ? 8 : 1;
    SQ_TRY(with_epl8(h->i8.row_bytes, [&](auto epl) {
        return launch<dense8_clip_stats_kernel<decltype(epl)::value>>(dim3(blocks), dim3(256), 0, nullptr, h->db, h->n, h->ld, h->d, w.center, w.nx64, ca, clipbuf.as<u32>(), clip_step);
    }));
    u32 counts[I8_NCLIP][I8_NCUT];
    SQ_HIP(hipMemcpy(counts, clipbuf.p, clip_bytes, hipMemcpyDeviceToHost));
    *best = i8_choose_clamp(counts, ca, h->d, h->n, clip_step);
    return SQ_OK;
}

// One quantise step, the build's (row_base 0, the step and cut just chosen) and an append's (from the unit the old rows
// ended in, the build's step and cut): the rows from row_base on quantised into the copy, +inf behind the last unit, the
// wide kernel's spare zeroed.  Rows beyond the cut become always-candidates first; the largest residual and the largest
// |x'|^2 read back are then of the rows that REMAIN under it (a row 100x the rest would otherwise set X for every query).
static int dense8_quantise(DenseHandle* h, Dense8Work& w, float dx, float cut, long long row_base, long long n_alloc, int stats_blocks, Dense8Stats* out) {
    Int8Copy& c = h->i8;
    const long long n = h->n;
    signed char* o8 = c.scan.as<signed char>();
    float *nr8 = c.nrow.as<float>(), *r2p = w.r2row.as<float>();
    SQ_HIP(hipMemset(w.tmp.p, 0, 64));
    SQ_TRY(with_epl8(c.row_bytes, [&](auto epl) {
        return launch<dense8_build_kernel<decltype(epl)::value>>(dim3((unsigned)((n_alloc - row_base + 3) / 4)), dim3(256), 0, nullptr, h->db, n, h->ld, h->d, n_alloc,
                                                                 w.center, w.nx64, 1.0f / dx, dx, o8, nr8, r2p, row_base, c.row_bytes);
    }));
    SQ_HIP(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(nr8 + n_alloc), 0x7f800000, 64));   // (+inf behind the last unit)
    if (dense8_spare(h)) SQ_HIP(hipMemset(o8 + (size_t)n_alloc * c.row_bytes, 0, dense8_spare(h)));
    Dense8Stats* dev = w.tmp.as<Dense8Stats>();
    SQ_TRY(launch<dense8_flag_kernel>(dim3((unsigned)((n - row_base + 255) / 256)), dim3(256), 0, nullptr, r2p, nr8, n, cut, &dev->flagged, row_base));
    SQ_TRY(launch<dense8_resid_stats_kernel>(dim3(stats_blocks), dim3(256), 0, nullptr, r2p + row_base, nr8 + row_base, n - row_base, &dev->sum_r2,
                                             reinterpret_cast<u32*>(&dev->max_r2)));
    SQ_HIP(hipMemcpy(out, dev, sizeof(*out), hipMemcpyDeviceToHost));
    SQ_HIP(hipDeviceSynchronize());
    c.n_pass = dense8_pass_rows(h, n), c.n_alloc = n_alloc;   // (what the copy covers now)
    return SQ_OK;
}

// decide, measure the rms, choose the clamp, quantise, publish
static int dense8_build(DenseHandle* h) {
    Int8Copy& c = h->i8;
    c.use = c.suspended = false, c.overflow = 0;
    Dense8DropUnused drop_unused{c};
    const bool wide = dense8_is_wide(h), cosine = h->metric == SQ_METRIC_COSINE;
    const long long n = h->n, n_alloc = (n + 127) / 128 * 128;
    const int d = h->d, stat_blocks = cu_count(h->device) * 8;
    // decide: what a handle without a copy would start now (a copy that was there is chosen again on the same terms)
    if (i8_append_action(h->opt.dense_int8, wide, dense8_wide_wanted(h), false, n, 0) != I8Action::build) return SQ_OK;
    c.n8_built = n;   // (an attempt counts whether or not the data is accepted: dense8_append tries again when the index has doubled)
    c.row_bytes = wide ? i8w_row_bytes(d) : i8_row_bytes(d);
    Dense8Work w(h);
    if (w.tmp.reserve(64) != SQ_OK || w.r2row.reserve((size_t)n_alloc * 4) != SQ_OK || c.scan.reserve((size_t)n_alloc * c.row_bytes + dense8_spare(h)) != SQ_OK ||
        c.nrow.reserve((size_t)(n_alloc + 64) * 4) != SQ_OK)   // (+ 64: a 32-row unit's DMA fetches 64 row terms)
        return (void)hipGetLastError(), SQ_OK;
    double rms = 0.0;
    SQ_TRY(dense8_measure_rms(h, w, stat_blocks, &rms));
    if (!(rms > 0.0) || !(rms < 1e30)) return SQ_OK;
    const Dense8ClipArgs ca = i8_clip_candidates(rms, d);
    I8Clamp best;
    SQ_TRY(dense8_choose(h, w, ca, stat_blocks, &best));
    if (!best.found()) return SQ_OK;
    const float dx = ca.dx[best.c];
    double cut = best.r * best.r * (1.0 + 1e-4);   // (the choice was made in float32)
    Dense8Stats res{};
    SQ_TRY(dense8_quantise(h, w, dx, (float)cut, 0, n_alloc, 1024, &res));
    if ((double)res.max_r2 < cut) cut = (double)res.max_r2 * (1.0 + 1e-6);   // nothing near the bound: R is simply the largest
    if ((double)res.flagged > 4.0 * i8_always_budget(n)) return SQ_OK;
    c.dx = dx;
    c.rmax = sqrt(cut) * (1.0 + 1e-6);
    c.xmax = cosine ? 1.0 + 1e-6 : sqrt((double)res.max_n) * (1.0 + 1e-6);   // (cosine: unit rows; their row term is 0)
    c.flagged = res.flagged;
    if (getenv("SQ_INT8_REPORT"))   // (measurement aid: what the build chose)
        fprintf(stderr, "[smqtk_hip] int8 filter: clamp %.2f rms, step %.5g, R %.5g (%.2f x the rounding residual), X %.5g, %u always-candidate rows of %lld\n",
                kClip[best.c], (double)dx, c.rmax, kCut[best.m], c.xmax, res.flagged, n);
    // appended rows are flagged against R^2 itself (rounded down): R may be smaller than the bound the build flagged with
    c.cut = (float)cut;
    if ((double)c.cut > cut) c.cut = __builtin_nextafterf(c.cut, 0.f);
    c.use = true;
    return SQ_OK;
}

// Everything an index derives from its float32 rows, built from scratch: the L2 filter's origin, the row statistics, the
// bfloat16 scan copy, the int8 copy.  sq_dense_create, and sq_dense_compact over the rows that are left.
static int dense_build_all(DenseHandle* h) {
    const int d_pad = h->d_pad;
    const bool cosine = h->metric == SQ_METRIC_COSINE;
    // the filter's origin (L2): the column means
    if (!cosine && d_pad <= MAX_DPAD && !h->opt.dense_no_center) SQ_TRY(dense_column_means(h, h->center, nullptr));
    // row statistics, then the bfloat16 scan copy (skipped for rows wider than the scan kernel covers)
    SQ_TRY(h->norms.reserve((size_t)h->n_pad * 4));
    if (!cosine) SQ_TRY(h->norms1.reserve((size_t)h->n_pad * 4));
    if (cosine) {
        SQ_TRY(h->cos_nx.reserve((size_t)h->n * 8));
        SQ_TRY(h->zeros.reserve(256));
        SQ_HIP(hipMemset(h->zeros.p, 0, 256));
    }
    // ("dense_bf16" = 1 only: -1 leaves the copy to the first search that streams it, 0 builds none)
    if (d_pad <= MAX_DPAD && h->opt.dense_bf16 == 1) SQ_TRY(h->scan.reserve((size_t)h->n_pad * d_pad * 2));
    SQ_TRY(dense_build_rows(h, 0));
    SQ_HIP(hipDeviceSynchronize());
    const auto t8 = std::chrono::steady_clock::now();
    SQ_TRY(dense8_build(h));
    SQ_HIP(hipDeviceSynchronize());
    h->build8_us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t8).count();
    return SQ_OK;
}

// The int8 copy after an append (h->n is the new row count; the rows are in place).  The step and the residual cut of
// the build stay: new rows are quantised with them, rows they do not suit become always-candidates like the build's own.
// An index that has doubled since its last attempt (i8_append_action) or collected too many always-candidates chooses again.
static int dense8_append(DenseHandle* h, long long n_old) {
    Int8Copy& c = h->i8;
    const long long n = h->n, n_alloc = (n + 127) / 128 * 128;
    const I8Action act = i8_append_action(h->opt.dense_int8, dense8_is_wide(h), dense8_wide_wanted(h), c.use, n, c.n8_built);
    if (act != I8Action::extend) return act == I8Action::build ? dense8_build(h) : SQ_OK;
    c.use = false;   // (until the copy holds the new rows)
    Dense8DropUnused drop_unused{c};
    Dense8Work w(h);
    if (grow_keep(c.scan, (size_t)c.n_alloc * c.row_bytes, (size_t)n_alloc * c.row_bytes + dense8_spare(h)) != SQ_OK ||
        grow_keep(c.nrow, (size_t)(c.n_alloc + 64) * 4, (size_t)(n_alloc + 64) * 4) != SQ_OK || w.tmp.reserve(64) != SQ_OK ||
        w.r2row.reserve((size_t)n_alloc * 4) != SQ_OK)
        return (void)hipGetLastError(), SQ_OK;   // (no memory for the copy is not an error: the index goes on without one)
    // the unit the old rows ended in is redone with the new ones; the largest |x'|^2 is of the new rows that are not flagged
    // (a flagged row needs no X)
    Dense8Stats res{};
    SQ_TRY(dense8_quantise(h, w, c.dx, c.cut, n_old / 128 * 128, n_alloc, 256, &res));
    if (h->metric != SQ_METRIC_COSINE && res.max_n > 0.f) c.xmax = std::max(c.xmax, sqrt((double)res.max_n) * (1.0 + 1e-6));
    // (the redone unit's old always-candidates are counted again: an over-estimate on the safe side)
    c.flagged += res.flagged;
    c.use = true;
    if ((double)c.flagged > 4.0 * i8_always_budget(n)) return dense8_build(h);   // the new rows do not look like the old ones: choose again
    return SQ_OK;
}

static void dense_set_rows(DenseHandle* h, long long n) { h->n = n, h->n_pad = (n + TILE_ROWS - 1) / TILE_ROWS * TILE_ROWS; }
// `n` rows of `d` floats into the owned matrix at `dst`, whose rows are padded with zeros to `ld` floats
static int dense_upload_rows(float* dst, long long ld, const float* rows, long long n, int d, hipMemcpyKind kind) {
    hipError_t e;
    if (ld == d) {
        e = hipMemcpy(dst, rows, (size_t)n * d * 4, kind);
    } else {
        e = hipMemset(dst, 0, (size_t)n * ld * 4);
        if (e == hipSuccess) e = hipMemcpy2D(dst, (size_t)ld * 4, rows, (size_t)d * 4, (size_t)d * 4, (size_t)n, kind);
    }
    return e == hipSuccess ? SQ_OK : fail(SQ_ERR_HIP, "copy of the rows failed: %s", hipGetErrorString(e));
}

// Room for `n_new` rows in every per-row buffer, contents kept (grow_keep: a stream of small appends copies the matrix
// O(log) times).
static int dense_grow(DenseHandle* h, long long n_new) {
    const long long n_pad_new = (n_new + TILE_ROWS - 1) / TILE_ROWS * TILE_ROWS;
    const bool cosine = h->metric == SQ_METRIC_COSINE;
    if (h->owned.p || h->n == 0) {
        SQ_TRY(grow_keep(h->owned, (size_t)h->n * h->ld * 4, (size_t)n_new * h->ld * 4));
        h->db = h->owned.as<float>();
    }
    SQ_TRY(grow_keep(h->norms, (size_t)h->n_pad * 4, (size_t)n_pad_new * 4));
    if (!cosine) SQ_TRY(grow_keep(h->norms1, (size_t)h->n_pad * 4, (size_t)n_pad_new * 4));
    if (cosine) SQ_TRY(grow_keep(h->cos_nx, (size_t)h->n * 8, (size_t)n_new * 8));
    // (an index without the bfloat16 copy -- "dense_bf16" -- is appended to without one)
    if (h->scan.p) SQ_TRY(grow_keep(h->scan, (size_t)h->n_pad * h->d_pad * 2, (size_t)n_pad_new * h->d_pad * 2));
    return SQ_OK;
}

}  // namespace sq

using namespace sq;

// What an index keeps resident and what its build cost (bench.py's `resident_bytes` / `index_build_ms`).
extern "C" int sq_dense_info(sq_handle_t hid, int64_t* out, int n_out) {
    auto* h = static_cast<DenseHandle*>(lookup_handle(hid, H_DENSE));
    if (!h) return fail(SQ_ERR_INVALID, "sq_dense_info: unknown handle");
    if (!out || n_out < SQ_DENSE_INFO_FIELDS) return fail(SQ_ERR_INVALID, "sq_dense_info: room for %d values needed", SQ_DENSE_INFO_FIELDS);
    std::lock_guard<std::mutex> l(h->mu);
    out[0] = h->n;
    out[1] = h->d;
    out[2] = (int64_t)h->n * h->ld * 4;                                  // the float32 rows (the re-rank reads them) ...
    out[3] = h->owned.p ? 1 : 0;                                          // ... owned by the library (1) or borrowed from the caller (0)
    out[4] = (int64_t)h->scan.cap;                                        // bfloat16 scan copy
    out[5] = (int64_t)h->i8.bytes();                                      // int8 scan copy + its row terms
    out[6] = (int64_t)(h->norms.cap + h->norms1.cap + h->cos_nx.cap + h->center.cap + h->zeros.cap);   // row statistics
    out[7] = h->i8.in_use() ? 1 : 0;                                      // the int8 first stage is in use
    out[8] = h->build_us;                                                 // sq_dense_create: wall time of the whole build
    out[9] = h->build8_us;                                                // ... of which the int8 copy (statistics, clamp choice, copy)
    return SQ_OK;
}

static int dense_create_impl(const float* db, int64_t n, int d, int metric, int mem, int64_t id_base,
                             const std::vector<std::pair<int Options::*, int>>& overrides, sq_handle_t* out) {
    const auto t_create = std::chrono::steady_clock::now();
    if (!db || !out || n <= 0 || d <= 0) return fail(SQ_ERR_INVALID, "sq_dense_create: bad argument");
    if (metric != SQ_METRIC_L2 && metric != SQ_METRIC_COSINE) return fail(SQ_ERR_INVALID, "sq_dense_create: unknown metric %d", metric);
    if (n >= (1ll << 32)) return fail(SQ_ERR_UNSUPPORTED, "sq_dense_create: more than 2^32-1 rows per shard");
    if (mem == SQ_MEM_DEVICE && ((reinterpret_cast<uintptr_t>(db) & 15u) != 0 || (d & 3) != 0))
        return fail(SQ_ERR_UNSUPPORTED, "sq_dense_create: a borrowed device matrix must be 16-byte aligned with d %% 4 == 0 (d=%d)", d);
    auto h = std::make_unique<DenseHandle>();
    h->kind = H_DENSE;
    dense_set_rows(h.get(), n);
    h->n_live = n;
    h->d = d;
    h->d_pad = (d + KT - 1) / KT * KT;
    h->metric = metric;
    h->id_base = id_base;
    h->overrides = overrides;   // (create-time choices -- "dense_int8" = 0: no int8 copy -- are the handle's own)
    h->refresh_options();
    if (hipGetDevice(&h->device) != hipSuccess) return fail(SQ_ERR_HIP, "sq_dense_create: no HIP device");
    if (mem == SQ_MEM_DEVICE) {
        h->db = db;
        h->ld = d;
    } else {
        // owned float32 copy, rows padded to a multiple of 4 floats so the exact kernel can use 16-byte loads
        h->ld = (d + 3) / 4 * 4;
        SQ_TRY(h->owned.reserve((size_t)n * h->ld * 4));
        h->db = h->owned.as<float>();
        SQ_TRY(dense_upload_rows(h->owned.as<float>(), h->ld, db, n, d, hipMemcpyHostToDevice));
    }
    SQ_TRY(dense_build_all(h.get()));
    h->build_us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t_create).count();
    *out = register_handle(h.release());
    return SQ_OK;
}

extern "C" int sq_dense_create(const float* db, int64_t n, int d, int metric, int mem, int64_t id_base,
                               sq_handle_t* out) {
    return dense_create_impl(db, n, d, metric, mem, id_base, {}, out);
}

extern "C" int sq_dense_create_opts(const float* db, int64_t n, int d, int metric, int mem, int64_t id_base,
                                    const char* const* opt_names, const int64_t* opt_values, int n_opts, sq_handle_t* out) {
    if (n_opts < 0 || (n_opts > 0 && (!opt_names || !opt_values))) return fail(SQ_ERR_INVALID, "sq_dense_create_opts: bad option arrays");
    std::vector<std::pair<int Options::*, int>> ov;
    for (int i = 0; i < n_opts; ++i) {
        int Options::*f = option_member(opt_names[i]);
        if (!f) return fail(SQ_ERR_INVALID, "sq_dense_create_opts: unknown option '%s'", opt_names[i] ? opt_names[i] : "(null)");
        ov.emplace_back(f, (int)opt_values[i]);
    }
    return dense_create_impl(db, n, d, metric, mem, id_base, ov, out);
}

extern "C" int sq_dense_append(sq_handle_t hid, const float* rows, int64_t n_add, int mem) {
    auto* h = static_cast<DenseHandle*>(lookup_handle(hid, H_DENSE));
    if (!h) return fail(SQ_ERR_INVALID, "sq_dense_append: unknown handle");
    if (!rows || n_add <= 0) return fail(SQ_ERR_INVALID, "sq_dense_append: bad argument");
    std::lock_guard<std::mutex> l(h->mu);
    h->refresh_options();
    if (!h->owned.p) return fail(SQ_ERR_UNSUPPORTED, "sq_dense_append: the index borrows the caller's device matrix");
    SQ_HIP(hipSetDevice(h->device));
    SQ_TRY(dense_sync_all(h));
    const long long n_old = h->n, n_new = n_old + n_add;
    if (n_new >= (1ll << 32)) return fail(SQ_ERR_UNSUPPORTED, "sq_dense_append: more than 2^32-1 rows per shard");
    SQ_TRY(dense_grow(h, n_new));
    if (h->dead.p) {   // the bitmap of removed rows follows the matrix (new rows are live; holes are not reused)
        const long long words = (n_new + 31) / 32;
        SQ_TRY(grow_keep(h->dead, (size_t)h->dead_words * 4, (size_t)words * 4));
        SQ_HIP(hipMemset(h->dead.as<u32>() + h->dead_words, 0, h->dead.cap - (size_t)h->dead_words * 4));
        h->dead_words = words;
    }
    SQ_TRY(dense_upload_rows(h->owned.as<float>() + n_old * h->ld, h->ld, rows, n_add, h->d, mem == SQ_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    dense_set_rows(h, n_new);
    // the tile the old rows ended in is rebuilt together with the new ones (its padding rows become real rows)
    h->n_live += n_add;
    SQ_TRY(dense_build_rows(h, n_old / TILE_ROWS * TILE_ROWS));
    SQ_TRY(dense8_append(h, n_old));
    // the tile and the int8 unit the old rows ended in were rebuilt from their rows (an index that has doubled rebuilds its
    // whole int8 copy): the removed rows among them leave again
    if (h->dead.p) {
        SQ_TRY(dense_dead_reapply(h, 0, nullptr));
        SQ_HIP(hipDeviceSynchronize());
    }
    return SQ_OK;
}

// ---- removal and compaction (sq_dense_remove.hpp; impls/nn_index/faiss.py:644-694)
extern "C" int sq_dense_count(sq_handle_t hid, int64_t* n_rows, int64_t* n_live) {
    auto* h = static_cast<DenseHandle*>(lookup_handle(hid, H_DENSE));
    if (!h) return fail(SQ_ERR_INVALID, "sq_dense_count: unknown handle");
    std::lock_guard<std::mutex> l(h->mu);
    if (n_rows) *n_rows = h->n;
    if (n_live) *n_live = h->n_live;
    return SQ_OK;
}

// sq_dense_remove under the handle's lock, the calls in flight finished; `fresh`: the handle has no bitmap yet
static int dense_remove_rows(DenseHandle* h, const int64_t* ids, int64_t m, bool fresh) {
    DevBuf ids_dev, won, status;
    if (fresh) {
        const long long words = (h->n + 31) / 32;
        if (const int rc = h->dead.reserve((size_t)words * 4)) return rc;
        if (hipMemset(h->dead.p, 0, h->dead.cap) != hipSuccess) return fail(SQ_ERR_HIP, "sq_dense_remove: memset failed");
        h->dead_words = words;
    }
    if (const int rc = ids_dev.reserve((size_t)m * 8)) return rc;
    if (const int rc = won.reserve((size_t)m * 4)) return rc;
    if (const int rc = status.reserve(4)) return rc;
    if (hipMemcpy(ids_dev.p, ids, (size_t)m * 8, hipMemcpyHostToDevice) != hipSuccess || hipMemset(status.p, 0, 4) != hipSuccess)
        return fail(SQ_ERR_HIP, "sq_dense_remove: copy of the ids failed");
    const dim3 grid((unsigned)((m + 255) / 256)), blk(256);
    // pass 1: validate and mark
    if (const int rc = launch<dense_remove_kernel>(grid, blk, 0, nullptr, ids_dev.as<long long>(), (long long)m, h->id_base, h->n, h->dead.as<u32>(),
                                                   won.as<u32>(), status.as<u32>()))
        return rc;
    u32 st = 0;
    if (hipMemcpy(&st, status.p, 4, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(SQ_ERR_HIP, "sq_dense_remove: %s", hipGetErrorString(hipGetLastError()));
    if (st != 0) {
        // pass 2, refused: the bits this call set are cleared again; nothing else was written
        if (const int rc = launch<dense_remove_undo_kernel>(grid, blk, 0, nullptr, ids_dev.as<long long>(), (long long)m, h->id_base, h->dead.as<u32>(),
                                                            won.as<u32>()))
            return rc;
        if (hipDeviceSynchronize() != hipSuccess) return fail(SQ_ERR_HIP, "sq_dense_remove: undo failed");
        return fail(SQ_ERR_INVALID, "sq_dense_remove: %s%s%s; nothing was removed", (st & DENSE_REMOVE_RANGE) ? "an id is out of range" : "",
                    st == 3u ? ", " : "", (st & DENSE_REMOVE_DEAD) ? "an id is already removed or listed twice" : "");
    }
    // pass 2: the per-row terms of every copy the handle keeps
    if (const int rc = launch<dense_remove_apply_kernel>(grid, blk, 0, nullptr, ids_dev.as<long long>(), (long long)m, h->id_base, dense_dead_terms(h)))
        return rc;
    if (hipDeviceSynchronize() != hipSuccess) return fail(SQ_ERR_HIP, "sq_dense_remove: %s", hipGetErrorString(hipGetLastError()));
    h->n_live -= m;
    return SQ_OK;
}

extern "C" int sq_dense_remove(sq_handle_t hid, const int64_t* ids, int64_t m) {
    auto* h = static_cast<DenseHandle*>(lookup_handle(hid, H_DENSE));
    if (!h) return fail(SQ_ERR_INVALID, "sq_dense_remove: unknown handle");
    if (!ids || m <= 0) return fail(SQ_ERR_INVALID, "sq_dense_remove: bad argument");
    std::lock_guard<std::mutex> l(h->mu);
    h->refresh_options();
    SQ_HIP(hipSetDevice(h->device));
    SQ_TRY(dense_sync_all(h));
    // (more ids than live rows: one of them is dead or listed twice; as many: the index would be left without a row,
    // which sq_dense_create does not build either)
    if (m >= h->n_live)
        return fail(SQ_ERR_INVALID, "sq_dense_remove: %lld ids for %lld live rows (an index keeps at least one row: destroy it instead)",
                    (long long)m, h->n_live);
    const bool fresh = h->dead.p == nullptr;
    const int rc = dense_remove_rows(h, ids, m, fresh);
    if (rc != SQ_OK && fresh) {   // a refused first removal leaves no bitmap behind
        h->dead.release();
        h->dead_words = 0;
    }
    return rc;
}

extern "C" int sq_dense_compact(sq_handle_t hid, int64_t* old_to_new) {
    auto* h = static_cast<DenseHandle*>(lookup_handle(hid, H_DENSE));
    if (!h) return fail(SQ_ERR_INVALID, "sq_dense_compact: unknown handle");
    std::lock_guard<std::mutex> l(h->mu);
    h->refresh_options();
    if (!h->owned.p) return fail(SQ_ERR_UNSUPPORTED, "sq_dense_compact: the index borrows the caller's device matrix");
    SQ_HIP(hipSetDevice(h->device));
    SQ_TRY(dense_sync_all(h));
    const long long n_old = h->n;
    if (!h->dead.p || h->n_live == n_old) {   // nothing to drop: the index stays as it is
        if (old_to_new)
            for (long long i = 0; i < n_old; ++i) old_to_new[i] = h->id_base + i;
        return SQ_OK;
    }
    const long long cpr = h->ld / 4;   // (the owned matrix: rows of whole 16-byte chunks)
    const long long words = (n_old + 31) / 32;
    DevBuf prefix, total, map, fresh_rows, bounce;
    if (const int rc = prefix.reserve((size_t)words * 8)) return rc;
    if (const int rc = total.reserve(8)) return rc;
    SQ_TRY(launch<dense_compact_scan_kernel>(dim3(1), dim3(1024), 0, nullptr, h->deadp(), n_old, words, prefix.as<unsigned long long>(),
                                             total.as<unsigned long long>()));
    unsigned long long live_dev = 0;
    if (hipMemcpy(&live_dev, total.p, 8, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(SQ_ERR_HIP, "sq_dense_compact: %s", hipGetErrorString(hipGetLastError()));
    const long long live = (long long)live_dev;
    if (live != h->n_live) return fail(SQ_ERR_INTERNAL, "sq_dense_compact: the bitmap holds %lld live rows, the handle counts %lld", live, h->n_live);
    if (old_to_new) {   // before anything changes: a failure here leaves the index as it was
        if (const int rc = map.reserve((size_t)n_old * 8)) return rc;
        SQ_TRY(launch<dense_compact_map_kernel>(dim3((unsigned)((n_old + 255) / 256)), dim3(256), 0, nullptr, h->deadp(), prefix.as<unsigned long long>(),
                                                n_old, h->id_base, map.as<long long>()));
        if (hipMemcpy(old_to_new, map.p, (size_t)n_old * 8, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(SQ_ERR_HIP, "sq_dense_compact: %s", hipGetErrorString(hipGetLastError()));
        map.release();   // (now: the gather below wants the room)
    }
    // every copy derived from the rows is rebuilt below: their memory goes first, so that the gather finds room
    for (DevBuf* b : {&h->scan, &h->norms, &h->norms1, &h->cos_nx, &h->center, &h->mid_cos_center, &h->mid_cos_rows}) b->release();
    h->i8.drop();
    const size_t row_bytes = (size_t)h->ld * 4;
    // rows of one gather launch: its grid stays below 2^30 workgroups
    const long long launch_rows = std::max<long long>(32, ((1ll << 30) * 256 / cpr) / 32 * 32);
    auto gather = [&](uint4* dst, long long r0, long long r1, long long dst_row0) {
        return launch<dense_compact_gather_kernel>(dim3((unsigned)(((r1 - r0) * cpr + 255) / 256)), dim3(256), 0, nullptr, h->owned.as<uint4>(), dst, cpr, r0,
                                                   r1, dst_row0, h->deadp(), prefix.as<unsigned long long>());
    };
    if (fresh_rows.reserve((size_t)live * row_bytes) == SQ_OK) {
        // a second buffer: one pass, and the matrix shrinks to the rows that are left
        for (long long r0 = 0; r0 < n_old; r0 += launch_rows)
            if (const int rc = gather(fresh_rows.as<uint4>(), r0, std::min(n_old, r0 + launch_rows), 0)) return rc;
        if (hipDeviceSynchronize() != hipSuccess) return fail(SQ_ERR_HIP, "sq_dense_compact: gather failed: %s", hipGetErrorString(hipGetLastError()));
        h->owned = std::move(fresh_rows);
    } else {
        // No room for a second matrix: in place, front to back, a piece of rows at a time through a bounce buffer.  Piece j
        // lands at rows [new(r0), new(r1)) with new(r1) <= r1: below every row a later piece has yet to read, and the piece
        // itself has been read into the bounce buffer completely (stream order) before it is written.
        (void)hipGetLastError();
        long long piece = std::min<long long>(launch_rows, std::max<long long>(32, (long long)(((size_t)64 << 20) / row_bytes) / 32 * 32));
        if (const int rc = bounce.reserve((size_t)piece * row_bytes)) return fail(rc, "sq_dense_compact: no memory for the gather; the index must be built again");
        std::vector<unsigned long long> pre((size_t)words);
        if (hipMemcpy(pre.data(), prefix.p, (size_t)words * 8, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(SQ_ERR_HIP, "sq_dense_compact: %s", hipGetErrorString(hipGetLastError()));
        for (long long r0 = 0; r0 < n_old; r0 += piece) {
            const long long r1 = std::min(n_old, r0 + piece);
            const long long d0 = (long long)pre[(size_t)(r0 >> 5)], d1 = r1 < n_old ? (long long)pre[(size_t)(r1 >> 5)] : live;
            if (d1 == d0) continue;
            if (const int rc = gather(bounce.as<uint4>(), r0, r1, d0)) return rc;
            if (hipMemcpyAsync(h->owned.as<char>() + (size_t)d0 * row_bytes, bounce.p, (size_t)(d1 - d0) * row_bytes, hipMemcpyDeviceToDevice, 0) != hipSuccess)
                return fail(SQ_ERR_HIP, "sq_dense_compact: copy failed: %s", hipGetErrorString(hipGetLastError()));
        }
        if (hipDeviceSynchronize() != hipSuccess) return fail(SQ_ERR_HIP, "sq_dense_compact: gather failed: %s", hipGetErrorString(hipGetLastError()));
    }
    h->db = h->owned.as<float>();
    dense_set_rows(h, live);
    h->n_live = live;
    h->dead.release();
    h->dead_words = 0;
    // the index sq_dense_create would build from these rows: origin, statistics, scan copies, filter state
    h->reset_filter_state();
    return dense_build_all(h);
}

extern "C" int sq_dense_search(sq_handle_t hid, const float* queries, int nq, int k, void* out_dist, int64_t* out_idx,
                               int mem, void* stream) {
    g_hostprof.start();
    auto* h = static_cast<DenseHandle*>(lookup_handle(hid, H_DENSE));
    if (!h) return fail(SQ_ERR_INVALID, "sq_dense_search: unknown handle");
    if (!queries || !out_dist || !out_idx || nq <= 0 || k <= 0) return fail(SQ_ERR_INVALID, "sq_dense_search: bad argument");
    std::lock_guard<std::mutex> lock(h->mu);
    h->refresh_options();
    SQ_HIP(hipSetDevice(h->device));
    g_hostprof.lap(0);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t dsz = h->metric == SQ_METRIC_COSINE ? 8 : 4;
    if (mem == SQ_MEM_DEVICE_ASYNC && nq <= kDenseQueryChunk) {
        // Call i is enqueued before call i - 1 is waited for: the device always has the next call's kernels
        // queued behind the running ones, and the host reads a call's status words (and redoes what the filter
        // could not certify) one call later.  With "dense_async_streams" = 2 the two slots run on streams of
        // their own, ordered behind the caller's stream by an event, so the small kernels at the end of call
        // i - 1 (re-rank, select) and at the start of call i (query prep, sample pass, threshold) overlap.
        const auto resolve = [h](DenseSlot& sl) { return dense_resolve(h, sl); };
        SQ_TRY(h->ring.set_depth(h->opt.dense_async_depth, resolve));
        DenseSlot& s = h->ring.next();
        SQ_TRY(resolve(s));  // (the call `depth` back; normally resolved during an earlier call)
        g_hostprof.lap(1);
        hipStream_t run = st;
        if (h->opt.dense_async_streams == 2) {
            // One query tile per wave (HBM bound): the two slots alternate between two streams, so neighbouring
            // calls overlap.  Larger batches (MFMA bound, and kept cheap in HBM traffic by all workgroups of an XCD
            // walking the same rows) must not run two scans at once -- two scans at different rows evict each
            // other's rows from L2 (256 queries: 1.17 -> 1.68 ms per call): they share slot 0's stream.
            // (a batch that is ONE group of query tiles -- up to 64 queries at two tiles per wave, 128 at four -- still
            // reads the matrix once: it overlaps like a one-tile batch)
            const int tiles = (nq + TILE_ROWS - 1) / TILE_ROWS;
            const bool one_group = tiles <= scan_query_tiles(h->opt, h->d_pad, tiles);
            SQ_TRY((one_group ? s : h->ring.slot[0]).sync.stream(&run));
            // the caller's earlier work on `stream` (the queries) comes first -- unless the caller vouches for them ("dense_async_order"
            // = 0: an event on a busy or foreign stream costs ~10 us of start latency per call, a small shard's whole sample pass)
            if (h->opt.dense_async_order) SQ_TRY(s.sync.order_behind(st, run));
        }
        g_hostprof.lap(2);
        SQ_TRY(dense_enqueue(h, s, queries, nq, k, out_dist, reinterpret_cast<long long*>(out_idx), run, true));
        g_hostprof.lap(3);
        g_hostprof.ns[5]++;
        DenseSlot& oldest = h->ring.advance();
        // the oldest call still in flight (depth - 1 calls back): its results are final on return -- unless the caller
        // asked not to wait here ("dense_async_wait" = 0): that call is then finished at the start of the next call (its
        // slot is the next one to be reused), and whatever the host does between the two calls overlaps the device
        if (!h->opt.dense_async_wait) return SQ_OK;
        const int rc_wait = resolve(oldest);
        g_hostprof.lap(4);
        return rc_wait;
    }
    SQ_TRY(dense_sync_all(h));
    if (mem != SQ_MEM_HOST)
        return dense_search_chunked(h, queries, nq, k, out_dist, reinterpret_cast<long long*>(out_idx), st);
    return staged_call(h->stage, st, {{h->q_dev, queries, (size_t)nq * h->d * 4}},
                       {{out_dist, h->out_dist_dev, (size_t)nq * k * dsz}, {out_idx, h->out_idx_dev, (size_t)nq * k * 8}}, [&] {
                           return dense_search_chunked(h, h->q_dev.as<float>(), nq, k, h->out_dist_dev.p, h->out_idx_dev.as<long long>(), st);
                       });
}

extern "C" int sq_dense_sync(sq_handle_t hid) {
    return handle_sync(static_cast<DenseHandle*>(lookup_handle(hid, H_DENSE)), "sq_dense_sync", [](DenseHandle* h) {
        if (g_hostprof.on && g_hostprof.ns[5] > 0) {
            const double c = (double)g_hostprof.ns[5] * 1e3;
            fprintf(stderr, "[smqtk_hip] host us per async call over %lld calls: entry %.2f | resolve of the slot %.2f | stream setup %.2f | enqueue %.2f | wait %.2f\n",
                    g_hostprof.ns[5], g_hostprof.ns[0] / c, g_hostprof.ns[1] / c, g_hostprof.ns[2] / c, g_hostprof.ns[3] / c, g_hostprof.ns[4] / c);
            for (auto& v : g_hostprof.ns) v = 0;
        }
        return dense_sync_all(h);
    });
}

extern "C" int sq_dense_destroy(sq_handle_t hid) {
    return handle_destroy(static_cast<DenseHandle*>(remove_handle(hid, H_DENSE)), "sq_dense_destroy", dense_sync_all);
}

template <class T>
static int distances_launch(const void* rows, long long n, int d, const void* q, int metric, void* out, hipStream_t st) {
    return launch<dense_distances_kernel<T>>(dim3((unsigned)((n + 31) / 32)), dim3(256), 0, st, (const T*)rows, n, d, (const T*)q, metric, (T*)out,
                                             (double*)out);
}

extern "C" int sq_dense_distances(const void* query, const void* rows, int dtype, int64_t n, int d, int metric,
                                  void* out, int mem, void* stream) {
    if (!query || !rows || !out || n <= 0 || d <= 0) return fail(SQ_ERR_INVALID, "sq_dense_distances: bad argument");
    if (metric != SQ_METRIC_L2 && metric != SQ_METRIC_COSINE) return fail(SQ_ERR_INVALID, "sq_dense_distances: unknown metric");
    if (dtype != SQ_DTYPE_F32 && dtype != SQ_DTYPE_F64) return fail(SQ_ERR_INVALID, "sq_dense_distances: unknown dtype");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t esz = dtype == SQ_DTYPE_F32 ? 4 : 8;
    const size_t osz = (metric == SQ_METRIC_COSINE || dtype == SQ_DTYPE_F64) ? 8 : 4;
    if (mem == SQ_MEM_DEVICE) {
        return dtype == SQ_DTYPE_F32 ? distances_launch<float>(rows, n, d, query, metric, out, st)
                                     : distances_launch<double>(rows, n, d, query, metric, out, st);
    }
    DevBuf dq, dr, dout;
    SQ_TRY(dq.reserve((size_t)d * esz));
    SQ_TRY(dr.reserve((size_t)n * d * esz));
    SQ_TRY(dout.reserve((size_t)n * osz));
    if (hipMemcpyAsync(dq.p, query, (size_t)d * esz, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(dr.p, rows, (size_t)n * d * esz, hipMemcpyHostToDevice, st) != hipSuccess)
        return fail(SQ_ERR_HIP, "sq_dense_distances: H2D copy failed");
    SQ_TRY(dtype == SQ_DTYPE_F32 ? distances_launch<float>(dr.p, n, d, dq.p, metric, dout.p, st)
                                 : distances_launch<double>(dr.p, n, d, dq.p, metric, dout.p, st));
    if (hipMemcpyAsync(out, dout.p, (size_t)n * osz, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail(SQ_ERR_HIP, "sq_dense_distances: kernel or D2H copy failed: %s", hipGetErrorString(hipGetLastError()));
    return SQ_OK;
}
