// ITQ hash-code generation (gfx950): rotation + sign + MSB-first packing.
//
// Replaces, for n descriptors at once, ItqFunctor.get_hash
// (smqtk_indexing/impls/lsh_functor/itq.py:389-408), its _norm_vector
// (itq.py:172-191) and bit_vector_to_int_large (utils/bits.py:4-20), i.e. the
// body of the hashing loop of LSHNearestNeighborIndex._build_index
// (impls/nn_index/lsh.py:316-321):
//     v = x / ||x||_2 (optional, in x's dtype, zero norm -> 1)
//     z = (v - mean) . R        float64 (mean, R are float64)
//     bit_j = z_j >= 0          (exact zero and -0.0 map to 1)
// The contraction runs on v_mfma_f64_16x16x4_f64 (A = 16 rows x 4 k of v,
// B = 4 k x 16 hash bits of R from LDS).  Sign bits leave the accumulators
// through wave ballots and are packed so that hash bit 0 is the most
// significant bit of the right-aligned uint64[W] code.
//
// This file is the host side: the plan of a call (itq_filter_route, itq_plan), the scratch layout, prep launch and
// error bounds the three certified filters share, one function per filter, and the C entry points.  The kernels are in
// sq_itq_exact.hpp (float64), sq_itq_fast.hpp (narrow), sq_itq_wide.hpp and sq_itq_xwide.hpp (slab).
#include <algorithm>

#include "sq_common.hpp"
#include "sq_itq_exact.hpp"
#include "sq_itq_fast.hpp"
#include "sq_itq_wide.hpp"
#include "sq_itq_xwide.hpp"

namespace sq {

// Stream-ordered scratch from a pool of the library's OWN (one per device).  The pool keeps up to kPoolKeepBytes
// across synchronisations, so small latency-bound calls (one query vector: ~100 KB) never pay for a fresh
// allocation, while the scratch of a bulk call (gigabytes for a 10 M-row hash from host memory) goes back to the
// driver at the next synchronisation instead of staying reserved for the life of the process.  (Round 1 raised the
// release threshold of the process-wide DEFAULT pool to "never": a global setting other users of that pool saw,
// and memory that hipMalloc-based buffers and torch's allocator could no longer get.)
static constexpr uint64_t kPoolKeepBytes = 256ull << 20;
static hipMemPool_t scratch_pool(int device) {
    static std::mutex mu;
    static hipMemPool_t pools[64] = {};
    static bool tried[64] = {};
    if (device < 0 || device >= 64) return nullptr;
    std::lock_guard<std::mutex> l(mu);
    if (!tried[device]) {
        tried[device] = true;
        hipMemPoolProps props{};
        props.allocType = hipMemAllocationTypePinned;
        props.handleTypes = hipMemHandleTypeNone;
        props.location.type = hipMemLocationTypeDevice;
        props.location.id = device;
        hipMemPool_t pool = nullptr;
        if (hipMemPoolCreate(&pool, &props) == hipSuccess) {
            uint64_t keep = kPoolKeepBytes;
            (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
            pools[device] = pool;
        } else {
            (void)hipGetLastError();
        }
    }
    return pools[device];
}
static hipError_t scratch_alloc(void** p, size_t bytes, hipStream_t st, int device) {
    hipMemPool_t pool = scratch_pool(device);
    if (pool) return hipMallocFromPoolAsync(p, bytes, pool, st);
    return hipMallocAsync(p, bytes, st);  // (no private pool: the default one, with its default threshold)
}

static size_t align256(size_t v) { return (v + 255) / 256 * 256; }

// A stream-ordered scratch block: given back to the pool, behind the work queued so far, when it leaves scope.
struct ItqScratch {
    unsigned char* p = nullptr;
    hipStream_t st = nullptr;
    int alloc(size_t bytes, hipStream_t s, int device) {
        st = s;
        SQ_HIP(scratch_alloc(reinterpret_cast<void**>(&p), bytes, s, device));
        return SQ_OK;
    }
    ~ItqScratch() { if (p) (void)hipFreeAsync(p, st); }
};

// What a resident model (sq_itq_model_*) hands to a launch: where the statistics of the call go, and a home for the
// extra-wide filter's image of R, which depends on the model alone (8 MB of float16 planes plus 16 MB of float64
// columns at 8192 x 256 bits, 32 MB + 64 MB at 8192 x 1024 bits: built once per model, not once per call).  The one-shot sq_itq_hash passes none.
struct ItqCallCtx {
    DevBuf* prep = nullptr;        // the model part of the extra-wide filter's scratch
    bool* prep_valid = nullptr;
    unsigned long long* cand_dev = nullptr;   // device counter: bits left to float64 (zeroed by the caller)
    long long filter_launches = 0;            // filter kernels that streamed the rows (the slab filter beyond 256 bits: one per column group)
    long long fallback_rows = 0;              // rows hashed by the float64 kernel
};

// ------------------------------------------------------------------ the plan: which kernel hashes a call
// Geometry of the filter for (d, words); stages == 0: the filter does not apply.
struct ItqFastGeom {
    int ku, ct, stages, waves;
    bool breg;
    size_t lds;
};
static ItqFastGeom itq_fast_geometry(int d, int words) {
    ItqFastGeom g{};
    if (d % 64 != 0 || d > 256 || words > 2) return g;
    g.ku = d / 64;
    g.ct = words * 2;
    // R's hi fragments in registers (lo planes in LDS), eight waves -- unless four column tiles of accumulators are
    // live as well (64-d -> 128 bits): that spilled, and a scratch reload in the loop drains the DMA ring
    g.breg = g.ku * g.ct <= 4 && g.ct <= 2;
    g.waves = g.breg ? ITQF_WAVES_BREG : ITQF_WAVES_LDSB;
    const int dp = (d + 127) / 128 * 128;
    // LDS copy of R: both bfloat16 planes, or only the lo planes when the hi fragments live in registers
    const size_t fixed = (size_t)g.ct * 32 * dp * (g.breg ? 2 : 4);
    for (int ns = g.breg ? 2 : 4; ns >= 2; --ns) {
        const size_t lds = fixed + (size_t)g.waves * ns * ITQF_UNIT_BYTES;
        if (lds <= 160 * 1024) {
            g.stages = ns;
            g.lds = lds;
            break;
        }
    }
    return g;
}

// Which certified filter hashes a shape: a pure function of (element size, d, words of the code).  The rule: a float32
// or float64 descriptor of up to 8192 elements whose row is a whole number of 16-byte pieces (float32: d % 4 == 0,
// float64: d % 2 == 0), codes up to 1024 bits, is hashed by a certified filter --
//   d % 64 == 0, d <= 256, float32, <= 128 bits   the narrow kernel (sq_itq_fast.hpp, whole 256-byte row units)
//   d % 64 == 0, d <= 512, <= 256 bits otherwise  the wide kernel   (sq_itq_wide.hpp, whole 256-byte row units)
//   every other d <= 8192 up to 256 bits, and
//   every d <= 8192 at 257 .. 1024 bits           the slab kernel   (sq_itq_xwide.hpp, 16-byte pieces guarded by k < d;
//                                                 beyond 256 bits one pass over the rows per 256 bits of the code)
// and everything else (codes beyond 1024 bits among it) by the float64 kernel.  What a call adds (itq_plan): at least 32 rows, a 16-byte aligned
// pointer, normalize None or 2, option itq_exact off -- otherwise the float64 kernel as well.
// (measured, profiles/itq_any_width.txt: the slab kernel at d = 100 / 300 / 500 against the float64 kernel and against
// the unit kernels on rows zero-padded to the next multiple of 64; profiles/itq_wide_codes.txt: 512 and 1024 bits)
enum ItqRoute { ITQ_ROUTE_F64 = 0, ITQ_ROUTE_NARROW, ITQ_ROUTE_WIDE, ITQ_ROUTE_XWIDE };
static ItqRoute itq_filter_route(size_t esz, int d, int words, ItqFastGeom* narrow = nullptr) {
    if (d < 1 || d > ITQX_MAX_D || words > ITQX_MAX_WORDS || ((size_t)d * esz) % 16 != 0) return ITQ_ROUTE_F64;
    if (d % 64 != 0 || d > 512 || words > 4) return ITQ_ROUTE_XWIDE;
    const ItqFastGeom g = itq_fast_geometry(d, words);
    if (esz != 4 || g.stages < 2) return ITQ_ROUTE_WIDE;
    if (narrow) *narrow = g;
    return ITQ_ROUTE_NARROW;
}

// Most rows a filter takes in one call: an undecided-bit entry keeps its row next to the column tile in one 32-bit word.
static constexpr long long ITQ_NARROW_MAX_ROWS = 1ll << 30;   // itq_fast_kernel: row | tile << 30 (4 column tiles)
static constexpr long long ITQ_WIDE_MAX_ROWS = 1ll << 29;     // itq_wide_kernel: row | tile << 29 (8 column tiles)
static constexpr long long ITQ_XWIDE_MAX_ROWS = 1ll << 29;    // itq_xwide_kernel: row | tile << 29 (8 tiles per column group)

// The route a call takes (ITQ_ROUTE_F64: the float64 kernel hashes every row), and the narrow kernel's geometry when
// that is the route.  The shape picks the filter (itq_filter_route); the call must be one a filter takes -- and fit
// that filter's entries.  A narrow shape the narrow kernel cannot take is the wide kernel's before it is the float64
// kernel's (today the wide limit is the lower one, so that step takes no call: the order is kept for the day it is not).
struct ItqPlan {
    ItqRoute route = ITQ_ROUTE_F64;
    ItqFastGeom narrow{};
};
static ItqPlan itq_plan(const ItqArgs& a, size_t esz) {
    ItqPlan p;
    if (a.n < 32 || (reinterpret_cast<uintptr_t>(a.x) & 15u) != 0 || a.exact || (a.norm != SQ_NORM_NONE && a.norm != SQ_NORM_L2))
        return p;   // (fewer rows than a tile, a misaligned pointer, the all-float64 option, the other norm orders)
    switch (itq_filter_route(esz, a.d, a.words, &p.narrow)) {
        case ITQ_ROUTE_NARROW:
            if (a.n < ITQ_NARROW_MAX_ROWS) {
                p.route = ITQ_ROUTE_NARROW;
                break;
            }
            [[fallthrough]];
        case ITQ_ROUTE_WIDE:
            if (a.n < ITQ_WIDE_MAX_ROWS) p.route = ITQ_ROUTE_WIDE;
            break;
        case ITQ_ROUTE_XWIDE:
            if (a.n < ITQ_XWIDE_MAX_ROWS) p.route = ITQ_ROUTE_XWIDE;
            break;
        case ITQ_ROUTE_F64:
            break;
    }
    return p;
}

// ------------------------------------------------------------------ what the three filters share
// Every filter's scratch has a model part -- what itq_fast_prep_kernel makes of (mean, R): the per-column coefficients,
// the float16 image, the column-major float64 copy of R -- and a call part: the undecided-bit segments, their counts
// and one extra region (the narrow kernel's dummy sink; the slab filter's temporary prep image).  Offsets, every
// region 256-byte aligned.  The model part lies inside the call's block (`model`) unless a model handle keeps it.
struct ItqLayout {
    size_t colnorm, cb, cberr, cabs, img, rt64, model_bytes;   // from the model part's base
    size_t seg, cnt, extra, model, call_bytes;                 // from the call block's base
    size_t img_bytes;
};
static size_t itq_take(size_t& off, size_t bytes) {
    const size_t at = off;
    off += align256(bytes);
    return at;
}
static ItqLayout itq_layout(int pc, int d, size_t img_bytes, size_t seg_bytes, size_t cnt_bytes, size_t extra_bytes, bool model_in_call) {
    ItqLayout l{};
    l.colnorm = itq_take(l.model_bytes, (size_t)pc * 4);
    l.cb = itq_take(l.model_bytes, (size_t)pc * 4);
    l.cberr = itq_take(l.model_bytes, (size_t)pc * 4);
    l.cabs = itq_take(l.model_bytes, (size_t)pc * 4);
    l.img = itq_take(l.model_bytes, img_bytes);
    l.rt64 = itq_take(l.model_bytes, (size_t)pc * d * 8);
    l.seg = itq_take(l.call_bytes, seg_bytes);
    l.cnt = itq_take(l.call_bytes, cnt_bytes);
    l.extra = itq_take(l.call_bytes, extra_bytes);
    l.model = itq_take(l.call_bytes, model_in_call ? l.model_bytes : 0);
    l.img_bytes = img_bytes;
    return l;
}

// (mean, R) -> the model part at `m`: one itq_fast_prep_kernel launch.  Its image goes to `img` (the model part's own,
// or the slab filter's temporary one), cleared first where the filter runs k beyond d under zero row fragments and
// must find finite numbers there.
static int itq_prep(const ItqArgs& a, double eps_rel, const ItqLayout& l, unsigned char* m, unsigned char* img, bool clear, hipStream_t st) {
    if (clear) SQ_HIP(hipMemsetAsync(img, 0, l.img_bytes, st));
    return launch<itq_fast_prep_kernel>(dim3((unsigned)(a.words * 64)), dim3(256), 0, st, a.mean, a.rot, a.d, a.bits, a.pad,
                                        reinterpret_cast<unsigned short*>(img), reinterpret_cast<float*>(m + l.colnorm),
                                        reinterpret_cast<float*>(m + l.cb), reinterpret_cast<float*>(m + l.cberr),
                                        reinterpret_cast<double*>(m + l.rt64), eps_rel, reinterpret_cast<float*>(m + l.cabs));
}

// eps_rel: the relative error of a filter's x . R_b per unit |x||R_b|, handed to the prep kernel (R's own residual is
// measured there and added to the column's coefficient).  The terms all three share:
static constexpr double ITQ_U20 = 9.5367431640625e-07;        // 2^-20: x as two round-toward-zero float16 planes; and again the
                                                              // float32 scale / subtract, the reference's float32 x/|x|
static constexpr double ITQ_U21 = 4.76837158203125e-07;       // 2^-21: the dropped x_lo R_lo
static constexpr double ITQ_U24 = 5.9604644775390625e-08;     // 2^-24: one float32 rounding of the accumulation
static constexpr double ITQ_U18 = 3.814697265625e-06;         // 2^-18: float32 |x|^2 (normalize=2)
static constexpr double ITQ_U10 = 9.765625e-04;               // 2^-10: |x_lo| / |x|
// narrow (sq_itq_fast.hpp): float32 accumulation of 3d products
static double itq_eps_narrow(int d, bool l2) {
    return ((ITQ_U20 + ITQ_U21) * 1.001 + 3.0 * d * ITQ_U24 + ITQ_U20 + (l2 ? ITQ_U18 : 0.0)) * 1.001;
}
// wide (sq_itq_wide.hpp): x_hi R_hi is summed per 256-k block (m = min(d, 256) products each, the blocks' bounds add up
// under Cauchy-Schwarz), the 2 d correction products are 2^-10 of that, three final additions
static double itq_eps_wide(int d, bool l2) {
    const int m = d < 256 ? d : 256;
    return ((ITQ_U20 + ITQ_U21) * 1.001 + 1.5 * (m + 8.0) * ITQ_U24 + 2.0 * d * ITQ_U24 * ITQ_U10 + ITQ_U20 + (l2 ? ITQ_U18 : 0.0)) * 1.001;
}
// slab (sq_itq_xwide.hpp): the accumulation is flushed per 64-k slab (192 products each, then ceil(d / 64) additions).
// Per column: the same for every column group.
static double itq_eps_xwide(int d, bool l2) {
    const int nslab = (d + ITQX_SLAB_K - 1) / ITQX_SLAB_K;
    return ((ITQ_U20 + ITQ_U21) * 1.001 + (1.5 * (3.0 * ITQX_SLAB_K + 8.0) + 1.5 * (nslab + 1.0)) * ITQ_U24 * (1.0 + 1.0 / 512.0) + ITQ_U20 +
            (l2 ? ITQ_U18 : 0.0)) * 1.001;
}

// The fields ItqFastArgs, ItqWideArgs and ItqXwideArgs share; `col0`: the first padded column of the launch (a column
// group of the slab filter).  The image and each filter's own fields stay with the caller.
template <class FilterArgs>
static FilterArgs itq_filter_args(const ItqArgs& a, const ItqLayout& l, unsigned char* m, unsigned char* call, int col0, long long seg_cap) {
    FilterArgs fa{};
    fa.x = static_cast<decltype(fa.x)>(a.x);
    fa.n = a.n;
    fa.d = a.d;
    fa.colnorm = reinterpret_cast<const float*>(m + l.colnorm) + col0;
    fa.cb32 = reinterpret_cast<const float*>(m + l.cb) + col0;
    fa.cberr = reinterpret_cast<const float*>(m + l.cberr) + col0;
    fa.cabs = reinterpret_cast<const float*>(m + l.cabs) + col0;
    fa.out = a.out;
    fa.words = a.words;
    fa.pad = a.pad;
    fa.bits = a.bits;
    fa.seg = reinterpret_cast<u64*>(call + l.seg);
    fa.seg_cnt = reinterpret_cast<u32*>(call + l.cnt);
    fa.seg_cap = seg_cap;
    fa.n_tiles = (a.n + 31) / 32;
    return fa;
}

// The grid of the wide and the slab filter: at most `nrb` workgroups of `waves` waves, no more waves than 32-row tiles;
// a wave's segment holds every (row, column tile) of its tiles.
struct ItqRowGrid {
    int ct, nrb;
    long long nwaves, seg_cap;
};
static ItqRowGrid itq_row_grid(int nrb, int waves, int ct, long long n_tiles) {
    if ((long long)nrb * waves > n_tiles) nrb = (int)((n_tiles + waves - 1) / waves);
    const long long nwaves = (long long)nrb * waves;
    return ItqRowGrid{ct, nrb, nwaves, ((n_tiles + nwaves - 1) / nwaves) * 32 * ct};
}

// After a filter launch and its fix-bits kernel: the filter pass and the bits it left to float64, for the statistics
// of a model handle.
static int itq_count_undecided(ItqCallCtx* ctx, const u64* seg, const u32* seg_cnt, long long seg_cap, long long nwaves, hipStream_t st) {
    if (!ctx) return SQ_OK;
    ctx->filter_launches += 1;
    if (!ctx->cand_dev) return SQ_OK;
    return launch<itq_count_undecided_kernel>(dim3((unsigned)nwaves), dim3(256), 0, st, seg, seg_cnt, seg_cap, ctx->cand_dev);
}

// ------------------------------------------------------------------ the narrow filter (sq_itq_fast.hpp)
template <int WAVES, int NSTAGE, int KU, int CT, bool NORMED, bool BREG>
static int itq_fast_launch_t(const ItqFastArgs& fa, size_t lds, hipStream_t st) {
    return launch_lds<itq_fast_kernel<WAVES, NSTAGE, KU, CT, NORMED, BREG>>(160 * 1024, dim3((unsigned)fa.nrb), dim3(WAVES * 64), lds,
                                                                            st, fa);
}

template <bool NORMED>
static int itq_fast_dispatch(const ItqFastArgs& fa, const ItqFastGeom& g, hipStream_t st) {
    if (g.breg) {
        switch (g.ku * 10 + g.ct) {
            case 12: return itq_fast_launch_t<8, 2, 1, 2, NORMED, true>(fa, g.lds, st);
            default: return itq_fast_launch_t<8, 2, 2, 2, NORMED, true>(fa, g.lds, st);  // 22
        }
    }
#define SQ_ITQF_CASE(KUv, CTv)                                                                                 \
    case KUv * 10 + CTv:                                                                                       \
        if (g.stages == 4) return itq_fast_launch_t<4, 4, KUv, CTv, NORMED, false>(fa, g.lds, st);             \
        if (g.stages == 3) return itq_fast_launch_t<4, 3, KUv, CTv, NORMED, false>(fa, g.lds, st);             \
        return itq_fast_launch_t<4, 2, KUv, CTv, NORMED, false>(fa, g.lds, st);
    switch (g.ku * 10 + g.ct) {
        SQ_ITQF_CASE(1, 4)
        SQ_ITQF_CASE(2, 4)
        SQ_ITQF_CASE(3, 2)
        SQ_ITQF_CASE(3, 4)
        SQ_ITQF_CASE(4, 2)
        SQ_ITQF_CASE(4, 4)
        default: return fail(SQ_ERR_UNSUPPORTED, "itq filter: no kernel for d=%d words=%d", g.ku * 64, g.ct / 2);
    }
#undef SQ_ITQF_CASE
}

// float32 rows through the filter; the bits it cannot decide through itq_fix_bits_kernel.
static int itq_fast_path(const ItqArgs& a, const ItqFastGeom& g, hipStream_t st, int device, ItqCallCtx* ctx) {
    const int pc = a.words * 64, dp = (a.d + 127) / 128 * 128;
    const bool l2 = a.norm == SQ_NORM_L2;
    const int nrb = cu_count(device);
    const long long n_tiles = (a.n + 31) / 32, nwaves = (long long)nrb * g.waves;
    const long long seg_cap = ((n_tiles + nwaves - 1) / nwaves) * 32 * g.ct;  // every (row, column tile) of a wave's tiles
    const ItqLayout l = itq_layout(pc, a.d, (size_t)pc * dp * 4, (size_t)nwaves * seg_cap * 8, (size_t)nwaves * 4, (size_t)nwaves * 8, true);
    ItqScratch s;
    SQ_TRY(s.alloc(l.call_bytes, st, device));
    unsigned char* m = s.p + l.model;
    SQ_TRY(itq_prep(a, itq_eps_narrow(a.d, l2), l, m, m + l.img, false, st));
    ItqFastArgs fa = itq_filter_args<ItqFastArgs>(a, l, m, s.p, 0, seg_cap);
    fa.rimage = reinterpret_cast<const uint4*>(m + l.img);
    fa.seg_dummy = reinterpret_cast<u64*>(s.p + l.extra);
    fa.nrb = nrb;
    fa.nstage = g.stages;
    SQ_TRY(l2 ? itq_fast_dispatch<true>(fa, g, st) : itq_fast_dispatch<false>(fa, g, st));
    // the undecided bits, one float64 dot product each, straight from the per-wave segments
    SQ_TRY(launch<itq_fix_bits_kernel>(dim3((unsigned)nwaves, ITQ_FIX_PARTS), dim3(256), 0, st, a, fa.seg, fa.seg_cnt, seg_cap,
                                       reinterpret_cast<const double*>(m + l.rt64)));
    return itq_count_undecided(ctx, fa.seg, fa.seg_cnt, seg_cap, nwaves, st);
}

// ------------------------------------------------------------------ the wide filter (sq_itq_wide.hpp)
// Measurement (option dense_debug bit 16): phase stamps of every workgroup of the wide kernel, cleared before the
// launch, read back (a blocking copy) and printed after it.
static int itq_stamps_reserve(int debug, int nrb, hipStream_t st, u64** stamps) {
    static DevBuf& buf = *new DevBuf;   // never destroyed: a static's destructor would call hipFree after the runtime has gone
    *stamps = nullptr;
    if (!(debug & 16)) return SQ_OK;
    SQ_TRY(buf.reserve((size_t)nrb * 64 * 8));
    SQ_HIP(hipMemsetAsync(buf.p, 0, (size_t)nrb * 64 * 8, st));
    *stamps = buf.as<u64>();
    return SQ_OK;
}
static int itq_stamps_print(const u64* stamps, int nrb) {
    if (!stamps) return SQ_OK;
    std::vector<unsigned long long> hst((size_t)nrb * 64);
    SQ_HIP(hipMemcpy(hst.data(), stamps, hst.size() * 8, hipMemcpyDeviceToHost));
    unsigned long long t0 = ~0ull;
    for (int b = 0; b < nrb; ++b) if (hst[(size_t)b * 64] && hst[(size_t)b * 64] < t0) t0 = hst[(size_t)b * 64];
    for (int b : {0, 1, 7, 100, 255}) {
        if (b >= nrb) continue;
        fprintf(stderr, "wg %3d:", b);
        for (int r = 0; r < 8; ++r)
            fprintf(stderr, " [r%d x %.1f mfma %.1f | start %.1f]", r, (hst[(size_t)b * 64 + 3 * r + 1] - hst[(size_t)b * 64 + 3 * r]) / 100.0,
                    (hst[(size_t)b * 64 + 3 * r + 2] - hst[(size_t)b * 64 + 3 * r + 1]) / 100.0, (hst[(size_t)b * 64 + 3 * r] - t0) / 100.0);
        fprintf(stderr, "\n");
    }
    return SQ_OK;
}

// float32 rows beyond the narrow kernel's shapes, float64 rows of every shape the wide kernel takes.
template <class T>
static int itq_wide_path(const ItqArgs& a, hipStream_t st, int device, ItqCallCtx* ctx) {
    const int pc = a.words * 64, ct = a.words * 2, dp = (a.d + 127) / 128 * 128;
    const bool l2 = a.norm == SQ_NORM_L2;
    const ItqRowGrid g = itq_row_grid(cu_count(device), ITQW_WAVES, ct, (a.n + 31) / 32);
    // (+ 1024 of slack on the image: the last k-block of a 384-wide plane is DMA'd whole)
    const ItqLayout l = itq_layout(pc, a.d, (size_t)pc * dp * 4 + 1024, (size_t)g.nwaves * g.seg_cap * 8, (size_t)g.nwaves * 4, 0, true);
    ItqScratch s;
    SQ_TRY(s.alloc(l.call_bytes, st, device));
    unsigned char* m = s.p + l.model;
    // (cleared: k beyond d inside a 256-k block runs with zero row fragments)
    SQ_TRY(itq_prep(a, itq_eps_wide(a.d, l2), l, m, m + l.img, true, st));
    ItqWideArgs wa = itq_filter_args<ItqWideArgs>(a, l, m, s.p, 0, g.seg_cap);
    wa.rimage = reinterpret_cast<const uint4*>(m + l.img);
    wa.ct = ct;
    wa.nrb = g.nrb;
    wa.debug = a.debug & 15;   // (measurement: the ablation bits of sq_itq_wide.hpp ride on option dense_debug)
    SQ_TRY(itq_stamps_reserve(a.debug, g.nrb, st, &wa.stamps));
    const size_t lds = 2 * (size_t)ITQW_CHUNK_BYTES + 4 * 256 * 4 + (size_t)ITQW_WAVES * ITQW_NSTAGE * ITQF_UNIT_BYTES + ITQW_WAVES * 2048;
    const dim3 grid((unsigned)g.nrb), block(ITQW_WAVES * 64);
    if (a.d <= 256)
        SQ_TRY(l2 ? launch_lds<itq_wide_kernel<T, true, 1>>(160 * 1024, grid, block, lds, st, wa)
                  : launch_lds<itq_wide_kernel<T, false, 1>>(160 * 1024, grid, block, lds, st, wa));
    else
        SQ_TRY(l2 ? launch_lds<itq_wide_kernel<T, true, 2>>(160 * 1024, grid, block, lds, st, wa)
                  : launch_lds<itq_wide_kernel<T, false, 2>>(160 * 1024, grid, block, lds, st, wa));
    SQ_TRY(itq_stamps_print(wa.stamps, g.nrb));
    SQ_TRY(launch<itq_fix_bits_wide_kernel<T>>(dim3((unsigned)g.nwaves, ITQ_FIX_PARTS), dim3(256), 0, st, a, wa.seg, wa.seg_cnt, g.seg_cap,
                                               reinterpret_cast<const double*>(m + l.rt64)));
    return itq_count_undecided(ctx, wa.seg, wa.seg_cnt, g.seg_cap, g.nwaves, st);
}

// ------------------------------------------------------------------ the extra-wide ("slab") filter (sq_itq_xwide.hpp)
template <class T, bool NORMED, int CT>
static int itq_xwide_launch_t(const ItqXwideArgs& xa, int nrb, hipStream_t st) {
    constexpr size_t lds = 2 * (size_t)CT * 8192 + 3 * (size_t)CT * 32 * 4;
    return launch_lds<itq_xwide_kernel<T, NORMED, CT>>(160 * 1024, dim3((unsigned)nrb), dim3(ITQX_WAVES * 64), lds, st, xa);
}

// Codes of 257 .. 1024 bits run in column groups of at most ITQX_GROUP_CT column tiles (256 bits, 4 code words): one
// filter pass over the rows per group (sq_itq_xwide.hpp, "Codes beyond 256 bits").  The passes are launched one
// after the other on the call's stream, each followed by the float64 evaluation of its own undecided bits, so ONE
// segment array serves every group: the stream orders pass g + 1 behind the fix kernel of pass g.
//
// d <= 8192, float32 or float64 rows of whole 16-byte pieces.  The model part -- with the slab image, group after
// group, as its image -- is built once per model handle (ItqCallCtx::prep) or once per one-shot call.
template <class T>
static int itq_xwide_path(const ItqArgs& a, hipStream_t st, int device, ItqCallCtx* ctx) {
    const int pc = a.words * 64, ct = a.words * 2, dp = (a.d + 127) / 128 * 128;
    const int groups = (ct + ITQX_GROUP_CT - 1) / ITQX_GROUP_CT;
    const bool l2 = a.norm == SQ_NORM_L2;
    // the segment array and its counts hold the largest group's (a last group of two column tiles runs twice the waves:
    // two workgroups per CU fit 256 registers only with two column tiles)
    ItqRowGrid grid[ITQX_MAX_WORDS * 2 / ITQX_GROUP_CT];
    size_t seg_bytes = 0, cnt_bytes = 0;
    for (int g = 0; g < groups; ++g) {
        const int ctg = std::min(ITQX_GROUP_CT, ct - g * ITQX_GROUP_CT);
        grid[g] = itq_row_grid(cu_count(device) * (ctg <= 2 ? 2 : 1), ITQX_WAVES, ctg, (a.n + 31) / 32);
        seg_bytes = std::max(seg_bytes, (size_t)(grid[g].nwaves * grid[g].seg_cap * 8));
        cnt_bytes = std::max(cnt_bytes, (size_t)grid[g].nwaves * 4);
    }
    const size_t img_bytes = (size_t)pc * dp * 4;
    const size_t group_img_bytes = (size_t)ITQX_GROUP_CT * 32 * dp * 4;   // a full group's slice of either image
    const bool keep = ctx && ctx->prep, cached = keep && *ctx->prep_valid;
    // (the extra region: prep's own image, while the model part is built)
    const ItqLayout l = itq_layout(pc, a.d, img_bytes, seg_bytes, cnt_bytes, cached ? 0 : img_bytes, !keep);
    if (keep) SQ_TRY(ctx->prep->reserve(l.model_bytes));   // (SQ_ERR_NOMEM: nothing is kept, the model stays usable)
    ItqScratch s;
    SQ_TRY(s.alloc(l.call_bytes, st, device));
    unsigned char* m = keep ? ctx->prep->as<unsigned char>() : s.p + l.model;
    if (!cached) {
        // (cleared: k beyond d meets finite zeros under zero row fragments)
        SQ_TRY(itq_prep(a, itq_eps_xwide(a.d, l2), l, m, s.p + l.extra, true, st));
        // prep's image is [column][plane][dp]: a group's columns are one contiguous slice of it, and of the slab image
        // (a group starts at a multiple of 256 columns, so prep's swizzle by column & 15 reads the same inside the slice)
        for (int g = 0; g < groups; ++g) {
            const long long chunks = (long long)grid[g].ct * 32 * dp * 4 / 16;
            SQ_TRY(launch<itq_xwide_relayout_kernel>(dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, st,
                                                     reinterpret_cast<const uint4*>(s.p + l.extra + (size_t)g * group_img_bytes),
                                                     reinterpret_cast<uint4*>(m + l.img + (size_t)g * group_img_bytes), dp, grid[g].ct, chunks));
        }
        if (keep) *ctx->prep_valid = true;
    }
    for (int g = 0; g < groups; ++g) {
        const int col0 = g * ITQX_GROUP_CT * 32;   // first padded column of the group
        const ItqRowGrid& gg = grid[g];
        ItqXwideArgs xa = itq_filter_args<ItqXwideArgs>(a, l, m, s.p, col0, gg.seg_cap);
        xa.ximage = reinterpret_cast<const uint4*>(m + l.img + (size_t)g * group_img_bytes);
        xa.word0 = col0 / 64;
        xa.pad = g == 0 ? a.pad : 0;   // (pad < 64: the leading zero columns lie in the first word, hence in group 0)
        xa.nslab = (a.d + ITQX_SLAB_K - 1) / ITQX_SLAB_K;
#define SQ_ITQX_CASE(CTv) \
    case CTv: SQ_TRY(l2 ? itq_xwide_launch_t<T, true, CTv>(xa, gg.nrb, st) : itq_xwide_launch_t<T, false, CTv>(xa, gg.nrb, st)); break;
        switch (gg.ct) {
            SQ_ITQX_CASE(2)
            SQ_ITQX_CASE(4)
            SQ_ITQX_CASE(6)
            default:
            SQ_ITQX_CASE(8)
        }
#undef SQ_ITQX_CASE
        SQ_TRY(launch<itq_fix_bits_xwide_kernel<T>>(dim3((unsigned)gg.nwaves, ITQ_FIX_PARTS), dim3(256), 0, st, a, xa.seg, xa.seg_cnt,
                                                    gg.seg_cap, reinterpret_cast<const double*>(m + l.rt64), col0));
        SQ_TRY(itq_count_undecided(ctx, xa.seg, xa.seg_cnt, gg.seg_cap, gg.nwaves, st));
    }
    return SQ_OK;
}

// ------------------------------------------------------------------ a call
template <class T>
static int itq_launch(const ItqArgs& a0, hipStream_t st, int device, ItqCallCtx* ctx) {
    const ItqPlan plan = itq_plan(a0, sizeof(T));
    switch (plan.route) {
        case ITQ_ROUTE_NARROW: return itq_fast_path(a0, plan.narrow, st, device, ctx);
        case ITQ_ROUTE_WIDE: return itq_wide_path<T>(a0, st, device, ctx);
        case ITQ_ROUTE_XWIDE: return itq_xwide_path<T>(a0, st, device, ctx);
        case ITQ_ROUTE_F64: break;
    }
    // the float64 kernel on every row
    ItqArgs a = a0;
    if (ctx) ctx->fallback_rows += a.n;
    ItqScratch nrm;
    if (a.norm != SQ_NORM_NONE) {  // stream-ordered scratch: [n] norms in x's dtype
        SQ_TRY(nrm.alloc((size_t)a.n * sizeof(T), st, device));
        long long gx = std::min<long long>((a.n + 31) / 32, 16ll * cu_count(device));
        SQ_TRY(launch<itq_norms_kernel<T>>(dim3((unsigned)gx), dim3(256), 0, st, reinterpret_cast<const T*>(a.x), a.n, a.d,
                                           reinterpret_cast<T*>(nrm.p), (const u32*)nullptr, (const u32*)nullptr, a.norm));
        a.nrm = nrm.p;
    }
    return a.words == 1 ? itq_launch_t<T, 4>(a, st, device) : a.words == 2 ? itq_launch_t<T, 8>(a, st, device) : itq_launch_t<T, 16>(a, st, device);
}
static int itq_launch_dtype(int x_dtype, const ItqArgs& a, hipStream_t st, int device, ItqCallCtx* ctx = nullptr) {
    return x_dtype == SQ_DTYPE_F32 ? itq_launch<float>(a, st, device, ctx) : itq_launch<double>(a, st, device, ctx);
}

// The fields of ItqArgs a call's shape and options fix; the caller adds its pointers (x, mean, rot, out).
static ItqArgs itq_make_args(long long n, int d, int bits, int norm, int x_dtype, int mean_dtype, int exact, int debug) {
    ItqArgs a{};
    a.n = n;
    a.d = d;
    a.bits = bits;
    a.words = (bits + 63) / 64;
    a.pad = a.words * 64 - bits;
    a.norm = norm;
    a.sub32 = (x_dtype == SQ_DTYPE_F32 && mean_dtype == SQ_DTYPE_F32) ? 1 : 0;
    a.exact = exact;
    a.debug = debug;
    a.d16 = (d + 15) / 16 * 16;
    return a;
}

static bool itq_norm_supported(int ord) {
    return ord == SQ_NORM_NONE || ord == SQ_NORM_L2 || ord == SQ_NORM_L1 || ord == SQ_NORM_L0 || ord == SQ_NORM_INF ||
           ord == SQ_NORM_NEG_INF;
}

// ------------------------------------------------------------------ resident model
// ItqFunctor's model (mean, rotation) kept on the device, with pinned staging for small batches: hashing ONE query
// vector -- the first thing every LSHNearestNeighborIndex.nn does (lsh.py:473) -- otherwise uploads the 64 KB
// rotation and the mean from pageable memory on every call (95 us per query, most of it copies).
struct ItqModelHandle : HandleBase {
    DevBuf mean, rot, x_dev, out_dev;
    DevBuf xprep;            // the extra-wide filter's image of the model (sq_itq_xwide.hpp), built by the first call that needs it
    bool xprep_valid = false;
    DevBuf cand;             // one device counter: bits the last call's filter left to float64
    HostPinned stage;   // [rows | codes] of one small batch
    HostPinned cand_host;
    int d = 0, bits = 0, norm = SQ_NORM_NONE, mean_dtype = SQ_DTYPE_F64;
};

}  // namespace sq

using namespace sq;

extern "C" int sq_itq_hash(const void* x, int x_dtype, int64_t n, int d, const double* mean, int mean_dtype,
                           const double* rotation, int bits, int norm_ord, uint64_t* out_codes, int mem, void* stream) {
    if (!x || !mean || !rotation || !out_codes || n <= 0 || d <= 0 || bits <= 0)
        return fail(SQ_ERR_INVALID, "sq_itq_hash: bad argument");
    if (x_dtype != SQ_DTYPE_F32 && x_dtype != SQ_DTYPE_F64) return fail(SQ_ERR_INVALID, "sq_itq_hash: unknown dtype %d", x_dtype);
    if (mean_dtype != SQ_DTYPE_F32 && mean_dtype != SQ_DTYPE_F64)
        return fail(SQ_ERR_INVALID, "sq_itq_hash: unknown mean dtype %d", mean_dtype);
    if (!itq_norm_supported(norm_ord))
        return fail(SQ_ERR_UNSUPPORTED, "sq_itq_hash: normalize code %d not supported on the device", norm_ord);
    int device = 0;
    SQ_HIP(hipGetDevice(&device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int words = (bits + 63) / 64;
    const size_t esz = x_dtype == SQ_DTYPE_F32 ? 4 : 8;
    ItqArgs a = itq_make_args(n, d, bits, norm_ord, x_dtype, mean_dtype, g_opt.itq_exact, g_opt.dense_debug);
    if (mem == SQ_MEM_DEVICE) {
        a.x = x;
        a.mean = mean;
        a.rot = rotation;
        a.out = reinterpret_cast<u64*>(out_codes);
        return itq_launch_dtype(x_dtype, a, st, device);
    }
    // Host buffers: ONE stream-ordered allocation for rows | mean | rotation | codes (the library's pool keeps up to
    // 256 MB across calls).  Four hipMalloc / hipFree pairs per call made hashing one query vector -- what every
    // LSHNearestNeighborIndex.nn does first -- cost 94 us.
    const size_t o_x = 0, o_m = align256(o_x + (size_t)n * d * esz), o_r = align256(o_m + (size_t)d * 8);
    const size_t o_out = align256(o_r + (size_t)d * bits * 8), total = o_out + (size_t)n * words * 8;
    ItqScratch s;
    SQ_TRY(s.alloc(total, st, device));
    unsigned char* base = s.p;
    if (hipMemcpyAsync(base + o_x, x, (size_t)n * d * esz, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(base + o_m, mean, (size_t)d * 8, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(base + o_r, rotation, (size_t)d * bits * 8, hipMemcpyHostToDevice, st) != hipSuccess)
        return fail(SQ_ERR_HIP, "sq_itq_hash: H2D copy failed");
    a.x = base + o_x;
    a.mean = reinterpret_cast<const double*>(base + o_m);
    a.rot = reinterpret_cast<const double*>(base + o_r);
    a.out = reinterpret_cast<u64*>(base + o_out);
    SQ_TRY(itq_launch_dtype(x_dtype, a, st, device));
    if (hipMemcpyAsync(out_codes, base + o_out, (size_t)n * words * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
        stream_wait(st) != hipSuccess)
        return fail(SQ_ERR_HIP, "sq_itq_hash: kernel or D2H copy failed: %s", hipGetErrorString(hipGetLastError()));
    return SQ_OK;
}

extern "C" int sq_itq_model_create(const double* mean, int mean_dtype, const double* rotation, int d, int bits,
                                   int norm_ord, sq_handle_t* out) {
    if (!mean || !rotation || !out || d <= 0 || bits <= 0) return fail(SQ_ERR_INVALID, "sq_itq_model_create: bad argument");
    if (mean_dtype != SQ_DTYPE_F32 && mean_dtype != SQ_DTYPE_F64)
        return fail(SQ_ERR_INVALID, "sq_itq_model_create: unknown mean dtype %d", mean_dtype);
    if (!itq_norm_supported(norm_ord))
        return fail(SQ_ERR_UNSUPPORTED, "sq_itq_model_create: normalize code %d not supported on the device", norm_ord);
    auto h = std::make_unique<ItqModelHandle>();
    h->kind = H_ITQ;
    h->d = d;
    h->bits = bits;
    h->norm = norm_ord;
    h->mean_dtype = mean_dtype;
    if (hipGetDevice(&h->device) != hipSuccess) return fail(SQ_ERR_HIP, "sq_itq_model_create: no HIP device");
    SQ_TRY(h->mean.reserve((size_t)d * 8));
    SQ_TRY(h->rot.reserve((size_t)d * bits * 8));
    SQ_TRY(h->cand.reserve(8));
    SQ_TRY(h->cand_host.reserve(8));
    if (hipMemcpy(h->mean.p, mean, (size_t)d * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->rot.p, rotation, (size_t)d * bits * 8, hipMemcpyHostToDevice) != hipSuccess)
        return fail(SQ_ERR_HIP, "sq_itq_model_create: H2D copy failed");
    *out = register_handle(h.release());
    return SQ_OK;
}

extern "C" int sq_itq_model_hash(sq_handle_t hid, const void* x, int x_dtype, int64_t n, uint64_t* out_codes, int mem,
                                 void* stream) {
    auto* h = static_cast<ItqModelHandle*>(lookup_handle(hid, H_ITQ));
    if (!h) return fail(SQ_ERR_INVALID, "sq_itq_model_hash: unknown handle");
    if (!x || !out_codes || n <= 0) return fail(SQ_ERR_INVALID, "sq_itq_model_hash: bad argument");
    if (x_dtype != SQ_DTYPE_F32 && x_dtype != SQ_DTYPE_F64) return fail(SQ_ERR_INVALID, "sq_itq_model_hash: unknown dtype %d", x_dtype);
    std::lock_guard<std::mutex> lock(h->mu);
    h->refresh_options();   // (a per-handle "itq_exact" / "dense_debug" wins over the process-wide value)
    SQ_HIP(hipSetDevice(h->device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int words = (h->bits + 63) / 64;
    const size_t esz = x_dtype == SQ_DTYPE_F32 ? 4 : 8;
    ItqArgs a = itq_make_args(n, h->d, h->bits, h->norm, x_dtype, h->mean_dtype, h->opt.itq_exact, h->opt.dense_debug);
    a.mean = h->mean.as<double>();
    a.rot = h->rot.as<double>();
    // statistics of this call (sq_get_stats on the model handle, smqtk_hip.h)
    ItqCallCtx ctx;
    ctx.prep = &h->xprep;
    ctx.prep_valid = &h->xprep_valid;
    ctx.cand_dev = h->cand.as<unsigned long long>();
    if (n >= 32) SQ_HIP(hipMemsetAsync(h->cand.p, 0, 8, st));   // (no filter takes fewer rows: one query vector pays nothing)
    auto record = [&](long long candidates) {
        h->stats = sq_stats_t{};
        h->stats.scan_launches = ctx.filter_launches;
        h->stats.fallback_queries = ctx.fallback_rows;
        h->stats.candidates = candidates;
        // (the rows are streamed once per filter pass: the slab filter's column groups beyond 256 bits)
        h->stats.bytes_scanned = (int64_t)((size_t)n * h->d * esz * (size_t)std::max<long long>(1, ctx.filter_launches));
    };
    if (mem == SQ_MEM_DEVICE) {
        a.x = x;
        a.out = reinterpret_cast<u64*>(out_codes);
        const int rc = itq_launch_dtype(x_dtype, a, st, h->device, &ctx);
        if (rc == SQ_OK) record(-1);   // (the call is asynchronous: the device counter is not read back)
        return rc;
    }
    const size_t xb = (size_t)n * h->d * esz, ob = (size_t)n * words * 8;
    SQ_TRY(h->x_dev.reserve(xb));
    SQ_TRY(h->out_dev.reserve(ob));
    // small batches go through pinned staging (an asynchronous copy from pageable memory is a blocking staged copy)
    const bool staged = xb + ob <= (1u << 20);
    const void* src = x;
    void* dst = out_codes;
    if (staged) {
        SQ_TRY(h->stage.reserve(xb + ob));
        memcpy(h->stage.p, x, xb);
        src = h->stage.p;
        dst = static_cast<char*>(h->stage.p) + xb;
    }
    SQ_HIP(hipMemcpyAsync(h->x_dev.p, src, xb, hipMemcpyHostToDevice, st));
    a.x = h->x_dev.p;
    a.out = h->out_dev.as<u64>();
    SQ_TRY(itq_launch_dtype(x_dtype, a, st, h->device, &ctx));
    SQ_HIP(hipMemcpyAsync(dst, h->out_dev.p, ob, hipMemcpyDeviceToHost, st));
    if (ctx.filter_launches) SQ_HIP(hipMemcpyAsync(h->cand_host.p, h->cand.p, 8, hipMemcpyDeviceToHost, st));
    SQ_HIP(stream_wait(st));
    if (staged) memcpy(out_codes, dst, ob);
    record(ctx.filter_launches ? (long long)*static_cast<unsigned long long*>(h->cand_host.p) : 0);
    return SQ_OK;
}

extern "C" int sq_itq_model_destroy(sq_handle_t hid) {
    auto* h = remove_handle(hid, H_ITQ);
    if (!h) return fail(SQ_ERR_INVALID, "sq_itq_model_destroy: unknown handle");
    (void)hipSetDevice(h->device);
    delete h;
    return SQ_OK;
}
