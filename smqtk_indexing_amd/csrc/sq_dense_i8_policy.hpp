// The host's arithmetic around the int8 first-stage copy (sq_dense_i8.hpp): the candidate clamps, the choice among
// them from the measured counts, and when an index builds, extends or leaves its copy.  Plain C++, no runtime header:
// tests/host/i8_policy_main.cpp runs it on the CPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

namespace sq {

// the candidate clamps (multiples of the element rms) and bounds of the choice dense8_clip_stats_kernel counts for
static constexpr int I8_NCLIP = 12, I8_NCUT = 10;
struct Dense8ClipArgs {
    float inv_dx[I8_NCLIP], dx[I8_NCLIP];
    float cut[I8_NCLIP][I8_NCUT];   // r_row^2 thresholds
};
// (1.75 rms: where a uniform distribution ends; 9-11 rms: one-sided data -- max(N(0,1), 0) reaches 8.4 rms of its centred
// self; 14-18 rms: sparse rows -- with 10 % of the elements set their rms is a third of an element's own scale)
static constexpr double kClip[I8_NCLIP] = {1.75, 2.5, 3.25, 4.0, 4.75, 5.5, 6.5, 7.5, 9.0, 11.0, 14.0, 18.0};
static constexpr double kCut[I8_NCUT] = {0.6, 0.8, 1.0, 1.10, 1.15, 1.20, 1.30, 1.50, 2.0, 3.0};   // R in units of Dx sqrt(d / 12)

// the twelve steps and their ten squared bounds for an element rms (what dense8_clip_stats_kernel counts against)
inline Dense8ClipArgs i8_clip_candidates(double rms, int d) {
    Dense8ClipArgs ca{};
    const double round_unit = sqrt((double)d / 12.0);
    for (int c = 0; c < I8_NCLIP; ++c) {
        ca.dx[c] = (float)(kClip[c] * rms / 127.0);
        ca.inv_dx[c] = 1.0f / ca.dx[c];
        for (int m = 0; m < I8_NCUT; ++m) {
            const double r = kCut[m] * (double)ca.dx[c] * round_unit;
            ca.cut[c][m] = (float)(r * r);
        }
    }
    return ca;
}

// rows beyond R are candidates of every query: a few hundred at most (a query has a few thousand candidates anyway)
inline double i8_always_budget(long long n) { return std::max(256.0, 2e-5 * (double)n); }

// The clamp c and cut m with the least bound r among each clamp's first cut that leaves no more rows beyond it than the
// budget; `counts` are of every clip_step-th row (scaled here, saturating).  c < 0: every clamp leaves too many rows
// beyond every bound (heavy tails): the bf16 filter's relative bound suits such data.
struct I8Clamp {
    int c = -1, m = -1;
    double r = 0.0;
    bool found() const { return c >= 0; }
};
inline I8Clamp i8_choose_clamp(const uint32_t (&counts)[I8_NCLIP][I8_NCUT], const Dense8ClipArgs& ca, int d, long long n, int clip_step) {
    const double round_unit = sqrt((double)d / 12.0), budget = i8_always_budget(n);
    I8Clamp best;
    for (int c = 0; c < I8_NCLIP; ++c)
        for (int m = 0; m < I8_NCUT; ++m) {
            const uint32_t rows = (uint32_t)std::min<unsigned long long>(0xffffffffull, (unsigned long long)counts[c][m] * (unsigned)clip_step);
            if ((double)rows <= budget) {
                const double r = kCut[m] * (double)ca.dx[c] * round_unit;
                if (!best.found() || r < best.r) best.c = c, best.m = m, best.r = r;
                break;
            }
        }
    return best;
}

// What an index does about its copy when its row count has changed to n (create: in_use false, n8_built 0).  Nothing where
// option "dense_int8" is 0, no copy below 65 536 rows, and no wide one (rows beyond 512 dimensions) is started unless
// "dense_int8_wide" asks for it -- one that exists follows the appends whatever the option says by now.  The clamp was
// chosen from n8_built rows: an index twice that size chooses again from all its rows (build: what a handle without a
// copy would not start is then not built again either), and one without a copy (too small, or declined) tries when it
// has doubled since its last attempt.
enum class I8Action { nothing, build, extend };
inline I8Action i8_append_action(int int8_opt, bool wide, bool wide_wanted, bool in_use, long long n, long long n8_built) {
    if (int8_opt == 0) return I8Action::nothing;
    const bool again = n >= 65536 && n >= 2 * n8_built;
    if (in_use) return again ? I8Action::build : I8Action::extend;
    return again && (!wide || wide_wanted) ? I8Action::build : I8Action::nothing;
}

}  // namespace sq
