// The host arithmetic of the int8 first-stage copy (smqtk_indexing_amd/csrc/sq_dense_i8_policy.hpp) on a CPU: compiled
// with -fsanitize=address,undefined and run by tests/test_host_logic_int8_policy.py, which also recomputes the printed
// clamp candidates from their formulas.
#include "../../smqtk_indexing_amd/csrc/sq_dense_i8_policy.hpp"

#include <cstdio>
#include <cstdlib>

using namespace sq;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

static const uint32_t OVER = 1000000u;   // beyond every budget used below but the saturation case's
typedef uint32_t Counts[I8_NCLIP][I8_NCUT];
static void fill(Counts& t, uint32_t v) {
    for (auto& row : t)
        for (uint32_t& x : row) x = v;
}

static void choice() {
    const int d = 128;
    const long long n = 100000;   // budget: the floor of 256
    const Dense8ClipArgs ca = i8_clip_candidates(1.0, d);
    const double unit = sqrt((double)d / 12.0);
    Counts t;
    // every count over the budget: none
    fill(t, OVER);
    CHECK(!i8_choose_clamp(t, ca, d, n, 1).found());
    // within one clamp the first cut inside the budget wins, not the tightest count and not the last
    t[3][4] = 256, t[3][7] = 0;
    I8Clamp b = i8_choose_clamp(t, ca, d, n, 1);
    CHECK(b.found() && b.c == 3 && b.m == 4);
    CHECK(b.r == kCut[4] * (double)ca.dx[3] * unit);
    // across clamps the smallest r wins: a later clamp with a smaller bound (0.6 x 5.5 rms against 1.15 x 4 rms) ...
    t[5][0] = 10;
    b = i8_choose_clamp(t, ca, d, n, 1);
    CHECK(b.c == 5 && b.m == 0 && b.r == kCut[0] * (double)ca.dx[5] * unit);
    // ... and not a later clamp with a larger one (3.0 x 18 rms)
    t[5][0] = OVER, t[11][9] = 0;
    b = i8_choose_clamp(t, ca, d, n, 1);
    CHECK(b.c == 3 && b.m == 4);
    // an earlier clamp with a smaller bound (0.6 x 1.75 rms) takes over
    t[0][0] = 1;
    b = i8_choose_clamp(t, ca, d, n, 1);
    CHECK(b.c == 0 && b.m == 0 && b.r == kCut[0] * (double)ca.dx[0] * unit);
}

static void budget() {
    const long long n0 = 12800000;   // 2e-5 n crosses the floor of 256 here
    CHECK(i8_always_budget(1) == 256.0 && i8_always_budget(65536) == 256.0);
    CHECK(i8_always_budget(n0 - 1) == 256.0);
    CHECK(i8_always_budget(n0) >= 256.0 && i8_always_budget(n0) < 256.00001);
    CHECK(i8_always_budget(n0 + 1) == 2e-5 * (double)(n0 + 1) && i8_always_budget(n0 + 1) > 256.0 && i8_always_budget(n0 + 1) < 256.0001);
    CHECK(i8_always_budget(100000000) == 2e-5 * 1e8);
    // ... and the choice compares against it: 256 rows pass below the crossing, 257 do not just above it, 2000 do at 100 M
    const Dense8ClipArgs ca = i8_clip_candidates(1.0, 64);
    Counts t;
    fill(t, OVER);
    t[2][1] = 256;
    CHECK(i8_choose_clamp(t, ca, 64, n0 - 1, 1).found());
    t[2][1] = 257;
    CHECK(!i8_choose_clamp(t, ca, 64, n0 - 1, 1).found() && !i8_choose_clamp(t, ca, 64, n0 + 1, 1).found());
    t[2][1] = 2000;
    CHECK(i8_choose_clamp(t, ca, 64, 100000000, 1).found() && !i8_choose_clamp(t, ca, 64, 99999999, 1).found());
}

static void clip_step() {
    const int d = 128;
    const Dense8ClipArgs ca = i8_clip_candidates(2.5, d);
    Counts t;
    fill(t, 0xffffffffu);
    // counts of every 8th row stand for eight times as many
    t[4][2] = 32;
    CHECK(i8_choose_clamp(t, ca, d, 100000, 8).found() && i8_choose_clamp(t, ca, d, 100000, 1).found());
    t[4][2] = 33;
    CHECK(!i8_choose_clamp(t, ca, d, 100000, 8).found() && i8_choose_clamp(t, ca, d, 100000, 1).found());
    // 2^32 + 8 saturates at 2^32 - 1: it neither wraps to 8 (which any budget admits) ...
    t[4][2] = 0x20000001u;
    CHECK(!i8_choose_clamp(t, ca, d, 100000, 8).found());
    // ... nor stays 2^32 + 8 (which this budget, 2^32 - 0.4, would refuse)
    const long long huge = 214748364780000ll;
    CHECK(i8_always_budget(huge) > 4294967295.0 && i8_always_budget(huge) < 4294967296.0);
    const I8Clamp b = i8_choose_clamp(t, ca, d, huge, 8);
    CHECK(b.found() && b.c == 0 && b.m == 0);   // (every entry saturates: the table's smallest bound)
}

static void append_action() {
    const I8Action N = I8Action::nothing, B = I8Action::build, E = I8Action::extend;
    const long long built = 70001;
    // option "dense_int8" = 0: nothing, whatever else holds
    for (int wide = 0; wide < 2; ++wide)
        for (int wanted = 0; wanted < 2; ++wanted)
            for (int in_use = 0; in_use < 2; ++in_use)
                for (long long n : {1000ll, 65536ll, built + 3, 2 * built, 10 * built}) {
                    CHECK(i8_append_action(0, wide, wanted, in_use, n, 0) == N);
                    CHECK(i8_append_action(0, wide, wanted, in_use, n, built) == N);
                }
    for (int opt : {1, -1}) {
        // born small (no attempt yet): the first try at 65 536 rows
        CHECK(i8_append_action(opt, false, false, false, 5000, 0) == N);
        CHECK(i8_append_action(opt, false, false, false, 65535, 0) == N);
        CHECK(i8_append_action(opt, false, false, false, 65536, 0) == B);
        // a copy that exists follows the appends until the index is twice the size the clamp was chosen from
        CHECK(i8_append_action(opt, false, false, true, built + 3, built) == E);
        CHECK(i8_append_action(opt, false, false, true, 2 * built - 1, built) == E);
        CHECK(i8_append_action(opt, false, false, true, 2 * built, built) == B);
        CHECK(i8_append_action(opt, false, false, true, 2 * built + 1, built) == B);
        // a declined build is tried again when the index has doubled since
        CHECK(i8_append_action(opt, false, false, false, built + 3, built) == N);
        CHECK(i8_append_action(opt, false, false, false, 2 * built - 1, built) == N);
        CHECK(i8_append_action(opt, false, false, false, 2 * built, built) == B);
        CHECK(i8_append_action(opt, false, false, false, 2 * built + 1, built) == B);
        // wide rows: none is started unless "dense_int8_wide" asks for it ...
        CHECK(i8_append_action(opt, true, false, false, built, 0) == N);
        CHECK(i8_append_action(opt, true, false, false, 2 * built, built) == N);
        CHECK(i8_append_action(opt, true, true, false, 65535, 0) == N);
        CHECK(i8_append_action(opt, true, true, false, built, 0) == B);
        CHECK(i8_append_action(opt, true, true, false, 2 * built - 1, built) == N);
        CHECK(i8_append_action(opt, true, true, false, 2 * built, built) == B);
        // ... one that exists follows the appends with and without it, and chooses again (or is declined) when doubled
        for (int wanted = 0; wanted < 2; ++wanted) {
            CHECK(i8_append_action(opt, true, wanted, true, built + 3, built) == E);
            CHECK(i8_append_action(opt, true, wanted, true, 2 * built - 1, built) == E);
            CHECK(i8_append_action(opt, true, wanted, true, 2 * built + 1, built) == B);
        }
    }
}

int main() {
    choice();
    budget();
    clip_step();
    append_action();
    // the candidates for one (rms, d), for the test to recompute
    const double rms = 0.8125;
    const int d = 100;
    const Dense8ClipArgs ca = i8_clip_candidates(rms, d);
    printf("candidates rms=%a d=%d nclip=%d ncut=%d\n", rms, d, I8_NCLIP, I8_NCUT);
    for (int c = 0; c < I8_NCLIP; ++c) {
        printf("clamp %a dx %a inv_dx %a cut", kClip[c], (double)ca.dx[c], (double)ca.inv_dx[c]);
        for (int m = 0; m < I8_NCUT; ++m) printf(" %a", (double)ca.cut[c][m]);
        printf("\n");
    }
    printf("cuts");
    for (int m = 0; m < I8_NCUT; ++m) printf(" %a", kCut[m]);
    printf("\ni8 policy ok\n");
    return 0;
}
