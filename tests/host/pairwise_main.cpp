// The tree walks of smqtk_indexing_amd/csrc/sq_pairwise.hpp (pw_tree / pw_tree_buffer, pw_tree_multi, pw_tree_depth) on
// a CPU at every row width: compiled with -fsanitize=address,undefined and run by tests/test_host_logic_pairwise.py,
// which compares every printed sum with numpy's own np.sum of the same elements, byte for byte.
//
// Only the walk is under test.  The leaf is this program's, written plainly from numpy's rule for 128 elements or
// fewer; it also checks what the walk hands it: leaves of 1 .. 128 elements, in order, adjoining, covering [0, n).
// Every width sums a copy of the data that is exactly n elements long, so a walk that leaves [0, n) is an address error.
//
//   pairwise_main FILE R L    FILE: R float32 vectors of L elements, then R float64 vectors of L elements
// prints
//   group_depth D             EXACT_GROUP_DEPTH
//   depth n D                 pw_tree_depth(n), n = 1 .. 8192
//   f32 n h .. h              bits of pw_tree<float> over the first n elements of each vector (R words)
//   f64 n h .. h              bits of pw_tree<double>
//   multi n h .. h            bits of pw_tree_multi<float, 3, EXACT_GROUP_DEPTH>, for the widths that depth takes
#include "../../smqtk_indexing_amd/csrc/sq_pairwise.hpp"

#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace sq;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

static_assert(pw_tree_depth(1) == 0 && pw_tree_depth(128) == 0, "one leaf");
static_assert(pw_tree_depth(129) == 1, "the first split");
static_assert(pw_tree_depth(8192) == 6, "128 * 2^6: six even levels");
static_assert(pw_tree_depth(7688) == 6 && pw_tree_depth(7689) == 7, "the first width below 8192 that needs 7 levels");
static_assert(pw_tree_depth(8191) == 7, "right parts of 4103, 2055, 1031, 519, 263, 135, 71 elements");
static_assert(pw_tree_depth(255) == 2 && pw_tree_depth(256) == 1, "255 = a leaf of 120 + a subtree of 135: deeper than 256 = 128 + 128");

static constexpr int G = 3;
static const int kBeyond[] = {8193, 8199, 8200, 8300, 12288, 16384, 16385, 20000};   // numpy's 8192-element buffers

// numpy's sum of n <= 128 contiguous elements
template <class T>
static T leaf_sum(const T* a, int n) {
    if (n < 8) {
        T r = (T)0;
        for (int i = 0; i < n; ++i) r = r + a[i];
        return r;
    }
    T r[8];
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    const int nfull = n - n % 8;
    for (int i = 8; i < nfull; i += 8)
        for (int j = 0; j < 8; ++j) r[j] = r[j] + a[i + j];
    T res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (int i = nfull; i < n; ++i) res = res + a[i];
    return res;
}

// What a walk over n elements may ask of its leaf: adjoining ranges of 1 .. 128 elements from 0 to n.
struct Cover {
    int n, next = 0, leaves = 0;
    explicit Cover(int n_) : n(n_) {}
    void take(int off, int m) {
        CHECK(m >= 1 && m <= 128);
        CHECK(off == next && off + m <= n);
        next = off + m;
        ++leaves;
    }
    void done() const { CHECK(next == n); }
};

template <class T>
static T walk_one(const T* a, int n) {
    Cover c(n);
    const T s = pw_tree<T>(
        [&](int off, int m) {
            c.take(off, m);
            return leaf_sum(a + off, m);
        },
        n);
    c.done();
    return s;
}

static uint32_t bits(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}
static uint64_t bits(double v) {
    uint64_t u;
    memcpy(&u, &v, 8);
    return u;
}

template <class T>
static std::vector<T> read_vectors(FILE* f, int r, int l) {
    std::vector<T> v((size_t)r * l);
    CHECK(fread(v.data(), sizeof(T), v.size(), f) == v.size());
    return v;
}

int main(int argc, char** argv) {
    CHECK(argc == 4);
    const int R = atoi(argv[2]), L = atoi(argv[3]);
    CHECK(R >= 1 && R <= 64 && L >= 20000);
    FILE* f = fopen(argv[1], "rb");
    CHECK(f != nullptr);
    const std::vector<float> a32 = read_vectors<float>(f, R, L);
    const std::vector<double> a64 = read_vectors<double>(f, R, L);
    CHECK(fgetc(f) == EOF);
    fclose(f);

    printf("group_depth %d\n", EXACT_GROUP_DEPTH);
    int deepest = 0;
    for (int n = 1; n <= PW_BUFSIZE; ++n) {
        const int dep = pw_tree_depth(n);
        printf("depth %d %d\n", n, dep);
        deepest = dep > deepest ? dep : deepest;
    }
    CHECK(deepest <= PW_MAX_DEPTH);   // the shift register of pw_tree_buffer holds every buffer's tree

    std::vector<int> widths;
    for (int n = 1; n <= PW_BUFSIZE; ++n) widths.push_back(n);
    for (int n : kBeyond) widths.push_back(n);

    for (int n : widths) {
        // exactly n elements of every vector, each in a block of its own
        std::vector<std::vector<float>> x32;
        std::vector<std::vector<double>> x64;
        for (int r = 0; r < R; ++r) {
            x32.emplace_back(a32.begin() + (size_t)r * L, a32.begin() + (size_t)r * L + n);
            x64.emplace_back(a64.begin() + (size_t)r * L, a64.begin() + (size_t)r * L + n);
        }
        printf("f32 %d", n);
        for (int r = 0; r < R; ++r) printf(" %08" PRIx32, bits(walk_one<float>(x32[r].data(), n)));
        printf("\nf64 %d", n);
        for (int r = 0; r < R; ++r) printf(" %016" PRIx64, bits(walk_one<double>(x64[r].data(), n)));
        printf("\n");
        if (n > PW_BUFSIZE || pw_tree_depth(n) > EXACT_GROUP_DEPTH) continue;
        // G sums per walk, as the exact path's group kernel makes them: vectors r0 .. r0 + G - 1 (the last group wraps)
        printf("multi %d", n);
        for (int r0 = 0; r0 < R; r0 += G) {
            Cover c(n);
            float out[G];
            pw_tree_multi<float, G, EXACT_GROUP_DEPTH>(
                [&](int off, int m, float(&v)[G]) {
                    c.take(off, m);
                    for (int g = 0; g < G; ++g) v[g] = leaf_sum(x32[(r0 + g) % R].data() + off, m);
                },
                n, out);
            c.done();
            for (int g = 0; g < G && r0 + g < R; ++g) printf(" %08" PRIx32, bits(out[g]));
        }
        printf("\n");
    }
    printf("pairwise ok\n");
    return 0;
}
