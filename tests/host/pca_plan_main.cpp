// sq_pca_plan.hpp under the host sanitizers (tests/test_host_logic_pca.py): for every (d_in, d_out) the LDS asked for and the
// tiles per wave; the triangle's tile walk; row chunks that cover [0, n) once.
#include <cstdio>
#include <initializer_list>

#include "../../smqtk_indexing_amd/csrc/sq_pca_plan.hpp"

using namespace sq;

static int d_in = 0, d_out = 0;
#define CHECK(c) do { if (!(c)) { std::printf("pca plan: %s failed at d_in = %d, d_out = %d (line %d)\n", #c, d_in, d_out, __LINE__); return 1; } } while (0)

int main() {
    int widest = 0, most_tiles = 0;
    for (d_out = 1; d_out <= kPcaMaxDout; ++d_out) {
        for (d_in = d_out; d_in <= kPcaMaxDin; ++d_in) {
            const PcaPlan p = pca_plan(d_in, d_out);
            CHECK(p.lds_bytes <= kPcaLdsMax && p.sx % 8 == 4 && p.sa % 8 == 4 && p.lda % 4 == 0 && p.lda >= d_in && p.lda < d_in + 4);
            CHECK(p.rw * p.cw == 4 && p.tile_rows == 32 * p.rw && p.cols == 32 * p.cw * p.tpw && p.cols >= d_out && p.tpw <= 8);
            CHECK(p.tpw == 1 || p.cols < 2 * d_out);                      // no more tiles than twice the width needs
            CHECK(p.nslab == (d_in + 31) / 32 && p.blocks_per_cu >= 1 && p.blocks_per_cu * p.lds_bytes <= kPcaLdsMax);
            widest = p.lds_bytes > widest ? p.lds_bytes : widest, most_tiles = p.tpw > most_tiles ? p.tpw : most_tiles;
            CHECK(pca_slab_steps(d_in, p.nslab - 1) >= 1 && pca_slab_steps(d_in, 0) * kPcaKStep >= (d_in < kPcaSlabK ? d_in : kPcaSlabK));
            CHECK(pca_tiles(p, p.tile_rows + 1) == 2 && pca_grid(p, 0, 256) == 1u && pca_grid(p, 1ll << 40, 256) == 256u * p.blocks_per_cu);
        }
    }
    d_out = 0;
    for (d_in = 1; d_in <= kPcaMaxDin; ++d_in) {
        for (long long n : {2ll, 1023ll, 1024ll, 1025ll, 3079ll, 40965ll, 1ll << 20, kPcaMaxN - 1, kPcaMaxN}) {
            for (int cus : {0, 1, 256, 304}) {
                const PcaMomentsPlan m = pca_moments_plan(n, d_in, cus);
                CHECK(m.nb == (d_in + 127) / 128 && m.tiles == m.nb * (m.nb + 1) / 2);
                CHECK(m.chunk_rows % kPcaRun == 0 && m.nchunks >= 1 && m.nchunks <= kPcaMaxChunks && m.mean_chunks >= 1 && m.mean_chunks <= kPcaMaxChunks);
                CHECK((m.nchunks - 1) * m.chunk_rows < n && m.nchunks * m.chunk_rows >= n);
                CHECK((m.mean_chunks - 1) * m.mean_chunk_rows < n && m.mean_chunks * m.mean_chunk_rows >= n);
                CHECK(m.tiles > 1 || cus < 2 || n <= kPcaRun || m.nchunks > 1);   // one tile, many units: the rows are split
            }
        }
        const int nb = (d_in + 127) / 128;
        int t = 0;
        for (int i = 0; i < nb; ++i)
            for (int j = i; j < nb; ++j, ++t) {
                int bi = -1, bj = -1;
                pca_tile_of(t, nb, &bi, &bj);
                CHECK(bi == i && bj == j);
            }
        CHECK(t == nb * (nb + 1) / 2);
    }
    std::printf("pca plan ok: widest_lds=%d most_tiles_per_wave=%d\n", widest, most_tiles);
    return 0;
}
