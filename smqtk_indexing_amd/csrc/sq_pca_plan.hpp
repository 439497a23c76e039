// The tile, slab and chunk arithmetic of the PCA library (sq_pca.hip), plain C++: how pca_apply_kernel's four waves split
// an output width, what a workgroup holds in LDS, how many workgroups a call launches; and for sq_pca_moments the
// triangle of 128 x 128 tiles and the row chunks.  tests/host/pca_plan_main.cpp walks every (d_in, d_out) under the host
// sanitizers.
#pragma once

#ifdef __HIPCC__
#define SQ_PCA_HD __host__ __device__
#else
#define SQ_PCA_HD
#endif

namespace sq {

// ------------------------------------------------------------------------------------------------ apply
static constexpr int kPcaMaxDin = 8192;        // widest input row sq_pca_create takes
static constexpr int kPcaMaxDout = 512;        // widest output row: sixteen 32-column MFMA tiles, all held as accumulators
static constexpr int kPcaSlabK = 32;           // k elements of A and of the row tile in LDS at a time
static constexpr int kPcaKStep = 8;            // k elements per 16-byte operand read: four MFMAs of k = 2, both lane halves
static constexpr int kPcaLdsMax = 160 * 1024;  // dynamic LDS a workgroup may ask for
static constexpr int kPcaBlocksPerCu = 8;      // workgroups a call launches per compute unit at the most

// LDS pitch of an operand row of `k` elements, in floats: k rounded up to the k step, and four more.  A 16-byte operand
// read per lane, lane l at row l % 32 and k offset 4 (l / 32): a pitch of 8 m + 4 floats is an odd multiple of four
// dwords, so 16 consecutive rows start at the 16 distinct multiples of four modulo 64 and their reads cover the 64 banks
// once (a pitch of 32 would put every row on the same four).
inline int pca_pitch(int k) { return (k + kPcaKStep - 1) / kPcaKStep * kPcaKStep + 4; }

struct PcaPlan {
    int d_in = 0, d_out = 0;
    int lda = 0;          // floats per row of the device copies of A and of the mean: d_in rounded up to 4, zero padded
    int rw = 0, cw = 0;   // the four waves as rw row groups of 32 rows x cw column groups; rw * cw == 4
    int tpw = 0;          // 32-column tiles a wave accumulates: cw * tpw * 32 >= d_out
    int tile_rows = 0;    // rows a workgroup owns at a time: 32 rw
    int cols = 0;         // columns of A staged per slab: 32 cw tpw
    int sx = 0, sa = 0;   // LDS pitches of the row slab and of the slab of A
    int nslab = 0;        // k slabs
    int lds_bytes = 0;    // dynamic LDS: [tile_rows][sx] then [cols][sa] floats
    int blocks_per_cu = 0;   // grid cap per compute unit: what the LDS leaves room for, at most kPcaBlocksPerCu
};

// Narrow outputs give every wave rows of its own (128-row tiles); from 33 columns on two row groups share the slab of A
// and each wave holds 1, 2, 4 or 8 column tiles, so that every output column of a tile is an accumulator for the whole
// k loop and a row is read from memory once.
inline PcaPlan pca_plan(int d_in, int d_out) {
    PcaPlan p;
    p.d_in = d_in;
    p.d_out = d_out;
    p.lda = (d_in + 3) / 4 * 4;
    p.rw = d_out <= 32 ? 4 : 2;
    p.cw = 4 / p.rw;
    p.tpw = d_out <= 64 ? 1 : d_out <= 128 ? 2 : d_out <= 256 ? 4 : 8;
    p.tile_rows = 32 * p.rw;
    p.cols = 32 * p.cw * p.tpw;
    p.sx = p.sa = pca_pitch(kPcaSlabK);
    p.nslab = (d_in + kPcaSlabK - 1) / kPcaSlabK;
    p.lds_bytes = (p.tile_rows * p.sx + p.cols * p.sa) * 4;
    const int fit = kPcaLdsMax / p.lds_bytes;
    p.blocks_per_cu = fit < 1 ? 1 : fit > kPcaBlocksPerCu ? kPcaBlocksPerCu : fit;
    return p;
}

// k steps of slab s that hold an element of the row: the steps behind them are never read
inline int pca_slab_steps(int d_in, int s) {
    const int left = d_in - s * kPcaSlabK;
    return ((left < kPcaSlabK ? left : kPcaSlabK) + kPcaKStep - 1) / kPcaKStep;
}

inline long long pca_tiles(const PcaPlan& p, long long n) { return (n + p.tile_rows - 1) / p.tile_rows; }
// workgroups of a call over `tiles` row tiles on `cus` compute units: workgroup b takes tiles b, b + grid, ...
inline unsigned pca_grid(const PcaPlan& p, long long tiles, int cus) {
    const long long cap = (long long)(cus > 0 ? cus : 1) * p.blocks_per_cu;
    return (unsigned)(tiles < cap ? (tiles > 0 ? tiles : 1) : cap);
}

// ---------------------------------------------------------------------------------------------- moments
static constexpr int kPcaRun = 1024;            // rows a float32 accumulator runs for before it is folded into float64
static constexpr int kPcaTile = 128;            // a scatter tile is 128 x 128: four waves x (2 x 2) MFMA tiles of 32 x 32
static constexpr int kPcaSlabRows = 32;         // rows of the centred slab in LDS at a time
static constexpr int kPcaSlabPitch = 160;       // floats per slab row: 128 + 32, so that the two rows of an MFMA step (lanes 0 .. 31 | 32 .. 63, 4-byte reads) fall on different halves of the 64 banks
static constexpr long long kPcaMaxN = 1ll << 26;
static constexpr int kPcaMeanCols = 64;         // columns per workgroup of the column-sum kernel (four row lanes each)
static constexpr int kPcaMeanChunkRows = 4096;  // rows per column-sum chunk at the least
static constexpr int kPcaMaxChunks = 256;       // chunks at the most, of either kind

struct PcaMomentsPlan {
    int nb = 0;                    // 128-column blocks
    int tiles = 0;                 // tiles of the upper triangle: nb (nb + 1) / 2
    long long chunk_rows = 0;      // rows per scatter chunk: a multiple of kPcaRun
    int nchunks = 0;
    long long mean_chunk_rows = 0;
    int mean_chunks = 0;
};

// Tile t of the upper triangle, row-major: (0,0) (0,1) ... (0,nb-1) (1,1) ...
SQ_PCA_HD inline void pca_tile_of(int t, int nb, int* bi, int* bj) {
    int i = 0;
    while (t >= nb - i) {
        t -= nb - i;
        ++i;
    }
    *bi = i;
    *bj = i + t;
}

// Where the triangle has fewer tiles than the device has compute units the rows are split into chunks, one workgroup
// per (tile, chunk); chunk c is rows [c chunk_rows, min(n, (c + 1) chunk_rows)).
inline PcaMomentsPlan pca_moments_plan(long long n, int d, int cus) {
    PcaMomentsPlan p;
    p.nb = (d + kPcaTile - 1) / kPcaTile;
    p.tiles = p.nb * (p.nb + 1) / 2;
    long long want = (cus > 0 ? cus : 1) / p.tiles;
    if (want < 1) want = 1;
    if (want > kPcaMaxChunks) want = kPcaMaxChunks;
    p.chunk_rows = ((n + want - 1) / want + kPcaRun - 1) / kPcaRun * kPcaRun;
    p.nchunks = (int)((n + p.chunk_rows - 1) / p.chunk_rows);
    p.mean_chunk_rows = (n + kPcaMaxChunks - 1) / kPcaMaxChunks;
    if (p.mean_chunk_rows < kPcaMeanChunkRows) p.mean_chunk_rows = kPcaMeanChunkRows;
    p.mean_chunks = (int)((n + p.mean_chunk_rows - 1) / p.mean_chunk_rows);
    return p;
}

}  // namespace sq
