/*
 * smqtk_hip_pca.h -- C ABI of libsmqtk_hip_pca.so, the PCA front stage of the inverted-list indexes (MI355X, gfx950).
 *
 * An extension library on top of libsmqtk_hip.so alone: it adds nothing to the other libraries' entry points.  Its handles
 * are registered with the main library, so sq_last_error, sq_get_stats, sq_handle_set_option("profile") /
 * sq_handle_reset_options work on them, and the conventions of smqtk_hip.h (return codes, `mem`, `stream`) hold here.
 */
#ifndef SMQTK_HIP_PCA_H
#define SMQTK_HIP_PCA_H

#include "smqtk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* PCA front stage
 * What FaissNearestNeighborsIndex reaches through a `factory_string` that starts with "PCAy,": every row and every query
 * is centred and projected onto the y leading principal directions of a training sample before the index behind sees it
 * (FAISS's PCAMatrix).  Two pieces: the second moments the training needs, and the projection.  The eigen-decomposition
 * is the plugin's, on the host in float64 (impls/nn_index/hip_ivf_pca.py).
 *
 *   sq_pca_moments  x [n][d] float32 in `mem` (SQ_MEM_HOST or SQ_MEM_DEVICE; mean_out and scatter_out in the same), dense
 *                   rows; blocking.
 *                     mean_out[i]       the float64 sum of column i, divided by n and rounded to float32 once.  The sum is
 *                                       a fixed tree (four row lanes per column inside chunks of rows that depend on n
 *                                       alone, the chunks added in order): no floating-point atomics, the same input gives
 *                                       the same bits.
 *                     scatter_out[i][j] sum_r (x[r][i] - mean_out[i]) * (x[r][j] - mean_out[j]), float64 [d][d], exactly
 *                                       symmetric -- about the float32 mean the call returns, so there is no hidden term.
 *                   pca_scatter_kernel: one workgroup of four waves per (128 x 128 tile of the upper triangle, chunk of
 *                   rows).  A slab of 32 rows x 128 columns per side is centred as it is staged into LDS (the next slab's
 *                   global loads in flight under the current slab's MFMAs); the MFMA's k is the row index, and both
 *                   operands of v_mfma_f32_32x32x2_f32 are read along rows of the slab (lane l: column l % 32 of row
 *                   2 kk + l / 32; 4-byte reads, consecutive lanes on consecutive banks, the two rows of a step on the two
 *                   halves of the banks by a pitch of 160 floats).  A wave holds 2 x 2 MFMA tiles; its float32 accumulators
 *                   run for at most SQ_PCA_RUN = 1024 rows and are then folded into 64 float64 accumulators per lane.
 *                   Where the triangle has fewer tiles than the device has compute units the rows are split into chunks;
 *                   pca_scatter_reduce_kernel adds the chunks' float64 tiles in chunk order and mirrors the lower triangle.
 *                   accuracy, against float64 arithmetic about the same float32 mean:
 *                     |S - S64| <= (gamma_{SQ_PCA_RUN + 2} + n 2^-53) * sum_r |x_ri - m_i| |x_rj - m_j|,
 *                   gamma_m = m u / (1 - m u), u = 2^-24: one rounding per centred operand, a float32 sum of at most 1024
 *                   products in any order, float64 folds.
 *   sq_pca_create   A [d_out][d_in] row-major and mean [d_in] (NULL: zeros) in host memory; the handle keeps device copies
 *                   with rows zero padded to a multiple of four floats.
 *   sq_pca_apply    y[r][j] = sum_i A[j][i] * (x[r][i] - mean[i]); x [n][d_in] and y [n][d_out], both in `mem`
 *                   (SQ_MEM_HOST or SQ_MEM_DEVICE), any alignment of a float, dense rows.  x and y must not overlap; equal
 *                   pointers are refused.  In device memory the call is enqueued on `stream` and returns (with option
 *                   "profile" it waits and sq_get_stats reports the kernel's scan_ms); in host memory it is blocking.
 *                   n = 0 succeeds and writes nothing.  One launch of pca_apply_kernel: a workgroup of four waves owns
 *                   tiles of rows (tile b, b + grid, ...) and holds ALL d_out output columns of a tile as MFMA accumulators
 *                   across the whole k loop -- up to eight 32 x 32 tiles per wave at d_out = 512, 64-row tiles; d_out <= 32:
 *                   128-row tiles, one tile per wave -- so every element of x is read from memory exactly once whatever
 *                   d_in.  x goes through LDS in slabs of 32 k with the mean subtracted as a slab is staged (one float32
 *                   subtraction per element; zeros behind d_in and behind n), A in slabs of [d_out][32] shared by the waves,
 *                   the next slabs' global loads in flight under the current MFMAs.  Rows are read in 16-byte pieces where
 *                   d_in % 4 == 0 and x is 16-byte aligned, element by element otherwise; never memory behind a row, and
 *                   nothing is written behind y.
 *                   accuracy, against the float64 evaluation of the same float32 inputs:
 *                     |y - y64| <= gamma_{d_in + 1} * sum_i |A[j][i]| * |x[r][i] - mean[i]|
 *                   (one rounding for the subtraction, then a float32 sum of d_in products in any order: Higham, Accuracy
 *                   and Stability of Numerical Algorithms, section 3.1).  A 0/1 selection matrix gives fl(x - mean) exactly.
 *   sq_pca_info     out[SQ_PCA_INFO_FIELDS] = { d_in, d_out, bytes resident on the device, rows of the last apply,
 *                   microseconds of the last apply as its caller saw them, rows per tile, workgroups per compute unit at
 *                   the most }.
 *   sq_get_stats    scan_launches, bytes_scanned (n * d_in * 4, the rows read), with "profile" scan_ms / total_ms.
 * Limits, refused before a device is touched: nulls, n < 0 (moments: n < 2), d < 1, overlapping or equal buffers:
 * SQ_ERR_INVALID; d_out > d_in, d_out > 512, d_in > 8192, moments of more than 2^26 rows (train on a sample), a `mem` other
 * than the two above: SQ_ERR_UNSUPPORTED; a handle of another kind: SQ_ERR_INVALID ("unknown handle").
 * Left out on purpose: whitening (eigen_power), a random rotation behind the projection (PCAR), float16 rows, cosine, and
 * moving OPQ's host cross-product onto the scatter kernel (it would change the trained rotation's bits). */
#define SQ_PCA_MAX_D_IN 8192
#define SQ_PCA_MAX_D_OUT 512
#define SQ_PCA_RUN 1024
#define SQ_PCA_INFO_FIELDS 7
int sq_pca_moments(const float* x, int64_t n, int d, float* mean_out, double* scatter_out, int mem);
int sq_pca_create(const float* A, const float* mean, int d_in, int d_out, sq_handle_t* out);
int sq_pca_apply(sq_handle_t h, const float* x, int64_t n, float* y, int mem, void* stream);
int sq_pca_info(sq_handle_t h, int64_t* out, int n_out);
int sq_pca_destroy(sq_handle_t h);

#ifdef __cplusplus
}
#endif
#endif /* SMQTK_HIP_PCA_H */
