/*
 * smqtk_hip_opq.h -- C ABI of libsmqtk_hip_opq.so, the linear transform in front of the product-quantised indexes of
 * libsmqtk_hip_pq.so (MI355X, gfx950).
 *
 * An extension library on top of libsmqtk_hip.so alone: it adds nothing to the other libraries' entry points.  Its handles
 * are registered with the main library, so sq_last_error, sq_get_stats, sq_handle_set_option("profile") /
 * sq_handle_reset_options work on them, and the conventions of smqtk_hip.h (return codes, `mem`, `stream`) hold here.
 */
#ifndef SMQTK_HIP_OPQ_H
#define SMQTK_HIP_OPQ_H

#include "smqtk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* OPQ transform
 * What FaissNearestNeighborsIndex reaches through the `factory_string` "OPQy,IVFx,PQy": a d x d matrix, trained to be the
 * orthonormal rotation under which a product quantiser reconstructs a sample best (Ge et al., "Optimized Product
 * Quantization"; FAISS's OPQMatrix), applied to every row before it is coded and to every query before its tables are
 * built.  The training loop is the plugin's (impls/nn_index/hip_ivf_opq.py); this library holds the matrix and applies it.
 *   product   y[r][j] = sum_i A[j][i] * x[r][i], r < n, j < d; float32 in, float32 out.  A need not be orthonormal.
 *   accuracy  NOT bit for bit: the sum runs on v_mfma_f32_32x32x2_f32, whose internal summation order is the hardware's.
 *             Promised, against the float64 product of the same float32 inputs:
 *                 |y[r][j] - y64[r][j]| <= gamma_d * sum_i |A[j][i]| * |x[r][i]|,  gamma_d = d u / (1 - d u),  u = 2^-24,
 *             the bound of a float32 sum of d products in any order, fused or not (Higham, Accuracy and Stability of
 *             Numerical Algorithms, section 3.1) -- derived, not tuned; inputs and partial sums in the normal range.
 *             Everything behind the transform (sq_pq_add, sq_pq_search, ...) keeps its bit contracts over the rows
 *             sq_opq_apply actually wrote.
 *   sq_opq_create   A [d][d] row-major in host memory; the handle keeps a device copy with its rows zero padded to a
 *                   multiple of four floats.
 *   sq_opq_apply    x [n][d] and y [n][d], both in `mem` (SQ_MEM_HOST or SQ_MEM_DEVICE), any alignment of a float, dense
 *                   rows.  x and y must not overlap; equal pointers are refused.  In device memory the call is enqueued on
 *                   `stream` and returns; y is final when the stream is (with option "profile" the call waits and
 *                   sq_get_stats reports the kernel's scan_ms).  In host memory the call is blocking.  n = 0 succeeds and
 *                   writes nothing.  One launch of opq_apply_kernel whatever n: a workgroup of four waves owns tiles of 64
 *                   rows (tile b, b + grid, ...; at most 8 workgroups per compute unit) and produces every output column
 *                   of a tile, 128 at a time, with accumulators in registers across k; A is staged through LDS in slabs of
 *                   32 k shared by the four waves, the next slab's global loads in flight under the current slab's MFMAs.
 *                   d <= 512: the row tile is read once into LDS and stays there across the column blocks; wider rows:
 *                   a 32-k slab of the tile is staged beside every slab of A (the tile's re-reads come from L2).  Rows are
 *                   read in 16-byte pieces where d % 4 == 0 and x is 16-byte aligned, element by element otherwise; padding
 *                   is zeros written to LDS, never memory behind a row; rows at and behind n are neither read nor written.
 *   sq_opq_info     out[SQ_OPQ_INFO_FIELDS] = { d, bytes resident on the device, rows of the last apply, microseconds of
 *                   the last apply as its caller saw them (a device-memory call without "profile": the enqueue) }.
 *   sq_get_stats    scan_launches, bytes_scanned (n * d * 4, the rows read), with "profile" scan_ms / total_ms.
 * Limits, refused before a device is touched: d < 1, a null A, x, y or out, n < 0, x == y: SQ_ERR_INVALID; d > 4096, a
 * `mem` other than the two above: SQ_ERR_UNSUPPORTED; a handle of another kind: SQ_ERR_INVALID ("unknown handle").
 * Left out on purpose: dimension reduction (d_out < d), a bias term, float16 / bfloat16 rows, asynchronous host calls. */
#define SQ_OPQ_MAX_D 4096
#define SQ_OPQ_INFO_FIELDS 4
int sq_opq_create(const float* A, int d, sq_handle_t* out);
int sq_opq_apply(sq_handle_t h, const float* x, int64_t n, float* y, int mem, void* stream);
int sq_opq_info(sq_handle_t h, int64_t* out, int n_out);
int sq_opq_destroy(sq_handle_t h);

#ifdef __cplusplus
}
#endif
#endif /* SMQTK_HIP_OPQ_H */
