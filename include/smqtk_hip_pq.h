/*
 * smqtk_hip_pq.h -- C ABI of libsmqtk_hip_pq.so, the IVF-PQ extension of libsmqtk_hip.so (MI355X, gfx950).
 *
 * An extension library on top of libsmqtk_hip.so and libsmqtk_hip_ivf.so: it adds nothing to their entry points.  Its
 * coarse index and its m codebook indexes are dense indexes of smqtk_hip.h, its training is sq_ivf_kmeans, its handles
 * are registered with the main library, so sq_last_error, sq_get_stats, sq_handle_set_option("ivf_key_budget_mb") /
 * sq_handle_reset_options work on them, and the conventions of smqtk_hip.h (return codes, `mem`, `stream`, result order,
 * padding) hold here unchanged.
 */
#ifndef SMQTK_HIP_PQ_H
#define SMQTK_HIP_PQ_H

#include "smqtk_hip_ivf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* IVF-PQ
 * Inverted lists whose rows are stored as product-quantiser codes: what FaissNearestNeighborsIndex reaches through the
 * `factory_string` "IVFx,PQy" (impls/nn_index/faiss.py:190-192, :385).  m sub-quantisers of ksub <= 256 entries each, one
 * byte per code; the point is memory: round_up(m, 4) + 4 bytes per row instead of 4 d.
 * Given centroids and codebooks everything is a function of the inputs.  With dsub = d / m and x_j = x[j dsub : (j+1) dsub],
 * all arithmetic float32 without contraction:
 *   list      a row belongs to the list of its nearest centroid by metrics.euclidean_distance (utils/metrics.py:73-86),
 *             ties to the lowest list: IVF-Flat's rule.
 *   code      code[j] is the nearest entry of codebook j to the row's own sub-vector x_j, same arithmetic, ties to the
 *             lowest entry.  The row is NOT coded as a residual against its centroid: one set of tables serves a query in
 *             every list it probes (residual mode, below, is the other choice).  On the device both are sq_dense_search with k = 1, over the coarse index and over m
 *             small dense indexes of the codebooks that the handle owns (float32 only, no scan copies).
 *   tables    T[j][c] = np.square(codebooks[j][c] - q_j).sum(): float32 in numpy's pairwise order, the square of
 *             euclidean_distance before its root.
 *   distance  acc = T[0][code[0]], then acc = acc + T[j][code[j]] for j = 1 .. m-1, left to right; the distance is the
 *             correctly rounded float32 square root of acc.
 *   result    the k smallest (distance, id) over the rows of the min(nprobe, nlist) probed lists (probe: the nearest
 *             centroids, ties by list number); ids id_base + insertion number; behind the last candidate -1 / +inf.
 *             Any k > 0.  An index with no rows answers with padding only.
 * Storage: the codes list-major in one device buffer (row stride round_up(m, 4) bytes, zero padded), ascending by id inside
 * a list, a uint32 insertion number per row and list_off[nlist + 1]; the float32 rows are not kept.  Up to 2^32-1 rows.
 *   sq_pq_train    codebook j is sq_ivf_kmeans over the contiguous copy of x[:, j dsub : (j+1) dsub] (a 2-D copy) from the
 *                  caller's initial entries, so the same input gives the same bits; x and codebooks both in `mem` (host
 *                  or device).  n < ksub: SQ_ERR_INVALID; at most 2^26 training rows.
 *   sq_pq_create   an empty index over `centroids` ([nlist][d]) and `codebooks` ([m][ksub][dsub]), both in host memory.
 *   sq_pq_add      assigns and codes the new rows (host or device memory) and scatters old and new codes into a new buffer
 *                  by IVF-Flat's stable counting sort, then swaps buffers.  Three adds leave the bytes one add of the same
 *                  rows leaves.  A failed allocation leaves the index as it was (SQ_ERR_NOMEM).
 *   sq_pq_lists    list_off[nlist + 1], the ids of all rows and their codes ([rows][m], without the padding), list by
 *                  list (host memory; any pointer may be NULL).
 *   sq_pq_info     out[SQ_PQ_INFO_FIELDS] = { rows, d, nlist, m, ksub, bytes of the codes, bytes of the insertion numbers
 *                  and offsets, bytes of the codebooks and the coarse index, microseconds of the last add, bytes of the key
 *                  budget in force }.
 *   sq_pq_search   mem = SQ_MEM_HOST or SQ_MEM_DEVICE, blocking, as sq_ivf_search; other modes: SQ_ERR_UNSUPPORTED.
 *                  Probe and candidate offsets as there; pq_tables_kernel writes the tables of a slice's queries;
 *                  pq_scan_kernel -- a workgroup stages ONE query's tables in m * ksub * 4 bytes of LDS and walks many
 *                  chunks of 256 of that query's candidates, a lane reads its row's code dwords and adds m table entries
 *                  in the order above; then the select with the conversion to (distance, id) and the padding.  The key
 *                  budget ("ivf_key_budget_mb") slices a batch as in sq_ivf_search, with the tables counted.
 *                  sq_get_stats: scan_launches (slices scanned), candidates, bytes_scanned (candidates x code stride), and
 *                  with option "profile" scan_ms / total_ms.
 *                  Option "profile" on a PQ handle: 1 = scan_ms is pq_scan_kernel's time and rerank_ms pq_tables_kernel's;
 *                  2 (measurement) = scan_ms is the time of a launch of pq_scan_kernel on the same grid that only stages
 *                  the tables and stores one word per lane; the real scan follows it untimed, the answers are the same.
 * Limits, refused before a device is touched: d % m != 0, m outside 1 .. 64, ksub outside 1 .. 256: SQ_ERR_INVALID;
 * nlist > 65536, a search mode other than the two blocking ones, and d / m > 16384 (pq_tables_kernel stages a query's
 * sub-vector in round_up(d / m, 4) * 4 <= 65536 bytes of dynamic LDS, what a plain launch takes): SQ_ERR_UNSUPPORTED.
 * d itself has no limit of its own: up to m * 16384.  The coarse index assigns and probes rows of any such width -- its
 * exact kernel stages a query of up to 40960 floats whole in a workgroup's LDS and a wider one two of numpy's
 * 8192-element buffers at a time (dense_exact_l2_pieces_kernel).  Before the tests ran m = 3 at d / m = 16384 an add of
 * rows wider than 40960 floats failed with SQ_ERR_HIP (a launch asking for more LDS than a workgroup has).
 * Run by the tests (tests/test_hip_pq.py): every m from 1 to 64 (padded code strides, both loads, both ways of staging
 * the tables), ksub 1, 13, 16, 255 and 256, m * ksub * 4 = 65536 bytes of tables, d / m at the 58 widths of
 * tests/width_cases.py and at 8193, 8199, 8200 and 16384 (65536 bytes of dynamic LDS pass pq_tables_kernel's plain launch),
 * scan workgroups that walk up to 16 chunks each, 700 lists, option "profile" 1 and 2, id_base beyond 2^32, a query
 * whose tables overflow to +inf (real ids ascending at +inf, -1 only behind the last candidate).
 *
 * Residual mode (sq_pq_create_residual): the same index with the rows coded as residuals against their list's centroid,
 * FAISS's default for "IVFx,PQy".  A handle made by sq_pq_create is untouched by it.  With the rules above, float32
 * without contraction:
 *   list      unchanged: l(x) is the nearest centroid, ties to the lowest list.
 *   residual  r = x - centroids[l(x)], element by element.
 *   code      code[j] is the nearest entry of codebook j to r_j (dense search with k = 1), ties to the lowest entry.
 *   tables    one set per query and probed list l: rq = q - centroids[l], T_l[j][c] = np.square(codebooks[j][c] - rq_j).sum()
 *             in numpy's pairwise order.
 *   distance  of a row of list l: sqrt_rn(((T_l[0][code[0]] + T_l[1][code[1]]) + ...) + T_l[m-1][code[m-1]]), left to right.
 *   result, padding, ids, k, nprobe: as above.
 *   sq_pq_create_residual   sq_pq_create's arguments; the handle also keeps the centroids on the device as
 *                  [nlist][round_up(d, 4)] float32, zero padded, counted in word 7 of sq_pq_info.
 *   sq_pq_residuals  out = x - centroids[l(x)] row by row (pq_residual_kernel behind the coarse assignment); x and out
 *                  both in `mem` (host or device; they may be the same buffer), centroids in host memory.  Codebooks for
 *                  this mode are sq_pq_train over its output.  nlist > 65536, more than 2^26 rows, other modes:
 *                  SQ_ERR_UNSUPPORTED, before a device is touched.
 *   sq_pq_add      codes pq_residual_kernel's output instead of the rows; everything else as above.
 *   sq_pq_search   a pair is (query of the slice, probe position), taken row-major.  pq_tables_res_kernel writes
 *                  [pair][m][ksub] tables (a pair with an empty list is skipped); pq_scan_res_kernel -- grid (groups,
 *                  pairs) -- stages its pair's tables in LDS and walks chunks g, g + groups, ... of 256 rows of that
 *                  pair's list, row i of the list at probe position jl writing its key at candidate pre[jl] + i; the
 *                  select is the one above.  groups = pq_scan_groups(chunks of the longest list, pairs, CUs).  The key
 *                  budget: queries per slice as above (one pair's tables counted per query); what the budget has left
 *                  beside the slice's keys holds the tables of clamp(.., 1, 65535) pairs, and a slice's pairs go in
 *                  ranges of that many, each one tables launch and one scan launch.  scan_launches counts the ranges;
 *                  option "profile" = 1 sums scan_ms / rerank_ms over them, 2 behaves as 1.
 * Run by the tests (tests/test_hip_pq_residual.py): nprobe 1 .. beyond nlist, k beyond the rows, host and device memory,
 * id_base beyond 2^32, an empty index, a query whose tables overflow, three adds against one, a list of 32 chunks in both
 * regimes of the scan grid, 64 KiB of tables in ranges that begin inside a query, m from 1 to 64, d / m from 1 to 16384,
 * sq_pq_residuals in host and device memory (d = 35 from an unaligned base, in place), and one list with a zero
 * centroid, where the answers are the plain mode's bits.
 * Left out on purpose: OPQ rotations, FAISS's precomputed-table decomposition of the residual distance, code sizes other than one byte, a refine stage over kept float32
 * rows, cosine, asynchronous calls, removal in place, retraining. */
#define SQ_PQ_INFO_FIELDS 10
int sq_pq_train(const float* x, int64_t n, int d, int m, int ksub,
                float* codebooks /* [m][ksub][d/m]; in: initial, out: trained */, int iters, int mem);
int sq_pq_create(const float* centroids, int nlist, int d, const float* codebooks, int m, int ksub,
                 int64_t id_base, sq_handle_t* out);
int sq_pq_create_residual(const float* centroids, int nlist, int d, const float* codebooks, int m, int ksub,
                          int64_t id_base, sq_handle_t* out);
int sq_pq_residuals(const float* x, int64_t n, int d, const float* centroids /* [nlist][d], host */, int nlist,
                    float* out /* [n][d], in `mem` as x */, int mem);
int sq_pq_add(sq_handle_t h, const float* rows, int64_t n_add, int mem);
int sq_pq_lists(sq_handle_t h, int64_t* list_off /* [nlist+1] */, int64_t* ids /* [rows] */,
                uint8_t* codes /* [rows][m], list by list */);
int sq_pq_info(sq_handle_t h, int64_t* out, int n_out);
int sq_pq_search(sq_handle_t h, const float* queries, int nq, int k, int nprobe,
                 float* out_dist, int64_t* out_idx, int mem, void* stream);
int sq_pq_destroy(sq_handle_t h);

#ifdef __cplusplus
}
#endif
#endif /* SMQTK_HIP_PQ_H */
