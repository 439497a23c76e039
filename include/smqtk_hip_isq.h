/*
 * smqtk_hip_isq.h -- C ABI of libsmqtk_hip_isq.so, the IVF-SQ extension of libsmqtk_hip.so (MI355X, gfx950).
 *
 * An extension library on top of libsmqtk_hip.so and libsmqtk_hip_ivf.so: it adds nothing to their entry points.  Its
 * coarse index is a dense index of smqtk_hip.h, its centroids come from sq_ivf_kmeans, its handles are registered with the
 * main library, so sq_last_error, sq_get_stats, sq_handle_set_option("ivf_key_budget_mb" / "profile") /
 * sq_handle_reset_options work on them, and the conventions of smqtk_hip.h (return codes, `mem`, `stream`, result order,
 * padding) hold here unchanged.
 */
#ifndef SMQTK_HIP_ISQ_H
#define SMQTK_HIP_ISQ_H

#include "smqtk_hip_ivf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* IVF-SQ
 * Inverted lists whose rows are stored element by element in a narrower number format: what FaissNearestNeighborsIndex
 * reaches through the `factory_string`s "IVFx,SQ8" (one byte per dimension) and "IVFx,SQfp16" (two) (impls/nn_index/
 * faiss.py:190-192, :385).  The store between IVF-Flat (4 d bytes per row) and IVF-PQ (tens of bytes per row): the only
 * approximation besides the choice of lists is one rounding per element.
 * Lists, probe, result order, padding, ids, k, nprobe and id_base are exactly those of smqtk_hip_ivf.h; a row's list is the
 * nearest centroid of its ORIGINAL float32 values.  All arithmetic float32 without contraction (every operation rounded once):
 *   SQ_ISQ_SQ8  parameters vmin[d] and step[d], float32, given at creation.
 *     encode    t = (x[i] - vmin[i]) / step[i] (a subtract, then a correctly rounded divide);
 *               code = t > 0 ? min(rint(t), 255) : 0, rint rounding half to even.  NaN and values at or below vmin code to
 *               0, +inf to 255, and every element of a column with step[i] == 0 to 0.
 *     decode    xd[i] = vmin[i] + step[i] * float32(code): the product rounded, then the sum rounded.
 *   SQ_ISQ_F16  no parameters.  code = float16(x[i]), round to nearest even, subnormal halves kept, overflow to +-inf;
 *               xd[i] = float32(code), exact.
 *   distance    metrics.euclidean_distance(xd, q) (utils/metrics.py:73-86) in float32 in numpy's pairwise order with a
 *               correctly rounded root: sq_ivf_search's arithmetic over the decoded row.  So a search returns, bit for
 *               bit, what sq_ivf_search returns over the decoded matrix with the lists of the original matrix, and with
 *               nprobe >= nlist the bits of sq_dense_search over the decoded matrix.
 * L2 only, blocking calls only, no removal in place; the rows are coded as they are, not as residuals.
 * Storage: the codes list-major in one device buffer, ascending by id inside a list; the row stride is
 * round_up(d * code bytes, 16) bytes, zero padded; a uint32 insertion number per row, list_off[nlist + 1], and vmin / step
 * padded to round_up(d, 4) floats.  The float32 rows are not kept: at d = 128, 132 bytes per row (SQ8) and 260 (F16)
 * against IVF-Flat's 516.  Up to 2^32-1 rows.
 *   sq_isq_train   vmin[i] = the minimum and vmax[i] = the maximum of column i of x ([n][d] float32; a NaN in a column makes
 *                  both NaN, as numpy's min / max do), step[i] = (vmax[i] - vmin[i]) / 255 in float32; a reduction on the
 *                  device (min and max do not depend on the order).  x, vmin and step all in `mem` (host or device).
 *   sq_isq_create  an empty index over `centroids` ([nlist][d]) -- and `vmin`, `step` ([d] each) for SQ_ISQ_SQ8, which must be
 *                  NULL for SQ_ISQ_F16 -- all in host memory; metric must be SQ_METRIC_L2.
 *   sq_isq_add     assigns the new rows (host or device memory; any alignment) as sq_ivf_add does (option "ivf_assign"; after an
 *                  add sq_get_stats holds scan_launches, candidates, fallback_queries and, with option "profile", scan_ms), codes them (isq_encode_kernel) and
 *                  scatters old and new code rows into a new buffer by IVF-Flat's stable counting sort, 16 bytes at a time,
 *                  then swaps buffers.  Three adds leave the bytes one add of the same rows leaves.  A failed allocation
 *                  leaves the index as it was (SQ_ERR_NOMEM).
 *   sq_isq_lists   list_off[nlist + 1], the ids of all rows and their codes ([rows][d] of uint8 or uint16, without the
 *                  padding), list by list (host memory; any pointer may be NULL).
 *   sq_isq_info    out[SQ_ISQ_INFO_FIELDS] = { rows, d, nlist, longest list, empty lists, bytes of the codes, bytes of the
 *                  insertion numbers and offsets, bytes of the coarse index and the parameters, microseconds of the last
 *                  add, bytes of the key budget in force, kind, row stride in bytes }.
 *   sq_isq_search  mem = SQ_MEM_HOST or SQ_MEM_DEVICE, blocking, as sq_ivf_search; other modes: SQ_ERR_UNSUPPORTED.  Probe,
 *                  candidate offsets, key slices, select and padding are sq_ivf_search's; the scan is isq_scan_kernel --
 *                  grid (chunks of 256 candidates, queries of the slice), one candidate per lane; the workgroup stages the
 *                  query (SQ8: interleaved with vmin and step, four dimensions of each side by side) in dynamic LDS, a lane
 *                  reads its code row 8 or 16 bytes at a time, decodes in registers and sums in numpy's order.
 *                  sq_get_stats: scan_launches (slices scanned), candidates, bytes_scanned (candidates x row stride), and
 *                  with option "profile" scan_ms / total_ms.  An index with no rows answers with padding only.
 *                  Option "isq_scan" (handle or process-wide) chooses the scan of a slice: 0 = isq_scan_kernel as above,
 *                  1 = the list-major scan wherever it can run, -1 (the default) = list-major for slices with at least R
 *                  (query, list) pairs per list of the index, R per kind as profiles/ivf_sq_shared_scan.txt measured it
 *                  (sq_isq_plan.hpp).  List-major: the slice's pairs are sorted by list on the device (sq_ivf_search's
 *                  grouping: no atomics, no host visit) and cut into groups of up to 8 queries of one list;
 *                  isq_scan_shared_kernel decodes 256 code rows of the list once per group -- a leaf of up to 128
 *                  elements in registers at a time, the ranges staged once beside the group's queries in LDS -- scores them
 *                  against the group's queries in the same order of sums and stores every key where isq_scan_kernel stores
 *                  it: the results are the same bits.  It takes rows whose staging -- (2 + 8) round_up(d, 4) * 4 bytes
 *                  (SQ8), 8 round_up(d, 4) * 4 bytes (F16) -- fits 160 KiB - 256 bytes (d up to 4088, or 5112) and slices
 *                  of up to 2^24 pairs; everything else runs isq_scan_kernel.  sq_get_stats: mid_tier_queries = the pairs
 *                  of non-empty lists the list-major scan served (0: every slice ran per query); the other fields are
 *                  unchanged.  sq_refine_search over an IVF-SQ base takes the scan by the base handle's option.
 * Limits, refused before a device is touched: a kind other than the two, SQ8 without vmin / step or F16 with them, a
 * non-finite vmin or step or a negative step: SQ_ERR_INVALID; a metric other than L2, nlist > 65536, a search mode other
 * than the two blocking ones, and a d whose staging -- 3 round_up(d, 4) * 4 bytes (SQ8), round_up(d, 4) * 4 bytes (F16) --
 * exceeds a workgroup's 160 KiB of LDS (d beyond 13652, or 40960): SQ_ERR_UNSUPPORTED.
 * Left out on purpose: residual coding, other bit widths (4, 6, bfloat16), cosine and inner product, asynchronous calls,
 * removal in place, a layout interleaved across rows for fully coalesced wave loads.  (The device refine stage that uses
 * these codecs behind IVF-PQ is smqtk_hip_refine.h.) */
#define SQ_ISQ_SQ8 0
#define SQ_ISQ_F16 1
#define SQ_ISQ_INFO_FIELDS 12
int sq_isq_train(const float* x, int64_t n, int d, float* vmin /* [d] */, float* step /* [d] */, int mem);
int sq_isq_create(const float* centroids, int nlist, int d, int kind, const float* vmin, const float* step,
                  int metric, int64_t id_base, sq_handle_t* out);
int sq_isq_add(sq_handle_t h, const float* rows, int64_t n_add, int mem);
int sq_isq_lists(sq_handle_t h, int64_t* list_off /* [nlist+1] */, int64_t* ids /* [rows] */,
                 void* codes /* [rows][d] uint8 (SQ8) or uint16 (F16), list by list */);
int sq_isq_info(sq_handle_t h, int64_t* out, int n_out);
int sq_isq_search(sq_handle_t h, const float* queries, int nq, int k, int nprobe,
                  float* out_dist, int64_t* out_idx, int mem, void* stream);
int sq_isq_destroy(sq_handle_t h);

#ifdef __cplusplus
}
#endif
#endif /* SMQTK_HIP_ISQ_H */
