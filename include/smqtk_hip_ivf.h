/*
 * smqtk_hip_ivf.h -- C ABI of libsmqtk_hip_ivf.so, the IVF-Flat extension of libsmqtk_hip.so (MI355X, gfx950).
 *
 * An extension library: it links against libsmqtk_hip.so and adds nothing to that library's entry points.  Its coarse
 * index is a dense index of smqtk_hip.h (sq_dense_create_opts / sq_dense_search), its handles are registered with that
 * library, so sq_last_error, sq_get_stats, sq_handle_set_option / sq_handle_reset_options work on them, and the
 * conventions of smqtk_hip.h (return codes, `mem`, `stream`, result order, padding) hold here unchanged.
 */
#ifndef SMQTK_HIP_IVF_H
#define SMQTK_HIP_IVF_H

#include "smqtk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* IVF-Flat
 * Inverted lists over the float32 rows: what FaissNearestNeighborsIndex reaches through a `factory_string` with an IVF
 * stage and its `ivf_nprobe` (impls/nn_index/faiss.py:190-192, 230-236; nprobe is set before every search, :785, and
 * "Maybe increase nprobe if this is an IVF index?" is the warning when fewer than n neighbours come back, :805-809).
 * L2 only, blocking calls only, no removal in place.  Given the centroids everything is a function of the inputs:
 *   assignment  a row belongs to the list of its nearest centroid by metrics.euclidean_distance in float32
 *               (utils/metrics.py:73-86, numpy's pairwise order), ties to the lowest list number;
 *   probe       a query probes the min(nprobe, nlist) nearest centroids, same arithmetic, ties by list number;
 *   result      the k smallest (distance, id) over the rows of the probed lists; distances float32, bit-identical to
 *               euclidean_distance(row, q); ids id_base + insertion number; behind the last candidate id -1 / +inf.
 * With nprobe >= nlist the result is sq_dense_search's, bit for bit.  Both exact stages ARE sq_dense_search, on a dense
 * index over the centroids that the handle owns (float32 centroids only, no scan copies); nlist <= 65536, where that
 * search works on exact keys of every centroid -- more lists give SQ_ERR_UNSUPPORTED.
 * Storage: the rows list-major in one device buffer (row stride round_up(d, 4) floats, zero padded), ascending by id
 * inside a list, a uint32 insertion number per row and list_off[nlist + 1]: 1.0 x the matrix + 4 bytes per row; no scan
 * copy of any kind.  Up to 2^32-1 rows (keys carry a 32-bit row number); more give SQ_ERR_UNSUPPORTED.
 *   sq_ivf_kmeans  Lloyd iterations from the caller's initial centroids (in: initial, out: trained; x and centroids both
 *                  in `mem`, host or device).  Assign: the dense search, k = 1, over a temporary index of the
 *                  iteration's centroids.  Update: the float64 sum of each list's rows in insertion order by a fixed
 *                  reduction tree (no floating-point atomics: the same input gives the same bits), divided by the
 *                  count, rounded to float32 once; an empty list keeps its centroid.  n < nlist: SQ_ERR_INVALID; at most
 *                  2^26 training rows (train on a sample).
 *   sq_ivf_create  an empty index over `centroids` ([nlist][d], host memory); metric must be SQ_METRIC_L2.
 *   sq_ivf_add     assigns the new rows (host or device memory) in slices of 1024, and scatters old and new rows into a
 *                  new buffer by a stable counting sort on the device, then swaps buffers: what add_with_ids does
 *                  (faiss.py:561-640).  Three adds leave the lists one add of the same rows leaves.  A failed allocation
 *                  leaves the index as it was (SQ_ERR_NOMEM); an add of more than 2^26 rows is several such sorts, each
 *                  of which leaves a complete index.
 *   sq_ivf_lists   list_off[nlist + 1] and the ids (id_base + insertion number) of all rows, list by list (host memory;
 *                  either pointer may be NULL).
 *   sq_ivf_info    out[SQ_IVF_INFO_FIELDS] = { rows, d, nlist, longest list, empty lists, bytes of the rows, bytes of the
 *                  insertion numbers and offsets, bytes of the coarse index, microseconds of the last add, bytes of the
 *                  key budget in force }.
 *   sq_ivf_search  mem = SQ_MEM_HOST or SQ_MEM_DEVICE (queries [nq][d] and both outputs there; out_dist float32
 *                  [nq][k], out_idx int64 [nq][k]); the call returns when the results are final.  Other modes:
 *                  SQ_ERR_UNSUPPORTED.  Any k > 0.  Four steps: probe (the dense search); per-query candidate offsets
 *                  from the probed lists' sizes (only the candidate total and the longest candidate list visit the
 *                  host); ivf_scan_kernel -- a work item is 256 candidates of one query's concatenated range, a lane
 *                  finds its list in the query's prefix array and computes its row's distance as the dense exact path
 *                  does; the select of the k smallest keys with the conversion to (distance, id) and the padding.
 *                  Key scratch is bounded: a batch runs in query slices such that keys, selected keys and (for k beyond
 *                  16384) the sort's buffers stay under 256 MiB -- option "ivf_key_budget_mb" (0 = that default) on the
 *                  handle or process-wide; a single query whose candidates alone exceed the budget still runs.
 *                  sq_get_stats: scan_launches (slices scanned), candidates (rows scanned, summed over queries),
 *                  bytes_scanned (candidates x row stride x 4), and with option "profile" scan_ms / total_ms.
 *                  An index with no rows answers with padding only.
 *                  Limits, as run on an MI355X under ROCm's HIP runtime: the scan stages a query in round_up(d, 4) * 4
 *                  bytes of dynamic LDS, so a row of more than 40960 floats (160 KiB) cannot be searched; the widest row
 *                  tested is 16389 floats (65568 bytes, which a plain launch takes).  The queries of a slice are the
 *                  second dimension of the scan's grid and nothing but the key budget bounds a slice; the runtime
 *                  reports 65536 as that dimension's maximum, accepts more, and a slice of 70000 queries is tested. */
#define SQ_IVF_INFO_FIELDS 10
int sq_ivf_kmeans(const float* x, int64_t n, int d, float* centroids /* in: initial, out: trained */,
                  int nlist, int iters, int mem);
int sq_ivf_create(const float* centroids, int nlist, int d, int metric, int64_t id_base, sq_handle_t* out);
int sq_ivf_add(sq_handle_t h, const float* rows, int64_t n_add, int mem);
int sq_ivf_lists(sq_handle_t h, int64_t* list_off /* [nlist+1] */, int64_t* ids /* [rows], list by list */);
int sq_ivf_info(sq_handle_t h, int64_t* out, int n_out);
int sq_ivf_search(sq_handle_t h, const float* queries, int nq, int k, int nprobe,
                  float* out_dist, int64_t* out_idx, int mem, void* stream);
int sq_ivf_destroy(sq_handle_t h);

#ifdef __cplusplus
}
#endif
#endif /* SMQTK_HIP_IVF_H */
