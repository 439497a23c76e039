/*
 * smqtk_hip_refine.h -- C ABI of libsmqtk_hip_refine.so, the refine stage behind the inverted-list indexes of
 * libsmqtk_hip.so (MI355X, gfx950).
 *
 * An extension library on top of libsmqtk_hip.so, libsmqtk_hip_ivf.so, libsmqtk_hip_pq.so and libsmqtk_hip_isq.so: it adds
 * nothing to their entry points.  Its handles are registered with the main library, so sq_last_error, sq_get_stats,
 * sq_handle_set_option("refine_direct" / "profile") / sq_handle_reset_options work on them, and the conventions of
 * smqtk_hip.h (return codes, `mem`, `stream`, result order, padding) hold here unchanged.
 */
#ifndef SMQTK_HIP_REFINE_H
#define SMQTK_HIP_REFINE_H

#include "smqtk_hip_isq.h"
#include "smqtk_hip_pq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Refine stage
 * What FaissNearestNeighborsIndex reaches through the `factory_string`s "IVFx,PQy,RFlat", "IVFx,PQy,Refine(SQfp16)" and
 * "IVFx,PQy,Refine(SQ8)": a coded index chooses k * k_factor candidates, and a second store of the rows, in id order and in
 * a wider code, ranks them again.  All arithmetic float32 without contraction (every operation rounded once).
 *   store     row i (insertion number) holds code(x_i); its id is id_base + i.  Kinds: SQ_REFINE_SQ8 (vmin[d], step[d] given
 *             at creation), SQ_REFINE_F16, SQ_REFINE_F32 (the row itself).  Encode and decode are those of smqtk_hip_isq.h
 *             -- the same device code -- so NaN, +inf, step == 0, half-to-even and subnormal halves behave as there.  The
 *             row stride is round_up(d * code bytes, 16) bytes, zero padded.  Up to 2^32-1 rows.
 *   distance  dist(id, q) = metrics.euclidean_distance(decode(store[id]), q) (utils/metrics.py:73-86) in numpy's pairwise
 *             order with a correctly rounded root: the arithmetic of sq_ivf_search / sq_isq_search.
 *   re-rank   cand[nq][kb] of int64.  Entries < id_base (the bases' -1 padding among them) and entries >= id_base + rows are
 *             skipped; the result is the k smallest (dist, id) over the others, ties by ascending id, and behind the last
 *             one -1 / +inf.  A query's valid candidates must be distinct ids (the bases' answers are).
 *   search    the base -- an IVF-Flat handle, an IVF-PQ handle of any mode (plain, residual, packed 4-bit) or an IVF-SQ
 *             handle -- answers kb candidates at nprobe into device scratch this handle owns; they are re-ranked.  So with
 *             kb >= the rows of the probed lists an F32 store returns, bit for bit, sq_ivf_search over the same centroids and
 *             rows, and an F16 / SQ8 store sq_isq_search of that kind, whatever the base.
 *   sq_refine_create  an empty store; vmin / step in host memory for SQ_REFINE_SQ8, NULL otherwise.
 *   sq_refine_add     codes the rows (host or device memory, any alignment; isq_encode_kernel) behind the rows already
 *                     there; the buffer grows on the device (by half again at least, a device-to-device copy).  A failed
 *                     allocation leaves the store as it was (SQ_ERR_NOMEM); three adds leave the bytes of one add.
 *   sq_refine_rows    the codes of rows [first, first + n) without the padding ([n][d] of uint8, uint16 or float32), host.
 *   sq_refine_info    out[SQ_REFINE_INFO_FIELDS] = { rows, d, kind, row stride in bytes, bytes of the codes, bytes of the
 *                     parameters, microseconds of the last add }.
 *   sq_refine_rerank  queries [nq][d], cand [nq][kb], the outputs [nq][k], all in `mem` (SQ_MEM_HOST or SQ_MEM_DEVICE),
 *                     blocking.  Three launches: refine_valid_kernel (one workgroup per query) keeps the valid entries in
 *                     their order as 32-bit row numbers and counts them; refine_rerank_kernel<KIND> -- grid (tiles of 32
 *                     candidates, queries), 256 lanes; the workgroup stages the query (SQ8: interleaved with vmin and step,
 *                     four dimensions of each side by side) in dynamic LDS, gathers the tile's 32 code rows from HBM into
 *                     LDS in 16-byte pieces, consecutive lanes on consecutive pieces of one row and all of a lane's loads
 *                     issued before the first is used, then eight lanes per candidate sum in numpy's order, lane j being
 *                     accumulator j of a leaf -- writes the keys (ordered distance, row number); the project's select
 *                     orders them, which is the (distance, id) order, and its post-op writes distances and ids.  Rows wider
 *                     than a 1024-byte slab are gathered slab by slab, each starting at the 16-byte piece that holds the
 *                     first element of the next leaf of numpy's tree; the tree's pending sums stay in registers across slabs.
 *                     Handle option "refine_direct": 1 runs the variant that reads the code rows straight from global
 *                     memory in the same order of operations (the same bits), 0 the LDS-staged gather described above,
 *                     -1 (the default) chooses by the kind as measured on gathers that miss the caches
 *                     (profiles/ivf_refine.txt, 32 queries x kb 400 / 1600 over 10 M x 128): the staged gather for F16
 *                     and F32 stores (0.94 - 0.96 x and 0.85 - 0.89 x the direct variant's time), direct loads for SQ8
 *                     (the staged gather takes 1.01 x / 1.11 x there).
 *                     A batch runs in slices of at most 32768 queries whose scratch (24 kb bytes per query) stays under
 *                     the IVF searches' key budget (option "ivf_key_budget_mb", 256 MB): nq has no limit of its own.
 *   sq_refine_search  as above behind a base index, slice by slice; the base's d, id_base and row count must equal the
 *                     store's, before the call and again after the base has answered a slice (a base added to in between:
 *                     SQ_ERR_INVALID).  As with every handle, the base must not be destroyed while a call uses it.
 *   sq_get_stats      candidates (valid ones), bytes_scanned (candidates x row stride), scan_launches, and with option
 *                     "profile" scan_ms (the refine kernel) / total_ms.
 * Limits, refused before a device is touched: an unknown kind, SQ8 without vmin / step or F16 / F32 with them, a
 * non-finite vmin or step or a negative step, kb < k, k, kb, nq or d below 1, a base whose d, id_base or row count differ:
 * SQ_ERR_INVALID; a `mem` other than the two blocking ones, a base of any other handle kind, and a d whose LDS -- 128 bytes
 * of row numbers, the staging of 3 round_up(d, 4) * 4 bytes (SQ8) or round_up(d, 4) * 4 bytes (F16, F32) and the tile of 32
 * slabs at a pitch of 1056 bytes -- exceeds a workgroup's 160 KiB (d beyond 10824 for SQ8, 32480 otherwise):
 * SQ_ERR_UNSUPPORTED.  kb (an int) has no other limit: up to 16384 keys per query the select works in one workgroup's LDS,
 * beyond from global memory, and k beyond 16384 takes the sorted select, as everywhere in the project.
 * Left out on purpose: cosine and inner product, asynchronous calls, removal in place, stores of other widths (4-bit,
 * 6-bit, bfloat16), a refine stage behind the Hamming / LSH path. */
#define SQ_REFINE_SQ8 0
#define SQ_REFINE_F16 1
#define SQ_REFINE_F32 2
#define SQ_REFINE_INFO_FIELDS 7
int sq_refine_create(int d, int kind, const float* vmin, const float* step, int64_t id_base, sq_handle_t* out);
int sq_refine_add(sq_handle_t h, const float* rows, int64_t n_add, int mem);
int sq_refine_rows(sq_handle_t h, int64_t first, int64_t n, void* codes);
int sq_refine_info(sq_handle_t h, int64_t* out, int n_out);
int sq_refine_rerank(sq_handle_t h, const float* queries, int nq, const int64_t* cand, int kb, int k,
                     float* out_dist, int64_t* out_idx, int mem, void* stream);
int sq_refine_search(sq_handle_t h, sq_handle_t base, const float* queries, int nq, int k, int kb, int nprobe,
                     float* out_dist, int64_t* out_idx, int mem, void* stream);
int sq_refine_destroy(sq_handle_t h);

#ifdef __cplusplus
}
#endif
#endif /* SMQTK_HIP_REFINE_H */
