/*
 * vdbhip.h -- C ABI of the MI355X-native distance / top-k engine (libvdbhip.so).
 *
 * This is the drop-in boundary for the one hot path of lab-1806-vec-db:
 * src/distance, src/vec_set, src/index_algorithm::{flat,hnsw,pq}.  The reference has no
 * FFI on this path (everything is generic Rust, monomorphised); the narrowest seam is
 * `DynamicIndex` (src/database/dynamic_index.rs:11-94) which forwards to the index traits
 * (src/index_algorithm/mod.rs:35-154).  Every entry point below names the reference
 * interface it replaces.  A Rust `extern "C"` block binds this 1:1.
 *
 * Conventions
 *  - plain pointers and sizes only; `usize` is uint64_t; DistanceAlgorithm is an int with
 *    the reference's bincode variant order (distance/mod.rs:17-28): 0 = L2Sqr, 1 = Cosine.
 *  - every function returns 0 on success, non-zero on failure; the message is available
 *    through vdb_last_error() (thread-local).  Nothing aborts the process.
 *  - read-side calls (knn*, row, len...) are re-entrant on one handle, like `&self` methods
 *    under the reference's RwLock read guard (database/mod.rs:248-256); write-side calls
 *    (add, swap_remove, remove_rows, update_rows, *_build, *_attach, *_clear) need external exclusion, like `&mut self`.
 *  - results for query q are written at out_idx[q*k .. q*k+out_count[q]) ascending by
 *    (distance, index) -- the order of `Vec<CandidatePair>` (candidate_pair.rs:36-41);
 *    out_count[q] = min(k, len) for Flat (flat_index.rs:163).
 *  - `*_device` variants take device pointers valid on the index's GPU and a hipStream_t
 *    (passed as void*); they are asynchronous unless noted.
 *  - there is NO CPU fallback: without a usable GPU every compute entry point fails.
 */
#ifndef VDBHIP_H
#define VDBHIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VDB_L2SQR 0
#define VDB_COSINE 1

#define VDB_OK 0
#define VDB_ERR_INVALID 1   /* bad argument (reference: bail!/assert!, e.g. database/mod.rs:427-429) */
#define VDB_ERR_HIP 2       /* HIP runtime error */
#define VDB_ERR_STATE 3     /* e.g. knn_pq without a PQ table */
#define VDB_ERR_NOGPU 4     /* no usable gfx950 device */

typedef struct vdb_index vdb_index;

/* thread-local message of the last failing call on this thread */
const char *vdb_last_error(void);
int vdb_version(void);
int vdb_device_count(int *out);

/* ---- VecSet<f32> + DynamicIndex::new ---------------------------------------------------
 * DynamicIndex::new(dim, dist) (dynamic_index.rs:17-19) -> an empty Flat index whose VecSet
 * (vec_set.rs:15-20) lives row-major in HBM on `device_id`. */
int vdb_index_create(int device_id, uint64_t dim, int dist, vdb_index **out);
int vdb_index_destroy(vdb_index *idx);
/* IndexIter::len / dim (index_algorithm/mod.rs:35-52), DynamicIndex::dist (:37-42) */
int vdb_index_len(const vdb_index *idx, uint64_t *out);
int vdb_index_dim(const vdb_index *idx, uint64_t *out);
int vdb_index_dist(const vdb_index *idx, int *out);
/* Index<usize> (vec_set.rs:22-30): copy row i to out[dim] */
int vdb_index_row(const vdb_index *idx, uint64_t i, float *out);
/* DynamicIndex::add / batch_add for Flat = VecSet::push (dynamic_index.rs:44-58, vec_set.rs:113-118);
 * for an index that currently has an HNSW graph = HNSWIndex::add (hnsw_index.rs:538-572) with
 * levels drawn from the index's own RNG stream.  rows is n x dim row-major; *first_id = id of rows[0]. */
int vdb_index_add(vdb_index *idx, const float *rows, uint64_t n, uint64_t *first_id);
/* same, rows already resident in HBM (no host copy is kept until one is needed) */
int vdb_index_add_device(vdb_index *idx, const void *d_rows, uint64_t n, uint64_t *first_id);
/* VecSet::swap_remove (vec_set.rs:131-137); Flat only (metadata_vec_table.rs:163-187) */
int vdb_index_swap_remove(vdb_index *idx, uint64_t i);
/* ---- bulk removal: MetadataVecTable::delete (metadata_vec_table.rs:163-187) as ONE call --------------------------------------
 * Removing the rows R (m of them) means swap_remove on every one of them in DESCENDING order; the state after that sequence is
 * what these calls work with.  With n' = n - m, its net effect is a list of moves (dst, src): the row that was at src >= n' is
 * now at dst < n', every other surviving row kept its place, and there are exactly |R below n'| moves.
 * vdb_remove_plan: host utility, works without a GPU (like vdb_merge_topk).  rows [m] must be strictly ascending and below n; anything
 * else is VDB_ERR_INVALID with a message, and nothing is written.  out_dst / out_src (room for m entries each) receive the moves in
 * the order the replayed sequence makes them (descending dst), *out_moves their number; out_dst = out_src = NULL: the number alone.
 * vdb_index_remove_rows: removes the LOCAL rows `rows` (same rules; id_offset plays no part) from the index in one pass -- one launch
 * moves the rows and their norms (csrc/k_remove.hip), one launch per live mirror rewrites the touched 16-row tiles, one stream
 * synchronisation for the whole call -- and leaves exactly the state the swap_remove sequence leaves: same rows in the same order,
 * the 8-bit / fp16 / split-bf16 mirrors kept in step (not rebuilt), masks made before it stale (VDB_ERR_STATE).  The last three
 * arguments return the plan, so that the caller can permute whatever it keeps per row (meta[dst] = meta[src], then truncate to
 * n'); all three may be NULL.  Write-side.  Flat only, refused like vdb_index_swap_remove under an HNSW graph, a PQ table or IVF
 * clusters.  An invalid list or a failed allocation leaves the index exactly as it was; m == 0 changes nothing (masks stay valid);
 * m == n leaves an empty index. */
int vdb_remove_plan(uint64_t n, const uint64_t *rows, uint64_t m, uint64_t *out_dst, uint64_t *out_src, uint64_t *out_moves);
int vdb_index_remove_rows(vdb_index *idx, const uint64_t *rows, uint64_t m, uint64_t *out_dst, uint64_t *out_src, uint64_t *out_moves);
/* ---- in-place update: new vectors for many rows as ONE call (no counterpart in the reference) --------------------------------------
 * The reference can only delete a row and add it again, which gives the row a new id, moves an unrelated row into the hole and makes
 * every mask stale.  These calls replace the VECTORS of the rows R (m of them) where they are; afterwards every search answers exactly
 * as it would on a table built with those rows replaced.
 * vdb_update_plan: host utility, works without a GPU (like vdb_remove_plan).  rows [m] must be distinct and below n (n < 2^32), in any
 * order; a NULL rows with m > 0, a row at or past n or a duplicate is VDB_ERR_INVALID with a message, and nothing is written.  out_tiles
 * (room for min(m, ceil(n / 16)) entries) receives the 16-row mirror tiles rows[j] / 16 the update touches, ascending and distinct,
 * *out_n_tiles their number; out_tiles = NULL: the number alone.
 * vdb_index_update_rows: vecs is m x dim row-major on the host, vecs[j] the new vector of LOCAL row rows[j] (same rules; id_offset plays
 * no part).  One launch scatters the rows and their norms (csrc/k_update.hip; the norms are the strict fold that vdb_index_add caches, so
 * they are bit-identical to those of a table built from the updated rows), one launch per live mirror rewrites the touched 16-row tiles:
 *   - split-bf16 mirror: rewritten in step;
 *   - fp16 mirror: rewritten in step, the measured rounding error of the new rows folded into its error terms, while the largest row
 *     norm still fits the mirror's scale; dropped and rebuilt by its next use when it does not, or when the mirror was behind the table;
 *   - 8-bit mirror: tiles, codes and row constants rewritten with the current mean / lambdas (they bound any row; only the tightness
 *     of the bound depends on them), not rebuilt; dropped when it was behind the table;
 *   - the row-major fp16 / 8-bit images of the HNSW walk and the IVF scan are dropped.
 * Host vectors are staged through a bounded workspace buffer (64 MiB at a time), never through an allocation the size of the input.
 * The row count, id_offset and every label column are untouched, and masks made BEFORE the call stay valid: a mask is a set of rows
 * and the set did not change (their cached copies of the 8-bit row constants are rebuilt by the next call that needs them).
 * "update_calls" / "update_rows" of vdb_get_stat count the calls and the rows.  Write-side.  Flat only, refused under an HNSW graph, a PQ
 * table or IVF clusters with a message each (clear them first), and on a VecSet<u8> index (f32 rows only).  An invalid list, a refusal
 * or a failed allocation leaves the index exactly as it was; m == 0 changes nothing and counts nothing.
 * vdb_index_update_rows_device: the same with the vectors already in HBM on the index's GPU (16-byte aligned); rows stays a host array.
 * The call returns synchronised; no host copy of the rows is kept until one is needed. */
int vdb_update_plan(uint64_t n, const uint64_t *rows, uint64_t m, uint32_t *out_tiles, uint64_t *out_n_tiles);
int vdb_index_update_rows(vdb_index *idx, const uint64_t *rows, uint64_t m, const float *vecs /* m x dim, host */);
int vdb_index_update_rows_device(vdb_index *idx, const uint64_t *rows /* host */, uint64_t m, const void *d_vecs);
/* row sharding: ids reported by knn* are local_row + offset */
int vdb_index_set_id_offset(vdb_index *idx, uint64_t offset);
/* calc_dist (pyo3/mod.rs:43-48): one distance, evaluated on the GPU in reference order */
int vdb_calc_dist(int device_id, const float *a, const float *b, uint64_t n, int dist, float *out);

/* ---- u8 scalar (DistanceScalar for u8, distance/mod.rs:79-95) ---------------------------
 * Every u8 element is converted with `as f32` (exact) before the f32 folds, so a VecSet<u8> index equals the f32
 * index of the converted rows bit for bit.  On an f32 index vdb_index_add_u8 converts and forwards (f32 rows in HBM); on an
 * index made by vdb_index_create_u8 it stores the bytes as they are. */
/* VecSet<u8> index (scalar.rs:117-119): rows stay at ONE byte per element in HBM (a quarter of the f32 bytes); the kernels
 * widen on the fly, the MFMA mirrors hold u8 values exactly.  Serves Flat search (vdb_flat_knn / vdb_flat_knn_u8, swap_remove,
 * row); PQ / HNSW / IVF need an f32 table, as in the reference (DynamicIndex instantiates f32 only, dynamic_index.rs:11-14).
 * Rows are added with vdb_index_add_u8; vdb_index_row returns them widened, vdb_index_row_u8 as stored. */
int vdb_index_create_u8(int device_id, uint64_t dim, int dist, vdb_index **out);
int vdb_index_row_u8(const vdb_index *idx, uint64_t i, uint8_t *out);
int vdb_index_is_u8(const vdb_index *idx, int *out);
int vdb_calc_dist_u8(int device_id, const uint8_t *a, const uint8_t *b, uint64_t n, int dist, float *out);
int vdb_index_add_u8(vdb_index *idx, const uint8_t *rows, uint64_t n, uint64_t *first_id);
int vdb_flat_knn_u8(vdb_index *idx, const uint8_t *queries, uint64_t nq, uint64_t dim, uint64_t k, uint64_t *out_idx,
                    float *out_dist, uint64_t *out_count);

/* ---- FlatIndex::knn (flat_index.rs:48-57), batched over nq queries --------------------
 * Any k: up to min(k, len) = 1024 results come from the register-resident select, beyond that from a full
 * (distance, index) radix sort per query.  More than 64 queries in one call are served 128 per corpus pass
 * (k_flat_gemm), fewer 2 x 32 per pass (k_flat_mfma); results do not depend on the batching. */
int vdb_flat_knn(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, uint64_t k,
                 uint64_t *out_idx, float *out_dist, uint64_t *out_count);
/* device-resident queries and outputs (out_idx u64[nq*k], out_dist f32[nq*k], out_count u64[nq]);
 * synchronises `stream` once at the end (certification read-back). */
int vdb_flat_knn_device(vdb_index *idx, const void *d_queries, uint64_t nq, uint64_t dim, uint64_t k,
                        void *d_out_idx, void *d_out_dist, void *d_out_count, void *stream);
/* The same call in two halves, for hosts that keep several independent query batches in flight (bench.rs:410-418 loops over
 * queries; a serving host loops over batches): _begin enqueues the whole search on one of the index's streams, ordered behind
 * `stream` by an event (no host wait), and returns a pending-call handle; _end waits for it, redoes uncertified queries and
 * frees the handle (also when it reports an error).  With begin(i+1) issued before end(i) the corpus passes of consecutive
 * batches run back to back and the exact stage of one batch overlaps the query preparation of the next.  Every begun call must
 * be ended before the index is destroyed or written to; outputs and query buffers of a pending call must stay untouched. */
typedef struct vdb_pending vdb_pending;
int vdb_flat_knn_device_begin(vdb_index *idx, const void *d_queries, uint64_t nq, uint64_t dim, uint64_t k, void *d_out_idx,
                              void *d_out_dist, void *d_out_count, void *stream, vdb_pending **out);
int vdb_flat_knn_device_end(vdb_pending *pending);
/* ---- exact range search over the Flat rows ------------------------------------------------------------------------------------
 * For query q with radius[q]: EVERY row whose distance D(row, q) -- the value FlatIndex::knn computes, bit for bit -- satisfies
 * D <= radius[q], ascending by (distance, index).  This is what MetadataVecTable::search(k, upper_bound) (metadata_vec_table.rs:194-212,
 * the comparison at :209) returns once k is at least the size of that set, without having to guess such a k: the boundary is inclusive,
 * a NaN distance is never inside, a NaN radius gives an empty result, negative radii are compared like any other value.
 * limit > 0: only the first `limit` pairs of every query's list, i.e. exactly search(k = limit, upper_bound = radius); 0 = no limit.
 * Ids are local_row + id_offset.  Works on f32 and VecSet<u8> indexes (queries are f32), L2Sqr and Cosine, any dim.
 * The output is variable-length: the call returns a result object that holds it on the index's device; read the CSR offsets with
 * vdb_range_lims (nq + 1 values, lims[0] = 0, query q owns [lims[q], lims[q + 1])), copy the pairs out with vdb_range_copy
 * (lims[nq] ids and distances each) and release it with vdb_range_destroy (NULL is fine).  The object does not depend on the index
 * after the call (it may outlive writes to it, and the index itself).
 * Read-side and re-entrant on one handle like vdb_flat_knn; nq == 0 and an empty index give empty results, a dim mismatch is an error.
 * Memory: 12 B per returned pair in the result object, and 8 B per pair of scratch while the call runs, on top of the k-NN path's
 * per-call scratch (128 KB per query of a 1024-query round on the 8-bit tier; 24 B per row and query of an 8-query scan pass whose radius
 * takes in the whole table).  A result that does not fit -- device memory, or the per-index ceiling "flat_range_max_results"
 * (vdb_set_param; pairs per call, 0 = none) -- fails the call with an error (vdb_last_error), nothing is returned and nothing aborts:
 * radius = +inf on 1M rows x 1000 queries would be 12 GB; such calls want a limit or fewer queries per call.
 * How it is answered (csrc/k_range.hip, docs/DESIGN_flat.md): tables of at least 16 384 f32 rows whose dimension the 8-bit pass takes run
 * ONE pass of the 8-bit filter with a threshold derived from the radius by the certification bound itself, evaluate every hit exactly and
 * cut at the radius; queries that bound cannot serve (NaN / infinite radius, more than 8192 hits, ...) and all other tables take the
 * strict-order scan, 8 queries per corpus pass.  vdb_flat_set_mode applies (1 = scan only, 2 = the tier wherever the shape allows).
 * vdb_get_stat: "flat_range_queries", "flat_range_i8_queries", "flat_range_scan_queries", "flat_range_hits" (hit-list lengths of the
 * tier's queries; "flat_range_hits_max": the longest of them), "flat_range_results". */
typedef struct vdb_range vdb_range;
int vdb_flat_range(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, const float *radius, uint64_t limit, vdb_range **out);
/* device-resident queries (f32 [nq][dim]) and radii (f32 [nq]); synchronises `stream` first and returns synchronised */
int vdb_flat_range_device(vdb_index *idx, const void *d_queries, uint64_t nq, uint64_t dim, const void *d_radius, uint64_t limit,
                          void *stream, vdb_range **out);
int vdb_range_lims(const vdb_range *r, uint64_t *out_lims);
int vdb_range_copy(const vdb_range *r, uint64_t *out_idx, float *out_dist);
int vdb_range_destroy(vdb_range *r);
/* ---- exact filtered search over the Flat rows: a row mask ------------------------------------------------------------------------
 * A vdb_mask is an allow-list over the LOCAL rows of ONE index: row i is allowed iff (bits[i >> 6] >> (i & 63)) & 1; `bits` holds
 * ceil(n_rows / 64) words, bits at and past n_rows are ignored, and n_rows must equal the index's length (else VDB_ERR_INVALID).
 * vdb_mask_count gives the number m of allowed rows.  id_offset is added to reported ids as everywhere else.
 * A mask belongs to the index it was made for AND to that state of its rows: a call with a mask of another index fails with
 * VDB_ERR_INVALID, a call with a mask made before a later vdb_index_add* / vdb_index_swap_remove with VDB_ERR_STATE (both set
 * vdb_last_error; nothing is computed).  vdb_index_update_rows* changes no row SET: masks made before it stay valid and are applied to
 * the new vectors (the copy of the row constants named below is rebuilt by the next call that needs it).  Creating a mask is read-side; destroy it (NULL is fine) when no call is using it and
 * before the index is destroyed.  Memory on the index's device: n/8 + 4 m bytes, plus 8 B per padded row once a call has run the
 * 8-bit tier under the mask (a copy of that tier's per-row constants in which every disallowed row carries a key of +inf).
 * vdb_flat_knn_filtered: per query the first min(k, m) pairs of FlatIndex::knn over the ALLOWED rows alone -- distances bit-exact,
 * ascending by (distance, id), out_count[q] = min(k, m), slots past the count zero.  Any k, any dim, L2Sqr and Cosine, f32 indexes
 * only: a VecSet<u8> index is VDB_ERR_INVALID ("needs f32 rows").  nq == 0, k == 0 and m == 0 give empty results; PQ / HNSW / IVF
 * state of the index is irrelevant.  Read-side and re-entrant like vdb_flat_knn; the _device form takes device-resident queries and
 * outputs (at most 32768 queries), synchronises `stream` first and returns synchronised.
 * How it is answered (csrc/k_filter.hip, docs/DESIGN_flat.md "Filtered search"): allow-lists of at most "flat_filtered_direct_max"
 * rows (vdb_set_param, per index, default 8192), k > 64, and every table the 8-bit pass does not serve take the DIRECT path: the
 * strict-order scan over the gathered allowed rows, 8 queries per fetch of a row.  Longer lists on tables of at least 16 384 rows
 * run the unfiltered search's 8-bit filter pass with the mask's row constants -- the same kernel over the same bytes -- and its exact
 * stage; a query that stage cannot close is redone by the direct path.  vdb_flat_set_mode applies (1 = direct only, 2 = the tier
 * wherever the shape allows).  The call never touches the unfiltered search's auto-off counters.
 * vdb_get_stat: "flat_filtered_queries", "flat_filtered_direct_queries", "flat_filtered_i8_queries" (queries through the tier),
 * "flat_filtered_fallback_queries" (of those, handed on to the direct path); vdb_prof_get: "flat_filtered_scan", "flat_filtered_i8".
 * vdb_flat_knn_filtered_multi: ONE MASK PER QUERY -- the multi-tenant batch.  Query q is answered exactly as vdb_flat_knn_filtered(idx,
 * query q, 1, dim, k, masks[mask_of[q]], ..) answers it: the first min(k, m) pairs over that mask's allowed rows, bit-exact, ascending
 * by (distance, id), out_count[q] = min(k, m of that mask), slots past the count zero, id_offset added.  `mask_of` is a HOST array of nq
 * indexes into `masks` in both forms, in any order; a mask may serve any number of queries, none included.  Checked before anything is
 * computed or written: EVERY mask of `masks` as for the single-mask call (another index: VDB_ERR_INVALID, stale: VDB_ERR_STATE),
 * mask_of[q] >= n_masks (VDB_ERR_INVALID), a VecSet<u8> index (VDB_ERR_INVALID); the _device form refuses more than 32768 queries.
 * nq == 0, k == 0 and n_masks == 0 with nq == 0 give empty results, a mask with m == 0 count 0 for its queries.  Read-side and
 * re-entrant; the _device form synchronises `stream` first and returns synchronised; no auto-off counter is touched.
 * How it is answered (csrc/multi_plan.hpp, k_filter.hip, docs/DESIGN_flat.md 4.1k): the queries are bucketed by mask on the host.
 *   GROUPED direct path -- masks with m <= "flat_filtered_direct_max" when k <= 1024: all such buckets of the call are scanned by ONE
 *   launch per chunk of queries (k_scan_gather_grouped: a workgroup per (mask, group of <= 8 of its queries, tile of 256 allowed rows)),
 *   followed by one selection pass and one finalize for the chunk.
 *   Single-mask machinery -- every other bucket (masks longer than "flat_filtered_direct_max", any mask when k > 1024): its queries are
 *   gathered into a contiguous block, answered as vdb_flat_knn_filtered answers them (the 8-bit tier with the mask's row constants, or
 *   the direct path) and scattered back.  vdb_flat_set_mode applies as above: with mode 1 long masks take the direct path per mask.
 * The "flat_filtered_*" counters advance as if the per-mask calls had been made; "flat_filtered_multi_calls" counts these calls,
 * "flat_filtered_grouped_queries" the queries the grouped launch answered; vdb_prof_get "flat_filtered_scan_grouped" is that kernel.
 * vdb_flat_range_filtered: vdb_flat_range over the allowed rows alone -- every ALLOWED row with D <= radius[q]; everything else as
 * documented there (f32 and VecSet<u8> indexes, the same tiers and counters).
 * vdb_flat_range_filtered_multi: the range search with ONE MASK PER QUERY.  Query q's slice of the result is exactly what
 * vdb_flat_range_filtered(idx, query q, 1, dim, &radius[q], limit, masks[mask_of[q]], ..) returns: every ALLOWED row with
 * D <= radius[q], D bit-exact, ascending by (distance, id), the first `limit` pairs when limit > 0, id_offset added; a NaN distance is
 * never inside and a NaN radius gives an empty slice.  The result object is vdb_flat_range's.  `mask_of` is a HOST array in both forms,
 * in any order; a mask may serve any number of queries, none included.  Checked before anything is computed, with *out left NULL and
 * every counter unchanged: EVERY mask of `masks` as for the single-mask call (another index: VDB_ERR_INVALID, stale: VDB_ERR_STATE),
 * mask_of[q] >= n_masks (VDB_ERR_INVALID), a dim mismatch; the _device form refuses more than 32768 queries.  nq == 0 gives an empty
 * result, a mask with m == 0 empty slices.  "flat_range_max_results" and a device-memory failure fail the whole call as documented for
 * vdb_flat_range: nothing is returned, nothing aborts, and the counters below are as the call found them ("flat_range_hits_max", a
 * high-water mark, excepted).  f32 and VecSet<u8> indexes.  Read-side and re-entrant; the _device form synchronises `stream` first and
 * returns synchronised.
 * How it is answered (csrc/multi_plan.hpp, k_filter.hip, docs/DESIGN_flat.md 4.1n): the queries are bucketed by mask on the host.
 *   GROUPED path -- f32 indexes, masks with m <= "flat_filtered_direct_max", in every vdb_flat_set_mode: ONE launch per chunk of queries
 *   (k_range_gather_grouped: a workgroup per (mask, group of <= 8 of its queries, tile of 256 allowed rows)) folds the gathered rows,
 *   tests D <= radius on the spot and appends the pair keys of the pairs inside to the query's row; one sort and one append per chunk.
 *   Per-mask route -- every other bucket (longer masks, every bucket of a u8 index): its queries and radii are gathered into a block and
 *   answered by vdb_flat_range_filtered's machinery (8-bit tier with the mask's row constants, or the scan of all rows).
 *   One pool of sorted keys and one gather into the result for the whole call.
 * vdb_get_stat: "flat_range_queries" += nq and "flat_range_results" as usual; "flat_range_multi_calls" counts these calls,
 * "flat_range_grouped_queries" the queries the grouped launch answered (they count in neither "flat_range_i8_queries" nor
 * "flat_range_scan_queries"; the per-mask route advances those as the per-mask calls would).  vdb_prof_get
 * "flat_range_gather_grouped" is the grouped kernel (bytes: the rows its work items fetch x dim x 4).
 * Not covered: sharded and replica contexts, _begin / _end pipelining, filtered PQ / HNSW / IVF searches, k-NN on u8 indexes, a
 * grouped path for u8 rows, the single-mask range call through the gathered path. */
typedef struct vdb_mask vdb_mask;
int vdb_mask_create(vdb_index *idx, const uint64_t *bits, uint64_t n_rows, vdb_mask **out);
int vdb_mask_count(const vdb_mask *m, uint64_t *out);
int vdb_mask_destroy(vdb_mask *m);
int vdb_flat_knn_filtered(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, uint64_t k, const vdb_mask *mask,
                          uint64_t *out_idx, float *out_dist, uint64_t *out_count);
int vdb_flat_knn_filtered_device(vdb_index *idx, const void *d_queries, uint64_t nq, uint64_t dim, uint64_t k, const vdb_mask *mask,
                                 void *d_out_idx, void *d_out_dist, void *d_out_count, void *stream);
int vdb_flat_knn_filtered_multi(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, uint64_t k, const vdb_mask *const *masks,
                                uint64_t n_masks, const uint32_t *mask_of, uint64_t *out_idx, float *out_dist, uint64_t *out_count);
int vdb_flat_knn_filtered_multi_device(vdb_index *idx, const void *d_queries, uint64_t nq, uint64_t dim, uint64_t k,
                                       const vdb_mask *const *masks, uint64_t n_masks, const uint32_t *mask_of, void *d_out_idx,
                                       void *d_out_dist, void *d_out_count, void *stream);
int vdb_flat_range_filtered(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, const float *radius, uint64_t limit,
                            const vdb_mask *mask, vdb_range **out);
int vdb_flat_range_filtered_multi(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, const float *radius, uint64_t limit,
                                  const vdb_mask *const *masks, uint64_t n_masks, const uint32_t *mask_of, vdb_range **out);
int vdb_flat_range_filtered_multi_device(vdb_index *idx, const void *d_queries, uint64_t nq, uint64_t dim, const void *d_radius,
                                         uint64_t limit, const vdb_mask *const *masks, uint64_t n_masks, const uint32_t *mask_of,
                                         void *stream, vdb_range **out);
/* ---- row labels on the device: masks built from them without a host pass ----------------------------------------------------------
 * An index has VDB_LABEL_COLUMNS logical label columns of uint32_t, one value per LOCAL row: the filterable attributes of the rows as
 * integer codes (the host keeps the dictionary; lab_1806_vec_db_amd/labels.py is one).  A column is allocated by its first write
 * (4 B per row in HBM, grown with the rows); a column never written reads as VDB_LABEL_NONE for every row and takes no memory.  The
 * allocated columns follow every change of the row set, on f32 and VecSet<u8> indexes alike: rows added by any call get
 * VDB_LABEL_NONE in every column, vdb_index_swap_remove and vdb_index_remove_rows move the labels with the rows.  Labels are
 * independent of PQ / HNSW / IVF state, and writing them does NOT make masks stale (a mask is a set of rows).
 * vdb_index_labels_set: rows [first_row, first_row + count) of one column from a host array.  Write-side with respect to mask
 * creation from labels (no vdb_mask_create_where* call may run on the index meanwhile); searches are not affected.  column >=
 * VDB_LABEL_COLUMNS or a range past vdb_index_len is VDB_ERR_INVALID and nothing is written; count == 0 is fine and allocates nothing.
 * vdb_index_labels_get: reads a range back (VDB_LABEL_NONE for a column never written); same errors; read-side.
 * vdb_mask_create_where: the mask of the rows r with label[columns[t]][r] == codes[t] for EVERY t < n_terms -- a conjunction of
 * equalities.  Plain equality: a term with code VDB_LABEL_NONE matches the unlabelled rows (all rows, for a column never written);
 * n_terms == 0 allows every row; two terms on one column with different codes give an empty mask.  More than VDB_MASK_MAX_TERMS terms
 * or a column >= VDB_LABEL_COLUMNS is VDB_ERR_INVALID.  Read-side, like vdb_mask_create, and the result IS the object vdb_mask_create
 * would have made from the equivalent bits: same owner / staleness rules, same lazily built row constants, usable with every call that
 * takes a vdb_mask.  An empty index gives a mask with m = 0.
 * vdb_mask_create_where_many: n_masks masks in ONE call; mask g's terms are entries [term_lims[g], term_lims[g + 1]) of columns /
 * codes, term_lims[0] == 0 and non-decreasing (n_masks + 1 entries); `out` has room for n_masks handles.  All-or-nothing: everything
 * is validated before anything is launched, and on any error every mask built so far is destroyed, every out[g] is NULL and the index
 * is unchanged.  n_masks == 0 succeeds.  The single form is this call with one mask.
 * vdb_mask_rows: reads a mask of either constructor back -- out_bits: ceil(n_rows / 64) words, out_ids: the m allowed rows, ascending
 * (vdb_mask_count gives m); either pointer may be NULL.
 * How the masks are built (csrc/k_labels.hip, docs/DESIGN_flat.md 4.1l): per chunk of up to 1024 masks, k_mask_rows<MaskEq> -- a 64-lane wave
 * owns one mask word, a lane one row; the lane compares its row's value in every term column and the wave's ballot is the word --
 * counts the allowed rows per workgroup, k_mask_scan turns the counts into offsets, one read-back of the totals sizes the allow-lists,
 * and k_mask_ids writes every allowed row at its offset: ascending without a sort.  Traffic per mask: 4 B x terms x rows read, rows / 8
 * + 4 m written.  vdb_prof_get "mask_where" times the three kernels; vdb_get_stat "mask_where_masks" counts the masks built this way,
 * "label_columns" the allocated columns ("hbm_bytes_per_row" includes them).
 * SET AND RANGE TERMS (vdb_mask_create_where_sets / _many; csrc/mask_sets.hpp, k_mask_rows<MaskAll>, docs/DESIGN_flat.md 4.1m): a term is
 * {column, lo, hi, flags, bitmap} and a mask the conjunction of its terms.  A row whose label in the column is v matches the term
 *   - when v == VDB_LABEL_NONE (no value, or a column never written): iff flags has VDB_TERM_NONE; VDB_TERM_NEGATE never inverts this;
 *   - otherwise: inside = lo <= v <= hi and (no bitmap, or bit (v - lo) of the bitmap); it matches iff inside != (flags has VDB_TERM_NEGATE).
 * Any predicate on one attribute is a set of its codes plus "rows without a value": the host evaluates the predicate over its dictionary
 * (one entry per distinct value), the device tests one bit per row -- IN, NOT IN, !=, order comparisons, existence.  Un-interned integers
 * (timestamps) need no bitmap: [lo, hi] is the range.  The equality term (c, code) of vdb_mask_create_where is {lo = hi = code, flags 0};
 * its term (c, VDB_LABEL_NONE) is {lo = 1, hi = 0, flags VDB_TERM_NONE}; both give bit-identical masks.
 * term_lims as in vdb_mask_create_where_many.  set_lims: n_terms + 1 word offsets into set_words, set_lims[0] == 0, non-decreasing; term t
 * carries a bitmap iff set_lims[t + 1] > set_lims[t], must then have lo <= hi and exactly ceil((uint64_t(hi) - lo + 1) / 64) words; bit j
 * of the bitmap stands for code lo + j, bits past hi - lo in the last word are ignored.  set_lims == NULL: no term has a bitmap
 * (set_words is not read).  A term without a bitmap and lo > hi is the empty range: legal, it matches nothing, or with VDB_TERM_NEGATE
 * every labelled row.  hi == 0xFFFFFFFF is legal (a labelled row never carries that value).  n_terms == 0 allows every row.
 * Everything is checked before anything is launched; VDB_ERR_INVALID with a message, every out[g] NULL, index and counters unchanged for:
 * more than VDB_MASK_MAX_TERMS terms in a mask, a column >= VDB_LABEL_COLUMNS, unknown flag bits, set_lims not starting at 0 or
 * decreasing, a bitmap on a term with lo > hi, a bitmap whose length does not match its span (computed in 64 bits), more than
 * VDB_MASK_MAX_SET_BITS bitmap bits in the call.  n_masks == 0 succeeds.  Read-side, all-or-nothing and chunked like
 * vdb_mask_create_where_many; the term table and all bitmaps of the call are uploaded once.  The result is the same vdb_mask object:
 * owner / staleness rules, lazily built row constants, f32 and VecSet<u8> indexes, every call that takes a vdb_mask.  Traffic per mask:
 * 4 B x terms x rows read as before plus one 8-byte bitmap gather per in-range row and bitmap term (from a block that stays cached).
 * vdb_get_stat "mask_where_set_masks" counts the masks built by these two calls ("mask_where_masks" keeps counting the equality calls
 * only); vdb_prof_get "mask_where_sets" times k_mask_rows<MaskAll> with its scan and ids launches.
 * OR OF CONJUNCTIONS (vdb_mask_create_where_any / _many; csrc/mask_any.hpp, k_mask_rows<MaskAny>, docs/DESIGN_flat.md 4.1o): a mask is the
 * OR of up to VDB_MASK_MAX_CLAUSES clauses, a clause the AND of up to VDB_MASK_MAX_TERMS terms, a term exactly the set / range term above
 * with the same match -- a filter expression in disjunctive normal form, NOT pushed down to the terms (toggling VDB_TERM_NEGATE and
 * VDB_TERM_NONE complements a term exactly).  Clause c's terms are entries [clause_lims[c], clause_lims[c + 1]) of the term arrays
 * (n_clauses + 1 entries, clause_lims[0] == 0, non-decreasing); in the _many form mask g's clauses are [mask_lims[g], mask_lims[g + 1])
 * (n_masks + 1 entries, the same rules); set_lims / set_words as above, over all terms of the call.
 *   - n_clauses == 0 gives the EMPTY mask (m = 0) -- unlike n_terms == 0 of the conjunction calls, which allows every row;
 *   - a clause with zero terms allows every row;
 *   - a mask of ONE clause is bit-identical to the vdb_mask_create_where_sets mask of that clause's terms.
 * Everything is checked before anything is launched; VDB_ERR_INVALID with a message, every out[g] NULL, index and counters unchanged for:
 * more than VDB_MASK_MAX_CLAUSES clauses in a mask, more than VDB_MASK_MAX_TERMS terms in a clause, mask_lims / clause_lims not starting
 * at 0 or decreasing, every argument error vdb_mask_create_where_sets_many lists, more than VDB_MASK_MAX_SET_BITS bitmap bits in the
 * call.  n_masks == 0 succeeds.  Read-side, all-or-nothing and chunked like the other _many calls; terms, clause limits and bitmaps of
 * the call are uploaded once.  One kernel pass per chunk: a wave owns a mask word and loops over the mask's clauses, so a column is
 * read once per term that names it (4 B x terms x rows over all clauses, repeated reads of a column served by cache).  The
 * result is the same vdb_mask object: owner / staleness rules, lazily built row constants, f32 and VecSet<u8> indexes, every call that
 * takes a vdb_mask.  vdb_get_stat "mask_where_any_masks" counts the masks built by these two calls (the older counters keep counting
 * only their own calls); vdb_prof_get "mask_where_any" times k_mask_rows<MaskAny> with its scan and ids launches.
 * MASK ALGEBRA (vdb_mask_combine; k_mask_combine): out = the AND (VDB_MASK_OP_AND) or OR (VDB_MASK_OP_OR) over n_in (1 .. 8) masks of
 * this index, input i complemented first when invert != NULL and invert[i] != 0; n_in == 1 with invert set is NOT.  For what the
 * columns cannot express: inputs may come from any constructor, host-built masks (vdb_mask_create) included.  A complement is taken
 * within the index's rows: bits at and past vdb_index_len are clear in the result.  Every input is checked as the filtered searches
 * check a mask -- a mask of another index: VDB_ERR_INVALID, a stale mask: VDB_ERR_STATE -- and n_in == 0, n_in > 8, a NULL input or
 * an unknown op is VDB_ERR_INVALID; nothing is computed on error and *out is NULL.  Read-side; the result is an ordinary mask.
 * vdb_get_stat "mask_combine_masks" counts them; vdb_prof_get "mask_combine" times k_mask_combine with its scan and ids launches.
 * ONE COLUMN GROUPED BY CODE (vdb_mask_create_partition, vdb_index_label_counts; csrc/mask_partition.hpp, k_mask_partition,
 * k_label_counts, docs/DESIGN_flat.md 4.1p): the masks of many values of one column, or the rows per value, from ONE read of the column
 * per chunk of 1024 codes instead of one read per value.
 * vdb_mask_create_partition: out[j] = the mask of the rows whose label in `column` equals codes[j] -- bit-identical (words, ascending
 * allow-list, m) to what vdb_mask_create_where(idx, &column, &codes[j], 1, ...) makes.  VDB_LABEL_NONE is a legal code (the unlabelled
 * rows; every row of a column never written); a code no row carries gives m = 0; the codes come in any order, arbitrarily sparse, and
 * the output order follows the input order.  The codes of a call are DISTINCT.  Everything is checked before anything is launched;
 * VDB_ERR_INVALID with a message, every out[j] NULL, index and counters unchanged for: a code named twice, column >= VDB_LABEL_COLUMNS,
 * a NULL array with n_codes > 0, n_codes >= 2^28 (`out` is not written then).  n_codes == 0 succeeds.  All-or-nothing on a
 * device-memory failure.  Read-side and re-entrant.  Each result is an ordinary vdb_mask: owner / staleness rules, lazily built row
 * constants, f32 and VecSet<u8> indexes, every call that takes a vdb_mask (vdb_mask_combine and vdb_mask_rows included), destroyed on
 * its own with vdb_mask_destroy, in any order.
 *   STORAGE: the masks of one chunk share two device allocations, one for their bit words and one for their allow-lists (the codes are
 *   distinct, so the masks are disjoint and the lists of a chunk hold at most n entries together); every mask holds a reference, and
 *   ONE SURVIVING MASK KEEPS ITS CHUNK'S TWO ALLOCATIONS ALIVE -- up to 1024 x ceil(n / 64) x 8 B of bit words.  A caller that keeps
 *   a few masks of a large partition for long should build those with vdb_mask_create_where.  Every mask starts 256-B aligned inside
 *   its slab, as a buffer of its own would.  (Under VDB_EFENCE every mask keeps allocations of its own.)
 *   How: the host sorts a chunk's codes; a workgroup stages the sorted table in LDS, a lane loads its row's code once and
 *   binary-searches it, and the wave walks its distinct codes -- the ballot of "my code is this one" is that mask's word.  The bit
 *   words and block counts are cleared first; k_mask_scan and k_mask_ids follow as for every other constructor.
 * vdb_index_label_counts: out_counts[j] = the number of rows allowed by `mask` (NULL: every row) whose label in `column` equals
 * codes[j]; the same code rules and errors (VDB_LABEL_NONE counts the unlabelled rows).  The mask is checked as the filtered searches
 * check one: another index is VDB_ERR_INVALID, a stale mask VDB_ERR_STATE; out_counts is not written on error.  Read-side and
 * re-entrant.  A workgroup keeps a chunk's counters in LDS and flushes the non-zero ones with integer adds; an index has fewer than
 * 2^32 rows, so no counter overflows.
 * vdb_get_stat "mask_partition_masks" counts the masks vdb_mask_create_partition built, "label_count_calls" the
 * vdb_index_label_counts calls (the older counters keep counting only their own calls); vdb_prof_get "mask_partition" times
 * k_mask_partition with its clears, scan and ids launches, "label_counts" k_label_counts with its clear.
 * KEY LOOKUP (vdb_index_label_lookup, vdb_label_lookup_plan; csrc/lookup_plan.hpp, csrc/k_lookup.hip, docs/DESIGN_flat.md 4.1aa): from a
 * list of codes to rows -- what an upsert or a fetch by a key field needs -- without a mask per code.
 * vdb_index_label_lookup: out_counts[j] = the number of rows whose label in `column` equals codes[j]; out_first[j] = the lowest such LOCAL
 * row, VDB_ROW_NONE when there is none.  The code rules are those of vdb_mask_create_partition / vdb_index_label_counts: distinct codes,
 * any order, arbitrarily sparse, VDB_LABEL_NONE (the unlabelled rows) allowed among them; a column never written reads as VDB_LABEL_NONE
 * in every row, without a load.  Refused with VDB_ERR_INVALID, outputs and every counter untouched: column >= VDB_LABEL_COLUMNS, a code
 * named twice, a NULL pointer with n_codes > 0 (n_codes >= 2^28 as well).  n_codes == 0 and an empty index (counts 0, VDB_ROW_NONE)
 * succeed.  Read-side, re-entrant on one handle, returns synchronised; f32 and VecSet<u8> indexes alike.  There is NO _device form: the
 * codes come from a dictionary the host keeps (value -> code), so the list is on the host when the call is made.
 *   How: a wave per 64-row word, grid-strided from 8 workgroups per CU ("label_lookup_max_blocks": another grid cap).  A lane loads its
 *   row's code once and resolves it to a position of the list; the wave walks its distinct positions by ballot, and one lane per
 *   distinct position adds the popcount and takes the min with its row.  Both outputs come from integer atomicAdd / atomicMin alone:
 *   the answer does not depend on the order of waves; no float, no second pass, no sort on the device.
 *   Two routes, chosen on the host.  SORTED (route 0): any codes, in chunks of 1024 -- the chunk's sorted table, counters and firsts in
 *   LDS, a binary search per row, one read of the column per chunk.  DIRECT (route 1): a table slot_of[code - base] of `span` u32 in
 *   workspace memory (span = highest - lowest + 1 over the codes other than VDB_LABEL_NONE, which never enters the table), filled by a
 *   scatter kernel; one gather per row and ONE read of the column whatever n_codes is.  Taken when n_codes > 1024 and 4 B x span <=
 *   "label_lookup_table_bytes" (vdb_set_param; default 64 MiB; a cap on scratch memory, not a tuned value; 0: sorted route only).
 * vdb_label_lookup_plan: host utility, works without a GPU: the argument check of (column, codes, n_codes) and, for table_bytes, the
 *   route, base, span and the number of column reads (chunks: ceil(n_codes / 1024) sorted, 1 direct, 0 without codes).  Any output may be
 *   NULL; on an error nothing is written.
 * vdb_get_stat: "label_lookup_calls" (accepted calls), "label_lookup_codes" (codes they named), "label_lookup_direct" (calls that ran
 * the direct route), "label_lookup_passes" (reads of the column, summed; none on an empty index).  vdb_prof_get "label_lookup" times the
 * fills, the table kernel and the lookup kernels.
 * Not covered: sharded and replica contexts, normal forms past VDB_MASK_MAX_CLAUSES clauses in one call (combine the parts with
 * vdb_mask_combine), partitions by more than one column, labels in bincode files, filtered k-NN on VecSet<u8> indexes. */
#define VDB_LABEL_COLUMNS 16
#define VDB_LABEL_NONE 0xFFFFFFFFu
#define VDB_MASK_MAX_TERMS 8
int vdb_index_labels_set(vdb_index *idx, uint32_t column, uint64_t first_row, const uint32_t *codes, uint64_t count);
int vdb_index_labels_get(const vdb_index *idx, uint32_t column, uint64_t first_row, uint64_t count, uint32_t *out);
/* ---- scattered label writes: the metadata of existing rows changed in place (no counterpart in the reference) -----------------------
 * vdb_index_labels_set copies one contiguous range of one column.  These calls write label[columns[c]][row] for rows that are no run,
 * n_cols columns in ONE kernel launch (csrc/k_labels.hip: k_labels_scatter, k_labels_set_mask; docs/DESIGN_flat.md 4.1t) and without a
 * host copy of a column: a lane owns one list entry, loads its row id once and stores one code per column with plain stores.
 * vdb_labels_scatter_plan: host utility, works without a GPU (like vdb_update_plan): the argument check of the list form over a table of
 *   n rows (n <= 2^32) -- n_cols in 1 .. VDB_LABEL_COLUMNS, every column below VDB_LABEL_COLUMNS and named once, rows distinct and below
 *   n, no NULL array with m > 0 -- and the ids as they are uploaded: out_ids32[j] = (uint32_t)rows[j].  out_ids32 may be NULL (check
 *   only).  On any error nothing is written.
 * vdb_index_labels_scatter: label[columns[c]][rows[j]] = codes[c * m + j]; rows are m DISTINCT LOCAL row ids on the host in any order
 *   (a duplicate is refused, as vdb_index_update_rows refuses it), codes [n_cols][m] on the host.  Ids (as u32) and codes are uploaded
 *   once each through workspace buffers: no allocation per call once the workspace has grown.
 * vdb_index_labels_scatter_device: d_ids = m u64 GLOBAL ids (row + id_offset) on the index's GPU, 8-byte aligned, exactly as
 *   vdb_flat_knn_device writes them; d_codes = u32 [n_cols][m] there; `columns` on the host.  Both arrays must be complete when the call
 *   is made (it runs on a stream of the library's).  The ids are range-checked on the device first (one flag read back): an id that is no
 *   row of the index is VDB_ERR_INVALID and nothing is written.  An id named twice with different codes gets one of them, whole; which
 *   one is unspecified.
 * vdb_index_labels_set_mask: label[columns[c]][r] = codes[c] for every row r the mask allows and every c < n_cols.  The list is the
 *   mask's own id list on the device and the (column, code) pairs travel as kernel arguments: nothing is uploaded.  A mask of another
 *   index is VDB_ERR_INVALID and a stale one VDB_ERR_STATE, as in the filtered searches.
 * Rules of all three:
 *   Check before write: everything is checked before anything is written or allocated.  On VDB_ERR_INVALID (and on VDB_ERR_STATE for a
 *   stale mask) no column has changed, no column has come to life ("label_columns" is unchanged) and no counter has moved.
 *   First write allocates: a target column never written before comes to life as in vdb_index_labels_set -- allocated for len rows,
 *   VDB_LABEL_NONE everywhere -- and then the listed rows are written.
 *   Empty calls: m == 0 (a mask without rows) succeeds, writes and allocates nothing and counts nothing; n_cols == 0 with m > 0 is
 *   VDB_ERR_INVALID, as are n_cols > VDB_LABEL_COLUMNS, a column >= VDB_LABEL_COLUMNS, a column named twice, a row >= len and a NULL
 *   array with m > 0.
 *   Codes: any u32; VDB_LABEL_NONE is legal and takes the value away from the row.
 *   They work on f32 and VecSet<u8> indexes alike.
 *   Write-side with respect to everything that reads label columns (vdb_mask_create_where*, vdb_mask_create_partition,
 *   vdb_index_label_counts, the grouped searches); they return synchronised.  They do NOT make masks stale: masks made before the call
 *   stay valid and keep selecting the rows they selected (a mask is a set of rows), vectors and mirrors are untouched, PQ / HNSW / IVF
 *   state is untouched.
 * vdb_get_stat: "labels_scatter_calls" (calls of the three that wrote rows: m > 0, not refused), "labels_scatter_rows" (rows they
 * wrote), "labels_scatter_span" (list entries one launch covers before its grid-stride loop wraps: 256 x 8 blocks per CU, or 256 x
 * "labels_scatter_max_blocks" when vdb_set_param gave one).  vdb_prof_get "labels_scatter" times the two kernels.
 * Not covered: the sharded contexts. */
int vdb_labels_scatter_plan(uint64_t n, const uint64_t *rows, uint64_t m, const uint32_t *columns, uint64_t n_cols, uint32_t *out_ids32);
int vdb_index_labels_scatter(vdb_index *idx, const uint64_t *rows /* host, LOCAL, distinct */, uint64_t m, const uint32_t *columns,
                             uint64_t n_cols, const uint32_t *codes /* host, [n_cols][m] */);
int vdb_index_labels_scatter_device(vdb_index *idx, const void *d_ids /* u64 GLOBAL ids, 8-B aligned */, uint64_t m,
                                    const uint32_t *columns /* host */, uint64_t n_cols, const void *d_codes /* u32 [n_cols][m] */);
int vdb_index_labels_set_mask(vdb_index *idx, const vdb_mask *mask, const uint32_t *columns, const uint32_t *codes /* one per column */,
                              uint64_t n_cols);
int vdb_mask_create_where(vdb_index *idx, const uint32_t *columns, const uint32_t *codes, uint64_t n_terms, vdb_mask **out);
int vdb_mask_create_where_many(vdb_index *idx, const uint64_t *term_lims, const uint32_t *columns, const uint32_t *codes,
                               uint64_t n_masks, vdb_mask **out);
#define VDB_TERM_NEGATE 1u
#define VDB_TERM_NONE 2u
#define VDB_MASK_MAX_SET_BITS (1ull << 27) /* bitmap bits per call, 16 MiB */
int vdb_mask_create_where_sets(vdb_index *idx, const uint32_t *columns, const uint32_t *lo, const uint32_t *hi, const uint32_t *flags,
                               const uint64_t *set_lims, const uint64_t *set_words, uint64_t n_terms, vdb_mask **out);
int vdb_mask_create_where_sets_many(vdb_index *idx, const uint64_t *term_lims, const uint32_t *columns, const uint32_t *lo,
                                    const uint32_t *hi, const uint32_t *flags, const uint64_t *set_lims, const uint64_t *set_words,
                                    uint64_t n_masks, vdb_mask **out);
#define VDB_MASK_MAX_CLAUSES 64
int vdb_mask_create_where_any(vdb_index *idx, const uint64_t *clause_lims, uint64_t n_clauses, const uint32_t *columns, const uint32_t *lo,
                              const uint32_t *hi, const uint32_t *flags, const uint64_t *set_lims, const uint64_t *set_words,
                              vdb_mask **out);
int vdb_mask_create_where_any_many(vdb_index *idx, const uint64_t *mask_lims, const uint64_t *clause_lims, const uint32_t *columns,
                                   const uint32_t *lo, const uint32_t *hi, const uint32_t *flags, const uint64_t *set_lims,
                                   const uint64_t *set_words, uint64_t n_masks, vdb_mask **out);
#define VDB_MASK_OP_AND 0
#define VDB_MASK_OP_OR 1
int vdb_mask_combine(vdb_index *idx, int op, const vdb_mask *const *in, const uint8_t *invert, uint64_t n_in, vdb_mask **out);
int vdb_mask_create_partition(vdb_index *idx, uint32_t column, const uint32_t *codes, uint64_t n_codes, vdb_mask **out);
int vdb_index_label_counts(vdb_index *idx, uint32_t column, const vdb_mask *mask, const uint32_t *codes, uint64_t n_codes,
                           uint64_t *out_counts);
#define VDB_ROW_NONE 0xFFFFFFFFFFFFFFFFull /* vdb_index_label_lookup: no row carries the code */
int vdb_label_lookup_plan(uint32_t column, const uint32_t *codes, uint64_t n_codes, uint64_t table_bytes, int *out_route, uint32_t *out_base,
                          uint64_t *out_span, uint64_t *out_chunks);
int vdb_index_label_lookup(vdb_index *idx, uint32_t column, const uint32_t *codes, uint64_t n_codes, uint64_t *out_first /* [n_codes] */,
                           uint64_t *out_counts /* [n_codes] */);
int vdb_mask_rows(const vdb_mask *m, uint64_t *out_bits, uint32_t *out_ids);
/* ---- near-duplicate grouping: a range self-join over the table's own rows and the connected components of its pairs ---------------------
 * "Which rows are copies, or near copies, of each other?"  (csrc/dup_plan.hpp, csrc/flat_dups.hip, csrc/k_components.hip;
 * docs/DESIGN_flat.md 4.1ab.)  The reference has no counterpart; this is the rule.
 *   EDGES.  For every allowed row i (all rows, or the rows of `mask`) take the list vdb_flat_range / vdb_flat_range_filtered returns for
 *     query = row i, radius, limit and the mask: every allowed row j with D(row j, row i) <= radius in the (distance, index) order, the first
 *     `limit` of them when limit > 0.  Every j != i on it is an edge {i, j}.  Edges are undirected: one exists if either end lists the
 *     other, so nothing rests on D being symmetric in its last bit.
 *   GROUPS.  The connected components of the allowed rows under these edges.  This is SINGLE LINKAGE at the radius: A-B and B-C put A and
 *     C into one group even when D(A, C) > radius.
 *   REPRESENTATIVE.  A group is named by its lowest row: out_group[i] = that LOCAL row + id_offset; a row alone in its group gets its own
 *     id, a row outside the mask VDB_ROW_NONE.
 *   What follows from the range search as it stands: a row with a NaN distance to everything is alone; identical rows are linked at
 *     radius 0; a negative radius links nothing; radius = +inf gives one group (of the rows without NaN); a disallowed row never bridges
 *     two allowed ones.
 *   LIMIT.  With limit > 0 a list may be cut; every edge is still a true one, so each returned group is a SUBSET of a true component and
 *     never a union of two.  out_stats[3] counts the rows whose list reached `limit`.
 *   out_stats [4]: groups of at least 2 rows | rows in them | non-self pairs seen (a pair both ends list counts twice) | truncated rows.
 *   The answer is a pure function of table, radius, mask and limit: not of launch order, "flat_dup_chunk" or run.
 * How: the allowed rows are the queries, "flat_dup_chunk" of them per range call (vdb_set_param; default 16384) -- in place on an unfiltered
 * f32 index, gathered (u8 rows: widened) otherwise; each chunk's CSR result is hooked into a union-find over 4 B per row (a lane per
 * pair, roots hooked under LOWER roots by an integer compare-and-swap, path halving; no float atomics, no waiting on another thread) and
 * dropped before the next chunk.  Peak memory: one chunk's range result + 8 B per row + the chunk's gathered queries.  The range calls
 * under it advance the "flat_range_*" counters as always and obey "flat_range_max_results" PER CHUNK.
 * Refused, outputs and the three counters below untouched: a NaN radius (VDB_ERR_INVALID), a mask of another index (VDB_ERR_INVALID) or a
 * stale one (VDB_ERR_STATE), a NULL output; a chunk whose range call fails fails the whole call the same way.  `limit` has no cap (the
 * range call has none).  An empty index succeeds (stats 0).  Read-side, re-entrant, f32 and VecSet<u8> indexes; both forms return
 * synchronised; the _device form writes d_out_group (u64 [len], 8-byte aligned, on the index's GPU) after waiting for `stream`.
 * vdb_link_pairs_device: the component stage alone over a caller-supplied CSR edge list on the index's GPU -- d_src [nq] the u64 ids of the
 *   lists' source rows, d_lims [nq + 1] u64 ascending from 0, d_ids [d_lims[nq]] u64 ids (row + id_offset, as the range calls write
 *   them; non-NULL whenever nq > 0), d_group [len] u64.  The limits and every id are checked on the device first; ONE read-back, and a
 *   descending limit or an id that is no row fails the call (VDB_ERR_INVALID) before any output is written, as vdb_group_cap_device does.
 *   Every row is allowed; out_stats[3] is 0.  nq == 0: every row alone.
 * vdb_dup_plan: host utility, works without a GPU: the argument check and, for (n_rows, dim, element type, masked, allowed rows, chunk),
 *   the number of range calls, the last chunk's length, whether the queries are gathered, and the scratch bytes besides a chunk's
 *   result.  Any output may be NULL; on an error nothing is written.
 * vdb_get_stat: "flat_dup_calls" (calls that succeeded), "flat_dup_chunks" (their range calls), "flat_dup_pairs" (non-self pairs they
 * saw).  vdb_prof_get "dup_hook" / "dup_flatten" time the component kernels. */
int vdb_dup_plan(uint64_t n_rows, uint64_t dim, int elem_u8, int masked, uint64_t m_allowed, float radius, uint64_t limit, uint64_t chunk,
                 uint64_t *out_chunks, uint64_t *out_last, int *out_gather, uint64_t *out_scratch_bytes);
int vdb_flat_dup_groups(vdb_index *idx, float radius, uint64_t limit, const vdb_mask *mask /* NULL: all rows */, uint64_t *out_group /* [len] */,
                        uint64_t *out_stats /* [4] */);
int vdb_flat_dup_groups_device(vdb_index *idx, float radius, uint64_t limit, const vdb_mask *mask, void *d_out_group, uint64_t *out_stats,
                               void *stream);
int vdb_link_pairs_device(vdb_index *idx, const void *d_src, const void *d_lims, const void *d_ids, uint64_t nq, void *d_group,
                          uint64_t *out_stats, void *stream);
/* ---- grouped Flat k-NN: at most group_size hits per value of one label column -----------------------------------------------------------
 * "The 10 nearest chunks, at most 2 per document": the label columns so far restrict WHICH rows may be found; this call shapes the answer.
 * For one query let L be its allowed rows in FlatIndex::knn's order -- ascending by (distance, id), NaN distances last; all rows, or
 * the rows of the query's mask.  Walking L from its start, a row whose label in `column` is VDB_LABEL_NONE (never labelled, or a column
 * never written) is always kept -- every such row is a group of its own -- and a row with label v is kept iff fewer than group_size
 * rows EARLIER IN L carry v.  The answer is the first k kept rows in L's order: out_idx / out_dist [nq][k], out_count[q] = min(k, kept
 * rows in all of L), slots past the count zero, id_offset added to the ids, distances the bit-exact f32 of the unfiltered search.  With
 * group_size at least the largest group, or a column never written, the answer is that of vdb_flat_knn / vdb_flat_knn_filtered_multi
 * at the same k, bit for bit.
 *   n_masks == 0: unfiltered, masks / mask_of are not read; otherwise they mean what they mean for vdb_flat_knn_filtered_multi.
 *   How: whether a row is kept depends only on the rows before it, so the capped walk of a prefix of L yields a prefix of the answer.
 *   Round 0 takes the exact sorted list of K' = min(m, k x "flat_grouped_oversample") rows per query (m: the query's allowed rows) from the
 *   existing exact search -- the unfiltered call exactly as vdb_flat_knn_device runs it, or the filtered call with a mask per query,
 *   whose counters advance as if those calls had been made -- and k_group_cap walks it: one wave per query, tiles of 64 positions, the
 *   labels gathered one tile ahead, a hash table label -> kept count (while fewer than k rows are kept it holds fewer than k labels,
 *   however long L is: in LDS, or in device scratch for a k past ~2000), ballots and prefix popcounts for the rank inside a tile and the
 *   output slot.  One read-back of a done byte per query ends the round; a query that neither kept k rows nor saw its whole allowed
 *   set goes round again in a compacted block with 4 x K', clamped to m, and the longer list is walked again from its start.  A list of
 *   m rows is everything, so the loop ends.  Later rounds run in sub-chunks of queries whose lists stay under 256 MiB.
 *   "flat_grouped_oversample" (vdb_set_param, per index, >= 1, default 2: the winner of the sweep of tools/bench_grouped.py) never changes an answer, only the rounds.  Under masks longer
 *   than "flat_filtered_direct_max" a K' above 64 takes the filtered call's direct path instead of its 8-bit tier, and without masks a K'
 *   above 64 leaves the 8-bit first pass of vdb_flat_knn: a step in cost either way (measured: DESIGN 4.1q).
 * vdb_flat_knn_grouped_device: queries and outputs on the index's GPU, at most 32768 queries, returns synchronised.
 * vdb_group_cap_device: the walk alone over caller-supplied lists -- d_ids (u64, id_offset included) / d_dists (f32) [nq][ld] in ANY
 * order, walked as given, and d_counts [nq] (u64; entries past min(count, ld) are not read) -- into d_out_idx / d_out_dist [nq][k] and
 * d_out_count [nq]: what a sharded merge needs behind its top-k merge, and how the tests drive the kernel.  Every counted id is checked
 * on the device first (one flag read back): an id that, after id_offset is subtracted, is not below len is VDB_ERR_INVALID with the
 * outputs untouched; nothing is gathered out of bounds.
 * Refused before anything is computed or written, counters unchanged (VDB_ERR_INVALID): group_size == 0, column >= VDB_LABEL_COLUMNS, a
 * VecSet<u8> index, and every mask / mask_of error of vdb_flat_knn_filtered_multi (a stale mask: VDB_ERR_STATE).  nq == 0, k == 0 and
 * m == 0 give empty results.  Read-side and re-entrant.
 * vdb_get_stat "flat_grouped_calls", "flat_grouped_queries", "flat_grouped_rounds" (sum over calls of the rounds run),
 * "flat_grouped_exhausted_queries" (queries whose last list was their whole allowed set); vdb_prof_get "group_cap" times k_group_cap.
 * Not covered: sharded and replica contexts, VecSet<u8> indexes, PQ / HNSW / IVF searches, grouping by more than one column, range
 * search. */
int vdb_flat_knn_grouped(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, uint64_t k, uint32_t column, uint64_t group_size,
                         const vdb_mask *const *masks, uint64_t n_masks, const uint32_t *mask_of, uint64_t *out_idx, float *out_dist,
                         uint64_t *out_count);
int vdb_flat_knn_grouped_device(vdb_index *idx, const void *d_queries, uint64_t nq, uint64_t dim, uint64_t k, uint32_t column,
                                uint64_t group_size, const vdb_mask *const *masks, uint64_t n_masks, const uint32_t *mask_of, void *d_out_idx,
                                void *d_out_dist, void *d_out_count, void *stream);
int vdb_group_cap_device(vdb_index *idx, const void *d_ids, const void *d_dists, const void *d_counts, uint64_t nq, uint64_t ld, uint64_t k,
                         uint32_t column, uint64_t group_size, void *d_out_idx, void *d_out_dist, void *d_out_count, void *stream);
/* ---- diversified Flat k-NN: maximal marginal relevance (MMR) over the fetch_k nearest allowed rows -------------------------------------
 * "The k results that are close to the query and not near-copies of each other": the max_marginal_relevance_search(query, k, fetch_k,
 * lambda_mult) of the common retrieval stacks, with the library's bit-exact distances and nothing dragged to the host.  Grouping needs
 * a label that says which rows are redundant; this call takes redundancy from the vectors themselves.
 *   All arithmetic is f32, one rounding per operation, no FMA.  For one query let L be its allowed rows in FlatIndex::knn's order --
 *   ascending by (distance, id), NaN distances last; all rows, or the rows of the query's mask -- m their number, F = min(fetch_k, m),
 *   C the first F entries of L (positions 0 .. F - 1) and d_p the distance the search reports for position p.  D(p, s) is the distance
 *   between the ROWS at positions p and s under the index's metric in the reference's arithmetic, DistanceAlgorithm::d(row_p, row_s):
 *   what vdb_flat_knn reports for row s when row p is the query (Cosine: norms = sqrtf of the cached strict-fold |x|^2, denominator
 *   max(na * nb, 1e-10)).  D is symmetric bit for bit under both metrics.  mu = 1.0f - lambda, kk = min(k, F).
 *   Selection: position 0 first.  Every later step gives each unselected p the score (lambda * d_p) - (mu * m_p), m_p = min over the
 *   selected s of D(p, s) -- m_p starts at +inf and takes D only if D < m_p, so a NaN D is ignored; a NaN score counts as +inf -- and
 *   selects the smallest score, ties (-0 == +0, +inf == +inf) to the lowest position, until kk are selected.
 *   Output: the selected rows IN SELECTION ORDER (not sorted by distance): out_idx (id_offset added) / out_dist (d_p) [nq][k],
 *   out_count[q] = kk, slots past the count zero.  On rows without NaN or inf, lambda = 1 is vdb_flat_knn /
 *   vdb_flat_knn_filtered_multi at the same k bit for bit; lambda = 0 is farthest-first traversal of C from the nearest row;
 *   fetch_k == k returns the rows of the plain search in another order.  fetch_k changes the answer: an argument, not a vdb_set_param.
 *   n_masks == 0: unfiltered, masks / mask_of are not read; otherwise they mean what they mean for vdb_flat_knn_filtered_multi.
 *   How: ONE round.  The exact sorted list of min(m, fetch_k) rows per query comes from the existing exact search -- the unfiltered
 *   call exactly as vdb_flat_knn_device runs it, or the filtered call with a mask per query, whose counters advance as if those calls
 *   had been made -- and k_mmr_select picks from it: one workgroup per query, a lane per candidate, d_p / m_p / selected flags in LDS,
 *   no F x F matrix: a step folds only D(p, row selected last) into m_p, the selected row staged in LDS (in pieces of 2048 floats when
 *   longer) while each lane walks its own candidate row with the reference's strict left fold; the argmin is a wave shuffle reduction
 *   and one LDS exchange.  At most (kk - 1) x F folds per query.  Queries run in sub-chunks whose lists stay under 256 MiB.  A fetch_k
 *   above 64 leaves the 8-bit first pass of the searches, a step in cost.
 * vdb_flat_knn_mmr_device: queries and outputs on the index's GPU, at most 32768 queries, returns synchronised.
 * vdb_mmr_select_device: the selection alone over caller-supplied lists -- d_ids (u64, id_offset included) / d_dists (f32) [nq][ld],
 * ld <= 4096, k <= ld, in ANY order, walked as given (list position is the tie order; position 0 is selected first), and d_counts [nq]
 * (u64; entries past min(count, ld) are not read) -- into d_out_idx / d_out_dist [nq][k] and d_out_count [nq]: what a sharded merge
 * needs behind its top-k merge, and how the tests drive the kernel.  Every counted id is checked on the device first (one flag read
 * back): an id that, after id_offset is subtracted, is not below len is VDB_ERR_INVALID with the outputs untouched; nothing is
 * gathered out of bounds.
 * Refused before anything is computed or written, counters unchanged (VDB_ERR_INVALID): lambda NaN or outside [0, 1], fetch_k < k,
 * fetch_k > 4096, a VecSet<u8> index, and every mask / mask_of error of vdb_flat_knn_filtered_multi (a stale mask: VDB_ERR_STATE).
 * nq == 0, k == 0 and m == 0 give empty results.  Read-side and re-entrant.
 * vdb_get_stat "flat_mmr_calls", "flat_mmr_queries" (the two search forms); vdb_prof_get "mmr_select" times k_mmr_select.
 * Not covered: sharded and replica contexts, VecSet<u8> indexes, candidates from PQ / HNSW / IVF searches, combination with grouping,
 * range search. */
int vdb_flat_knn_mmr(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, uint64_t k, uint64_t fetch_k, float lambda,
                     const vdb_mask *const *masks, uint64_t n_masks, const uint32_t *mask_of, uint64_t *out_idx, float *out_dist,
                     uint64_t *out_count);
int vdb_flat_knn_mmr_device(vdb_index *idx, const void *d_queries, uint64_t nq, uint64_t dim, uint64_t k, uint64_t fetch_k, float lambda,
                            const vdb_mask *const *masks, uint64_t n_masks, const uint32_t *mask_of, void *d_out_idx, void *d_out_dist,
                            void *d_out_count, void *stream);
int vdb_mmr_select_device(vdb_index *idx, const void *d_ids, const void *d_dists, const void *d_counts, uint64_t nq, uint64_t ld, uint64_t k,
                          float lambda, void *d_out_idx, void *d_out_dist, void *d_out_count, void *stream);
/* ---- search by example rows ("recommend", "more like this"): positives, negatives, the examples left out ------------------------------
 * "More like these rows, and not like those": the query vector is made on the device from rows the index already holds, searched
 * exactly, and the examples are taken out of the answer -- no vector is dragged to the host and no k is guessed.
 *   All arithmetic is f32, one rounding per operation, no FMA.  For query q the caller gives two lists of rows, positives P_q with
 *   |P_q| >= 1 and negatives N_q, which may be empty; each is read in list order and a repeat counts as often as it appears.
 *   Query vector, per element j: sp = +0.0f, then sp = sp + row[j] for each positive in list order (a strict left fold);
 *   ap = sp / (float)|P_q|.  With negatives an is the same fold and divide over N_q and query[j] = (ap + ap) - an; without,
 *   query[j] = ap (so one positive gives the row itself, with -0.0 turned into +0.0).  This is the usual "average vector" rule
 *   avg_pos + (avg_pos - avg_neg).  It holds for both metrics: Cosine needs no extra normalisation, the search treats this query as it
 *   treats any other.  A NaN element keeps no particular sign or payload.
 *   Search: let L be the query's allowed rows in FlatIndex::knn's order -- ascending by (distance, id), NaN distances last; all rows,
 *   or the rows of the query's mask (masks / mask_of mean what they mean for vdb_flat_knn_filtered_multi; n_masks == 0: unfiltered,
 *   they are not read).  exclude != 0: the answer is the first k entries of L whose row is in neither P_q nor N_q; exclude == 0: the
 *   first k entries of L.  out_idx (id_offset added) / out_dist [nq][k]; the distances are bit for bit those of the plain search for
 *   that query vector; out_count[q] is the number written, slots past the count are zero.
 *   How: ONE round.  e_max = max over q of (|P_q| + |N_q|) -- the lists as given, not distinct rows: an upper bound that needs no
 *   read-back -- and K' = min(max_m, k + e_max) when excluding, else min(max_m, k), max_m the longest allowed set.  A list of K' rows
 *   always holds k rows that are no examples whenever that many exist.  k_like_build writes the query vectors (a thread per element,
 *   wave-uniform row ids, 64-bit row offsets); the exact sorted list of K' rows per query comes from the existing search, unchanged --
 *   the unfiltered call exactly as vdb_flat_knn_device runs it, or the filtered call with a mask per query, whose counters advance as
 *   if those calls had been made -- and k_like_drop compacts it: one wave per query, tiles of 64, a lane tests its id against the
 *   query's example ids staged in LDS, a ballot and a prefix popcount give the output slot, it stops at k.  Queries run in sub-chunks
 *   whose lists stay under 256 MiB.  K' never changes an answer, only the cost: past 64 it leaves the 8-bit first pass of the
 *   searches, the step in cost DESIGN 4.1q and 4.1u measured.
 * The lims arrays are HOST pointers in every form (as mask_of is): pos_lims [nq + 1] with pos_lims[0] == 0, query q's positives are
 * entries pos_lims[q] .. pos_lims[q + 1] of the list; neg_lims likewise, or NULL when no query has negatives.  At most 1024 examples
 * per query, positives plus negatives.  Host forms take LOCAL row ids (u64, below len); device forms take u64 GLOBAL ids (row +
 * id_offset) on the index's GPU, 8-byte aligned, as vdb_index_get_rows_device does, and check them on the device with one flag
 * read-back: nothing is gathered out of bounds.
 * vdb_like_queries: the builder alone, into nq x dim f32 on the host.  vdb_like_queries_device: into device memory (4-byte aligned),
 * returns synchronised; its output is a valid d_queries for every *_device search -- range, grouped, MMR, HNSW, IVF: that is how those
 * combine with examples, no further variants exist.
 * vdb_flat_knn_like_device: outputs on the index's GPU, at most 32768 queries, returns synchronised.
 * vdb_drop_listed_device: the compaction alone over caller-supplied lists -- d_ids (u64, id_offset included) / d_dists (f32) [nq][ld]
 * in ANY order, walked as given, and d_counts [nq] (u64; entries past min(count, ld) are not read) -- against the global ids
 * d_drop_ids under the HOST limits drop_lims [nq + 1] (a query's list may be empty, at most 1024 ids), into d_out_idx / d_out_dist
 * [nq][k] and d_out_count [nq]: the first k entries whose id is not listed, in list order; the same id twice in a list is dropped
 * twice.  What a sharded merge needs behind its top-k merge, and how the tests drive the kernel.  Every counted id and every listed
 * id is checked on the device first: one that is no row of the index is VDB_ERR_INVALID with the outputs untouched.
 * Refused before anything is computed or written, counters unchanged (VDB_ERR_INVALID): limits that do not start at 0 or descend, a
 * query without a positive or with more than 1024 examples, a NULL list with entries, a row or id that is no row of the index, a
 * VecSet<u8> index, and every mask / mask_of error of vdb_flat_knn_filtered_multi (a stale mask: VDB_ERR_STATE).  nq == 0, k == 0
 * and m == 0 give empty results.  Read-side and re-entrant.
 * vdb_get_stat "flat_like_calls", "flat_like_queries" (the two search forms), "like_example_rows" (list entries the builder walked,
 * all four forms); vdb_prof_get "like_build", "like_drop" time the two kernels.
 * Not covered: the "best score" strategy (every candidate scored against every example), per-example weights, VecSet<u8> indexes,
 * sharded and replica contexts, PQ / HNSW / IVF candidate lists (beyond feeding them the built queries through
 * vdb_like_queries_device), combination with group_by / mmr_lambda at the VecDB level. */
int vdb_like_queries(vdb_index *idx, const uint64_t *pos_lims, const uint64_t *pos_rows, const uint64_t *neg_lims, const uint64_t *neg_rows,
                     uint64_t nq, float *out_queries);
int vdb_like_queries_device(vdb_index *idx, const uint64_t *pos_lims, const void *d_pos_ids, const uint64_t *neg_lims, const void *d_neg_ids,
                            uint64_t nq, void *d_out_queries, void *stream);
int vdb_flat_knn_like(vdb_index *idx, const uint64_t *pos_lims, const uint64_t *pos_rows, const uint64_t *neg_lims, const uint64_t *neg_rows,
                      uint64_t nq, uint64_t k, int exclude, const vdb_mask *const *masks, uint64_t n_masks, const uint32_t *mask_of,
                      uint64_t *out_idx, float *out_dist, uint64_t *out_count);
int vdb_flat_knn_like_device(vdb_index *idx, const uint64_t *pos_lims, const void *d_pos_ids, const uint64_t *neg_lims, const void *d_neg_ids,
                             uint64_t nq, uint64_t k, int exclude, const vdb_mask *const *masks, uint64_t n_masks, const uint32_t *mask_of,
                             void *d_out_idx, void *d_out_dist, void *d_out_count, void *stream);
int vdb_drop_listed_device(vdb_index *idx, const void *d_ids, const void *d_dists, const void *d_counts, uint64_t nq, uint64_t ld, uint64_t k,
                           const uint64_t *drop_lims, const void *d_drop_ids, void *d_out_idx, void *d_out_dist, void *d_out_count, void *stream);
/* ---- fused multi-query Flat search: several searches of one question joined into one ranked answer (RRF, min-distance) ----------------
 * One question sent as several query vectors (paraphrases, a HyDE passage, sub-questions), or as one vector under several filters, and
 * the lists joined by reciprocal rank fusion or by "nearest to any of them" -- on the device, exact, deterministic, nothing dragged to
 * the host.
 *   All arithmetic is f32, one rounding per operation, no FMA; the divide is the correctly rounded one.  A call holds nq FUSED queries.
 *   Fused query q owns the sub-queries lims[q] .. lims[q + 1] - 1 of one flat array of query vectors (S_q of them); lims [nq + 1] is a HOST
 *   array in every form (as mask_of and pos_lims are), lims[0] == 0.  Each sub-query may have its own mask: masks / mask_of are indexed by
 *   SUB-query and mean what they mean for vdb_flat_knn_filtered_multi; n_masks == 0: unfiltered, they are not read.
 *   For sub-query s let L_s be its allowed rows in FlatIndex::knn's order -- ascending by (distance, id), NaN distances last -- m_s their
 *   number, F_s = min(fetch_k, m_s), C_s the first F_s entries of L_s, p_s(row) a row's 0-based position in C_s and d_s(row) its reported
 *   distance.  U_q = the rows that occur in at least one C_s of the fused query.
 *   VDB_FUSE_RRF: the score of a row of U_q starts at acc = +0.0f; for s ascending over the sub-queries whose C_s holds the row:
 *     den = (float)(p_s + 1) + c, term = w_s / den, acc = acc + term.  c = rrf_c, finite and >= 0 (the usual value is 60); w_s =
 *     weights[s], finite and > 0, a NULL `weights` (HOST, one per sub-query) means 1.0f everywhere.  The answer is the first
 *     min(k, |U_q|) rows of U_q by score DESCENDING, ties by ascending row id; out_dist carries the score.
 *   VDB_FUSE_MIN: the score is the smallest d_s(row) over the sub-queries whose C_s holds the row, "smallest" under the knn order (a NaN
 *     loses to any number, -0 == +0), with the bits of the first s that attains it; `weights` must be NULL.  The answer is ascending by
 *     (score, id), NaN last.  For fetch_k >= k this is EXACTLY the k allowed rows nearest to any of the sub-queries over the whole table
 *     (a row allowed to sub-query s counts with d_s): take a row r of that true top-k and the list s* in which its true minimum d* sits.
 *     If C_s* did not fetch r, C_s* holds fetch_k >= k rows that are before r in L_s*, each with a minimum at or before (d*, their id) --
 *     k rows better than r, a contradiction.  So r is in C_s*, its fused score is d*, and every other row of U_q carries its true
 *     minimum or something larger: the first k of U_q are the true top-k, bit for bit.
 *   Outputs: out_idx (id_offset added) / out_dist [nq][k], out_count[q] = min(k, |U_q|); slots past the count are zero.  fetch_k changes
 *   the answer: an argument, not a vdb_set_param.  1 <= S_q <= 32, k <= fetch_k <= 4096, S_q x fetch_k <= 16384.  With S_q == 1, MIN is
 *   vdb_flat_knn / vdb_flat_knn_filtered_multi at the same k bit for bit, and RRF returns the same rows in the same order.
 *   How: ONE round per sub-chunk of fused queries (their lists, S_max x K' x 12 B each with K' = min(fetch_k, longest allowed set), stay
 *   under 256 MiB).  The exact sorted lists of ALL its sub-queries come from ONE existing exact search -- the unfiltered call exactly as
 *   vdb_flat_knn_device runs it, or the filtered call with a mask per query, whose counters advance as if those calls had been made --
 *   then ONE k_fuse_lists launch (csrc/k_fuse.hip), a workgroup per fused query: the lists are walked in ascending s, which IS the fold
 *   order, a tile of 256 positions at a time; the rows live in an open-addressing table keyed by the local row (key, accumulator,
 *   stamp; load <= 1/2; in LDS up to 8192 slots, past that the same code on a slice of device scratch).  A lane claims its slot with a
 *   compare-and-swap, raises the slot's stamp to (s << 16) | (0xFFFF - position) with an atomic max, and after a barrier only the lane
 *   whose value IS the stamp folds its term in: one writer per slot per list, no float atomic, no order-dependent sum.  The occupied
 *   slots are then sorted as (score key, row) pairs and the first k leave with the accumulator's own bits.  A fetch_k above 64 leaves
 *   the 8-bit first pass of the searches, a step in cost.
 * vdb_fuse_plan: host utility, works without a GPU (like vdb_fetch_plan): *out_code = 0 when (mode, lims, nq, k, fetch_k, weights, rrf_c)
 *   is a call the search forms accept, otherwise which refusal: 1 mode, 2 NULL lims, 3 lims[0] != 0, 4 a descent, 5 a fused query without
 *   a sub-query, 6 more than 32, 7 fetch_k < k, 8 fetch_k > 4096, 9 S x fetch_k > 16384, 10 weights with MIN, 11 a weight that is NaN,
 *   inf or <= 0, 12 rrf_c NaN, inf or negative -- the first that applies, in this order; nothing else is written then.  Accepted:
 *   *out_s_max = the most sub-queries of a fused query, *out_table_lg = lg of the kernel's table for lists of fetch_k rows (2^lg slots,
 *   the smallest power of two >= 2 x S_max x fetch_k, at least 64), *out_in_lds = 1 when it lives in LDS (lg <= 13), *out_scratch_bytes =
 *   device scratch per fused query otherwise (16 B per slot), *out_sub_chunk = fused queries per sub-chunk under `budget` bytes of lists
 *   (0: the 256 MiB the calls use; also at most 16384 sub-queries, and the scratch under the same budget).  Any output but out_code may
 *   be NULL.
 * vdb_flat_knn_fused_device: queries and outputs on the index's GPU, at most 32768 SUB-queries, returns synchronised.
 * vdb_fuse_lists_device: the fusion alone over caller-supplied lists -- d_ids (u64, id_offset included) / d_dists (f32) [n_lists][ld],
 *   d_counts [n_lists] (u64), HOST lims [nq + 1] over the lists, HOST weights [n_lists] or NULL -- into d_out_idx / d_out_dist [nq][k] and
 *   d_out_count [nq]: what a sharded merge would call, and how the tests drive the kernel.  Lists are walked as given; position is the
 *   rank; entries past min(count, ld) are not read; k may exceed ld.  If an id occurs more than once in ONE list only its FIRST
 *   occurrence counts, for the rank and for the distance.  ld <= 4096, S_q x ld <= 16384.  Every counted id is checked on the device
 *   first (one flag read back): an id that is no row of the index is VDB_ERR_INVALID with the outputs untouched.
 * Refused before anything is computed or written, counters unchanged (VDB_ERR_INVALID): everything vdb_fuse_plan reports, a VecSet<u8>
 * index, and every mask / mask_of error of vdb_flat_knn_filtered_multi (a stale mask: VDB_ERR_STATE).  nq == 0, k == 0 and empty lists
 * give empty results.  Read-side and re-entrant.
 * vdb_get_stat "flat_fused_calls", "flat_fused_queries" (fused queries), "flat_fused_lists" (sub-queries) count the two search forms;
 * vdb_prof_get "fuse_lists" times k_fuse_lists.
 * Not covered: distribution-based score fusion, lists from PQ / HNSW / IVF searches (beyond feeding them to vdb_fuse_lists_device),
 * VecSet<u8> indexes, sharded and replica contexts, combination with mmr_lambda (fusion by a label: vdb_flat_knn_fused_groups below). */
#define VDB_FUSE_RRF 0
#define VDB_FUSE_MIN 1
int vdb_fuse_plan(int mode, const uint64_t *lims, uint64_t nq, uint64_t k, uint64_t fetch_k, const float *weights, float rrf_c, uint64_t budget,
                  int *out_code, uint64_t *out_s_max, uint32_t *out_table_lg, int *out_in_lds, uint64_t *out_scratch_bytes,
                  uint64_t *out_sub_chunk);
int vdb_flat_knn_fused(vdb_index *idx, const float *queries, const uint64_t *lims, uint64_t nq, uint64_t dim, uint64_t k, uint64_t fetch_k,
                       int mode, const float *weights, float rrf_c, const vdb_mask *const *masks, uint64_t n_masks, const uint32_t *mask_of,
                       uint64_t *out_idx, float *out_dist, uint64_t *out_count);
int vdb_flat_knn_fused_device(vdb_index *idx, const void *d_queries, const uint64_t *lims, uint64_t nq, uint64_t dim, uint64_t k,
                              uint64_t fetch_k, int mode, const float *weights, float rrf_c, const vdb_mask *const *masks, uint64_t n_masks,
                              const uint32_t *mask_of, void *d_out_idx, void *d_out_dist, void *d_out_count, void *stream);
int vdb_fuse_lists_device(vdb_index *idx, const void *d_ids, const void *d_dists, const void *d_counts, const uint64_t *lims, uint64_t nq,
                          uint64_t ld, uint64_t k, int mode, const float *weights, float rrf_c, void *d_out_idx, void *d_out_dist,
                          void *d_out_count, void *stream);
/* ---- document-level fused Flat search: the lists of several sub-queries joined by the value of a label column ------------------------
 * Rows are chunks and a label column says which document a chunk belongs to: a question asked as several vectors (paraphrases,
 * sub-questions, the token vectors of a late-interaction query) ranks DOCUMENTS.  The unit of ranking is a GROUP: all rows that share a
 * value of label column `column`.
 *   The lists, the limits `lims`, masks / mask_of, fetch_k, C_s and the knn order (ascending by (distance, id), -0 == +0, every NaN equal
 *   and last) are exactly those of vdb_flat_knn_fused.
 *   Group of a row: if the row's code is not VDB_LABEL_NONE its group is that code; an unlabelled row (VDB_LABEL_NONE, or a column never
 *   written) is a group of its own, as the grouped search always keeps unlabelled rows.  The two key spaces are distinct: unlabelled row 5
 *   and label code 5 are different groups.
 *   Per list s and group g: p_s(g) is the smallest position in C_s of a row of g (the first-occurrence rule; in a sorted list that row is
 *   the group's nearest), r_s(g) that row and d_s(g) its distance; rho_s(g) is the number of distinct groups whose first occurrence lies
 *   before p_s(g) -- the group's 0-based RANK AMONG GROUPS, not its row position; f_s is the distance of the LAST counted entry of list s
 *   (position min(count, length) - 1, whatever its id).  A list with no counted entry is SKIPPED in every fold below.  List s is
 *   truncated when it counts at least trunc_len entries; trunc_len is fetch_k in the search forms and an argument of the list form
 *   (its ld, usually).  One refinement in the search forms: when fetch_k reaches the longest allowed set among the sub-queries of the
 *   call (the table, unfiltered; per block of 16384 sub-queries in the host form) every list is whole and none is truncated.
 *   U_q = the groups that occur in at least one C_s of the fused query.
 *   Scores: each a strict left fold over s ascending, f32, one rounding per operation, no FMA, no float atomic.
 *   VDB_FUSE_RRF: acc = +0.0f; for each non-empty list that holds g: den = (float)(rho_s(g) + 1) + c, term = w_s / den, acc = acc + term.
 *     Descending by score, ties by representative id ascending.
 *   VDB_FUSE_MIN: the smallest d_s(g) under the knn order, the bits of the first list that attains it; ascending; weights must be NULL.
 *   VDB_FUSE_SUM (late interaction): acc = +0.0f; for EVERY non-empty list s ascending: term = d_s(g) if C_s holds g, else f_s;
 *     acc = acc + term.  Ascending, NaN last; weights must be NULL.  A row the list did not fetch is at least as far as f_s, so when
 *     list s is truncated the score is a LOWER BOUND of the true sum of per-vector best-chunk distances (f32 addition is monotone); it IS
 *     that sum when no list is truncated.  IEEE 754 leaves the payload of a NaN sum open: a NaN score is reported as 0x7FC00000.
 *   Representative of a group: the row r_s*(g) of the list that minimises (order key of d_s(g), s).  Ties in MIN and SUM go to the lower
 *   representative id as well.  Over a column never written every row is a group of its own: MIN is vdb_flat_knn_fused bit for bit, and so
 *   is RRF where no id occurs twice in a list (a repeat moves the row POSITIONS behind it, not the group ranks).
 *   Outputs: out_idx (the representative, id_offset added) / out_dist (the group's score: the accumulator's own bits) [nq][k], slots
 *   behind the count zero; out_count[q] = min(k, |U_q|); out_exact[q] (u8, may be NULL): RRF and SUM: 1 iff no list of the query is
 *   truncated; MIN: 1 iff no list is truncated, or count == k and the order key of the k-th score is STRICTLY below the key of f_s for
 *   every truncated list s -- every unfetched row is then at or beyond some f_s, so the k groups are the true k nearest groups over the
 *   whole table with their true distances (a tie AT f_s gives 0).  k == 0: nothing is fetched or ranked, counts and out_exact are zero.
 *   Limits as vdb_fuse_plan: 1 <= S_q <= 32, k <= fetch_k <= 4096, S_q x fetch_k <= 16384.
 *   How: the ONE list call per sub-chunk of vdb_flat_knn_fused, then ONE k_fuse_groups launch (csrc/k_fuse_groups.hip), a workgroup per
 *   fused query: every lane gathers the label of its entry (the gathers of the next tile of 256 positions issued before this one is
 *   worked on); the groups live in an open-addressing table keyed by a 64-bit key (the code, or bit 32 | row for an unlabelled row) --
 *   per slot the key, accumulator, stamp, representative row and its distance, 28 B with the sort key: in LDS up to 4096 slots (112 KiB
 *   of the 160 KiB of a CU), past that the same code on a slice of device scratch.  Claim by compare-and-swap, stamp by atomic max of
 *   (s << 16) | (0xFFFF - position), and after a barrier only the stamp's owner writes: one writer per slot per list.  The owners of a
 *   tile are the first occurrences of their groups: wave ballots, prefix popcounts and per-wave sums give rho_s.  Under SUM a group first
 *   seen in list s starts from the fold of f_0 .. f_(s-1), and after list s the occupied slots it did not stamp add f_s.
 * vdb_fuse_groups_plan: host utility, works without a GPU: vdb_fuse_plan's codes 1 .. 12 in its order with VDB_FUSE_SUM an accepted
 *   mode, 13 weights with VDB_FUSE_SUM (where 10 stands), 14 column >= VDB_LABEL_COLUMNS (last).  Accepted: the outputs of vdb_fuse_plan for
 *   this kernel's table (lg as there; in LDS when lg <= 12; 28 B of scratch per slot otherwise).
 * vdb_flat_knn_fused_groups_device: queries and outputs on the index's GPU, at most 32768 SUB-queries, returns synchronised.
 * vdb_fuse_groups_device: the fusion alone over caller-supplied lists, the arguments of vdb_fuse_lists_device plus column, trunc_len
 *   (>= 1) and d_out_exact: what a sharded merge would call, and how the tests drive the kernel.  If a group occurs more than once in
 *   ONE list only its FIRST occurrence counts.  Every counted id is checked on the device first: an id that is no row of the index is
 *   VDB_ERR_INVALID with the outputs untouched.
 * Refused before anything is computed or written, counters unchanged (VDB_ERR_INVALID): everything vdb_fuse_groups_plan reports, a
 * VecSet<u8> index, every mask / mask_of error of vdb_flat_knn_filtered_multi (a stale mask: VDB_ERR_STATE), trunc_len == 0.
 * vdb_get_stat "flat_fused_groups_calls", "flat_fused_groups_queries", "flat_fused_groups_lists" count the two search forms (the list
 * call under them advances its own counters); vdb_prof_get "fuse_groups" times k_fuse_groups.
 * Not covered: rounds that grow fetch_k until MIN is exact (out_exact tells the caller), exact rescoring of candidate documents over
 * all their rows, weighted SUM, sharded contexts, VecSet<u8> indexes, lists from PQ / HNSW / IVF beyond feeding them to the list form. */
#define VDB_FUSE_SUM 2
int vdb_fuse_groups_plan(int mode, const uint64_t *lims, uint64_t nq, uint64_t k, uint64_t fetch_k, const float *weights, float rrf_c,
                         uint32_t column, uint64_t budget, int *out_code, uint64_t *out_s_max, uint32_t *out_table_lg, int *out_in_lds,
                         uint64_t *out_scratch_bytes, uint64_t *out_sub_chunk);
int vdb_flat_knn_fused_groups(vdb_index *idx, const float *queries, const uint64_t *lims, uint64_t nq, uint64_t dim, uint64_t k,
                              uint64_t fetch_k, int mode, const float *weights, float rrf_c, uint32_t column, const vdb_mask *const *masks,
                              uint64_t n_masks, const uint32_t *mask_of, uint64_t *out_idx, float *out_dist, uint64_t *out_count,
                              uint8_t *out_exact);
int vdb_flat_knn_fused_groups_device(vdb_index *idx, const void *d_queries, const uint64_t *lims, uint64_t nq, uint64_t dim, uint64_t k,
                                     uint64_t fetch_k, int mode, const float *weights, float rrf_c, uint32_t column,
                                     const vdb_mask *const *masks, uint64_t n_masks, const uint32_t *mask_of, void *d_out_idx,
                                     void *d_out_dist, void *d_out_count, void *d_out_exact, void *stream);
int vdb_fuse_groups_device(vdb_index *idx, const void *d_ids, const void *d_dists, const void *d_counts, const uint64_t *lims, uint64_t nq,
                           uint64_t ld, uint64_t k, int mode, const float *weights, float rrf_c, uint32_t column, uint64_t trunc_len,
                           void *d_out_idx, void *d_out_dist, void *d_out_count, void *d_out_exact, void *stream);
/* ---- bulk row fetch: the vectors of many rows as ONE call (no counterpart in the reference) ----------------------------------------
 * vdb_index_row reads one row with one blocking copy.  These calls return the vectors of a LIST of rows: out[j] = row rows[j].  The
 * list only names what is read, so its order is free and repeats are allowed (m may exceed len); every rows[j] must be below len, and a
 * NULL list or a NULL out with m > 0, or a row at or past len, is VDB_ERR_INVALID with a message: nothing is read, `out` and the counters
 * below are untouched.  m == 0 succeeds, touches nothing and counts nothing.
 * vdb_fetch_plan: host utility, works without a GPU (like vdb_update_plan): how a list over a table of n rows is carried out.
 *   *out_route = VDB_FETCH_DIRECT when the list is one ascending run of consecutive rows (rows[j] == rows[0] + j, m >= 1): the result
 *   is a contiguous piece of the table; VDB_FETCH_GATHER otherwise.  The gathered route passes the result through a bounded staging
 *   buffer in chunks: *out_chunk_rows = max(1, chunk_bytes / out_row_bytes) output rows each, *out_n_chunks = ceil(m / that).
 *   out_row_bytes and chunk_bytes at least 1; m x out_row_bytes must fit 64 bits.  Any output pointer may be NULL.
 * vdb_index_get_rows: rows are LOCAL row ids (id_offset plays no part), out is m x dim f32 row-major on the host; a VecSet<u8> index is
 *   widened exactly ((float)byte).  On the DIRECT route of an index that needs no widening: ONE copy straight out of the table, no
 *   kernel.  Otherwise the ids are uploaded once as u32 and per chunk one launch (csrc/k_fetch.hip) gathers the rows into one of TWO
 *   device staging buffers, from which the chunk is copied straight into `out`; the gather of the next chunk runs while the current
 *   one is copied.  Extra device memory: 2 x "fetch_chunk_bytes" (vdb_set_param, per index, >= 1: one row per chunk; default 128 MiB, the winner of the sweep of tools/bench_fetch.py)
 *   plus 4 m bytes of ids, whatever m is.  No host copy of the table is built or read.
 * vdb_index_get_rows_u8: the same with the rows as stored, m x dim bytes; a VecSet<u8> index only (as vdb_index_row_u8).
 * vdb_index_get_rows_mask: the mask's allowed rows in ascending order, vdb_mask_count(mask) x dim f32: the mask's own id list on
 *   the device is the gather list, nothing is uploaded.  A mask of another index is VDB_ERR_INVALID and a stale one VDB_ERR_STATE, as in
 *   the filtered searches; an empty mask succeeds and writes nothing.
 * vdb_index_get_rows_device: d_ids = m u64 GLOBAL ids (row + id_offset) on the index's GPU, as the *_device searches write them;
 *   d_out = m x dim f32 there (a u8 index is widened), 4-byte aligned -- 16-byte alignment gets the 16-byte copy, anything else a
 *   narrower one.  The ids are checked on the device first (one flag read back): an id that is no row of the index is VDB_ERR_INVALID
 *   and d_out is untouched.  Then ONE gather launch straight into d_out.  Everything runs on `stream`; the call returns synchronised.
 * All four are read-side: re-entrant with each other and with the searches on one handle.
 * vdb_get_stat: "fetch_calls" (calls that fetched rows: m > 0, not refused), "fetch_rows" (rows they returned), "fetch_chunks" (gather
 * launches: the chunks of the host forms, one per device call), "fetch_direct" (calls answered by the plain copy).
 * Not covered: the sharded contexts, PQ codes, graph export. */
#define VDB_FETCH_GATHER 0
#define VDB_FETCH_DIRECT 1
int vdb_fetch_plan(uint64_t n, const uint64_t *rows, uint64_t m, uint64_t out_row_bytes, uint64_t chunk_bytes, int *out_route,
                   uint64_t *out_chunk_rows, uint64_t *out_n_chunks);
int vdb_index_get_rows(vdb_index *idx, const uint64_t *rows, uint64_t m, float *out /* m x dim, host */);
int vdb_index_get_rows_u8(vdb_index *idx, const uint64_t *rows, uint64_t m, uint8_t *out /* m x dim, host */);
int vdb_index_get_rows_mask(vdb_index *idx, const vdb_mask *mask, float *out /* count x dim, host */);
int vdb_index_get_rows_device(vdb_index *idx, const void *d_ids, uint64_t m, void *d_out, void *stream);
/* the approximate keys the Flat shortlist pass compares with its threshold, for EVERY row, from the same kernel in its dense
 * mode (test / measurement entry point behind the certification-bound tests): out_keys [nq][len];
 * L2Sqr: key = |x|^2 - 2 S~, approximate distance = key + |q|^2;  Cosine: key = -S~ / |x|, approximate distance = 1 + key / |q|.
 * tier 0 = scaled fp16 operands, 1 = split-bf16 operands.  out_qsq [nq] = |q|^2 (strict fold), out_qerr [nq] = measured
 * |q - q~| of the fp16 query images (0 for tier 1), out_dx4 = {max |dx_r|, max |dx_r| / |x_r|, max |x|^2, min positive |x|^2}.
 * nq <= 1024; any of the last three outputs may be NULL. */
int vdb_flat_shortlist_keys(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, int tier, float *out_keys,
                            float *out_qsq, float *out_qerr, float *out_dx4);
/* tuning / test hooks for the Flat path:
 *   mode 0 = auto (MFMA shortlist + exact re-rank + certification, exact scan for small inputs),
 *   mode 1 = exact scan only (strict-order f32 fold for every row),
 *   mode 2 = MFMA path forced (still certified, still falls back per query). */
int vdb_flat_set_mode(vdb_index *idx, int mode);
/* developer tuning knobs (kernel variants); results never depend on them.  "flat_half", "flat_half_kmul", "flat_i8",
 * "flat_i8_rows", "flat_gemm", "flat_gemm_debug" and "flat_tail" are per index; ALL OTHER names set process-wide switches (the handle only routes the
 * call) and are not synchronised: set them before concurrent searches start, never while one is running.  Names:
 *   "flat_half"        fp16 first pass of the Flat pipeline: 0 auto (off once > 1/8 of its queries needed the redo), 1 off, 2 on
 *   "flat_half_kmul"   its shortlist = max(64, kmul * k) rows per query (default 4)
 *   "flat_i8"          8-bit first pass in FRONT of it (L2Sqr over f32 rows, k <= 64, dim % 4 == 0 with a 64-column block count divisible by
 *                      2, 3 or 5): a centred int8 mirror at 1 B/element whose keys are lower bounds of the distances; the exact stage walks the
 *                      hit list until the k-th exact distance is below the next bound; what it cannot close goes on to the fp16 pass.
 *                      0 auto (off once > 1/8 of its queries were handed on), 1 off, 2 on.  While it is the first tier the fp16 mirror is
 *                      built by its first use instead of at add time (set "flat_i8" = 1 BEFORE adding rows to have it built at add time)
 *   "flat_i8_rows"     rows its exact stage may walk per query before handing the query on (multiple of 64, default 256)
 *   "flat_gemm_coop"   the same sets for the fp16 / split-bf16 filter kernel (0 auto = on, 1 off)
 *   "flat_gemm8_coop"  cooperative sets of the resident form (calls whose group count is even, tables of >= 98 304 rows, 256-CU chips): the 32
 *                      workgroups of an XCD in sets of 8 / 4 / 2 that take different query groups and walk the same rows at the same time, so
 *                      a row comes from HBM once per set and from the XCD's L2 for the other members; 0 auto = on, 1 off
 *   "flat_gemm8_res"   its kernel keeps the query group's whole 1-B/element image in LDS (dimensions up to 960: no workgroup barrier per chunk;
 *                      0 auto = on when the image fits, 1 off = chunked staging through two buffers)
 *   "flat_gemm8_epi"   unit epilogue of its kernel: 0 (default) keys from scalar f32 multiply / fma and the wave's stage of passed lanes carried
 *                      over units; 1 the earlier form (packed f32 arithmetic, one drain per unit).  Same key bits, same hit lists
 *   "flat_gemm8_kc", "flat_gemm8_burst", "flat_gemm8_nt"   variants of its kernel: k-blocks per Q chunk (0 auto, 5 / 3 / 2), staging of
 *                      the next chunk (0 auto, 1 per k-block, 2 one burst per chunk), cache policy of the row stream (as "flat_gemm_nt")
 *   "flat_gemm"        128-queries-per-pass kernel: 0 auto, 1 off (small-batch kernel), 2 forced
 *   "flat_gemm_tw"     row tiles per wave (3 default, 2);  "flat_gemm_stagger" workgroup start delays (0 default)
 *   "flat_gemm_block_rows"  filter pass in row blocks, one launch per block over all query groups (measurement switch): 0 off, n rows
 *   "flat_gemm_nt"     cache policy of the row stream: 0 auto (non-temporal when the mirror exceeds the Infinity Cache), 1 default, 2 non-temporal
 *   "flat_tail"        exact stage: 0 fused launch when the shortlist fits 64 rows, 1 separate kernels
 *   "flat_tail_lb_nw"  form of the 8-bit pass's exact stage (k_flat_tail_lb): 0 auto (= 40), 40 / 41 four waves per query with ONE fold chain
 *                      per lane (products by all four waves, adds by one; row loads 3 / 5 chunks deep), 8 / 4 / 2 / 1 that many waves with the
 *                      chains on the lanes that fetched the rows (process-wide)
 *   "flat_tail_lb_walk"  how that stage walks a hit list: 0 (default) one selection of 256 keys serves four rounds and rounds after the first
 *                      fetch no row that the k-th distance so far excludes, 1 a selection in every round and every row fetched; same rounds,
 *                      same answers, same flags and statistics (process-wide)
 *   "flat_share", "mfma_variant", "flat_sample_thin", "flat_gemm_debug"   small-batch kernel / sample plan / measurement hooks
 *   "pq_adc_fast", "hnsw_dma"   inner-loop variants of the ADC scan and of the HNSW walk (hnsw_dma: 1 rows staged through
 *                      registers (default), 2 through LDS by DMA, 0 plain per-lane loads)
 *   "hnsw_half"        certified half-precision pre-pass of the exact HNSW walk (a row-major fp16 image of the rows, 2 B per
 *                      element, built on first use; rows it cannot rule out are scored exactly as always): 1 auto (default: calls of >= 768
 *                      queries, where the walk is bound by bytes rather than by latency), 0 off, 2 always
 *   "ivf_half"         the same pre-pass for the IVF probe-list scan (offers that cannot be among the k nearest are dropped before the
 *                      f32 rows are fetched; same results): 1 auto (default), 0 off
 *   "ivf_q8"           an 8-bit tier in front of it for long probe lists (1 B/element image with a scale and a measured error per row,
 *                      exact integer dot products; cluster-major for calls of 256 .. 16 384 (query, probe) pairs): 1 auto (default), 0 off, 2 query-major only
 *   "hnsw_build_gpu"   candidate phase of batched HNSW builds (vdb_hnsw_build with batch >= 256): 0 auto = the level-0 searches of a
 *                      batch and the distances between its members run on the GPU (same graph as the all-host builder), 1 off
 *   "hnsw_pool_cap"    most live candidates the fast HNSW walk keeps in LDS (it uses min(this, ef + max_m0 + 64); maximum 2048) before a query is handed to
 *                      the heap walk; tests lower it to exercise that hand-over
 *   "pq_adc16"         quantised first pass of the threshold-filter ADC scan (16-bit tables, 8 queries per pass; exact f32
 *                      sums for its candidates): 0 auto (4-bit codes of any m: L2Sqr 8 and Cosine 7 queries per pass; 8-bit codes, L2Sqr: one
 *                      query per pass on a one-byte table), 1 off
 *   "pq_sample16"      the threshold sample of that scan on the quantised tables as well (L2Sqr): 0 auto (on), 1 off (exact f32 sample).
 *                      The threshold only decides how many rows the scan keeps; the count is checked and short lists are redone
 *   "flat_small"       FlatIndex::knn of a few queries over a small table in ONE launch (the db.search() shape; dim % 4 == 0, k <= 64):
 *                      0 auto (flat mode 0; tables of at most "flat_small_max_rows" = 16 384 rows: calls of fewer than 32 queries; larger
 *                      tables: while rows x (0.9 queries - 0.3) < 75 000, i.e. one query up to ~125k rows, where the MFMA pipeline's
 *                      fixed ~0.1 ms of dependent launches costs more than re-reading the rows per query), 1 off, 2 whenever the shape allows */
int vdb_set_param(vdb_index *idx, const char *name, int64_t value);
/* Builds NOW the operand mirrors the first Flat search of this index would otherwise build inside that search (the centred 8-bit
 * mirror, or the fp16 / split-bf16 mirror where the 8-bit pass does not apply); all_tiers != 0: the mirrors of the tiers behind it too
 * (what a query the first pass cannot certify needs).  A latency-sensitive caller calls it after add / batch_add
 * (metadata_vec_table.rs:63-86 has no counterpart: the reference's Flat index has nothing to build).  A mirror that does not fit the
 * device memory is skipped -- searches then use the next tier, down to the exact scan over the rows -- and is not an error. */
int vdb_index_prepare(vdb_index *idx, int all_tiers);
/* number of queries whose MFMA shortlist failed certification and were redone by the exact scan */
int vdb_flat_fallback_count(const vdb_index *idx, uint64_t *out);
/* counters of the Flat pipeline (diagnostics; results never depend on them):
 *   "flat_fallback"      = vdb_flat_fallback_count,
 *   "flat_half_queries"  queries that went through the fp16 first pass,
 *   "flat_half_redo"     of those, the ones it could not certify (redone with the split-bf16 pass),
 *   "pq_adc16_queries"   queries whose ADC scan ran on the quantised 16-bit tables (k_pq_adc16) since the table was attached,
 *   "pq_adc16_redo"      of those, the ones it handed to the f32 scan (candidate list overflowed, or fewer than ef rows at or
 *                        below the threshold),
 *   "flat_half_valid"    1 when the index holds the fp16 mirror,
 *   "flat_i8_queries", "flat_i8_redo", "flat_i8_valid"  the same three for the 8-bit first pass (queries through it, queries it handed
 *                        on to the next tier, mirror present),
 *   "flat_bf16_mirror"   1 once the split-bf16 mirror (4 B/element) has been built -- lazily, by the first search that
 *                        needs it (redo tier, flat_half = 1, calls without an fp16 mirror),
 *   "hnsw_heap_walk_queries"  HNSW queries answered by the any-size heap walk (max(ef, k) > 1024, or the LDS candidate
 *                        pool of the fast walk overflowed),
 *   "hnsw_half_dropped"  of the last HNSW call's distance evaluations (vdb_hnsw_last_stats), the rows its certified
 *                        half-precision pre-pass ruled out without fetching the f32 row,
 *   "ivf_last_offers", "ivf_last_kept_q8", "ivf_last_kept"  (while vdb_prof_enable is on) rows the last IVF call offered to its result
 *                        sets, the ones the 8-bit tier passed on (0: tier not run) and the ones that reached the exact stage; "ivf_last_rows_fetched_q8":
 *                        rows the cluster-major 8-bit tier read, once each (0: query-major),
 *   "mask_where_masks"   masks built on the device from the label columns (vdb_mask_create_where*); "mask_where_set_masks": the ones
 *                        built from set / range terms (vdb_mask_create_where_sets*); "mask_where_any_masks": the ones built from an OR of
 *                        conjunctions (vdb_mask_create_where_any*); "mask_combine_masks": the ones vdb_mask_combine made;
 *                        "mask_partition_masks": the ones vdb_mask_create_partition made; "label_count_calls":
 *                        vdb_index_label_counts calls; "label_columns": allocated columns,
 *   "label_lookup_calls" vdb_index_label_lookup calls that were accepted; "label_lookup_codes": the codes they named;
 *                        "label_lookup_direct": the calls that ran the direct route; "label_lookup_passes": reads of the column, summed,
 *   "flat_dup_calls"     vdb_flat_dup_groups / _device calls that succeeded; "flat_dup_chunks": the range calls under them;
 *                        "flat_dup_pairs": the non-self pairs they saw,
 *   "update_calls"       vdb_index_update_rows / _device calls that changed rows (m > 0, not refused); "update_rows": the rows they rewrote,
 *   "fetch_calls"        vdb_index_get_rows* calls that fetched rows (m > 0, not refused); "fetch_rows": the rows they returned;
 *                        "fetch_chunks": their gather launches; "fetch_direct": the calls answered by one plain copy,
 *   "hbm_bytes_per_row"  resident HBM bytes per row over all per-row buffers (rows, norms, mirrors, PQ codes, level-0 links, label
 *                        columns). */
int vdb_get_stat(const vdb_index *idx, const char *name, uint64_t *out);

/* ---- PQTable (distance/pq_table.rs) ----------------------------------------------------
 * centroids: group g, centroid c at k_c*gstart[g] + c*len(g) (pq_groups, pq_table.rs:38-53),
 * k_c = 1<<n_bits, total k_c*dim floats.  codes: n x ceil(m*n_bits/8), 4-bit low nibble = even
 * group (pq_table.rs:66-91); NULL -> encoded on the GPU (pq_encode + find_nearest_base). */
int vdb_pq_attach(vdb_index *idx, uint64_t n_bits, uint64_t m, const float *centroids, const uint8_t *codes);
/* PQTable::from_vec_set (pq_table.rs:141-191): sample train_n rows (0 = all), per-group k-means
 * (k_means.rs:61-162) on the host, encode on the GPU.  RNG = splitmix64(seed). */
int vdb_pq_build(vdb_index *idx, uint64_t n_bits, uint64_t m, uint64_t train_n, uint64_t max_iter, float tol,
                 uint64_t seed);
int vdb_pq_clear(vdb_index *idx);                 /* MetadataVecTable::clear_pq_table :154-156 */
int vdb_pq_has(const vdb_index *idx, int *out);
int vdb_pq_info(const vdb_index *idx, uint64_t *n_bits, uint64_t *m, uint64_t *enc_dim);
int vdb_pq_export(const vdb_index *idx, float *centroids, uint8_t *codes);
/* PQTable::create_lookup (pq_table.rs:195-224) for nq queries, as the search kernels build it: out_lut [nq][m * k_c]
 * row-major [group][centroid] (l2 of the query slice to the centroid for L2Sqr, their dot product for Cosine),
 * out_qcache [nq] = PQLookupTable::dist_cache (0 for L2Sqr, |q| for Cosine).  Either output may be NULL. */
int vdb_pq_create_lookup(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, float *out_lut, float *out_qcache);
/* the ADC adapter DistanceAdapter<[u8], PQLookupTable> (pq_table.rs:239-301) of every code row: out [nq][len], the values
 * the knn_pq scan ranks (strict group-order f32 sums; Cosine: 1 - sum / max(sqrt(sum cent_cache) * |q|, 1e-10)) */
int vdb_pq_adc_all(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, float *out);
/* FlatIndex::knn_pq (flat_index.rs:84-104) */
int vdb_flat_knn_pq(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, uint64_t k, uint64_t ef,
                    uint64_t *out_idx, float *out_dist, uint64_t *out_count);

/* device-pointer variant (queries / outputs on the index's GPU); returns synchronised */
int vdb_flat_knn_pq_device(vdb_index *idx, const void *d_queries, uint64_t nq, uint64_t dim, uint64_t k, uint64_t ef,
                           void *d_out_idx, void *d_out_dist, void *d_out_count, void *stream);

/* ---- HNSWIndex (index_algorithm/hnsw_index.rs) -----------------------------------------
 * Graph layout (fields :98-141): level0 = n x max_m0 u32 (max_m0 = 2*min(M,10000)), len0[n];
 * vec_level[n]; upper = CSR over nodes, node v level L>=1 at ((sum_{u<v} vec_level[u]) + L-1)*m,
 * upper_len likewise. */
int vdb_hnsw_build(vdb_index *idx, uint64_t M, uint64_t ef_construction, uint64_t seed, uint64_t batch,
                   int nthreads);                  /* build_on_vec_set :595-611 (host builder) */
int vdb_hnsw_attach(vdb_index *idx, uint64_t M, uint64_t ef_construction, const uint32_t *level0,
                    const uint64_t *len0, const uint64_t *vec_level, const uint32_t *upper,
                    const uint64_t *upper_len, int has_enter, uint64_t enter_point, uint64_t enter_level);
int vdb_hnsw_clear(vdb_index *idx);               /* MetadataVecTable::clear_hnsw_index :100-106 */
int vdb_hnsw_has(const vdb_index *idx, int *out);
int vdb_hnsw_info(const vdb_index *idx, uint64_t *m, uint64_t *max_m0, uint64_t *upper_total, int *has_enter,
                  uint64_t *enter_point, uint64_t *enter_level, uint64_t *default_ef);
int vdb_hnsw_export(const vdb_index *idx, uint32_t *level0, uint64_t *len0, uint64_t *vec_level, uint32_t *upper,
                    uint64_t *upper_len);
/* HNSWIndex::knn_with_ef (:619-634); ef = 0 -> default_ef (knn, :614-618).
 * A walk is one wavefront and the chip keeps 2048 of them resident (8 per CU): throughput is flat from ~4096 queries per call
 * on (584k QPS at 1M x 960, ef = 128), a call of ~1000 queries is one round of walks and bounded by the longest of them
 * (2.6 ms), smaller calls take the time of one walk.  Any k / ef (beyond 1024 the heap walk answers). */
int vdb_hnsw_knn(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, uint64_t k, uint64_t ef,
                 uint64_t *out_idx, float *out_dist, uint64_t *out_count);
/* HNSWIndex::knn_pq (:672-697) */
int vdb_hnsw_knn_pq(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, uint64_t k, uint64_t ef,
                    uint64_t *out_idx, float *out_dist, uint64_t *out_count);
/* device-pointer variant of knn_with_ef (use_pq = 0) / knn_pq (use_pq = 1); returns synchronised */
int vdb_hnsw_knn_device(vdb_index *idx, const void *d_queries, uint64_t nq, uint64_t dim, uint64_t k, uint64_t ef,
                        int use_pq, void *d_out_idx, void *d_out_dist, void *d_out_count, void *stream);
/* per-call work counters of the last vdb_hnsw_knn on this index (SURVEY 8d bytes/query) */
int vdb_hnsw_last_stats(const vdb_index *idx, uint64_t *n_dist, uint64_t *n_expanded);

/* ---- shard merge ------------------------------------------------------------
 * Merge S per-shard result lists (each [nq][k], ascending, counts[s][q] valid entries, global ids)
 * into the global top-k by (distance, index).  Host utility used after the RCCL all-gather. */
int vdb_merge_topk(const float *dists, const uint64_t *ids, const uint64_t *counts, uint64_t n_shards,
                   uint64_t nq, uint64_t k, uint64_t *out_idx, float *out_dist, uint64_t *out_count);

/* same merge on the index's GPU (inputs = the all-gathered tensors, ids < 2^32); returns synchronised.
 * The three device merges keep an id in 32 bits of a pair key: every id in the lists must be below 2^32 (the host merge above carries
 * 64).  The lists are not inspected; a call is refused when `idx` itself reports id_offset + len > 2^32, when n_shards is 0, or
 * when k is outside 1..1024. */
int vdb_merge_topk_device(vdb_index *idx, const void *d_dists, const void *d_ids, const void *d_counts,
                          uint64_t n_shards, uint64_t nq, uint64_t k, void *d_out_idx, void *d_out_dist,
                          void *d_out_count, void *stream);

/* same merge reading the S per-rank blocks of ONE all-gather buffer in place (block s at s*block_bytes; ids, distances
 * and counts at the given byte offsets inside a block): no repacking between the collective and the merge.  Ids < 2^32 and
 * n_shards >= 1, as for vdb_merge_topk_device. */
int vdb_merge_topk_gathered(vdb_index *idx, const void *d_gathered, uint64_t block_bytes, uint64_t off_ids,
                            uint64_t off_dists, uint64_t off_counts, uint64_t n_shards, uint64_t nq, uint64_t k,
                            void *d_out_idx, void *d_out_dist, void *d_out_count, void *stream);

/* the same, ENQUEUED on `stream` (the stream the all-gather was issued on) without any host synchronisation, k <= 64: the
 * exchange of one step can then run under the next step's search (outputs are valid once `stream` has passed this point).
 * Ids < 2^32 and n_shards >= 1, as for vdb_merge_topk_device. */
int vdb_merge_topk_gathered_async(vdb_index *idx, const void *d_gathered, uint64_t block_bytes, uint64_t off_ids,
                                  uint64_t off_dists, uint64_t off_counts, uint64_t n_shards, uint64_t nq, uint64_t k,
                                  void *d_out_idx, void *d_out_dist, void *d_out_count, void *stream);

/* ---- merge of range results (row shards; csrc/k_range_merge.hip) ------------------------------------------------------------------
 * Shard s of a row-sharded corpus answers a range search (vdb_flat_range with GLOBAL ids, vdb_index_set_id_offset) with a CSR result:
 * lims_s [nq + 1] (lims_s[0] = 0, relative to the shard's own pairs) and its pairs, per query ascending by (distance, id).  The answer
 * on the whole corpus is the union of the shards' pairs in the same order, cut after `limit` pairs per query (0 = no limit) -- the first
 * `limit` of the union are among the first `limit` of every shard, so the shards may have been asked with the same limit.
 *   lims  [n_shards][nq + 1];  ids (u64) / dists (f32) of shard s start at element s * pair_stride of their arrays (pair_stride >= the
 *   largest lims_s[nq]: the padded blocks of an all-gather).  Ids are full 64-bit values (id_offset + row may pass 2^32) and must differ
 *   between shards; no NaN distances (a NaN is never inside a radius); -0.0 and +0.0 compare equal (the id decides), as in every search.
 *   Pairs that are equal in distance AND id across shards are taken in shard order.
 * vdb_range_merge: host utility, works without a GPU (the twin of vdb_merge_topk).  out_lims [nq + 1] is always written:
 * out_lims[q + 1] - out_lims[q] = min(limit, sum over s of the query's count).  out_idx / out_dist hold out_lims[nq] pairs; pass both as
 * NULL to obtain the offsets (and so the size) alone.
 * vdb_range_merge_device: the same on the index's GPU from device buffers (the all-gathered tensors), at most 256 shards; synchronises
 * `stream` first, returns synchronised, and hands back a result object to be read with vdb_range_lims / vdb_range_copy and released
 * with vdb_range_destroy.  One lane per input pair places it by rank (its position in its own list + S - 1 binary searches in the
 * others); a query of at most 4096 pairs is searched in LDS, longer ones in global memory.  Memory: 12 B per returned pair in the result
 * object + 16 B per query.  A result above the index's "flat_range_max_results" ceiling, or one that cannot be allocated, fails the call
 * with an error as in vdb_flat_range: nothing is returned, nothing aborts.
 * Both calls reject lims that do not start at 0, decrease, or declare more pairs than pair_stride (an error, not a crash); with
 * consistent lims the device merge stays inside its buffers whatever the pairs hold.  "range_merge" in vdb_prof_get is the kernel's time. */
int vdb_range_merge(const uint64_t *lims, const uint64_t *ids, const float *dists, uint64_t n_shards, uint64_t nq, uint64_t pair_stride,
                    uint64_t limit, uint64_t *out_lims, uint64_t *out_idx, float *out_dist);
int vdb_range_merge_device(vdb_index *idx, const void *d_lims, const void *d_ids, const void *d_dists, uint64_t n_shards, uint64_t nq,
                           uint64_t pair_stride, uint64_t limit, void *stream, vdb_range **out);

/* ---- IVFIndex (index_algorithm/ivf_index.rs) ------------------------------
 * from_vec_set (:66-118): k-means over all columns on train_n sampled rows (0 = all; host, RNG = splitmix64(seed),
 * parity unpinned), then every row joins its nearest centroid (k_means.rs:40-57: CandidatePair order) -- computed on
 * the GPU in reference arithmetic, bit-exact given the centroids.  Writes to the index (add) drop the clusters. */
int vdb_ivf_build(vdb_index *idx, uint64_t k_clusters, uint64_t train_n, uint64_t max_iter, float tol, uint64_t seed);
/* centroids: k_clusters x dim; assign: cluster of every row (n values) or NULL -> computed as above */
int vdb_ivf_attach(vdb_index *idx, uint64_t k_clusters, const float *centroids, const uint64_t *assign);
int vdb_ivf_clear(vdb_index *idx);
int vdb_ivf_info(const vdb_index *idx, int *present, uint64_t *k_clusters, uint64_t *default_n_probes);
int vdb_ivf_export(vdb_index *idx, float *centroids, uint64_t *assign);
/* IVFIndex::knn_with_ef (:143-154), ef = n_probes (0 -> default_n_probes = 4, :108): probes by find_n_nearest
 * (k_means.rs:174-190), then ResultSet::add over the probed clusters in probe order, rows ascending */
int vdb_ivf_knn(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, uint64_t k, uint64_t n_probes,
                uint64_t *out_idx, float *out_dist, uint64_t *out_count);

/* device-pointer variant; returns synchronised */
int vdb_ivf_knn_device(vdb_index *idx, const void *d_queries, uint64_t nq, uint64_t dim, uint64_t k, uint64_t n_probes,
                       void *d_out_idx, void *d_out_dist, void *d_out_count, void *stream);

/* ---- row-sharded FlatIndex::knn_pq -------------------------------------------
 * pq_resort (candidate_pair.rs:102-108) replays ResultSet::add in the GLOBAL (ADC distance, id) order, so the
 * exchange carries, per shard and query, max(ef,k) pair keys twice: the ADC key row (ascending) and the exact-distance
 * key of the same row at the same position.  A pair key is orderable(f32) << 32 | global row id (id_offset + local
 * row, < 2^32); ~0 pads rows shorter than max(ef,k).  Layout [nq][max(ef,k)] u64 each. */
int vdb_flat_knn_pq_shard(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, uint64_t k, uint64_t ef,
                          uint64_t *out_adc_keys, uint64_t *out_exact_keys);
int vdb_flat_knn_pq_shard_device(vdb_index *idx, const void *d_queries, uint64_t nq, uint64_t dim, uint64_t k,
                                 uint64_t ef, void *d_out_adc_keys, void *d_out_exact_keys, void *stream);
/* merge of the all-gathered rows ([n_shards][nq][efk], efk = max(ef,k)) to the global ADC top-efk, then the
 * reference's re-sort (flat_index.rs:100-103): out [nq][k] ascending exact distances, global ids.  Host utility. */
int vdb_pq_merge_resort(const uint64_t *adc_keys, const uint64_t *exact_keys, uint64_t n_shards, uint64_t nq,
                        uint64_t efk, uint64_t k, uint64_t *out_idx, float *out_dist, uint64_t *out_count);
/* same on the index's GPU; returns synchronised */
int vdb_pq_merge_resort_device(vdb_index *idx, const void *d_adc_keys, const void *d_exact_keys, uint64_t n_shards,
                               uint64_t nq, uint64_t efk, uint64_t k, void *d_out_idx, void *d_out_dist,
                               void *d_out_count, void *stream);

/* ---- multi-GPU context (vdb_ctx_create; SURVEY 8e: row shards + one RCCL all-gather) ------------------------
 * The library owns the RCCL communicator and the exchange: a host needs no collective library of its own.
 *   vdb_ctx_create        ONE process drives n_dev GPUs (ncclCommInitAll): the layout of a Rust host, whose DynamicIndex
 *                         (dynamic_index.rs:11-94) lives in one process;
 *   vdb_ctx_create_rank   one process per GPU (ncclCommInitRank): rank 0 obtains a 128-byte id from vdb_ctx_unique_id, the
 *                         host distributes it (MPI, a file, torch.distributed's store ...), every rank passes it in.
 * RCCL is loaded at run time (dlopen) by the first context that needs a communicator (world > 1).
 * Two environment variables, both read when a context is created, exist for the tests of this layer on a 1-GPU box:
 *   VDB_CTX_FORCE_RCCL=1  builds the communicator even for one rank, so that the real (1-rank) ncclAllGather calls run;
 *   VDB_CTX_LOOPBACK=1    vdb_ctx_create only: the same device id may appear more than once, every entry becomes a rank of its own
 *                         (world = n_dev, ranks 0..n_dev-1), NO communicator is built (vdb_ctx_info: has_comm = 0) and the exchange
 *                         is done with device copies between the local shards.  Partition, block layouts, merges, the two-phase
 *                         range exchange, the replica query split and the per-shard host threads then run as they do with n_dev
 *                         GPUs.  A test seam, not a way to gain throughput: S shards of one GPU share that GPU and add the
 *                         exchange on top.  Refused (invalid argument) together with VDB_CTX_FORCE_RCCL=1; vdb_ctx_create_rank
 *                         ignores it. */
typedef struct vdb_ctx vdb_ctx;
typedef struct vdb_sharded vdb_sharded;
int vdb_ctx_create(const int *device_ids, int n_dev, vdb_ctx **out);
int vdb_ctx_unique_id(void *out_id, uint64_t out_bytes /* >= 128 */);
int vdb_ctx_create_rank(int device_id, const void *id, int rank, int world, vdb_ctx **out);
int vdb_ctx_destroy(vdb_ctx *ctx);
int vdb_ctx_info(const vdb_ctx *ctx, int *world, int *n_local, int *first_rank, int *has_comm);
/* DynamicIndex::new(dim, dist) over all GPUs of the context: rank r of S holds rows [r * ceil(N/S), (r+1) * ceil(N/S))
 * of the corpus handed to vdb_sharded_set_rows (every process passes the same N x dim view) and reports global ids. */
int vdb_sharded_create(vdb_ctx *ctx, uint64_t dim, int dist, vdb_sharded **out);
int vdb_sharded_destroy(vdb_sharded *sh);
int vdb_sharded_set_rows(vdb_sharded *sh, const float *rows, uint64_t n_total);
int vdb_sharded_len(const vdb_sharded *sh, uint64_t *out);
/* borrowed handle of this process's i-th shard (statistics, tuning switches, exports); owned by the sharded index */
int vdb_sharded_local(vdb_sharded *sh, int i, vdb_index **out);
/* FlatIndex::knn (flat_index.rs:48-57) over the whole corpus: per-shard top-k, ONE all-gather of [nq,k] ids / distances /
 * counts per rank, exact merge by (distance, index) -- equal to the unsharded answer.  k <= 1024. */
int vdb_sharded_flat_knn(vdb_sharded *sh, const float *queries, uint64_t nq, uint64_t dim, uint64_t k, uint64_t *out_idx,
                         float *out_dist, uint64_t *out_count);
/* PQTable replicated on every shard (same centroids; codes encoded per shard on its GPU) and FlatIndex::knn_pq
 * (flat_index.rs:84-104) over the whole corpus: ADC key rows + exact key rows gathered, merged in (adc, idx) order, then
 * pq_resort (candidate_pair.rs:102-108) -- equal to the unsharded answer. */
int vdb_sharded_pq_attach(vdb_sharded *sh, uint64_t n_bits, uint64_t m, const float *centroids);
int vdb_sharded_knn_pq(vdb_sharded *sh, const float *queries, uint64_t nq, uint64_t dim, uint64_t k, uint64_t ef,
                       uint64_t *out_idx, float *out_dist, uint64_t *out_count);
/* REPLICA layout ("HNSW: replicas only"): every GPU of the context keeps ALL rows (ids are global as they are);
 * a search splits the QUERIES instead -- rank r of S answers the block [r * ceil(nq/S), min(nq, (r+1) * ceil(nq/S)))
 * (vdb_replica_query_block) and ONE fixed-size all-gather concatenates the blocks on every rank; no merge.  All of
 * DynamicIndex's searches (dynamic_index.rs:68-93) run in this layout: vdb_sharded_flat_knn and vdb_sharded_knn_pq accept it
 * as well as the row layout (any k), the HNSW searches below exist only here (a graph's edges cross any row partition).
 * vdb_sharded_layout: 0 = no rows yet, 1 = row blocks (vdb_sharded_set_rows), 2 = replicas. */
int vdb_sharded_set_rows_replica(vdb_sharded *sh, const float *rows, uint64_t n_total);
int vdb_sharded_layout(const vdb_sharded *sh, int *out);
int vdb_replica_query_block(uint64_t nq, uint64_t world, uint64_t rank, uint64_t *q0, uint64_t *q1);
/* HNSWIndex over the replicas: built once per process on its first GPU (hnsw_index.rs:391-457 through vdb_hnsw_build's host
 * builder; deterministic for a given seed / batch / thread count, so the processes of a multi-process job hold equal graphs)
 * or attached from arrays (vdb_hnsw_attach's layout), then mirrored to the process's other GPUs. */
int vdb_sharded_hnsw_build(vdb_sharded *sh, uint64_t M, uint64_t ef_construction, uint64_t seed, uint64_t batch, int nthreads);
int vdb_sharded_hnsw_attach(vdb_sharded *sh, uint64_t M, uint64_t ef_construction, const uint32_t *level0, const uint64_t *len0,
                            const uint64_t *vec_level, const uint32_t *upper, const uint64_t *upper_len, int has_enter,
                            uint64_t enter_point, uint64_t enter_level);
/* HNSWIndex::knn_with_ef (hnsw_index.rs:619-634; ef = 0 -> the graph's default) / knn_pq (:672-697) with the queries split
 * over the replicas -- equal to the single-GPU answer row by row. */
int vdb_sharded_hnsw_knn(vdb_sharded *sh, const float *queries, uint64_t nq, uint64_t dim, uint64_t k, uint64_t ef, uint64_t *out_idx,
                         float *out_dist, uint64_t *out_count);
int vdb_sharded_hnsw_knn_pq(vdb_sharded *sh, const float *queries, uint64_t nq, uint64_t dim, uint64_t k, uint64_t ef, uint64_t *out_idx,
                            float *out_dist, uint64_t *out_count);
/* IVFIndex over the replicas (ivf_index.rs:66-154): clusters built once per process (seeded, so equal in every process) and
 * mirrored to its other GPUs; knn_with_ef(ef = n_probes; 0 -> the default 4) with the queries split. */
int vdb_sharded_ivf_build(vdb_sharded *sh, uint64_t k_clusters, uint64_t train_n, uint64_t max_iter, float tol, uint64_t seed);
int vdb_sharded_ivf_knn(vdb_sharded *sh, const float *queries, uint64_t nq, uint64_t dim, uint64_t k, uint64_t n_probes, uint64_t *out_idx,
                        float *out_dist, uint64_t *out_count);
/* Exact range search (the vdb_flat_range block above) over the whole corpus of a sharded index: the answer of vdb_flat_range on the
 * unsharded rows, pair for pair, with global ids, on every rank.  The result object lives on the process's FIRST local GPU and, like
 * every vdb_range, does not depend on the sharded index after the call (it may outlive vdb_sharded_destroy).
 * ROWS layout: every shard runs the local range search with the same radii and limit, then a two-phase exchange per chunk of 2048
 * queries: phase 1, fixed size, carries every rank's nq + 1 CSR offsets, one status word and the rank's result ceiling; phase 2 the pairs, every rank's block padded
 * to the largest shard total phase 1 reported (ids and distances in one block), skipped when that is 0; then the device merge of
 * vdb_range_merge_device on the first local GPU.  REPLICA layout: rank r answers the query block vdb_replica_query_block(chunk, world, r),
 * the same two phases, and the blocks are concatenated in query order (no merge).  Without a communicator (one rank) the local result is
 * the answer and nothing is exchanged.
 * Memory, on top of vdb_flat_range's on every shard: the send block (largest shard total of the chunk x 12 B) and the receive buffer
 * (S x that) on every local GPU while the chunk is exchanged -- released when the call returns -- and the result (12 B per pair).
 * nq == 0, an index without rows, a dim mismatch, NaN / infinite / negative radii: as for vdb_flat_range.  vdb_flat_set_mode and
 * vdb_set_param of the local indexes (vdb_sharded_local) apply.  "flat_range_max_results" bounds every shard's local result of a chunk,
 * and the SMALLEST value set on any rank bounds the chunk's merged (ROWS) / concatenated (REPLICA) result.
 * Failure: a LOCAL range search that fails (the ceiling, device memory) still takes part in phase 1, with status != 0 and no pairs; every
 * rank reads the same status words, skips phase 2 and returns the same error.  Likewise a chunk whose merged total -- known on every rank
 * from phase 1's offsets -- passes the smallest ceiling fails on every rank before phase 2.  In both cases the object is NOT poisoned and
 * the next call may succeed.  An error inside a collective, or after phase 1 has committed the ranks to phase 2 (the staging buffers or
 * the result cannot be allocated), poisons the object in a multi-process job as below.
 * Exercised on hardware with ONE rank over RCCL (both phases as real 1-rank ncclAllGather calls under VDB_CTX_FORCE_RCCL=1, the merge with
 * S = 1) and with 3 and 8 ranks on one GPU through the loopback exchange (VDB_CTX_LOOPBACK=1: both phases, the merge, the concatenation,
 * a failing rank's status word and the merged-total check with S > 1).  World > 1 over RCCL itself -- several GPUs, several processes -- is
 * correct by construction, not by test. */
int vdb_sharded_flat_range(vdb_sharded *sh, const float *queries, uint64_t nq, uint64_t dim, const float *radius, uint64_t limit,
                           vdb_range **out);
/* Failed sharded calls.  vdb_sharded_set_rows[_replica] is all-or-nothing: when one GPU fails (out of memory, say) every
 * shard is rolled back to an empty index and the call may be repeated.  A SEARCH that fails on one rank of a multi-PROCESS
 * context (vdb_ctx_create_rank, world > 1) may leave the other ranks inside the all-gather; the object is then "poisoned"
 * (vdb_sharded_poisoned -> 1) and refuses further searches with VDB_ERR_STATE-style errors: destroy it on every rank.
 * RCCL has run on hardware with ONE rank only (the test boxes have one GPU): ncclCommInitAll and grouped all-gathers over several
 * local GPUs, cross-process ordering and the poisoning above are correct by construction, not by test.  Everything around the
 * collective runs with up to 8 ranks on one GPU under VDB_CTX_LOOPBACK=1 (tests/test_ctx_many_shards_gpu.py). */
int vdb_sharded_poisoned(const vdb_sharded *sh, int *out);

/* ---- measurement hooks -------------------------------------------------------------------
 * When enabled, the dominant kernels are bracketed by HIP events on their own stream and the
 * elapsed time is accumulated per kernel name ("flat_mfma", "flat_exact", "pq_adc", "hnsw"). */
int vdb_prof_enable(vdb_index *idx, int on);
/* attainable HBM read bandwidth of this box: a pure streaming read of `bytes` (> the 256-MB Infinity Cache)
 * repeated `iters` times, best of two access patterns, in GB/s (1e9 B/s).  Allocates and frees its own buffer. */
int vdb_stream_probe(int device_id, uint64_t bytes, int iters, double *out_gbps);
/* the same bytes read the way the Flat filter would have to read them if its fp16 operand were the ROW-MAJOR image the graph
 * walks gather from (one fp16 copy of the rows instead of two): MFMA A-fragment loads, 16 rows x 64 B per instruction, rows of
 * row_bytes (a multiple of 128, e.g. 1920 = a 960-d fp16 row).  The A/B behind DESIGN's "two fp16 images" note.  Measurement hook. */
int vdb_stream_probe_rows(int device_id, uint64_t bytes, int iters, uint32_t row_bytes, double *out_gbps);
/* matrix-pipe rate of this box under sustained load: v_mfma_f32_16x16x32_f16 (the Flat filter's instruction) issued back to back
 * by `waves_per_simd` waves on every SIMD, `iters` x 8 independent tiles per wave; dense TFLOP/s of the launch and the shader
 * clock (GHz) the chip held meanwhile.  Measurement hook. */
int vdb_mfma_probe(int device_id, int waves_per_simd, int iters, double *out_tflops, double *out_clock_ghz);
/* the same for v_mfma_i32_16x16x64_i8, the instruction of the 8-bit Flat filter (k_gemm8.hip): dense integer TOP/s.  The filter's
 * matrix-pipe roofline is quoted against the chip's nominal int8 peak AND against this sustained rate.  Measurement hook. */
int vdb_mfma_probe_i8(int device_id, int waves_per_simd, int iters, double *out_tops, double *out_clock_ghz);
/* latency of one DEPENDENT HBM access on this box: a single lane follows a random cycle over the 128-B lines of a `bytes`-sized
 * buffer (larger than L2 and the Infinity Cache) for `hops` loads; nanoseconds per load.  The floor of the graph walks
 * (hnsw_index.rs:258-291 is a chain of dependent accesses per expansion) is quoted on it.  Measurement hook. */
int vdb_latency_probe(int device_id, uint64_t bytes, uint32_t hops, double *out_ns_per_load);
/* latency of one DEPENDENT f32 add: the reference's distances are strict left folds (distance/mod.rs:72-77), so a d-column row
 * is a chain of d of them on whatever hardware; nanoseconds per add over a chain of `adds`.  Measurement hook. */
int vdb_fold_probe(int device_id, uint32_t adds, double *out_ns_per_add);
int vdb_prof_reset(vdb_index *idx);
int vdb_prof_get(vdb_index *idx, const char *kernel, double *total_ms, uint64_t *launches, double *bytes);

#ifdef __cplusplus
}
#endif
#endif /* VDBHIP_H */
