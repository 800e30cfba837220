// kernels.hpp -- launch wrappers of the gfx950 kernels (definitions in k_*.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dup_plan.hpp"
#include "fuse_groups_plan.hpp"
#include "fuse_plan.hpp"
#include "grouped_plan.hpp"
#include "labels_scatter_plan.hpp"
#include "like_plan.hpp"
#include "lookup_plan.hpp"
#include "mask_any.hpp"
#include "mask_partition.hpp"
#include "mask_sets.hpp"
#include "mmr_plan.hpp"

namespace vdb {

// how a (row, query) pair turns into a distance; all folds are strict left-to-right f32
enum Metric : int {
    MET_L2_DIRECT = 0,  // sum (x-q)^2                     distance/mod.rs:75-77   (Flat, re-sorts)
    MET_COSINE = 1,     // 1 - dot/max(|x||q|,1e-10)       distance/mod.rs:60-69
    MET_L2_CACHED = 2,  // (xx + qq) - 2*dot(x,q)          distance/mod.rs:54-57   (HNSW)
};

// ---- k_exact.hip ---------------------------------------------------------------------------
// sq[i] = dot(x_i, x_i) in reference order (DistanceAlgorithm::dist_cache, distance/mod.rs:31-36)
void launch_row_sqnorm(const float *X, uint64_t n, uint32_t dim, float *sq, hipStream_t s);
// dense exact distances out[b*ld + i] for nq (<= 8) queries against rows [0,n)
void launch_scan_exact(const float *X, uint64_t n, uint32_t dim, const float *Q, uint32_t nq, int metric,
                       const float *xsq, const float *qsq, float *out, uint64_t ld, bool use_lds, hipStream_t s);
// exact distance of every candidate: in/out are pair keys [nq][ldc]; PAIR_NONE entries pass through
void launch_rerank(const float *X, uint32_t dim, const float *Q, uint32_t nq, int metric, const float *xsq,
                   const float *qsq, const uint64_t *cand, uint64_t *out, uint32_t ncand, uint32_t ldc,
                   hipStream_t s, const uint32_t *cnt = nullptr);  // cnt: counted lists (first cnt[q] slots of a row)
// first `ksel` pair keys of each query -> (u64 id + id_offset, f32 distance) at out[q*kstride + j],
// out_count[q] = number of valid pairs
void launch_finalize(const uint64_t *keys, uint32_t ldk, uint32_t nq, uint32_t ksel, uint32_t kstride,
                     uint64_t id_offset, uint64_t *out_idx, float *out_dist, uint64_t *out_count, hipStream_t s);
// certification of an MFMA shortlist (see k_exact.hip): flags[q] = 1 when the exact top-k might
// not be contained in the shortlist
void launch_iota_keys(uint64_t *rows, uint32_t nq, uint32_t n, uint32_t ld, hipStream_t s);
// rounding of the shortlist keys' operands: qerr == nullptr -> split-bf16 (format constants); otherwise the measured
// errors of the fp16 operands (k_half.hip): dx_abs = max |dx_r|, dx_rel = max |dx_r| / |x_r|, qerr[q] = |dq|
struct SplitErr {
    const float *qerr = nullptr;
    float dx_abs = 0.0f, dx_rel = 0.0f;
    // 8-bit pass (k_gemm8.hip / k_i8.hip): the keys are lower bounds, D(r, q) >= key + qoff[q]; |mu| of the centring vector
    const float *qoff = nullptr;
    float mu_norm = 0.0f;
};
void launch_flat_finish(const uint64_t *exact_sorted, uint32_t lde, const uint64_t *approx_sorted, uint32_t lda,
                        uint32_t nq, uint32_t ksel, uint32_t kstride, uint32_t kprime, uint64_t n_rows, const float *qsq,
                        float xsq_max, float xsq_min_pos, int cosine, uint32_t dim, SplitErr se, const uint32_t *cnt, uint32_t cap,
                        uint64_t id_offset, uint8_t *flags, uint64_t *out_idx, float *out_dist, uint64_t *out_count,
                        hipStream_t s);
// the exact stage of the Flat pipeline fused into one launch (k' <= 64, k <= 64, dim % 4 == 0): counted select of the hit
// list + re-rank + sort + certification + outputs (k_exact.hip)
constexpr uint32_t FLAT_CAND_CAP = 8192;  // slots of a query's hit list in every Flat filter pass
struct FlatTailArgs {
    const uint64_t *cand;  // [nq][cap] hit lists of the filter pass
    uint32_t cap;
    const uint32_t *cnt;   // [nq]
    uint32_t kprime, ksel, kstride;
    const float *X;        // row-major rows
    uint32_t dim;
    const float *Q;
    int metric;            // MET_L2_DIRECT or MET_COSINE
    const float *xsq, *qsq;
    uint64_t n_rows;
    float xsq_max, xsq_min_pos;
    int cosine;
    SplitErr se;
    uint64_t id_offset;
    uint8_t *flags;
    uint64_t *out_idx;
    float *out_dist;
    uint64_t *out_count;
    unsigned long long *stamps = nullptr;  // k_flat_tail_lb, builds with -DVDB_TAIL_STAMPS: [nq][32] phase stamps (s_memtime)
    const float *tau = nullptr;  // k_flat_tail_lb: the filter pass's thresholds (the bound of every row outside the hit list)
    uint32_t *qstat = nullptr;   // k_flat_tail_lb, optional (flat_i8_stats): per query rounds walked | hit count << 8
};
// the exact stage behind the 8-bit pass: walks the hit list in key order, 64 keys per round (kprime / 64 rounds at most)
bool flat_tail_lb_supported(uint32_t dim, uint32_t kprime, uint32_t ksel);
void launch_flat_tail_lb(const FlatTailArgs &a, uint32_t nq, hipStream_t s);
// all candidates of a few queries evaluated at once (the second 8-bit attempt of a handful of queries): exact_keys nq x a.cap, topk nq x topk_capacity(ksel)
void launch_flat_full_lb(const FlatTailArgs &a, uint32_t nq, uint64_t *exact_keys, uint64_t *topk, hipStream_t s);
void flat_tail_lb_set_nw(int v);  // waves per query: 0 auto, 8 / 4 / 2 / 1
void flat_tail_lb_set_walk(int v);  // 0: a selection per four rounds, rows the k-th distance excludes not fetched; 1: a selection per round
bool flat_tail64_supported(uint32_t dim, uint32_t kprime, uint32_t ksel);
void launch_flat_tail64(const FlatTailArgs &a, uint32_t nq, hipStream_t s);
// k_small.hip: FlatIndex::knn of a few queries over a small table in ONE launch (the db.search() shape): coalesced rows ->
// products -> strict fold per lane -> in-kernel (distance, index) top-k -> outputs.  dim % 4 == 0, k <= 64, nq <= 64.
struct FlatSmallArgs {
    const float *X;        // row-major rows
    uint64_t n;
    uint32_t dim;
    const float *Q;        // [nq][dim]; device memory or device-visible pinned host memory
    int metric;            // MET_L2_DIRECT or MET_COSINE
    const float *xsq;      // row norms (Cosine)
    uint64_t *part;        // flat_small_part_keys() pair keys of scratch
    uint32_t *counter;     // [nq] arrival counters, zero on entry, zero again on exit
    uint32_t ksel, kstride;
    uint64_t id_offset;
    uint64_t *out_idx;     // device memory or device-visible pinned host memory
    float *out_dist;
    uint64_t *out_count;
};
bool flat_small_supported(uint64_t n, uint32_t dim, uint64_t nq, uint64_t k);
uint32_t flat_small_rows_per_wg(uint64_t n, int num_cu);
size_t flat_small_part_keys(uint64_t n, uint64_t nq, uint32_t ksel, int num_cu);
void launch_flat_small(const FlatSmallArgs &a, uint32_t nq, int num_cu, hipStream_t s);
void launch_certify(const uint64_t *exact_sorted, uint32_t lde, const uint64_t *approx_sorted, uint32_t lda,
                    uint32_t nq, uint32_t k, uint32_t kprime, uint64_t n_rows, const float *qsq, float xsq_max,
                    float xsq_min_pos, int cosine, uint32_t dim, uint8_t *flags, hipStream_t s);

void launch_extract_tau(const uint64_t *sorted, uint32_t ld, uint32_t nq, uint32_t kprime, float *tau, hipStream_t s);
void launch_flag_overflow(const uint32_t *cnt, uint32_t cap, uint32_t min_hits, uint32_t nq, uint8_t *flags,
                          hipStream_t s);

// ---- k_topk.hip ----------------------------------------------------------------------------
// rows per level-1 list
// keys one wave of k_topk_dense selects from: short key rows (threshold samples) are cut finer so that nq x lists
// waves fill the chip; long rows keep the level-2 merge small
uint32_t topk_chunk(uint64_t n);
uint32_t topk_num_lists(uint64_t n);
// tau[q] = kth smallest of keys[q][0..n) (k_select_tau, n <= select_tau_max_n())
// queries >= nq_real (batch padding) get tau = -inf
void launch_select_tau(const float *keys, uint64_t ld, uint32_t n, uint32_t nq, uint32_t nq_real, uint32_t kth, float *tau,
                       hipStream_t s);
uint32_t select_tau_max_n();
uint32_t topk_capacity(uint32_t k);  // entries per list (multiple of 64, >= k)
// level 1: dense f32 keys[q*ld + i], i in [0,n) -> lists[q][list][cap] sorted ascending pair keys
void launch_topk_dense(const float *keys, uint64_t ld, uint64_t n, uint32_t nq, uint32_t k, uint64_t *lists,
                       hipStream_t s);
// level 2: merge `nlists` lists of `cap_in` pair keys per query -> out[q][cap] sorted ascending
void launch_topk_merge(const uint64_t *lists, uint32_t nlists, uint32_t cap_in, uint32_t nq, uint32_t k,
                       uint64_t *out, hipStream_t s);

// level 2 over ONE list per query of which only the first min(cnt[q], cap_in) entries are scanned
void launch_topk_merge_counted(const uint64_t *lists, uint32_t cap_in, const uint32_t *cnt, uint32_t nq, uint32_t k,
                               uint64_t *out, hipStream_t s);
// shard merge for k <= 64 in one launch (wave per query); strides in BYTES between consecutive shards' arrays
void launch_merge_shards64(const float *dists, const uint64_t *ids, const uint64_t *counts, uint64_t stride_d,
                           uint64_t stride_i, uint64_t stride_c, uint32_t S, uint32_t nq, uint32_t k, uint64_t *out_idx,
                           float *out_dist, uint64_t *out_count, hipStream_t s);
void launch_pack_pairs(const float *dists, const uint64_t *ids, const uint64_t *counts, uint64_t stride_d,
                       uint64_t stride_i, uint64_t stride_c /* bytes between shards */, uint32_t S, uint32_t nq, uint32_t k,
                       uint32_t cap_in, uint64_t *lists, hipStream_t s);

// ---- k_u8.hip: VecSet<u8> rows at one byte per element (scalar.rs:117-119, distance/mod.rs:79-95) -------------------
void launch_widen_u8(const uint8_t *in, uint64_t count, float *out, hipStream_t s);
void launch_scan_exact_u8(const uint8_t *X, uint64_t n, uint32_t dim, const float *Q, uint32_t nq, int metric, const float *xsq,
                          const float *qsq, float *out, uint64_t ld, hipStream_t s);
void launch_rerank_u8(const uint8_t *X, uint32_t dim, const float *Q, uint32_t nq, int metric, const float *xsq, const float *qsq,
                      const uint64_t *cand, uint64_t *out, uint32_t ncand, uint32_t ldc, hipStream_t s);

// ---- k_probe.hip ---------------------------------------------------------------------------
// attainable HBM read bandwidth in GB/s: pure streaming read of `bytes`, `iters` timed passes, best of two patterns
double stream_probe(int device, uint64_t bytes, int iters);
double stream_probe_pattern(int device, uint64_t bytes, int iters, int pattern, uint32_t row_bytes);  // 1: MFMA-fragment loads from row-major rows
void mfma_probe(int device, int waves_per_simd, int iters, double *tflops, double *clock_ghz, int i8 = 0);
double latency_probe(int device, uint64_t bytes, uint32_t hops);
double fold_probe(int device, uint32_t adds);  // ns per dependent f32 add (the strict fold's chain)  // ns per dependent HBM load (pointer chase over 128-B lines)

// ---- k_sort.hip (k > 1024) -----------------------------------------------------------------
size_t sort_pairs_temp_bytes(uint64_t n);
void launch_sort_pairs(const float *dist, uint64_t n, uint64_t *tmp_keys, uint64_t *out, void *temp, size_t temp_bytes,
                       hipStream_t s);

// any-size fallbacks (k, ef, n_probes beyond the 1024 pairs the register-resident selects hold):
// every row of pair keys [nq][ld] sorted ascending (in != out); temp = sort_rows_temp_bytes(nq, ld) bytes
size_t sort_rows_temp_bytes(uint64_t nq, uint64_t ld);
void launch_sort_rows(const uint64_t *in, uint64_t *out, uint64_t nq, uint64_t ld, void *temp, size_t temp_bytes, hipStream_t s);
void launch_pair_keys_rows(const float *dist, uint64_t ldd, uint64_t n, uint32_t nq, uint64_t *keys, uint64_t ldk, hipStream_t s);
void launch_copy_prefix(const uint64_t *in, uint64_t ld_in, uint64_t *out, uint64_t ld_out, uint64_t count, uint32_t nq, hipStream_t s);
// ResultSet::add replayed over the offers [nq][ldc] (first ncand of every row, in order; PAIR_NONE skipped), set capacity
// k: out [nq][ldo >= k] = the set, unsorted, PAIR_NONE padded
void launch_resort_big(const uint64_t *offers, uint32_t ncand, uint32_t ldc, uint32_t nq, uint32_t k, uint64_t *out, uint32_t ldo,
                       hipStream_t s);

// ---- k_mfma.hip ----------------------------------------------------------------------------
uint32_t mfma_batch(uint32_t dim);  // queries per workgroup batch: 32 (dim <= 1024), 16 (dim <= 2048), 0 = unsupported
// Q [nq][dim] -> ceil(nq/32) fragment-ordered split-bf16 images of mfma_qfrag_floats(dim) floats each
void launch_mfma_pack_queries(const float *Q, uint32_t nq, uint32_t nq_cover, uint32_t dim, float *qfrag, hipStream_t s);
// fragment-ordered mirror of rows: tiles [tile0, tile1) of 16 rows each; T holds ceil(n/16) tiles rounded up to 4
void launch_tile_rows(const float *X, uint64_t n, uint32_t dim, uint64_t tile0, uint64_t tile1, float *T,
                      hipStream_t s);
// the list forms of the three re-tiling kernels (launch_tile_rows, _h, _i8): the n_tiles tiles named by the device array `tiles`
// (ascending, no duplicates), same bytes per tile as the range forms
void launch_tile_rows_list(const float *X, uint64_t n, uint32_t dim, const uint32_t *tiles, uint64_t n_tiles, float *T, hipStream_t s);
// approximate keys key(i,q) = xsq[i] - 2*dot(x_i, q); XT = fragment-ordered mirror; qfrag = nbatch images.
// sample: keys of a strided sample of rows, dense: out[q*ld + j], j < mfma_sample_rows(n, step) (+inf past n)
// cosine != 0: keys are -dot(x_i,q)/|x_i| (0 for zero rows), which rank like the cosine distance
void launch_flat_mfma_sample(const float *XT, uint64_t n, uint32_t dim, const float *qfrag, uint32_t nbatch,
                             const float *xsq, int cosine, uint32_t step, float *out, uint64_t ld, int num_cu,
                             hipStream_t s);
// filter: ONE launch walks all nbatch passes; pair keys of all rows with key <= tau[q] land in cand[q][0..cap)
// (cnt[q] counts every hit, so cnt[q] > cap means candidates were dropped)
void launch_flat_mfma_filter(const float *XT, uint64_t n, uint32_t dim, const float *qfrag, uint32_t nbatch,
                             const float *xsq, int cosine, const float *tau, uint64_t *cand, uint32_t *cnt,
                             uint32_t cap, uint32_t *sync /* mfma_sync_words() zeroed words */, int num_cu, hipStream_t s);
size_t mfma_sync_words(uint32_t nbatch, int num_cu);
// k_gemm.hip: the same filter for groups of gemm_group() = 128 queries per corpus pass; qfrag = images packed with
// launch_mfma_pack_queries_nh(.., 8, ..), tau / cand / cnt indexed by the global query number as above
// qmul == nullptr: split-bf16 operands (launch_tile_rows / launch_mfma_pack_queries_nh); otherwise the scaled fp16
// operands of k_half.hip and qmul[q] = 1 / (row scale * query scale).  cnt[ngroups * 128 .. + 127] are the arrival counters of the
// cooperative sets: ZERO on entry (launch_query_prep_h / the caller's memset), part of the same allocation as cnt
void launch_flat_gemm_filter(const float *XT, uint64_t n, uint32_t dim, const float *qfrag, const float *qmul, uint32_t ngroups,
                             const float *xsq, int cosine, const float *tau, uint64_t *cand, uint32_t *cnt,
                             uint32_t cap, int debug, int num_cu, hipStream_t s);
uint32_t gemm_group();
// threshold sample with the same kernel: every unit_step-th unit of rows, dense keys out[q*ld + j]
uint64_t gemm_sample_rows(uint64_t n, uint32_t unit_step);
void launch_flat_gemm_sample(const float *XT, uint64_t n, uint32_t dim, const float *qfrag, const float *qmul, uint32_t ngroups,
                             const float *xsq, int cosine, uint32_t unit_step, float *out, uint64_t ld, int num_cu,
                             hipStream_t s);
void gemm_set_tw(int v);
void gemm_set_zigzag(int v);   // odd query groups walk the corpus backwards: 0 auto, 1 off, 2 on
void gemm_set_nt(int v);       // X-stream cache policy of the filter pass: 0 auto (non-temporal when the mirror exceeds the Infinity Cache), 1 default policy, 2 non-temporal
void gemm_set_block_rows(uint64_t v);  // filter pass in row blocks (one launch per block, all query groups): 0 off (default), n rows
void gemm_set_stagger(int v);  // 0 (default): workgroups start together; n: start delays of up to n unit steps
bool gemm_f16_supported(uint32_t dim);
// k_half.hip: scaled fp16 mirror / query images for the GEMM_F16 variant and their measured rounding errors
void launch_tile_rows_h(const float *X, uint64_t n, uint32_t dim, uint64_t tile0, uint64_t tile1, float sx, void *T,
                        hipStream_t s);
void launch_tile_rows_h_list(const float *X, uint64_t n, uint32_t dim, const uint32_t *tiles, uint64_t n_tiles, float sx, void *T,
                             hipStream_t s);
void launch_row_split_err(const float *X, const float *xsq, uint64_t row0, uint64_t row1, uint32_t dim, float sx,
                          uint32_t *out2 /* [2] float bits: max |dx|^2, max |dx|^2/|x|^2 (atomicMax) */, hipStream_t s);
void launch_rows_to_half(const float *X, uint64_t count, float sx, uint16_t *H, hipStream_t s);
void launch_rows_to_q8(const float *X, uint64_t n, uint32_t dim, int8_t *Q8, float *scale, float *err, hipStream_t s);
void launch_query_prep_h(const float *Q, uint32_t nq, uint32_t nq_pad, uint32_t dim, float sx, float *qsq /* out: |q|^2, strict order */,
                         float *qscale, float *qmul, float *qerr, uint32_t *hits /* zeroed */,
                         void *qfrag /* non-null: also write the query image of launch_pack_queries_h(.., NH = 8, ..) */, hipStream_t s);
void launch_pack_queries_h(const float *Q, uint32_t nq, uint32_t nq_cover, uint32_t dim, uint32_t NH, const float *qscale,
                           void *qfrag, hipStream_t s);
void launch_mfma_pack_queries_nh(const float *Q, uint32_t nq, uint32_t nq_cover, uint32_t dim, uint32_t NH, float *qfrag,
                                 hipStream_t s);
// k_gemm8.hip / k_i8.hip: the 8-bit pass (centred int8 mirror, lower-bound keys)
constexpr uint32_t I8_MEAN_CHUNKS = 64;
bool gemm8_supported(uint32_t dim);
void gemm8_set_nt(int v);
void gemm8_set_kc(int v);
void gemm8_set_burst(int v);
uint32_t gemm8_last_coop();   // set size of the most recent 8-bit filter launch (0: no cooperative sets)
uint32_t gemm_last_coop();
void gemm_set_coop(int v);    // the same for the fp16 / split-bf16 filter kernel
void gemm8_set_grid(int v);   // measurement: workgroups of the cooperative 8-bit filter (0 = one per CU; else a multiple of 32, throws otherwise)
void gemm8_set_epi(int v);    // unit epilogue of k_flat_gemm8: 0 = scalar key arithmetic, stage carried over units; 1 = packed arithmetic, one drain per unit
void gemm8_set_coop(int v);   // 0 auto (the workgroups of an XCD share one row stream through its L2 when the shape allows), 1 off
void gemm8_set_res(int v);
void gemm8_set_sample_res(int v);    // 0 auto (the query group's whole image resident in LDS when it fits), 1 off (chunked staging)
uint64_t gemm8_sample_rows(uint64_t n, uint32_t unit_step);
// (cnt[ngroups * 128 .. + 127]: the arrival counters of the cooperative sets, zero on entry -- launch_query_prep_i8 clears them)
void launch_flat_gemm8_filter(const void *XT, uint64_t n, uint32_t dim, const void *qfrag, const float *qscale, uint32_t ngroups,
                              const float *rowc, const float *tau, uint64_t *cand, uint32_t *cnt, uint32_t cap, int debug, int num_cu,
                              hipStream_t s, uint32_t hits_expected = 0);
void launch_flat_gemm8_sample(const void *XT, uint64_t n, uint32_t dim, const void *qfrag, const float *qscale, uint32_t ngroups,
                              const float *rowc, uint32_t unit_step, float *out, uint64_t ld, int num_cu, hipStream_t s, int unit_min = 0);
uint64_t gemm8_sample_units(uint64_t n, uint32_t unit_step);
// xsq_cos != null / cosine != 0: the Cosine form -- unit rows / unit queries (k_i8.hip); xsq_cos = the rows' cached strict-fold |x|^2
void launch_i8_col_mean(const float *X, uint64_t n, uint32_t dim, float *part /* I8_MEAN_CHUNKS * dim */, float *mu, hipStream_t s,
                        const float *xsq_cos = nullptr);
void launch_i8_row_stats(const float *X, uint64_t n, uint32_t dim, const float *mu, uint64_t n_s, uint64_t stride,
                         float *stats /* 2 * round_up(n_s, 16) */, hipStream_t s, const float *xsq_cos = nullptr);
void launch_tile_rows_i8(const float *X, uint64_t n, uint32_t dim, uint64_t tile0, uint64_t tile1, const float *mu, float l1, float l2,
                         void *T, float *rowc, hipStream_t s, const float *xsq_cos = nullptr);
void launch_tile_rows_i8_list(const float *X, uint64_t n, uint32_t dim, const uint32_t *tiles, uint64_t n_tiles, const float *mu, float l1,
                              float l2, void *T, float *rowc, hipStream_t s, const float *xsq_cos = nullptr);
// k_remove.hip: moves[2 j] = dst, [2 j + 1] = src -- row src -> row dst (row_bytes bytes each) and sq[src] -> sq[dst]; every src above
// every dst (a removal plan, remove_plan.hpp)
void launch_rows_move(void *rows, uint64_t row_bytes, float *sq, const uint32_t *moves, uint64_t n_moves, int num_cu, hipStream_t s);
// k_update.hip: row j of src (m contiguous rows) -> row ids[j] of `rows` and sq_new[j] -> sq[ids[j]]; the ids are distinct (update_plan.hpp)
void launch_rows_scatter(void *rows, uint64_t row_bytes, float *sq, const uint32_t *ids, const void *src, const float *sq_new, uint64_t m,
                         int num_cu, hipStream_t s);
// k_fetch.hip: row ids[j] - id_offset of `rows` -> row j of dst (m contiguous rows); ids: u32 local rows (id_offset 0) or, ids_u64, u64
// global ids; any order, repeats allowed; the ids are checked by the caller (fetch_plan.hpp, launch_fetch_check).  dst of any alignment.
void launch_rows_gather(const void *rows, uint64_t row_bytes, const void *ids, bool ids_u64, uint64_t id_offset, void *dst, uint64_t m,
                        int num_cu, hipStream_t s);
// ... over u8 rows of `dim` bytes into f32 output rows, (float)byte
void launch_rows_gather_widen(const uint8_t *rows, uint64_t dim, const void *ids, bool ids_u64, uint64_t id_offset, float *dst, uint64_t m,
                              int num_cu, hipStream_t s);
// *flag = 1 when some ids[j] - id_offset is not in [0, n) (flag zeroed by the caller)
void launch_fetch_check(const uint64_t *ids, uint64_t m, uint64_t n, uint64_t id_offset, uint32_t *flag, int num_cu, hipStream_t s);
// the same for an id of the counted part ids[b][0 .. min(counts[b], ld)) of a list b < nq of an [nq][ld] block
void launch_list_check(const uint64_t *ids, const uint64_t *counts, uint64_t nq, uint64_t ld, uint64_t n, uint64_t id_offset, uint32_t *flag,
                       hipStream_t s);
void launch_query_prep_i8(const float *Q, uint32_t nq, uint32_t nq_pad, uint32_t dim, const float *mu, float l1, float l2, float *qsq,
                          float *qscale, float *qoff, uint32_t *hits, void *qfrag, hipStream_t s, int cosine = 0);
// k_redo.hip: second attempts of a Flat call
void launch_gather_rows_f32(const float *src, const uint64_t *rows, uint64_t nr, uint32_t width, float *dst, hipStream_t s);
void launch_scatter_results(const uint64_t *ri, const float *rd, const uint64_t *rc, const uint64_t *rows, uint64_t nr, uint32_t k,
                            uint64_t *o_idx, float *o_dist, uint64_t *o_cnt, hipStream_t s);
void launch_gather_dk(const float *o_dist, const uint64_t *o_cnt, const uint64_t *rows, uint64_t nr, uint32_t k, uint32_t ksel, float *dk,
                      hipStream_t s);
// tighter lower-bound keys for the hit lists of the 8-bit pass from the row-major fp16 image (k_redo.hip); max_hits = longest list to cover
void launch_flat_refine_half(const uint16_t *rows_h, uint32_t dim, float sx, float dx_abs, float dx_rel, int cosine, const float *Q, const float *xsq,
                             const float *qsq, const float *qoff, uint64_t *cand, uint32_t cap, const uint32_t *cnt, uint32_t nq, uint32_t max_hits,
                             hipStream_t s);
void launch_i8_tau_from_dk(const float *dk, uint32_t nq, uint32_t nq_pad, const float *qoff, const float *qsq, float xsq_max, float mu_norm,
                           uint32_t dim, int cosine, float *tau, hipStream_t s);
// k_range.hip: exact Flat range search (Index::flat_range_device)
constexpr uint32_t RANGE_LEFT = 0xFFFFFFFFu;  // launch_range_cut's count of a query the 8-bit tier does not answer
// tau[q] (launch_i8_tau_from_dk with dk = radius) -> -inf unless flat_lb_excludes(radius[q], tau[q]) holds (common.hpp)
void launch_range_admit(const float *radius, uint32_t nq, const float *qoff, const float *qsq, float xsq_max, float xsq_min_pos, float mu_norm,
                        uint32_t dim, int cosine, float *tau, hipStream_t s);
// keys [nq][cap]: exact pair keys of the counted hit lists -> first o_cnt[q] slots of the row = the pairs with distance <= radius[q], ascending;
// o_cnt[q] = RANGE_LEFT for a query that was not admitted (tau = -inf) or whose list overflowed; o_hits[q] = length of its hit list
void launch_range_cut(uint64_t *keys, uint32_t cap, const uint32_t *cnt, const float *radius, const float *tau, uint32_t nq, uint32_t *o_cnt,
                      uint32_t *o_hits, hipStream_t s);
// dense distances [nq][ld] of rows [0, n): blk [nq][range_scan_blocks(n)] = first output slot of every row segment, total[q] = rows inside the radius
uint32_t range_scan_blocks(uint64_t n);
void launch_range_scan_select(const float *dist, uint64_t ld, uint64_t n, const float *radius, uint32_t nq, uint32_t *blk, uint32_t *total,
                              hipStream_t s);
// ... their pair keys in row order at out[q * ldo ..) (slots past total[q] are left as they are)
void launch_range_compact(const float *dist, uint64_t ld, uint64_t n, const float *radius, uint32_t nq, const uint32_t *blk_off, uint64_t *out,
                          uint64_t ldo, hipStream_t s);
// pool[off[q] + j] = keys[q * ld + j], j < take[q] <= max_take;  off / take / lims: device memory or device-visible pinned host memory
void launch_range_append(const uint64_t *keys, uint64_t ld, const uint64_t *off, const uint32_t *take, uint32_t nq, uint64_t max_take, uint64_t *pool,
                         hipStream_t s);
// out_idx / out_dist [lims[q], lims[q + 1]) = the pairs pool[off[q] ..) as (row + id_offset, distance)
void launch_range_gather(const uint64_t *pool, const uint64_t *off, const uint64_t *lims, uint64_t nq, uint64_t max_take, uint64_t id_offset,
                         uint64_t *out_idx, float *out_dist, hipStream_t s);
// k_filter.hip: filtered Flat search over a row allow-list (Index::flat_knn_masked_device, the mask of Index::flat_range_device)
// dense exact distances out[q * ld + j] = D(row ids[j], query q), j < m, for any nq (8 queries per fetch of a row; ids ascending, u32)
void launch_scan_gather(const float *X, const uint32_t *ids, uint64_t m, uint32_t dim, const float *Q, uint32_t nq, int metric, const float *xsq,
                        const float *qsq, float *out, uint64_t ld, bool use_lds, hipStream_t s);
// launch_finalize for pair keys whose low word is a COLUMN of that output: the id written is ids[column] + id_offset
void launch_filter_finalize(const uint64_t *keys, uint64_t ldk, uint32_t nq, uint32_t ksel, uint32_t kstride, const uint32_t *ids, uint64_t m,
                            uint64_t id_offset, uint64_t *out_idx, float *out_dist, uint64_t *out_count, hipStream_t s);
// The gathered scan for MANY (mask, query group) pairs in one launch (Index::flat_knn_masked_multi_device, multi_plan.hpp): one workgroup
// per work item.  An item's queries are the slots [slot, slot + nb) of the chunk, slot s being query slot_q[s] of Q / qsq and row s of out.
struct GroupedItem {
    const uint32_t *ids;  // the mask's ascending allow-list (device)
    uint32_t m;           // its length
    uint32_t tile;        // the item's allowed rows: columns [tile * 256, min(m, tile * 256 + 256))
    uint32_t slot;        // first slot
    uint32_t nb;          // 1..8 slots
};
// out[(slot + b) * ld + j] = D(row ids[j], query slot_q[slot + b]) for every item, b < nb and column j of its tile; any dim
void launch_scan_gather_grouped(const float *X, uint32_t dim, const GroupedItem *items, uint64_t nitems, const uint32_t *slot_q, const float *Q,
                                int metric, const float *xsq, const float *qsq, float *out, uint64_t ld, hipStream_t s);
// The same work items for a RANGE call (Index::flat_range_masked_multi_device): instead of storing D, every pair with
// D <= radius[slot_q[slot + b]] appends its key (orderable(D), ROW ids[j]) to keys[(slot + b) * ld + ..] at the position cnt[slot + b]
// hands out (cnt: zeroed u32 per slot; keys: filled with PAIR_NONE, ld >= every m).  Unordered within a slot; cnt[s] <= m afterwards.
void launch_range_gather_grouped(const float *X, uint32_t dim, const GroupedItem *items, uint64_t nitems, const uint32_t *slot_q, const float *Q,
                                 int metric, const float *xsq, const float *qsq, const float *radius, uint64_t *keys, uint64_t ld, uint32_t *cnt,
                                 hipStream_t s);
// launch_filter_finalize with a list, a length and an output position per slot: slot s holds the keys of query slot_q[s] over the columns
// of slot_ids[s] (slot_m[s] of them); columns at and past slot_m[s] are padding.  Writes all kstride slots and the count of that query.
void launch_filter_finalize_grouped(const uint64_t *keys, uint64_t ldk, uint32_t nslots, uint32_t ksel, uint32_t kstride, const uint32_t *const *slot_ids,
                                    const uint32_t *slot_m, const uint32_t *slot_q, uint64_t id_offset, uint64_t *out_idx, float *out_dist,
                                    uint64_t *out_count, hipStream_t s);
// out[r] = bit r of `bits` set or r >= n ? rowc[r] : {+inf, 0}, r < rows_pad (the {C_r, M_r} pairs of the 8-bit pass)
void launch_mask_rowc(const float *rowc, const uint64_t *bits, uint64_t n, uint64_t rows_pad, float *out, hipStream_t s);
// tau[q] = min(tau[q], FLT_MAX), NaN -> -inf: no threshold lets the +inf key of a masked row through
void launch_tau_clamp(float *tau, uint32_t nq, hipStream_t s);
// dist[q * ld + i] = NaN for the rows i < n whose bit is clear
void launch_mask_dense_nan(float *dist, uint64_t ld, uint64_t n, uint32_t nq, const uint64_t *bits, hipStream_t s);
// k_labels.hip: label columns (Index::d_labels) and the row masks built from them on the device (index_masks.hip)
constexpr uint32_t LABEL_COLUMNS = 16;       // VDB_LABEL_COLUMNS
constexpr uint32_t LABEL_NONE = 0xFFFFFFFFu;  // VDB_LABEL_NONE: a row without a value in that column
constexpr uint32_t MASK_MAX_TERMS = 8;        // VDB_MASK_MAX_TERMS
static_assert(SETS_LABEL_COLUMNS == LABEL_COLUMNS && SETS_LABEL_NONE == LABEL_NONE && SETS_MAX_TERMS == MASK_MAX_TERMS, "mask_sets.hpp and kernels.hpp agree");
struct LabelCols {  // the allocated columns of an index (kernel argument, by value)
    uint32_t *col[LABEL_COLUMNS];
    uint32_t n;
};
struct MaskTerm {
    const uint32_t *col;  // the term's column, nullptr: never written (every row reads LABEL_NONE)
    uint32_t code;
};
struct MaskJob {
    uint64_t *bits;   // the mask's d_bits
    uint32_t t0, t1;  // its terms: [t0, t1) of the term table
};
// col[r] = LABEL_NONE, r0 <= r < r1, in every column of cols
void launch_label_fill(const LabelCols &cols, uint64_t r0, uint64_t r1, int num_cu, hipStream_t s);
// col[moves[2 j]] = col[moves[2 j + 1]], j < n_moves, in every column of cols (the move list of launch_rows_move) / the one move dst <- src
void launch_label_move(const LabelCols &cols, const uint32_t *moves, uint64_t n_moves, int num_cu, hipStream_t s);
void launch_label_move_one(const LabelCols &cols, uint32_t dst, uint32_t src, hipStream_t s);
// Scattered label writes (labels_scatter_plan.hpp; k_labels_scatter, k_labels_set_mask), ONE launch per call whatever the column count.
static_assert(SCATTER_LABEL_COLUMNS == LABEL_COLUMNS, "labels_scatter_plan.hpp and kernels.hpp agree");
struct LabelSet {  // (column, code) pairs of a write by mask (kernel argument, by value)
    uint32_t *col[LABEL_COLUMNS];
    uint32_t code[LABEL_COLUMNS];
    uint32_t n;
};
// list entries one launch covers before its grid-stride loop wraps: 256 x (max_blocks, or 8 blocks per CU when max_blocks is 0)
uint64_t labels_scatter_span(int num_cu, uint32_t max_blocks);
// cols.col[c][ids[j] - id_offset] = codes[c * m + j], c < cols.n, j < m; ids: u32 local rows (id_offset 0) or, ids_u64, u64 global ids,
// checked by the caller (labels_scatter_plan.hpp, launch_fetch_check); cols here = the TARGET columns in the caller's order
void launch_labels_scatter(const LabelCols &cols, const void *ids, bool ids_u64, uint64_t id_offset, const uint32_t *codes, uint64_t m,
                           int num_cu, uint32_t max_blocks, hipStream_t s);
// set.col[c][ids[j]] = set.code[c], c < set.n, j < m; ids = a RowMask's d_ids
void launch_labels_set_mask(const LabelSet &set, const uint32_t *ids, uint64_t m, int num_cu, uint32_t max_blocks, hipStream_t s);
// workgroups per mask of the mask kernels = entries per mask of blockcnt: four 64-row words each
inline uint32_t mask_where_blocks(uint64_t n) { return (uint32_t)(((n + 63) / 64 + 3) / 4); }
// The three predicates a mask is built from (k_mask_rows<Pred>; kernel argument, by value; the bodies are in k_labels.hip).  A job's
// [t0, t1) indexes `terms` -- for MaskAny the clause table clims, whose clims[c] .. clims[c + 1] are the clause's terms.
struct MaskEq {  // every `column == code` term (Index::masks_where)
    const MaskTerm *terms;
    __device__ bool operator()(const MaskJob &job, uint64_t row, bool in) const;
};
struct MaskAll {  // every set / range term (Index::masks_where_sets; the term table of mask_sets.hpp, bitmaps resident on the device)
    const SetTerm *terms;
    __device__ bool operator()(const MaskJob &job, uint64_t row, bool in) const;
};
struct MaskAny {  // every term of some clause (Index::masks_where_any; mask_any.hpp)
    const SetTerm *terms;
    const uint32_t *clims;
    __device__ bool operator()(const MaskJob &job, uint64_t row, bool in) const;
};
// bit words of n_masks masks over rows [0, n) from their jobs under pred, then blockcnt [n_masks][mask_where_blocks(n)] = exclusive prefix
// of the allowed rows per block and totals[g] = allowed rows of mask g  (k_mask_rows<Pred> + k_mask_scan; n_masks <= 65535; the three above)
template <class Pred>
void launch_mask_rows(Pred pred, const MaskJob *jobs, uint32_t n_masks, uint64_t n, uint32_t *blockcnt, uint32_t *totals, hipStream_t s);
// out = AND / OR over the bit words of n_in finished masks over the same n rows, input i complemented first when bit i of invert is set;
// bits at and past n clear; blockcnt / totals as above for the one mask  (k_mask_combine + k_mask_scan)
constexpr uint32_t MASK_COMBINE_MAX = 8;
constexpr int MASK_OP_AND = 0, MASK_OP_OR = 1;  // VDB_MASK_OP_AND / VDB_MASK_OP_OR
struct MaskCombine {  // (kernel argument, by value)
    const uint64_t *in[MASK_COMBINE_MAX];
    uint32_t n_in, invert;
    int op;
};
void launch_mask_combine(const MaskCombine &a, uint64_t *out, uint64_t n, uint32_t *blockcnt, uint32_t *totals, hipStream_t s);
// ids[g][0 .. totals[g]) = the allowed rows of mask g, ascending (k_mask_ids; after launch_mask_rows on the same stream)
void launch_mask_ids(const MaskJob *jobs, uint32_t *const *ids, uint32_t n_masks, uint64_t n, const uint32_t *blockoff, hipStream_t s);
// One column grouped by code (mask_partition.hpp; k_mask_partition, k_label_counts).  table = the chunk's nb (<= PART_MAX_CHUNK) distinct
// codes ascending, then for each the mask (index into jobs) it belongs to: 2 nb u32 on the device.
static_assert(PART_LABEL_COLUMNS == LABEL_COLUMNS && PART_LABEL_NONE == LABEL_NONE, "mask_partition.hpp and kernels.hpp agree");
// The bit words of the nb masks "col == code" and blockcnt / totals as launch_mask_rows leaves them (k_mask_partition + k_mask_scan).
// The caller has zeroed the bit words of every mask and blockcnt [nb][mask_where_blocks(n)] on the same stream; col == nullptr: a
// column never written.
void launch_mask_partition(const uint32_t *col, const uint32_t *table, uint32_t nb, const MaskJob *jobs, uint64_t n, uint32_t *blockcnt,
                           uint32_t *totals, hipStream_t s);
// counts[i] += the rows allowed by bits (nullptr: every row) whose code is table[i]; the caller has zeroed counts [nb] on the same stream
void launch_label_counts(const uint32_t *col, const uint32_t *table, uint32_t nb, const uint64_t *bits, uint64_t n, uint32_t *counts,
                         int num_cu, hipStream_t s);
// The key lookup over one column (k_lookup.hip, lookup_plan.hpp): counts[i] += the rows whose code is entry i, first[i] = min(first[i],
// the lowest such row); the caller has set counts [..] to zero and first [..] to LOOKUP_ROW_NONE32 on the same stream.  Sorted route:
// table = a chunk's nb (<= PART_MAX_CHUNK) codes ascending, entry i = table[i].  Direct route: entry = slot_of[code - base] for codes in
// [base, base + span), none_slot for LABEL_NONE (LOOKUP_NO_SLOT: not asked for); launch_lookup_table fills slot_of [span] (set to
// LOOKUP_NO_SLOT by the caller) from the list's codes.  Grid: min(mask_where_blocks(n), max_blocks ? max_blocks : 8 x num_cu), grid-stride.
void launch_label_lookup(const uint32_t *col, const uint32_t *table, uint32_t nb, uint64_t n, uint32_t *counts, uint32_t *first, int num_cu,
                         uint32_t max_blocks, hipStream_t s);
void launch_label_lookup_direct(const uint32_t *col, const uint32_t *slot_of, uint32_t base, uint32_t span, uint32_t none_slot, uint64_t n,
                                uint32_t *counts, uint32_t *first, int num_cu, uint32_t max_blocks, hipStream_t s);
void launch_lookup_table(const uint32_t *codes, uint64_t n_codes, uint32_t base, uint32_t span, uint32_t *slot_of, int num_cu, hipStream_t s);
// Connected components over CSR edge lists (k_components.hip, dup_plan.hpp): a union-find over parent [n] (u32 per row), size [n] beside it.
// init: parent[i] = i, size[i] = 0.  hook: the pairs [0, total) of a CSR list over nq queries (lims [nq + 1] from 0, ids u64 = row +
// id_offset, checked by the caller); query q's source row is src64[q] - id_offset, else src32[q], else src_base + q; roots are hooked under
// lower roots by atomicCAS; counters[2] += the pairs whose ends differ, counters[3] += the lists of exactly `limit` entries (limit > 0).
// flatten: parent[i] = its root, group[i] = root + id_offset (DUP_ROW_NONE for a row bits -- nullptr: every row -- does not allow),
// size[root] = its rows, counters[0] += the roots of at least 2 rows, counters[1] += the rows under them.  counters: 4 u64, zeroed by the
// caller.  Integer atomics only: the answer does not depend on the order of waves.
void launch_comp_init(uint32_t *parent, uint32_t *size, uint64_t n, int num_cu, hipStream_t s);
void launch_comp_hook(const uint64_t *src64, const uint32_t *src32, uint64_t src_base, const uint64_t *lims, const uint64_t *ids, uint64_t nq,
                      uint64_t total, uint64_t id_offset, uint64_t limit, uint32_t *parent, uint64_t *counters, int num_cu, hipStream_t s);
void launch_comp_flatten(uint32_t *parent, const uint64_t *bits, uint64_t n, uint64_t id_offset, uint64_t *group, uint32_t *size, uint64_t *counters,
                         int num_cu, hipStream_t s);
// out[0] |= 1 when lims[0] != 0, the limits descend, or some src[q] / ids[j < lims[nq]] is no row of the index; out[1] = lims[nq]; out
// zeroed by the caller; nq > 0
void launch_pairs_check(const uint64_t *src, const uint64_t *lims, const uint64_t *ids, uint64_t nq, uint64_t n, uint64_t id_offset, uint64_t *out,
                        int num_cu, hipStream_t s);
// The capped walk of the grouped k-NN (k_group.hip, grouped_plan.hpp): query b's list ids / dists [b][0 .. min(counts[b], ld)) walked in the order
// given, at most g rows kept per value of `labels` (u32 per LOCAL row = id - id_offset; nullptr: a column never written; a row without a
// label is always kept), the first k kept pairs to row slot_q[b] (nullptr: b) of out_idx / out_dist [..][k] with zeros behind them, their
// number to out_cnt[that row], done[b] = k rows were kept | counts[b] < ld.  An id that is no row of the index is not gathered (it reads as
// unlabelled).  scratch: group_cap_scratch_bytes(nq, k, ld) bytes, 0 when the walk's table fits LDS.
size_t group_cap_scratch_bytes(uint64_t nq, uint64_t k, uint64_t ld);
void launch_group_cap(const uint64_t *ids, const float *dists, const uint64_t *counts, uint64_t nq, uint64_t ld, const uint32_t *labels, uint64_t n,
                      uint64_t id_offset, uint32_t k, uint32_t g, uint32_t *scratch, const uint32_t *slot_q, uint64_t *out_idx, float *out_dist,
                      uint64_t *out_cnt, uint8_t *done, hipStream_t s);
// The greedy selection of the diversified k-NN (k_mmr.hip, mmr_plan.hpp): from query b's list ids / dists [b][0 .. F), F = min(counts[b], ld),
// 1 <= ld <= MMR_MAX_FETCH, position 0 and then min(k, F) - 1 times the unselected position with the smallest
// (lambda * d_p) - ((1 - lambda) * min over the selected s of D(p, s)), ties to the lowest position; D = the exact distance between the ROWS
// id - id_offset of X [n][dim] (cosine: 1 - dot / max(|a| |b|, 1e-10) with xsq = the rows' strict-fold |x|^2; otherwise sum (a - b)^2).
// The selected pairs go in selection order to row slot_q[b] (nullptr: b) of out_idx / out_dist [..][k] with zeros behind them, their
// number to out_cnt[that row].  An id that is no row of the index is not gathered (its distances read as NaN).
void launch_mmr_select(const uint64_t *ids, const float *dists, const uint64_t *counts, uint64_t nq, uint64_t ld, const float *X, const float *xsq,
                       uint64_t n, uint32_t dim, bool cosine, uint64_t id_offset, uint32_t k, float lambda, const uint32_t *slot_q, uint64_t *out_idx,
                       float *out_dist, uint64_t *out_cnt, hipStream_t s);
// The search by example rows (k_like.hip, like_plan.hpp).  launch_like_build: out[q][j] for q < nq, j < dim = the "average vector" of query
// q's example rows of X [n][dim] -- ap = (strict left fold of the positives pos_ids[pos_lims[q] .. pos_lims[q + 1]) in list order) /
// their number; with negatives (neg_lims != nullptr and the query's range not empty) an likewise and (ap + ap) - an, otherwise ap.  The
// ids are u32 LOCAL rows, or (global_ids) u64 row + id_offset; the lims are device arrays of nq + 1 entries; out of any 4-byte alignment.
void launch_like_build(const void *pos_ids, const uint64_t *pos_lims, const void *neg_ids, const uint64_t *neg_lims, bool global_ids, uint64_t nq,
                       const float *X, uint64_t n, uint32_t dim, uint64_t id_offset, float *out, hipStream_t s);
// launch_like_drop: from query b's list ids / dists [b][0 .. min(counts[b], ld)), in the order given, the first k entries whose id is in
// neither a_ids[a_lims[b] .. a_lims[b + 1]) nor b_ids[b_lims[b] .. ) (a null lims: no such list; at most LIKE_MAX_EXAMPLES ids per query
// in all; u32 LOCAL rows to which id_offset is added, or u64 global ids) to out_idx / out_dist [b][k] with zeros behind them, their
// number to out_cnt[b].  k >= 1.
void launch_like_drop(const uint64_t *ids, const float *dists, const uint64_t *counts, uint64_t nq, uint64_t ld, const void *a_ids,
                      const uint64_t *a_lims, const void *b_ids, const uint64_t *b_lims, bool global_ids, uint64_t id_offset, uint32_t k,
                      uint64_t *out_idx, float *out_dist, uint64_t *out_cnt, hipStream_t s);
// The fusion of the fused multi-query search (k_fuse.hip, fuse_plan.hpp): fused query b owns the lists lims[b] .. lims[b + 1] - 1 (device
// array of nq + 1 entries; at most FUSE_MAX_LISTS each); list l is ids / dists [l - list_base][0 .. min(counts[l - list_base], ld)), walked as
// given, its weight weights[l] (nullptr: 1.0f).  mode FUSE_RRF: score = the left fold over the lists, ascending, of
// w / ((float)(position + 1) + c) at the row's FIRST position in the list, the answer descending by (score, then ascending row);
// FUSE_MIN: score = the smallest distance under the knn order, the bits of the first list that attains it, ascending by (score, row).
// The first min(k, distinct rows) go to out_idx (id_offset added) / out_dist [b][k] with zeros behind them, their number to out_cnt[b].
// lg = fuse_table_lg(most lists of a fused query, ld); scratch: fuse_scratch_bytes(nq, lg) bytes, unused while the table fits LDS.
// Every counted id must be a row of the index (id - id_offset < 2^32 - 1).
void launch_fuse_lists(const uint64_t *ids, const float *dists, const uint64_t *counts, uint64_t nq, uint64_t ld, const uint64_t *lims,
                       uint64_t list_base, const float *weights, int mode, float c, uint64_t id_offset, uint32_t k, uint32_t lg, uint32_t *scratch,
                       uint64_t *out_idx, float *out_dist, uint64_t *out_cnt, hipStream_t s);
// The fusion of the document-level fused search (k_fuse_groups.hip, fuse_groups_plan.hpp): the lists as for launch_fuse_lists, joined by
// GROUP -- the value of `labels` (u32 per LOCAL row; nullptr: a column never written) at the row, a row without one being a group of its
// own.  Per list a group counts at its first position: FUSE_RRF folds w / ((float)(rank among the list's groups + 1) + c), descending;
// FUSE_MIN takes the smallest such distance, ascending; FUSE_SUM folds that distance, or the list's last distance where the list does
// not hold the group, over every non-empty list, ascending.  The representative of a group is its row of the smallest (distance, list);
// ties in the order go to the lower representative.  The first min(k, groups) go to out_idx (representative + id_offset) / out_dist
// (score) [b][k] with zeros behind them, their number to out_cnt[b]; out_exact[b] (nullptr: not wanted) = no list counts trunc_len
// entries or more, or (FUSE_MIN) k groups came out and the k-th score is strictly before the last distance of every such list.
// lg = fuse_table_lg(most lists of a fused query, ld); scratch: fuse_groups_scratch_bytes(nq, lg) bytes, unused while the table fits LDS.
void launch_fuse_groups(const uint64_t *ids, const float *dists, const uint64_t *counts, uint64_t nq, uint64_t ld, const uint64_t *lims,
                        uint64_t list_base, const float *weights, const uint32_t *labels, uint64_t n, int mode, float c, uint64_t id_offset,
                        uint64_t trunc_len, uint32_t k, uint32_t lg, uint32_t *scratch, uint64_t *out_idx, float *out_dist, uint64_t *out_cnt,
                        uint8_t *out_exact, hipStream_t s);
// ---- k_pq.hip: product quantisation -- lookup tables, the ADC scans and their exact stages, encoder, re-sort, shard merge ----------
// The argument structs are filled by the search drivers (pq.hip); every launcher works out its own grid and dynamic LDS bytes.  Where a
// driver has to ASK whether a scan's LDS image fits before it chooses that scan, the same *_lds_bytes() the launcher uses answers.
void launch_pq_lut(const float *Q, uint32_t dim, const float *cent, const uint64_t *gstart, uint32_t m, uint32_t kc, int cosine, uint32_t nq,
                   float *lut, hipStream_t s);
void launch_pq_encode(const float *X, uint64_t n, uint32_t dim, const float *cent, const float *cent_cache, const uint64_t *gstart, uint32_t m,
                      uint32_t kc, uint32_t n_bits, int cosine, uint32_t enc_dim, uint8_t *codes, hipStream_t s);
// word-major mirror of the code rows: (n rounded up to 64) * nwords 16-B words
void launch_pq_tile_codes(const uint8_t *codes, uint64_t n, uint32_t enc_dim, uint32_t nwords, uint4 *tiled, hipStream_t s);
void launch_pq_resort(const uint64_t *exact_keys, uint32_t ncand, uint32_t ldc, uint32_t nq, uint32_t k, uint64_t *out, hipStream_t s);
// the f32 scan (k_pq_adc): MODE 0 dense, MODE 1 filter -- see the kernel
struct AdcArgs {
    const uint8_t *codes;
    uint64_t n;
    uint32_t enc_dim, m;
    const float *lut;         // [BQ][m*kc]
    const float *cent_cache;  // [m*kc]
    const float *qsq;         // [BQ]
    uint32_t nq;              // valid queries of this pass (<= BQ)
    int cosine;
    uint32_t blk_step;
    float *out;               // MODE 0
    uint64_t ld;
    const float *tau;         // MODE 1: [BQ]
    uint64_t *cand;           //         [BQ][cap]
    uint32_t *cnt;            //         [BQ]
    uint32_t cap;
    uint32_t nq_total;        // queries of the whole launch; blockIdx.y selects the sub-batch of BQ queries
    int fast;                 // batched-lookup inner loop (tuning switch, vdb_set_param "pq_adc_fast")
};
// queries per pass = as many f32 lookup tables (lut_bytes each; Cosine: the |centroid|^2 table beside them) as fit in 120 KB of LDS
// (<= 4), and the rows per row block = workgroup size that goes with it: 1024 with the tables in LDS, else 256 (tables through L1 / L2)
struct AdcPlan {
    uint32_t BQ, nt;
    bool in_lds;
};
AdcPlan pq_adc_plan(size_t lut_bytes, bool cosine);
void launch_pq_adc(const AdcArgs &a, uint32_t n_bits, int mode, int num_cu, hipStream_t s);
// 4-bit codes on 16-bit tables, 8 queries (Cosine: 7) per pass (k_pq_quant16, k_pq_adc16, k_pq_adc_exact)
constexpr uint32_t ADC16_Q = 8;          // queries per workgroup pass
struct Adc16Args {
    const uint4 *codes_t;    // word-major mirror of the code rows (k_pq_tile_codes)
    uint64_t n;
    uint32_t enc_dim, m;     // m = groups of the IMAGE (32 per code word, >= the table's m); enc_dim = bytes of a code row
    const uint4 *img;        // [ceil(nq/8)][m*16] 16-B entries
    const double *qM, *qD;   // [nq]
    const double *qMC, *qDC; // [nq] Cosine: offset / step of the |centroid|^2 table (identical for all queries)
    const float *qsq;        // [nq] Cosine: |q|^2
    const uint32_t *qflag;   // [nq]
    const float *tau;        // [nq]
    uint32_t nq;
    uint64_t rows_per_wg;    // multiple of 64
    uint64_t *cand;          // [nq][cap] row ids (upper word 0)
    uint32_t *cnt;           // [nq]
    uint32_t cap;
    // SAMPLE mode (threshold sample on the quantised tables): every blk_step-th 1024-row block, dense sums out
    uint32_t blk_step;       // >= 1
    float *s16_out;          // [nq][ld_s] quantised sums of the sampled rows as floats (exact: <= 65000 + m), +inf past n
    uint64_t ld_s;
};
size_t pq_adc16_lds_bytes(uint32_t nwords);  // nwords = 16-B code words per row
void launch_pq_quant16(const float *lut, const float *cent_cache, uint32_t m, uint32_t m_pad, uint32_t nq, int cosine, uint16_t *img, double *qM,
                       double *qD, double *qMC, double *qDC, uint32_t *qflag, hipStream_t s);
// sample: the strided sample of a.blk_step (L2Sqr only), as few workgroups per image group as still fill the chip; else the filter scan
void launch_pq_adc16(const Adc16Args &a, bool cosine, bool sample, uint32_t nwords, int num_cu, hipStream_t s);
void launch_pq_adc_exact(bool cosine, const uint8_t *codes, uint32_t enc_dim, uint32_t m, const float *lut, const float *cent_cache, const float *qsq,
                         const float *tau, uint64_t *cand, const uint32_t *cnt, uint32_t cap, uint32_t *valid, uint32_t nq, hipStream_t s);
// tau[q] = M + D (s* + m/2) from the r-th smallest quantised sample sum s* (in tau[q] on entry); +inf for a flagged table
void launch_pq_tau_from16(float *tau, const double *qM, const double *qD, const uint32_t *qflag, uint32_t m, uint32_t nq, hipStream_t s);
// 8-bit codes, one query per pass on a one-byte table (k_pq_quant8, k_pq_adc8)
struct Adc8Args {
    const uint4 *codes_t;   // word-major mirror of the (zero-padded) code rows
    uint64_t n;
    uint32_t nwords, m;     // 16-B code words per row; groups of the table (the image holds 16 * nwords of them)
    const uint8_t *img;     // [nq][16 * nwords * 256]
    const double *qM, *qD;
    const uint32_t *qflag;
    const float *tau;
    uint32_t nq;
    uint64_t rows_per_wg;   // multiple of 64
    uint64_t *cand;         // [nq][cap] row ids
    uint32_t *cnt;          // [nq]
    uint32_t cap;
    uint32_t blk_step;      // SAMPLE: every blk_step-th 1024-row block
    float *s8_out;          // SAMPLE: [nq][ld_s] quantised sums as floats, +inf past n
    uint64_t ld_s;
};
size_t pq_adc8_lds_bytes(uint32_t nwords);
void launch_pq_quant8(const float *lut, uint32_t m, uint32_t m_pad, uint32_t nq, uint8_t *img, double *qM, double *qD, uint32_t *qflag, hipStream_t s);
// sample: every workgroup loads its query's table -- few workgroups per query, enough of them to fill the chip; else the filter scan
void launch_pq_adc8(const Adc8Args &a, bool sample, int num_cu, hipStream_t s);
// 8-bit codes on sliced images: eight queries per pass on 16-bit entries (k_pq_adc16x8), sixteen on one-byte entries (k_pq_adc8x16)
constexpr uint32_t ADC16X8_RPT = 4;       // rows per thread
constexpr uint32_t ADC16X8_GS = 32;       // groups per slice (two 16-B code words)
constexpr uint32_t ADC8X16_RPT = 2;       // rows per thread
constexpr uint32_t ADC8X16_GS = 16;       // groups per slice (one 16-B code word): 16 x 256 x 16 B = 64 KB, two blocks in LDS
struct Adc16x8Args {
    const uint4 *codes_t;   // word-major mirror of the (zero-padded) code rows
    uint64_t n;
    uint32_t nwords, m;     // 16-B code words per row; groups of the table
    uint32_t nslices;       // slices of 32 groups of the image (m_pad = 32 nslices)
    const uint4 *img;       // [ngrp][m_pad * 256] 16-B entries
    const double *qM, *qD;  // [nq] of the 16-bit quantisation
    const uint32_t *qflag;
    const float *tau;
    uint32_t nq;
    uint64_t rows_per_wg;   // multiple of 64
    uint64_t *cand;         // [nq][cap] row ids
    uint32_t *cnt;          // [nq]
    uint32_t cap;
    // k_pq_adc8x16<SAMPLE>: the quantised sums of every blk_step-th block of 1024 rows, as floats (+inf past the table), [nq][ld_s]
    uint32_t blk_step = 0;
    uint64_t n_sb = 0;      // sampled blocks
    float *s8_out = nullptr;
    uint64_t ld_s = 0;
};
size_t pq_adc16x8_lds_bytes();
size_t pq_adc8x16_lds_bytes();
// per query the group minima mn [nq][m], M, D = sum of the ranges / divisor and the flag, then the image of ceil(nq / 8) (sixteen: / 16)
// query groups, m_pad groups each (k_pq_quant16x8_stats + k_pq_quant16x8_img | k_pq_quant8x16_img)
void launch_pq_quant_sliced(bool sixteen, const float *lut, uint32_t m, uint32_t m_pad, uint32_t nq, double divisor, float *mn, double *qM, double *qD,
                            uint32_t *qflag, uint4 *img, hipStream_t s);
void launch_pq_adc16x8(const Adc16x8Args &a, hipStream_t s);
void launch_pq_adc8x16(const Adc16x8Args &a, bool sample, hipStream_t s);
// exact f32 sums of the candidates of the 8-bit scans (k_pq_adc_exact8)
void launch_pq_adc_exact8(const uint8_t *codes, uint32_t enc_dim, const uint4 *codes_t, uint32_t nwords, uint32_t m, const float *lut,
                          const float *tau, uint64_t *cand, const uint32_t *cnt, uint32_t cap, uint32_t *valid, uint32_t nq, hipStream_t s);
// row-sharded knn_pq: a shard's key rows with global ids, and the merge of n_shards sorted rows per query by ADC key
void launch_pq_export_keys(const uint64_t *adc, const uint64_t *exact, uint32_t ld, uint32_t efk_local, uint32_t efk_out, uint64_t id_offset,
                           uint64_t *out_adc, uint64_t *out_exact, uint32_t nq, hipStream_t s);
void launch_pq_shard_merge(const uint64_t *adc, const uint64_t *exact, uint32_t n_shards, uint32_t nq, uint32_t efg, uint64_t *merged, hipStream_t s);

void mfma_set_sample_thin(int v);
void mfma_sample_plan(uint64_t n, uint32_t kprime, uint32_t *step, uint32_t *rank, uint32_t target_floor = 1024);  // target_floor: expected hits per query
uint64_t mfma_sample_rows(uint64_t n, uint32_t step);
size_t mfma_qfrag_floats(uint32_t dim);
uint32_t mfma_dim_pad(uint32_t dim);  // columns of the mirror / Q images (dim rounded up to 64, zero filled)
void mfma_set_variant(int v);  // tuning hook (0 = default)
void mfma_set_share(int v);    // query batches (of 32) that ride one HBM pass through XCD-local L2 sharing (1, 2, 4, 8)
uint32_t mfma_share();
uint64_t mfma_row_pad();
bool mfma_supported(uint32_t dim);

}  // namespace vdb
