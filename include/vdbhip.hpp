// vdbhip.hpp -- C++ host-side mirror of the reference's `DynamicIndex` (src/database/dynamic_index.rs:11-94) and of
// the index traits it forwards to (src/index_algorithm/mod.rs:35-154), header-only over the C ABI of vdbhip.h.
//
// The reference's host code is Rust; where a Rust toolchain is present the binding is the `extern "C"` block of
// INTEGRATION.md.  This header is the same seam for a C++ host: same method names, argument meaning and error
// behaviour (recoverable errors -> an exception carrying vdb_last_error(), the counterpart of anyhow::Result ->
// PyRuntimeError, pyo3/mod.rs:65,85; dimension mismatch is an error, database/mod.rs:427-429).
// There is no CPU path behind it: without a GPU every call throws.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "vdbhip.h"

namespace vdbhip {

enum class DistanceAlgorithm : int { L2Sqr = VDB_L2SQR, Cosine = VDB_COSINE };  // distance/mod.rs:17-28

// candidate_pair.rs:9-16
struct CandidatePair {
    uint64_t index;
    float distance;
};

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};
inline void check(int status) {
    if (status != VDB_OK) throw Error(status, vdb_last_error());
}

// the pairs of a range result object, per query; releases the object
inline std::vector<std::vector<CandidatePair>> take_range(vdb_range *r, uint64_t nq) {
    std::vector<uint64_t> lims(nq + 1), idx;
    std::vector<float> d;
    int rc = vdb_range_lims(r, lims.data());
    if (rc == VDB_OK) {
        idx.resize(lims[nq]);
        d.resize(lims[nq]);
        rc = vdb_range_copy(r, idx.data(), d.data());
    }
    vdb_range_destroy(r);
    check(rc);
    std::vector<std::vector<CandidatePair>> out(nq);
    for (uint64_t q = 0; q < nq; q++)
        for (uint64_t j = lims[q]; j < lims[q + 1]; j++) out[q].push_back({idx[j], d[j]});
    return out;
}

// DynamicIndex: starts as the Flat arm; build_hnsw() switches to the HNSW arm like
// MetadataVecTable::build_hnsw_index (metadata_vec_table.rs:112-135), clear_hnsw() back (:137-152).
// A row allow-list of one DynamicIndex (vdb_mask; DynamicIndex::make_mask): valid until rows are added to or removed from that index,
// destroyed before it.
class Mask {
public:
    Mask() = default;
    explicit Mask(vdb_mask *h) : h_(h) {}
    ~Mask() {
        if (h_) vdb_mask_destroy(h_);
    }
    Mask(const Mask &) = delete;
    Mask &operator=(const Mask &) = delete;
    Mask(Mask &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Mask &operator=(Mask &&o) noexcept {
        if (this != &o) {
            if (h_) vdb_mask_destroy(h_);
            h_ = o.h_;
            o.h_ = nullptr;
        }
        return *this;
    }
    uint64_t count() const {  // allowed rows
        uint64_t m = 0;
        check(vdb_mask_count(h_, &m));
        return m;
    }
    const vdb_mask *handle() const { return h_; }

private:
    vdb_mask *h_ = nullptr;
};

// The PQ table hangs off the index handle (the reference passes &PQTable into knn_pq; here it is attached state).
class DynamicIndex {
public:
    DynamicIndex(uint64_t dim, DistanceAlgorithm dist, int device = 0) : dim_(dim), dist_(dist) {
        check(vdb_index_create(device, dim, (int)dist, &h_));
    }
    ~DynamicIndex() {
        if (h_) vdb_index_destroy(h_);
    }
    DynamicIndex(const DynamicIndex &) = delete;
    DynamicIndex &operator=(const DynamicIndex &) = delete;
    DynamicIndex(DynamicIndex &&o) noexcept : h_(o.h_), dim_(o.dim_), dist_(o.dist_) { o.h_ = nullptr; }

    uint64_t len() const {
        uint64_t n = 0;
        check(vdb_index_len(h_, &n));
        return n;
    }
    bool is_empty() const { return len() == 0; }
    uint64_t dim() const { return dim_; }
    DistanceAlgorithm dist() const { return dist_; }
    // Index<usize> for VecSet (vec_set.rs:22-30)
    std::vector<float> row(uint64_t i) const {
        std::vector<float> v(dim_);
        check(vdb_index_row(h_, i, v.data()));
        return v;
    }
    // the vectors of many rows in one call (vdb_index_get_rows): ids.size() x dim row-major, row j = row ids[j]; any order, repeats allowed
    std::vector<float> rows(const std::vector<uint64_t> &ids) {
        std::vector<float> v(ids.size() * dim_);
        check(vdb_index_get_rows(h_, ids.data(), ids.size(), v.data()));
        return v;
    }

    // add / batch_add (dynamic_index.rs:44-58): returns the index of the (first) new vector
    uint64_t add(const std::vector<float> &vec) {
        require_dim(vec.size());
        uint64_t first = 0;
        check(vdb_index_add(h_, vec.data(), 1, &first));
        return first;
    }
    uint64_t batch_add(const float *rows, uint64_t n) {
        uint64_t first = 0;
        check(vdb_index_add(h_, rows, n, &first));
        return first;
    }
    void swap_remove(uint64_t i) { check(vdb_index_swap_remove(h_, i)); }  // vec_set.rs:131-137
    // swap_remove on every row of `rows` (strictly ascending) in descending order, as one call (MetadataVecTable::delete,
    // metadata_vec_table.rs:163-187).  Returns the moves (dst, src): the row that was at src is now at dst, all others kept their place.
    std::vector<std::pair<uint64_t, uint64_t>> remove_rows(const std::vector<uint64_t> &rows) {
        std::vector<uint64_t> dst(rows.size()), src(rows.size());
        uint64_t moves = 0;
        check(vdb_index_remove_rows(h_, rows.data(), rows.size(), dst.data(), src.data(), &moves));
        std::vector<std::pair<uint64_t, uint64_t>> out(moves);
        for (uint64_t j = 0; j < moves; j++) out[j] = {dst[j], src[j]};
        return out;
    }
    // new vectors (rows.size() x dim, row-major) for the distinct rows `rows`, in place: ids, labels and masks stay (vdb_index_update_rows)
    void update_rows(const std::vector<uint64_t> &rows, const float *vecs) { check(vdb_index_update_rows(h_, rows.data(), rows.size(), vecs)); }

    // knn (dynamic_index.rs:66-73): Flat -> FlatIndex::knn, HNSW -> HNSWIndex::knn (default ef)
    std::vector<CandidatePair> knn(const std::vector<float> &query, uint64_t k) const {
        return has_hnsw() ? search(vdb_hnsw_knn, query, k, 0) : search_flat(query, k);
    }
    // knn_with_ef (:74-80): Flat ignores ef
    std::vector<CandidatePair> knn_with_ef(const std::vector<float> &query, uint64_t k, uint64_t ef) const {
        return has_hnsw() ? search(vdb_hnsw_knn, query, k, ef) : search_flat(query, k);
    }
    // knn_pq (:82-93)
    std::vector<CandidatePair> knn_pq(const std::vector<float> &query, uint64_t k, uint64_t ef) const {
        return has_hnsw() ? search(vdb_hnsw_knn_pq, query, k, ef) : search(vdb_flat_knn_pq, query, k, ef);
    }
    // batched form of knn for hosts that collect their pending queries (one corpus pass serves up to 128 of them)
    std::vector<std::vector<CandidatePair>> knn_batch(const float *queries, uint64_t nq, uint64_t k) const {
        std::vector<uint64_t> idx(nq * (k ? k : 1)), cnt(nq);
        std::vector<float> d(nq * (k ? k : 1));
        check(vdb_flat_knn(h_, queries, nq, dim_, k, idx.data(), d.data(), cnt.data()));
        std::vector<std::vector<CandidatePair>> out(nq);
        for (uint64_t q = 0; q < nq; q++)
            for (uint64_t j = 0; j < cnt[q]; j++) out[q].push_back({idx[q * k + j], d[q * k + j]});
        return out;
    }

    // exact range search over the Flat rows (vdb_flat_range): per query every pair with distance <= radius[q], ascending by
    // (distance, index) -- search(k, upper_bound) (metadata_vec_table.rs:194-212) without having to guess k; limit > 0 = at most
    // that many per query (the nearest ones)
    std::vector<std::vector<CandidatePair>> range_search_batch(const float *queries, uint64_t nq, const float *radius, uint64_t limit = 0) const {
        vdb_range *r = nullptr;
        check(vdb_flat_range(h_, queries, nq, dim_, radius, limit, &r));
        return take_range(r, nq);
    }
    std::vector<CandidatePair> range_search(const std::vector<float> &query, float radius, uint64_t limit = 0) const {
        require_dim(query.size());
        return range_search_batch(query.data(), 1, &radius, limit)[0];
    }

    // filtered exact searches over a row mask (vdb_mask_create): `allow[i]` says whether local row i may be returned
    Mask make_mask(const std::vector<bool> &allow) const {
        std::vector<uint64_t> bits((allow.size() + 63) / 64, 0);
        for (size_t i = 0; i < allow.size(); i++)
            if (allow[i]) bits[i >> 6] |= 1ull << (i & 63);
        vdb_mask *m = nullptr;
        check(vdb_mask_create(h_, bits.data(), allow.size(), &m));
        return Mask(m);
    }
    // label columns (vdb_index_labels_set) and the mask of the rows whose label in terms[t].first equals terms[t].second for every t,
    // built on the device (vdb_mask_create_where); no terms: every row
    void set_labels(uint32_t column, const std::vector<uint32_t> &codes, uint64_t first_row = 0) {
        check(vdb_index_labels_set(h_, column, first_row, codes.data(), codes.size()));
    }
    // scattered label writes: codes[c * rows.size() + j] to column columns[c] of row rows[j] (vdb_index_labels_scatter; distinct LOCAL
    // rows, distinct columns), and codes[c] to column columns[c] of every row a mask allows (vdb_index_labels_set_mask)
    void set_labels_rows(const std::vector<uint64_t> &rows, const std::vector<uint32_t> &columns, const std::vector<uint32_t> &codes) {
        if (codes.size() != rows.size() * columns.size()) throw std::invalid_argument("set_labels_rows: codes is columns x rows");
        check(vdb_index_labels_scatter(h_, rows.data(), rows.size(), columns.data(), columns.size(), codes.data()));
    }
    void set_labels_mask(const Mask &mask, const std::vector<uint32_t> &columns, const std::vector<uint32_t> &codes) {
        if (codes.size() != columns.size()) throw std::invalid_argument("set_labels_mask: one code per column");
        check(vdb_index_labels_set_mask(h_, mask.handle(), columns.data(), codes.data(), columns.size()));
    }
    Mask make_mask_where(const std::vector<std::pair<uint32_t, uint32_t>> &terms) const {
        std::vector<uint32_t> cols, codes;
        for (const auto &t : terms) {
            cols.push_back(t.first);
            codes.push_back(t.second);
        }
        vdb_mask *m = nullptr;
        check(vdb_mask_create_where(h_, cols.data(), codes.data(), terms.size(), &m));
        return Mask(m);
    }
    // set / range terms (vdb_mask_create_where_sets): a row with label v in `column` matches a term when v == VDB_LABEL_NONE ? none
    // : (lo <= v <= hi && (set.empty() || bit (v - lo) of set)) != negate; `set` is empty or ceil((hi - lo + 1) / 64) words
    struct LabelTerm {
        uint32_t column = 0, lo = 1, hi = 0;
        bool negate = false, none = false;
        std::vector<uint64_t> set;
    };
    Mask make_mask_where_sets(const std::vector<LabelTerm> &terms) const {
        std::vector<uint32_t> cols, lo, hi, flags;
        std::vector<uint64_t> lims{0}, words;
        for (const auto &t : terms) {
            cols.push_back(t.column);
            lo.push_back(t.lo);
            hi.push_back(t.hi);
            flags.push_back((t.negate ? VDB_TERM_NEGATE : 0u) | (t.none ? VDB_TERM_NONE : 0u));
            words.insert(words.end(), t.set.begin(), t.set.end());
            lims.push_back(words.size());
        }
        vdb_mask *m = nullptr;
        check(vdb_mask_create_where_sets(h_, cols.data(), lo.data(), hi.data(), flags.data(), lims.data(), words.data(), terms.size(), &m));
        return Mask(m);
    }
    // an OR of conjunctions of such terms (vdb_mask_create_where_any): a row is allowed when it matches every term of SOME clause; no
    // clauses: the empty mask; a clause without terms: every row
    Mask make_mask_where_any(const std::vector<std::vector<LabelTerm>> &clauses) const {
        std::vector<uint32_t> cols, lo, hi, flags;
        std::vector<uint64_t> clims{0}, lims{0}, words;
        for (const auto &c : clauses) {
            for (const auto &t : c) {
                cols.push_back(t.column);
                lo.push_back(t.lo);
                hi.push_back(t.hi);
                flags.push_back((t.negate ? VDB_TERM_NEGATE : 0u) | (t.none ? VDB_TERM_NONE : 0u));
                words.insert(words.end(), t.set.begin(), t.set.end());
                lims.push_back(words.size());
            }
            clims.push_back(cols.size());
        }
        vdb_mask *m = nullptr;
        check(vdb_mask_create_where_any(h_, clims.data(), clauses.size(), cols.data(), lo.data(), hi.data(), flags.data(), lims.data(), words.data(), &m));
        return Mask(m);
    }
    // the AND (VDB_MASK_OP_AND) or OR (VDB_MASK_OP_OR) of 1 .. 8 masks of this index, mask i complemented within the rows first when
    // invert[i] (vdb_mask_combine); `invert` is empty or as long as `masks`
    Mask combine_masks(int op, const std::vector<const Mask *> &masks, const std::vector<bool> &invert = {}) const {
        std::vector<const vdb_mask *> hs;
        for (const Mask *mk : masks) hs.push_back(mk->handle());
        std::vector<uint8_t> inv(invert.begin(), invert.end());
        inv.resize(masks.size(), 0);
        vdb_mask *m = nullptr;
        check(vdb_mask_combine(h_, op, hs.data(), invert.empty() ? nullptr : inv.data(), hs.size(), &m));
        return Mask(m);
    }
    // per query the first min(k, mask.count()) pairs of knn_batch over the allowed rows alone (vdb_flat_knn_filtered)
    std::vector<std::vector<CandidatePair>> knn_filtered_batch(const float *queries, uint64_t nq, uint64_t k, const Mask &mask) const {
        std::vector<uint64_t> idx(nq * (k ? k : 1)), cnt(nq);
        std::vector<float> d(nq * (k ? k : 1));
        check(vdb_flat_knn_filtered(h_, queries, nq, dim_, k, mask.handle(), idx.data(), d.data(), cnt.data()));
        std::vector<std::vector<CandidatePair>> out(nq);
        for (uint64_t q = 0; q < nq; q++)
            for (uint64_t j = 0; j < cnt[q]; j++) out[q].push_back({idx[q * k + j], d[q * k + j]});
        return out;
    }
    // range_search_batch over the allowed rows alone (vdb_flat_range_filtered)
    std::vector<std::vector<CandidatePair>> range_search_filtered_batch(const float *queries, uint64_t nq, const float *radius, const Mask &mask,
                                                                        uint64_t limit = 0) const {
        vdb_range *r = nullptr;
        check(vdb_flat_range_filtered(h_, queries, nq, dim_, radius, limit, mask.handle(), &r));
        return take_range(r, nq);
    }
    // the same with one mask per query: query q under *masks[mask_of[q]] (vdb_flat_range_filtered_multi)
    std::vector<std::vector<CandidatePair>> range_search_filtered_multi_batch(const float *queries, uint64_t nq, const float *radius,
                                                                              const std::vector<const Mask *> &masks,
                                                                              const std::vector<uint32_t> &mask_of, uint64_t limit = 0) const {
        if (mask_of.size() != nq) throw std::runtime_error("mask_of: one entry per query is needed");
        std::vector<const vdb_mask *> hs;
        for (const Mask *m : masks) hs.push_back(m->handle());
        vdb_range *r = nullptr;
        check(vdb_flat_range_filtered_multi(h_, queries, nq, dim_, radius, limit, hs.data(), hs.size(), mask_of.data(), &r));
        return take_range(r, nq);
    }
    // per query the first k pairs of knn_batch of which at most group_size carry any one value of label column `column`; rows without a
    // label are always kept (vdb_flat_knn_grouped).  masks empty: over all rows; otherwise query q under *masks[mask_of[q]]
    std::vector<std::vector<CandidatePair>> knn_grouped_batch(const float *queries, uint64_t nq, uint64_t k, uint32_t column, uint64_t group_size = 1,
                                                              const std::vector<const Mask *> &masks = {},
                                                              const std::vector<uint32_t> &mask_of = {}) const {
        if (!masks.empty() && mask_of.size() != nq) throw std::runtime_error("mask_of: one entry per query is needed");
        std::vector<const vdb_mask *> hs;
        for (const Mask *m : masks) hs.push_back(m->handle());
        std::vector<uint64_t> idx(nq * (k ? k : 1)), cnt(nq);
        std::vector<float> d(nq * (k ? k : 1));
        check(vdb_flat_knn_grouped(h_, queries, nq, dim_, k, column, group_size, hs.data(), hs.size(), mask_of.data(), idx.data(), d.data(), cnt.data()));
        std::vector<std::vector<CandidatePair>> out(nq);
        for (uint64_t q = 0; q < nq; q++)
            for (uint64_t j = 0; j < cnt[q]; j++) out[q].push_back({idx[q * k + j], d[q * k + j]});
        return out;
    }
    // diversified k-NN, maximal marginal relevance (vdb_flat_knn_mmr): per query, from the first min(fetch_k, allowed rows) pairs of
    // knn_batch, the nearest and then greedily the pair with the smallest lambda * d(query, row) - (1 - lambda) * min over the selected rows
    // of d(row, selected); the pairs come in SELECTION order.  masks empty: over all rows; otherwise query q under *masks[mask_of[q]]
    std::vector<std::vector<CandidatePair>> knn_mmr_batch(const float *queries, uint64_t nq, uint64_t k, uint64_t fetch_k, float lambda = 0.5f,
                                                          const std::vector<const Mask *> &masks = {},
                                                          const std::vector<uint32_t> &mask_of = {}) const {
        if (!masks.empty() && mask_of.size() != nq) throw std::runtime_error("mask_of: one entry per query is needed");
        std::vector<const vdb_mask *> hs;
        for (const Mask *m : masks) hs.push_back(m->handle());
        std::vector<uint64_t> idx(nq * (k ? k : 1)), cnt(nq);
        std::vector<float> d(nq * (k ? k : 1));
        check(vdb_flat_knn_mmr(h_, queries, nq, dim_, k, fetch_k, lambda, hs.data(), hs.size(), mask_of.data(), idx.data(), d.data(), cnt.data()));
        std::vector<std::vector<CandidatePair>> out(nq);
        for (uint64_t q = 0; q < nq; q++)
            for (uint64_t j = 0; j < cnt[q]; j++) out[q].push_back({idx[q * k + j], d[q * k + j]});
        return out;
    }

    // search by example rows (vdb_like_queries / vdb_flat_knn_like): positives[q] / negatives[q] are the LOCAL rows of query q's examples
    // (negatives empty: none; otherwise one list per query).  The query vector is the strict-fold f32 average of the positives, plus its
    // difference from the average of the negatives; like_batch returns per query the first k pairs of knn_batch for it whose row is no
    // example (exclude = false: the first k pairs).  masks empty: over all rows; otherwise query q under *masks[mask_of[q]]
    std::vector<float> like_queries(const std::vector<std::vector<uint64_t>> &positives,
                                    const std::vector<std::vector<uint64_t>> &negatives = {}) const {
        const LikeArgs a(positives, negatives);
        std::vector<float> out(positives.size() * dim_);
        check(vdb_like_queries(h_, a.pl.data(), a.pr.data(), a.nl_ptr(), a.nr.data(), positives.size(), out.data()));
        return out;
    }
    std::vector<std::vector<CandidatePair>> like_batch(const std::vector<std::vector<uint64_t>> &positives, uint64_t k,
                                                       const std::vector<std::vector<uint64_t>> &negatives = {}, bool exclude = true,
                                                       const std::vector<const Mask *> &masks = {},
                                                       const std::vector<uint32_t> &mask_of = {}) const {
        const uint64_t nq = positives.size();
        if (!masks.empty() && mask_of.size() != nq) throw std::runtime_error("mask_of: one entry per query is needed");
        const LikeArgs a(positives, negatives);
        std::vector<const vdb_mask *> hs;
        for (const Mask *m : masks) hs.push_back(m->handle());
        std::vector<uint64_t> idx(nq * (k ? k : 1)), cnt(nq);
        std::vector<float> d(nq * (k ? k : 1));
        check(vdb_flat_knn_like(h_, a.pl.data(), a.pr.data(), a.nl_ptr(), a.nr.data(), nq, k, exclude ? 1 : 0, hs.data(), hs.size(), mask_of.data(),
                                idx.data(), d.data(), cnt.data()));
        std::vector<std::vector<CandidatePair>> out(nq);
        for (uint64_t q = 0; q < nq; q++)
            for (uint64_t j = 0; j < cnt[q]; j++) out[q].push_back({idx[q * k + j], d[q * k + j]});
        return out;
    }

    // fused multi-query search (vdb_flat_knn_fused): fused query q owns the sub-queries lims[q] .. lims[q + 1] - 1 of `queries` (lims[0] ==
    // 0, 1 to 32 each); every sub-query contributes its first min(fetch_k, allowed rows) pairs of knn_batch and the lists are joined on the
    // device.  mode VDB_FUSE_RRF: distance = the score, the f32 left fold over the sub-queries of weight / ((rank + 1) + rrf_c), pairs by
    // score descending (ties: ascending id); VDB_FUSE_MIN: the smallest distance over the sub-queries, pairs ascending (weights must be
    // empty).  weights empty: all 1.  masks empty: over all rows; otherwise SUB-query j under *masks[mask_of[j]]
    std::vector<std::vector<CandidatePair>> knn_fused_batch(const float *queries, const std::vector<uint64_t> &lims, uint64_t k, uint64_t fetch_k,
                                                            int mode = VDB_FUSE_RRF, const std::vector<float> &weights = {}, float rrf_c = 60.0f,
                                                            const std::vector<const Mask *> &masks = {},
                                                            const std::vector<uint32_t> &mask_of = {}) const {
        if (lims.empty()) throw std::runtime_error("lims: nq + 1 entries are needed");
        const uint64_t nq = lims.size() - 1, nsub = lims.back();
        if (!masks.empty() && mask_of.size() != nsub) throw std::runtime_error("mask_of: one entry per sub-query is needed");
        if (!weights.empty() && weights.size() != nsub) throw std::runtime_error("weights: one entry per sub-query is needed");
        std::vector<const vdb_mask *> hs;
        for (const Mask *m : masks) hs.push_back(m->handle());
        std::vector<uint64_t> idx(nq * (k ? k : 1)), cnt(nq);
        std::vector<float> d(nq * (k ? k : 1));
        check(vdb_flat_knn_fused(h_, queries, lims.data(), nq, dim_, k, fetch_k, mode, weights.empty() ? nullptr : weights.data(), rrf_c, hs.data(),
                                 hs.size(), mask_of.data(), idx.data(), d.data(), cnt.data()));
        std::vector<std::vector<CandidatePair>> out(nq);
        for (uint64_t q = 0; q < nq; q++)
            for (uint64_t j = 0; j < cnt[q]; j++) out[q].push_back({idx[q * k + j], d[q * k + j]});
        return out;
    }

    // MetadataVecTable::build_hnsw_index / clear_hnsw_index, build_pq_table / clear_pq_table
    void build_hnsw(uint64_t M = 16, uint64_t ef_construction = 200, uint64_t seed = 42, uint64_t batch = 64,
                    int nthreads = 16) {
        check(vdb_hnsw_build(h_, M, ef_construction, seed, batch, nthreads));
    }
    void clear_hnsw() { check(vdb_hnsw_clear(h_)); }
    bool has_hnsw() const {
        int v = 0;
        check(vdb_hnsw_has(h_, &v));
        return v != 0;
    }
    void build_pq(uint64_t n_bits, uint64_t m, uint64_t train_n = 0, uint64_t max_iter = 20, float tol = 1e-6f,
                  uint64_t seed = 42) {
        check(vdb_pq_build(h_, n_bits, m, train_n, max_iter, tol, seed));
    }
    void clear_pq() { check(vdb_pq_clear(h_)); }
    bool has_pq() const {
        int v = 0;
        check(vdb_pq_has(h_, &v));
        return v != 0;
    }
    vdb_index *handle() const { return h_; }

private:
    typedef int (*search_ef_fn)(vdb_index *, const float *, uint64_t, uint64_t, uint64_t, uint64_t, uint64_t *, float *,
                                uint64_t *);
    void require_dim(size_t got) const {
        if (got != dim_)
            throw Error(VDB_ERR_INVALID, "dimension mismatch: index dim " + std::to_string(dim_) + ", got " + std::to_string(got));
    }
    std::vector<CandidatePair> collect(const std::vector<uint64_t> &idx, const std::vector<float> &d, uint64_t cnt) const {
        std::vector<CandidatePair> out;
        for (uint64_t j = 0; j < cnt; j++) out.push_back({idx[j], d[j]});
        return out;
    }
    std::vector<CandidatePair> search_flat(const std::vector<float> &query, uint64_t k) const {
        std::vector<uint64_t> idx(k ? k : 1);
        std::vector<float> d(k ? k : 1);
        uint64_t cnt = 0;
        check(vdb_flat_knn(h_, query.data(), 1, query.size(), k, idx.data(), d.data(), &cnt));
        return collect(idx, d, cnt);
    }
    std::vector<CandidatePair> search(search_ef_fn fn, const std::vector<float> &query, uint64_t k, uint64_t ef) const {
        std::vector<uint64_t> idx(k ? k : 1);
        std::vector<float> d(k ? k : 1);
        uint64_t cnt = 0;
        check(fn(h_, query.data(), 1, query.size(), k, ef, idx.data(), d.data(), &cnt));
        return collect(idx, d, cnt);
    }
    // the example lists of like_queries / like_batch as the C ABI takes them: limits of nq + 1 entries and the rows behind each other
    struct LikeArgs {
        std::vector<uint64_t> pl, pr, nl, nr;
        LikeArgs(const std::vector<std::vector<uint64_t>> &positives, const std::vector<std::vector<uint64_t>> &negatives) {
            if (!negatives.empty() && negatives.size() != positives.size()) throw std::runtime_error("negatives: one list per query is needed");
            pl.push_back(0);
            for (const auto &p : positives) {
                pr.insert(pr.end(), p.begin(), p.end());
                pl.push_back(pr.size());
            }
            if (negatives.empty()) return;
            nl.push_back(0);
            for (const auto &g : negatives) {
                nr.insert(nr.end(), g.begin(), g.end());
                nl.push_back(nr.size());
            }
        }
        const uint64_t *nl_ptr() const { return nl.empty() ? nullptr : nl.data(); }
    };
    vdb_index *h_ = nullptr;
    uint64_t dim_;
    DistanceAlgorithm dist_;
};

// The same index over ALL GPUs of one host process (vdb_ctx_create + vdb_sharded_*): rows in contiguous blocks, per-shard
// top-k, ONE RCCL all-gather inside the library, exact merge.  What a multi-GPU `DynamicIndex::Gpu`
// arm forwards to; answers equal the single-GPU index's.
class ShardedIndex {
public:
    ShardedIndex(uint64_t dim, DistanceAlgorithm dist, const std::vector<int> &devices) : dim_(dim) {
        check(vdb_ctx_create(devices.data(), (int)devices.size(), &ctx_));
        int rc = vdb_sharded_create(ctx_, dim, (int)dist, &h_);
        if (rc != VDB_OK) {
            std::string msg = vdb_last_error();
            vdb_ctx_destroy(ctx_);
            throw Error(rc, msg);
        }
    }
    ~ShardedIndex() {
        if (h_) vdb_sharded_destroy(h_);
        if (ctx_) vdb_ctx_destroy(ctx_);
    }
    ShardedIndex(const ShardedIndex &) = delete;
    ShardedIndex &operator=(const ShardedIndex &) = delete;
    void set_rows(const float *rows, uint64_t n) { check(vdb_sharded_set_rows(h_, rows, n)); }
    // REPLICA layout: every GPU keeps all rows and a search splits the queries -- the layout the HNSW searches need
    // ("replicas only"); knn_batch / knn_pq_batch work in it as well
    void set_rows_replica(const float *rows, uint64_t n) { check(vdb_sharded_set_rows_replica(h_, rows, n)); }
    void build_hnsw(uint64_t ef_construction = 200, uint64_t M = 16, uint64_t seed = 42, uint64_t batch = 1, int nthreads = 0) {
        check(vdb_sharded_hnsw_build(h_, M, ef_construction, seed, batch, nthreads));  // metadata_vec_table.rs:84-98
    }
    // IndexKNNWithEf::knn_with_ef / HNSWIndex::knn_pq over the replicas (dynamic_index.rs:76-93)
    std::vector<std::vector<CandidatePair>> knn_with_ef_batch(const float *queries, uint64_t nq, uint64_t k, uint64_t ef) const {
        return run(nq, k, [&](uint64_t *i, float *d, uint64_t *c) { return vdb_sharded_hnsw_knn(h_, queries, nq, dim_, k, ef, i, d, c); });
    }
    std::vector<std::vector<CandidatePair>> hnsw_knn_pq_batch(const float *queries, uint64_t nq, uint64_t k, uint64_t ef) const {
        return run(nq, k, [&](uint64_t *i, float *d, uint64_t *c) { return vdb_sharded_hnsw_knn_pq(h_, queries, nq, dim_, k, ef, i, d, c); });
    }
    bool poisoned() const {
        int v = 0;
        check(vdb_sharded_poisoned(h_, &v));
        return v != 0;
    }
    uint64_t len() const {
        uint64_t n = 0;
        check(vdb_sharded_len(h_, &n));
        return n;
    }
    std::vector<std::vector<CandidatePair>> knn_batch(const float *queries, uint64_t nq, uint64_t k) const {
        return run(nq, k, [&](uint64_t *i, float *d, uint64_t *c) { return vdb_sharded_flat_knn(h_, queries, nq, dim_, k, i, d, c); });
    }
    // every pair within radius[q] over the whole corpus (vdb_sharded_flat_range): DynamicIndex::range_search_batch's answer, global ids
    std::vector<std::vector<CandidatePair>> range_search_batch(const float *queries, uint64_t nq, const float *radius, uint64_t limit = 0) const {
        vdb_range *r = nullptr;
        check(vdb_sharded_flat_range(h_, queries, nq, dim_, radius, limit, &r));
        return take_range(r, nq);
    }
    void attach_pq(uint64_t n_bits, uint64_t m, const std::vector<float> &centroids) {
        check(vdb_sharded_pq_attach(h_, n_bits, m, centroids.data()));
    }
    std::vector<std::vector<CandidatePair>> knn_pq_batch(const float *queries, uint64_t nq, uint64_t k, uint64_t ef) const {
        return run(nq, k, [&](uint64_t *i, float *d, uint64_t *c) { return vdb_sharded_knn_pq(h_, queries, nq, dim_, k, ef, i, d, c); });
    }

private:
    template <class F>
    std::vector<std::vector<CandidatePair>> run(uint64_t nq, uint64_t k, F fn) const {
        std::vector<uint64_t> idx(nq * (k ? k : 1)), cnt(nq);
        std::vector<float> d(nq * (k ? k : 1));
        check(fn(idx.data(), d.data(), cnt.data()));
        std::vector<std::vector<CandidatePair>> out(nq);
        for (uint64_t q = 0; q < nq; q++)
            for (uint64_t j = 0; j < cnt[q]; j++) out[q].push_back({idx[q * k + j], d[q * k + j]});
        return out;
    }
    vdb_ctx *ctx_ = nullptr;
    vdb_sharded *h_ = nullptr;
    uint64_t dim_;
};

// calc_dist (pyo3/mod.rs:43-48)
inline float calc_dist(const std::vector<float> &a, const std::vector<float> &b, DistanceAlgorithm dist, int device = 0) {
    float out = 0;
    check(vdb_calc_dist(device, a.data(), b.data(), a.size() < b.size() ? a.size() : b.size(), (int)dist, &out));
    return out;
}

}  // namespace vdbhip
