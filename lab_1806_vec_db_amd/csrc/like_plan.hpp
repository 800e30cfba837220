// like_plan.hpp -- the host arithmetic of the search by example rows (Index::flat_knn_like_device / Index::like_queries_device /
// Index::drop_listed_device, k_like.hip: "more like these rows, and not like those"): the check of the list limits, the longest example
// list of a call, the list length of its one round and the sub-chunks of queries that bound a call's candidate lists.  Host only: no
// HIP and no other header of the library (tests/cpp/like_plan_asan.cpp builds it on its own).  docs/DESIGN_flat.md 4.1v.
//
// A call is ONE round: k_like_build writes a query vector per query from its example rows, the existing exact search returns the sorted
// list of K' rows per query, and k_like_drop compacts the list to the first k rows that are no example.  K' = k + e_max always holds k
// rows that are no example whenever that many exist, so K' changes the cost of a call and never its answer.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "list_plan.hpp"

namespace vdb {

constexpr uint64_t LIKE_MAX_EXAMPLES = 1024;  // examples of one query, positives plus negatives, as listed (repeats count)

// nullptr when lims[0 .. nq] is a list of limits: lims[0] == 0 and no descent.  (nq == 0: lims[0] is still read.)
inline const char *like_check_one_lims(const uint64_t *lims, uint64_t nq) {
    if (!lims) return "like: null list limits";
    if (lims[0] != 0) return "like: list limits must start at 0";
    for (uint64_t q = 0; q < nq; q++)
        if (lims[q + 1] < lims[q]) return "like: list limits must not decrease";
    return nullptr;
}

// nullptr when (pos_lims, neg_lims) describe the example lists of nq queries, otherwise what is wrong with them: both as
// like_check_one_lims wants them, every query with at least one positive and at most LIKE_MAX_EXAMPLES examples in all.
// neg_lims == nullptr: no query has negatives.
inline const char *like_check_lims(const uint64_t *pos_lims, const uint64_t *neg_lims, uint64_t nq) {
    if (const char *bad = like_check_one_lims(pos_lims, nq)) return bad;
    if (neg_lims)
        if (const char *bad = like_check_one_lims(neg_lims, nq)) return bad;
    for (uint64_t q = 0; q < nq; q++) {
        const uint64_t p = pos_lims[q + 1] - pos_lims[q], g = neg_lims ? neg_lims[q + 1] - neg_lims[q] : 0;
        if (p == 0) return "like: every query needs at least one positive example";
        if (p > LIKE_MAX_EXAMPLES || g > LIKE_MAX_EXAMPLES || p + g > LIKE_MAX_EXAMPLES) return "like: at most 1024 examples per query";
    }
    return nullptr;
}

// the list form (vdb_drop_listed_device): one list per query, which may be empty, at most LIKE_MAX_EXAMPLES ids each
inline const char *like_check_drop_lims(const uint64_t *lims, uint64_t nq) {
    if (const char *bad = like_check_one_lims(lims, nq)) return bad;
    for (uint64_t q = 0; q < nq; q++)
        if (lims[q + 1] - lims[q] > LIKE_MAX_EXAMPLES) return "like: at most 1024 listed ids per query";
    return nullptr;
}

// the longest example list of the call, positives plus negatives as listed (not distinct rows: an upper bound that needs no read-back);
// the limits have passed like_check_lims
inline uint64_t like_e_max(const uint64_t *pos_lims, const uint64_t *neg_lims, uint64_t nq) {
    uint64_t e = 0;
    for (uint64_t q = 0; q < nq; q++)
        e = std::max(e, pos_lims[q + 1] - pos_lims[q] + (neg_lims ? neg_lims[q + 1] - neg_lims[q] : 0));
    return e;
}

// list length K' of the call's one round: k + e_max when the examples are dropped (k otherwise), clamped to the longest allowed set among
// its queries, at least 1 (max_m == 0 or k == 0: one slot is still asked for so that every buffer has a size)
inline uint64_t like_list_len(uint64_t k, uint64_t e_max, bool exclude, uint64_t max_m) {
    return list_len(exclude ? (k > ~uint64_t(0) - e_max ? ~uint64_t(0) : k + e_max) : k, max_m);
}

// queries per sub-chunk of a call with lists of kp rows (list_plan.hpp); 0 for nq == 0
inline uint64_t like_sub_chunk(uint64_t nq, uint64_t kp, uint64_t budget = LIST_BUDGET) { return nq ? list_sub_chunk(nq, kp, budget) : 0; }

}  // namespace vdb
