// grouped_plan.hpp -- the host arithmetic of the grouped Flat k-NN (Index::flat_knn_grouped_device, k_group.hip: at most g hits per
// value of one label column): the list length of every round, the sub-chunks of queries that bound a round's memory, the compaction of
// the queries a round leaves unfinished, and the capacity of the walk's hash table.  Host only: no HIP and no other header of the
// library (tests/cpp/grouped_plan_asan.cpp builds it on its own).  docs/DESIGN_flat.md 4.1q.
//
// A round asks the exact search for the K' nearest allowed rows of every query still open and walks those lists with the cap.  A query is
// finished when k rows were kept or when its list was its whole allowed set (m rows: nothing is left to fetch).  The others go round
// again, compacted into a block, with 4 x K' -- so the lists of a round never exceed the longest allowed set among its queries, and the
// round whose K' reaches that finishes everything: the loop ends.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "list_plan.hpp"

namespace vdb {

// "flat_grouped_oversample": round 0 fetches min(m, k x this) rows per query.  2 had the smallest summed median of the sweep 1, 2, 4, 8, 16
// of tools/bench_grouped.py (profiles/flat_grouped_1M.json; docs/DESIGN_flat.md 4.1q has the sweep and what decided it)
constexpr uint64_t GROUPED_OVERSAMPLE_DEFAULT = 2;
constexpr uint64_t GROUPED_GROWTH = 4;              // every later round: 4 x the list length of the one before
constexpr uint32_t GROUPED_TILE = 64;                // positions the walk takes per step (one wave)
constexpr uint32_t GROUPED_LDS_MAX_LG = 12;          // tables of up to 2^12 entries (32 KiB) live in LDS, larger ones in global scratch

// list length of round 0: k x oversample (saturating; oversample 0 counts as 1), at least 1, at most max_m (the longest allowed set
// among the queries of the round; 0: nothing is allowed -- one slot is still asked for so that every buffer has a size)
inline uint64_t grouped_first_k(uint64_t k, uint64_t oversample, uint64_t max_m) {
    return list_len(list_sat_mul(k, std::max<uint64_t>(oversample, 1)), max_m);
}
// list length of the round after one of length kp, for queries whose longest allowed set is max_m (> kp, or nothing would be open)
inline uint64_t grouped_next_k(uint64_t kp, uint64_t max_m) { return list_len(list_sat_mul(kp, GROUPED_GROWTH), max_m); }
// queries per sub-chunk of a round with lists of kp rows (list_plan.hpp)
inline uint64_t grouped_sub_chunk(uint64_t nq, uint64_t kp, uint64_t budget = LIST_BUDGET) { return list_sub_chunk(nq, kp, budget); }
// a list of kp rows is the whole allowed set of a query with m allowed rows
inline bool grouped_exhausts(uint64_t kp, uint64_t m) { return m <= kp; }

// The queries of `active` (positions in the call, ascending) that the round with lists of kp rows leaves open: done[i] == 0 and the
// list was not the whole allowed set (m_of[active[i]] > kp).  `next` receives them in the same order -- the compaction map of the next
// round, whose block holds query next[j] at position j; returns the longest allowed set among them (0: none is open).  `exhausted`
// is advanced by the queries that this round finished with their whole allowed set walked.
inline uint64_t grouped_compact(const std::vector<uint64_t> &active, const uint8_t *done, const uint64_t *m_of, uint64_t kp,
                                std::vector<uint64_t> &next, uint64_t &exhausted) {
    next.clear();
    uint64_t max_m = 0;
    for (size_t i = 0; i < active.size(); i++) {
        const uint64_t q = active[i];
        if (grouped_exhausts(kp, m_of[q])) {
            exhausted++;
            continue;
        }
        if (done[i]) continue;
        next.push_back(q);
        max_m = std::max(max_m, m_of[q]);
    }
    return max_m;
}

// log2 of the capacity of the walk's open-addressing table for result size k over lists of ld positions: while fewer than min(k, ld)
// rows are kept the table holds fewer than that many labels, and the tile that completes the answer adds at most GROUPED_TILE more;
// twice that bound, rounded up to a power of two, keeps the load at or under one half.  At least 2^7.
inline uint32_t grouped_table_lg(uint64_t k, uint64_t ld) {
    const uint64_t need = 2 * (std::min(k, ld) + GROUPED_TILE);
    uint32_t lg = 7;
    while ((1ull << lg) < need) lg++;
    return lg;
}
// where a label starts probing in a table of 2^lg entries (Fibonacci hashing; the device restates it in k_group.hip)
inline uint32_t grouped_hash(uint32_t label, uint32_t lg) { return (label * 2654435761u) >> (32 - lg); }

}  // namespace vdb
