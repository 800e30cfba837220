// remove_plan.hpp -- the net effect of many swap_removes as one list of row moves.  Host only: no HIP, no other header of the library
// (tests/cpp/remove_plan_asan.cpp builds it on its own).
//
// Removing the rows R (m of them) from a table of n rows means, by definition, VecSet::swap_remove (vec_set.rs:131-137) on every i in R
// in DESCENDING order -- what MetadataVecTable::delete does (metadata_vec_table.rs:163-187).  With n' = n - m, that sequence
//  - never writes a slot outside R (swap_remove(i) writes slot i only), so every surviving row below n' stays where it is;
//  - fills every removed slot below n' exactly once, with a surviving row of the old tail [n', n): when slot i < n' is written, all of
//    R above i is gone already, and the row at the end of the table then is a tail row that was never removed;
//  - so its net effect is |R below n'| moves whose sources lie in [n', n) and whose destinations lie in [0, n'): two disjoint ranges,
//    no move reads what another one writes, and they can be applied in any order or all at once.
// WHICH tail row lands in which hole has no closed form (removals inside the tail reshuffle it), so the sequence is replayed on the
// tail slots alone: cur[j] = the original row that currently sits in slot n' + j.  O(m) time and memory.
#pragma once
#include <cstdint>
#include <vector>

namespace vdb {

// nullptr: rows[0..m) is strictly ascending and below n; otherwise what is wrong with it
inline const char *remove_plan_check(uint64_t n, const uint64_t *rows, uint64_t m) {
    if (m && !rows) return "remove_rows: null rows";
    for (uint64_t j = 0; j < m; j++) {
        if (rows[j] >= n) return "remove_rows: row index out of bounds";
        if (j && rows[j] <= rows[j - 1]) return "remove_rows: rows must be strictly ascending (sorted, no duplicates)";
    }
    return nullptr;
}

// the number of moves: |R below n - m|  (rows checked)
inline uint64_t remove_plan_count(uint64_t n, const uint64_t *rows, uint64_t m) {
    const uint64_t n1 = n - m;
    uint64_t lo = 0, hi = m;  // first j with rows[j] >= n1
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (rows[mid] < n1)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// the moves in the order the replay emits them (descending dst): row src of the old table ends up in slot dst  (rows checked)
inline void remove_plan(uint64_t n, const uint64_t *rows, uint64_t m, std::vector<uint64_t> &dst, std::vector<uint64_t> &src) {
    const uint64_t n1 = n - m, moves = remove_plan_count(n, rows, m);
    dst.clear();
    src.clear();
    dst.reserve(moves);
    src.reserve(moves);
    std::vector<uint64_t> cur(m);
    for (uint64_t j = 0; j < m; j++) cur[j] = n1 + j;
    uint64_t len = n;  // running length of the table
    for (uint64_t j = m; j-- > 0; len--) {
        const uint64_t i = rows[j], c = cur[len - 1 - n1];  // swap_remove(i): the last row takes slot i
        if (i >= n1) {
            cur[i - n1] = c;
        } else {
            dst.push_back(i);
            src.push_back(c);
        }
    }
}

}  // namespace vdb
