// update_plan.hpp -- which 16-row mirror tiles an in-place update of many rows touches.  Host only: no HIP, no other header of the library
// (tests/cpp/update_plan_asan.cpp builds it on its own).
//
// Index::update_rows writes new vectors into the rows R (m of them, distinct, in any order).  No row moves, so the plan is only the set of
// 16-row tiles { r / 16 : r in R } that every live fragment-ordered mirror has to rewrite, each once: ascending and distinct, as the list
// forms of the re-tiling kernels take them.  O(m log m) time, O(m) memory.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace vdb {

// nullptr: rows[0..m) are distinct and below n (any order); otherwise what is wrong with it
inline const char *update_plan_check(uint64_t n, const uint64_t *rows, uint64_t m) {
    if (m && !rows) return "update_rows: null rows";
    for (uint64_t j = 0; j < m; j++)
        if (rows[j] >= n) return "update_rows: row index out of bounds";
    if (m > n) return "update_rows: duplicate row ids";  // (more ids than rows; also bounds the copy below)
    std::vector<uint64_t> sorted(rows, rows + m);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return "update_rows: duplicate row ids";
    return nullptr;
}

// the ascending, distinct tiles rows[j] / 16  (rows checked: every tile number is below 2^32 for the tables the library holds)
inline void update_plan(uint64_t n, const uint64_t *rows, uint64_t m, std::vector<uint32_t> &tiles) {
    (void)n;
    tiles.resize(m);
    for (uint64_t j = 0; j < m; j++) tiles[j] = uint32_t(rows[j] / 16);
    std::sort(tiles.begin(), tiles.end());
    tiles.erase(std::unique(tiles.begin(), tiles.end()), tiles.end());
}

}  // namespace vdb
