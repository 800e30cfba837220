// update_plan.hpp -- which 16-row mirror tiles an in-place update of many rows touches.  Host only: no HIP, no other header of the library
// (tests/cpp/update_plan_asan.cpp builds it on its own).
//
// Index::update_rows writes new vectors into the rows R (m of them, distinct, in any order).  No row moves, so the plan is only the set of
// 16-row tiles { r / 16 : r in R } that every live fragment-ordered mirror has to rewrite, each once: ascending and distinct, as the list
// forms of the re-tiling kernels take them.  O(m log m) time, O(m) memory (the row check: O(m) time over a bitmap of at most 4 words per row).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace vdb {

// THE check of a list of rows that a write goes through (update_rows here, the label scatter of labels_scatter_plan.hpp): ROWS_OK when
// rows[0..m) are distinct and below n (any order); otherwise what is wrong with it
enum RowsCheck : int { ROWS_OK = 0, ROWS_NULL = 1, ROWS_OUT_OF_BOUNDS = 2, ROWS_DUPLICATE = 3 };
inline RowsCheck distinct_rows_check(uint64_t n, const uint64_t *rows, uint64_t m) {
    if (m && !rows) return ROWS_NULL;
    for (uint64_t j = 0; j < m; j++)
        if (rows[j] >= n) return ROWS_OUT_OF_BOUNDS;
    if (m > n) return ROWS_DUPLICATE;  // (more ids than rows; also bounds the copies below)
    // A list that is not tiny against the table marks its rows in a bitmap over [0, n): one clear of n / 64 words and one pass over the
    // list, against a sort of the list (docs/DESIGN_flat.md 4.1t has what the sort cost a label write of 100 000 of 1M rows).  The bitmap
    // is taken when it has at most 4 words per listed row, so that the clear costs no more than a few list passes; a short list over
    // a large table keeps the sort, which touches O(m) memory whatever n is.
    const uint64_t words = n / 64 + 1;
    if (words / 4 <= m) {
        std::vector<uint64_t> seen(words, 0);
        for (uint64_t j = 0; j < m; j++) {
            uint64_t &w = seen[rows[j] >> 6];
            const uint64_t bit = uint64_t(1) << (rows[j] & 63);
            if (w & bit) return ROWS_DUPLICATE;
            w |= bit;
        }
        return ROWS_OK;
    }
    std::vector<uint64_t> sorted(rows, rows + m);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return ROWS_DUPLICATE;
    return ROWS_OK;
}

// nullptr: rows[0..m) are distinct and below n (any order); otherwise what is wrong with it
inline const char *update_plan_check(uint64_t n, const uint64_t *rows, uint64_t m) {
    switch (distinct_rows_check(n, rows, m)) {
    case ROWS_NULL: return "update_rows: null rows";
    case ROWS_OUT_OF_BOUNDS: return "update_rows: row index out of bounds";
    case ROWS_DUPLICATE: return "update_rows: duplicate row ids";
    default: return nullptr;
    }
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
