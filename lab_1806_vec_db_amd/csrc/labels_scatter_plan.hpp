// labels_scatter_plan.hpp -- the argument check and the upload of a scattered label write (Index::labels_scatter).  Host only: no HIP,
// and of the library only update_plan.hpp, whose check of a list of distinct rows it shares (tests/cpp/labels_scatter_plan_asan.cpp
// builds it on its own).
//
// A scattered write sets label[columns[c]][rows[j]] = codes[c][j] for m distinct rows and n_cols distinct columns.  The plan is the
// check -- everything below is known BEFORE a column is allocated or written -- and the ids narrowed to u32 for the upload; the codes
// travel as they are, [n_cols][m].  Time and memory are the row check's (update_plan.hpp: a bitmap over the table, or a sort of a short list).
#pragma once
#include <cstdint>

#include "update_plan.hpp"

namespace vdb {

constexpr uint32_t SCATTER_LABEL_COLUMNS = 16;  // = LABEL_COLUMNS (kernels.hpp asserts it)

// nullptr: 1 <= n_cols <= SCATTER_LABEL_COLUMNS (0 allowed with m == 0), every column below SCATTER_LABEL_COLUMNS and named once;
// otherwise what is wrong with it
inline const char *labels_scatter_columns_check(uint64_t m, const uint32_t *columns, uint64_t n_cols) {
    if (n_cols > SCATTER_LABEL_COLUMNS) return "labels_scatter: more columns than an index has";
    if (n_cols == 0) return m ? "labels_scatter: rows without a column to write" : nullptr;
    if (!columns) return "labels_scatter: null columns";
    uint32_t seen = 0;
    for (uint64_t c = 0; c < n_cols; c++) {
        if (columns[c] >= SCATTER_LABEL_COLUMNS) return "labels_scatter: column out of range";
        if ((seen >> columns[c]) & 1u) return "labels_scatter: a column is named twice";
        seen |= 1u << columns[c];
    }
    return nullptr;
}

// ... and rows[0..m) distinct and below n (any order)
inline const char *labels_scatter_check(uint64_t n, const uint64_t *rows, uint64_t m, const uint32_t *columns, uint64_t n_cols) {
    if (const char *why = labels_scatter_columns_check(m, columns, n_cols)) return why;
    switch (distinct_rows_check(n, rows, m)) {
    case ROWS_NULL: return "labels_scatter: null rows";
    case ROWS_OUT_OF_BOUNDS: return "labels_scatter: row index out of bounds";
    case ROWS_DUPLICATE: return "labels_scatter: duplicate row ids";
    default: return nullptr;
    }
}

// the ids as uploaded (rows checked, n at most 2^32: every id fits); the narrowing of every host id list (Index::upload_ids)
inline void labels_scatter_ids(const uint64_t *rows, uint64_t m, uint32_t *out_ids32) {
    for (uint64_t j = 0; j < m; j++) out_ids32[j] = uint32_t(rows[j]);
}

}  // namespace vdb
