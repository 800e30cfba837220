// fetch_plan.hpp -- how a bulk row fetch (Index::get_rows) is carried out.  Host only: no HIP, no other header of the library
// (tests/cpp/fetch_plan_asan.cpp builds it on its own).
//
// A fetch reads the rows R (m of them, in any order, repeats allowed: the call only reads) into m contiguous output rows.  The plan is
// the route and, for the gathered route, how the output is cut into chunks that pass through a bounded staging buffer:
//   DIRECT  R is one ascending run of consecutive rows (rows[j] == rows[0] + j, m >= 1): the output is a contiguous piece of the table
//           and is copied from it as it stands, no kernel;
//   GATHER  everything else (m == 0 included, which does nothing): chunk_rows = max(1, chunk_bytes / out_row_bytes) output rows per
//           chunk, n_chunks = ceil(m / chunk_rows).
// O(m) time, no memory.
#pragma once
#include <cstdint>

namespace vdb {

enum FetchRoute : int { FETCH_GATHER = 0, FETCH_DIRECT = 1 };

struct FetchPlan {
    int route = FETCH_GATHER;
    uint64_t chunk_rows = 1;  // output rows per chunk
    uint64_t n_chunks = 0;    // ceil(m / chunk_rows)
};

// nullptr: rows[0..m) are all below n (any order, repeats allowed) and m * row_bytes fits 64 bits; otherwise what is wrong with it
inline const char *fetch_plan_check(uint64_t n, const uint64_t *rows, uint64_t m, uint64_t row_bytes = 1) {
    if (m && !rows) return "get_rows: null rows";
    if (row_bytes && m > ~uint64_t(0) / row_bytes) return "get_rows: the result does not fit the address space";
    for (uint64_t j = 0; j < m; j++)
        if (rows[j] >= n) return "get_rows: row index out of bounds";
    return nullptr;
}

// the chunking alone: what a list that is known not to be a run (a mask's rows, a widened u8 fetch) takes
inline FetchPlan fetch_plan_chunks(uint64_t m, uint64_t out_row_bytes, uint64_t chunk_bytes) {
    FetchPlan p;
    const uint64_t per = out_row_bytes ? chunk_bytes / out_row_bytes : chunk_bytes;
    p.chunk_rows = per ? per : 1;
    p.n_chunks = m / p.chunk_rows + (m % p.chunk_rows ? 1 : 0);  // (no m + chunk_rows - 1: that sum may wrap)
    return p;
}

// rows checked by fetch_plan_check
inline FetchPlan fetch_plan(const uint64_t *rows, uint64_t m, uint64_t out_row_bytes, uint64_t chunk_bytes) {
    FetchPlan p = fetch_plan_chunks(m, out_row_bytes, chunk_bytes);
    bool run = m >= 1;
    for (uint64_t j = 1; run && j < m; j++) run = rows[j] - rows[0] == j;  // (unsigned: a smaller row wraps to a huge difference)
    p.route = run ? FETCH_DIRECT : FETCH_GATHER;
    return p;
}

}  // namespace vdb
