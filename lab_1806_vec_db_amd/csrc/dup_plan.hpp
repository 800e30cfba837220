// dup_plan.hpp -- the host part of the near-duplicate grouping (Index::flat_dup_groups_device / k_components.hip: a range self-join over
// the table's own rows, then the connected components of the pairs it returns): the argument check of vdb_flat_dup_groups and the
// layout of the chunks of queries the driver walks.  Host only: no HIP and no other header of the library
// (tests/cpp/dup_plan_asan.cpp builds it on its own).  docs/DESIGN_flat.md 4.1ab.
//
// The m allowed rows (all n rows without a mask) are the queries, in ascending row order, `chunk` of them per range call.  A chunk's
// queries are read where they lie only on an unfiltered f32 index; under a mask they are gathered, on a u8 index widened, into a buffer
// of chunk_len x dim f32.  Beside that buffer the call keeps 4 B per row of the table for `parent` and 4 B for the group sizes, the
// chunk's radii (the scalar broadcast) and CSR limits, and its counters.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>

namespace vdb {

constexpr uint64_t DUP_CHUNK_DEFAULT = 16384;      // "flat_dup_chunk": the winner of the sweep of tools/bench_dedup.py
constexpr uint64_t DUP_CHUNK_MAX = 1ull << 20;     // what vdb_set_param accepts
constexpr uint64_t DUP_ROW_NONE = ~uint64_t(0);    // = VDB_ROW_NONE: a row outside the mask
constexpr uint64_t DUP_STATS = 4;                  // groups of >= 2 rows | rows in them | non-self pairs seen | truncated rows
constexpr uint64_t DUP_COUNTER_BYTES = 64;         // the device counters of a call (4 x u64) and the two words of the list check

struct DupPlan {
    uint64_t m = 0;              // queries = allowed rows
    uint64_t chunk_len = 0;      // queries of every chunk but the last: min(chunk, m)
    uint64_t n_chunks = 0;       // range calls: ceil(m / chunk)
    uint64_t last_len = 0;       // queries of the last chunk (0 without queries)
    bool gather = false;         // the queries are copied into a buffer first (a mask, or u8 rows)
    uint64_t scratch_bytes = 0;  // device bytes the call holds besides a chunk's range result
};

// Everything vdb_flat_dup_groups refuses that is no property of the index's state: "" when the call is accepted.  The range call has
// no cap on `limit` (0: none), so none is added here; a radius of +-inf or below zero is a valid question (one group; no pairs).
inline std::string dup_check_args(uint64_t n_rows, uint64_t m_allowed, bool masked, float radius, uint64_t chunk) {
    if (radius != radius) return "dup groups: the radius is NaN";
    if (n_rows >= (1ull << 32)) return "dup groups: an index of 2^32 rows or more";
    if (chunk < 1 || chunk > DUP_CHUNK_MAX) return "dup groups: flat_dup_chunk must be in 1 .. 2^20";
    if (masked ? m_allowed > n_rows : m_allowed != n_rows)
        return "dup groups: " + std::to_string(m_allowed) + " allowed rows, the index holds " + std::to_string(n_rows);
    return "";
}

// the plan of CHECKED arguments
inline DupPlan dup_plan(uint64_t n_rows, uint64_t dim, bool elem_u8, bool masked, uint64_t m_allowed, uint64_t chunk) {
    DupPlan p;
    p.m = m_allowed;
    p.chunk_len = std::min(chunk, m_allowed);
    p.n_chunks = (m_allowed + chunk - 1) / chunk;
    p.last_len = m_allowed ? m_allowed - (p.n_chunks - 1) * chunk : 0;
    p.gather = masked || elem_u8;
    p.scratch_bytes = 2 * n_rows * sizeof(uint32_t) + p.chunk_len * sizeof(float) + (p.chunk_len + 1) * sizeof(uint64_t) + DUP_COUNTER_BYTES +
                      (p.gather ? p.chunk_len * dim * sizeof(float) : 0);
    return p;
}

}  // namespace vdb
