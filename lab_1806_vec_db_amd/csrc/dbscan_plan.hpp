// dbscan_plan.hpp -- the host part of the density clustering (Index::flat_dbscan_device / k_dbscan.hip: the range self-join of the
// near-duplicate grouping, then core test, components of the core rows, border rows and noise): the argument check of vdb_flat_dbscan and
// the layout of a call.  Host only: no HIP.  docs/DESIGN_flat.md 4.1ae.
//
// The rule.  The allowed rows are all rows, or the rows of a mask.
//   Neighbourhood.  N(i) is the set of allowed rows the exact range search lists for query = row i at radius eps with no limit: the list
//     flat_range_device returns, boundary included.  Row i itself is on it when D(i, i) <= eps.  A NaN row lists nothing.
//   Core.  Row i is CORE iff |N(i)| >= min_samples.  The row itself counts, as in scikit-learn.
//   Clusters.  Two core rows are linked when one is in the other's neighbourhood.  A CLUSTER is a connected component of the core rows.
//     It is named by its LOWEST CORE ROW.
//   Border.  A non-core row with at least one core row in N(i) is a BORDER row.  It joins the cluster of the core row with the smallest
//     (distance, row) key, the order the range list already has.
//   Noise.  Every other allowed row is NOISE.
//   Determinism.  The answer is a function of the table, eps, min_samples and the mask alone.  The order of waves, chunks and launches
//     does not matter.
//   There is no `limit`: a truncated list breaks the core test.
//
// The chunks of queries are those of the near-duplicate grouping (dup_plan.hpp, "flat_dup_chunk").  Beside the chunk's gathered queries,
// radii and limits a call keeps per row of the table 4 B for `parent`, 8 B for `border` (the best (distance, core row) key offered to the
// row so far) and 1 B for `kind`, and its counters.
#pragma once
#include <cstdint>
#include <string>

#include "dup_plan.hpp"

namespace vdb {

constexpr uint64_t DBSCAN_ROW_NONE = ~uint64_t(0);         // = VDB_ROW_NONE: a row outside the mask
constexpr uint64_t DBSCAN_ROW_NOISE = ~uint64_t(0) - 1;    // = VDB_ROW_NOISE
constexpr uint64_t DBSCAN_STATS = 5;                       // clusters | core rows | border rows | noise rows | non-self pairs seen
constexpr uint64_t DBSCAN_COUNTER_BYTES = 64;              // the device counters of a call (5 x u64, one spare) and the two words of the list check
constexpr uint8_t DBSCAN_OUTSIDE = 0, DBSCAN_NOISE = 1, DBSCAN_BORDER = 2, DBSCAN_CORE = 3;  // `kind`

struct DbscanPlan {
    DupPlan walk;                // the chunks of queries: the walk of the near-duplicate grouping
    uint64_t scratch_bytes = 0;  // device bytes the call holds besides a chunk's range result
};

// "" when min_samples is one the core test can be made with
inline std::string dbscan_check_min_samples(uint64_t min_samples) {
    if (min_samples < 1 || min_samples >= (1ull << 32)) return "dbscan: min_samples must be in 1 .. 2^32 - 1";
    return "";
}

// Everything vdb_flat_dbscan refuses that is no property of the index's state: "" when the call is accepted.  An eps of +-inf or below zero
// is a valid question (one cluster of the rows without NaN when it is large enough to be core; all noise).
inline std::string dbscan_check_args(uint64_t n_rows, uint64_t m_allowed, bool masked, float eps, uint64_t min_samples, uint64_t chunk) {
    if (eps != eps) return "dbscan: eps is NaN";
    const std::string ms = dbscan_check_min_samples(min_samples);
    if (!ms.empty()) return ms;
    if (n_rows >= (1ull << 32)) return "dbscan: an index of 2^32 rows or more";
    if (chunk < 1 || chunk > DUP_CHUNK_MAX) return "dbscan: flat_dup_chunk must be in 1 .. 2^20";
    if (masked ? m_allowed > n_rows : m_allowed != n_rows)
        return "dbscan: " + std::to_string(m_allowed) + " allowed rows, the index holds " + std::to_string(n_rows);
    return "";
}

// the plan of CHECKED arguments
inline DbscanPlan dbscan_plan(uint64_t n_rows, uint64_t dim, bool elem_u8, bool masked, uint64_t m_allowed, uint64_t chunk) {
    DbscanPlan p;
    p.walk = dup_plan(n_rows, dim, elem_u8, masked, m_allowed, chunk);
    const uint64_t len = p.walk.chunk_len;
    const uint64_t radii = (len * sizeof(float) + 7) & ~uint64_t(7);  // (the limits behind them are 8-byte aligned)
    p.scratch_bytes = n_rows * (sizeof(uint32_t) + sizeof(uint64_t) + sizeof(uint8_t)) + radii + (len + 1) * sizeof(uint64_t) +
                      DBSCAN_COUNTER_BYTES + (p.walk.gather ? len * dim * sizeof(float) : 0);
    return p;
}

}  // namespace vdb
