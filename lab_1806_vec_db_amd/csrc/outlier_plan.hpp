// outlier_plan.hpp -- the host part of the k-NN self-join and the outlier scores on it (Index::flat_knn_graph_device /
// Index::flat_outliers_device / Index::lof_lists_device; k_outlier.hip): the argument check, the chunks of queries the driver walks, the
// bytes of the graph and the lane-group width of the two score stages.  Host only: no HIP.  docs/DESIGN_flat.md 4.1ah.
//
// The rule.  A is the allowed rows (all rows, or the rows of one mask), m = |A|.  For p in A:
//   N(p)        the first kk = min(k, m - 1) rows of A \ {p} in the (distance, index) order of the exact f32 pair distance, NaN greatest.
//               Exactly kk members, no tie extension (what sklearn.neighbors.LocalOutlierFactor does).
//   kdist(p)    the distance of the last member of N(p).
//   reach(p, o) max(kdist(o), d(p, o)).
//   lrd(p)      1 / (mean over o in N(p) of reach(p, o) + 1e-10).
//   lof(p)      (mean over o in N(p) of lrd(o)) / lrd(p).
//   m = 1 gives kk = 0: the count is 0 and all three values are NaN.  A NaN anywhere propagates (the max included).
//   Means, reciprocals and the quotient are f64 over the f32 distances the search returned; each output is rounded to f32 once.  No float
//   atomics and a fixed summation order: two calls give the same bits.
//   Self-exclusion is by ID: the kp = min(k + 1, m) nearest allowed rows are fetched; p is dropped where it stands, else the last entry is.
//
// The m allowed rows are the queries, in ascending row order, chunk_len of them per search call at kp: `chunk` ("flat_dup_chunk", the
// self-joins' parameter) clipped so that one chunk's lists stay under LIST_BUDGET.  A call holds the graph [m][k] (4 B local row + 4 B
// distance per slot), 4 B per position for the counts, and per row of the table 4 B for kdist and 8 B for the f64 lrd -- indexed by ROW, so
// the gathers of the score stages need no row-to-position map under a mask.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>

#include "dup_plan.hpp"
#include "list_plan.hpp"

namespace vdb {

constexpr uint64_t OUTLIER_MAX_K = 1023;  // the search underneath is asked for k + 1 <= 1024 rows (its register-resident select)

struct OutlierPlan {
    uint64_t m = 0;              // queries = allowed rows
    uint64_t kk = 0;             // members of every N(p): min(k, m - 1)
    uint64_t kp = 0;             // rows fetched per query: min(k + 1, m)
    uint64_t chunk_len = 0;      // queries of every chunk but the last
    uint64_t n_chunks = 0;       // search calls
    uint64_t last_len = 0;       // queries of the last chunk (0 without queries)
    bool gather = false;         // the queries are copied into a buffer first (a mask)
    uint32_t group = 0;          // lanes per source row in the score stages: pow2ceil(k) for k <= 64; 0: a wave per row, strided
    uint64_t graph_bytes = 0;    // 8 B x m x k
    uint64_t scratch_bytes = 0;  // device bytes an outliers call holds besides what the search itself takes
};

// lanes that share one source row in k_lof_lrd / k_lof_score: the next power of two at or above k while a wave holds it, else 0
inline uint32_t outlier_group(uint64_t k) {
    if (k > 64) return 0;
    uint32_t g = 1;
    while (g < k) g *= 2;
    return g;
}

// "" when k is one the graph can be built with
inline std::string outlier_check_k(uint64_t k) {
    if (k < 1 || k > OUTLIER_MAX_K) return "outliers: k must be in 1 .. 1023";
    return "";
}

// Everything vdb_flat_knn_graph / vdb_flat_outliers refuse that is no property of the index's state: "" when the call is accepted
inline std::string outlier_check_args(uint64_t n_rows, uint64_t m_allowed, bool masked, bool elem_u8, uint64_t k, uint64_t chunk) {
    if (elem_u8) return "outliers: needs f32 rows (a u8 index is not scored)";
    const std::string bad = outlier_check_k(k);
    if (!bad.empty()) return bad;
    if (n_rows >= (1ull << 32)) return "outliers: an index of 2^32 rows or more";
    if (chunk < 1 || chunk > DUP_CHUNK_MAX) return "outliers: flat_dup_chunk must be in 1 .. 2^20";
    if (masked ? m_allowed > n_rows : m_allowed != n_rows)
        return "outliers: " + std::to_string(m_allowed) + " allowed rows, the index holds " + std::to_string(n_rows);
    return "";
}

// the plan of CHECKED arguments
inline OutlierPlan outlier_plan(uint64_t n_rows, uint64_t dim, bool masked, uint64_t m_allowed, uint64_t k, uint64_t chunk) {
    OutlierPlan p;
    p.m = m_allowed;
    p.kk = m_allowed ? std::min(k, m_allowed - 1) : 0;
    p.kp = std::min(k + 1, m_allowed);
    const uint64_t per = list_sub_chunk(chunk, p.kp);  // `chunk`, or what the list budget holds
    p.chunk_len = std::min(per, m_allowed);
    p.n_chunks = (m_allowed + per - 1) / per;
    p.last_len = m_allowed ? m_allowed - (p.n_chunks - 1) * per : 0;
    p.gather = masked;
    p.group = outlier_group(k);
    p.graph_bytes = 2 * sizeof(uint32_t) * m_allowed * k;
    p.scratch_bytes = p.graph_bytes + m_allowed * sizeof(uint32_t) + n_rows * (sizeof(float) + sizeof(double)) +
                      p.chunk_len * (p.kp * LIST_PAIR_BYTES + sizeof(uint64_t)) + (p.gather ? p.chunk_len * dim * sizeof(float) : 0);
    return p;
}

}  // namespace vdb
