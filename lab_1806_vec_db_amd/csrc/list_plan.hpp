// list_plan.hpp -- the host arithmetic that the Flat list re-rankers share (flat_rerank.hip: grouped, MMR, by-example and fused search;
// grouped_plan.hpp, mmr_plan.hpp, like_plan.hpp, fuse_plan.hpp): the byte budget of the candidate lists of one sub-chunk of queries, the
// queries that fit it and the clamp of a list length.  Host only: no HIP and no other header of the library
// (tests/cpp/list_plan_asan.cpp builds it on its own).  docs/DESIGN_flat.md 4.1x.
#pragma once
#include <algorithm>
#include <cstdint>

namespace vdb {

// the candidate lists of one sub-chunk -- rows x K' x (8 B id + 4 B distance) -- stay at or under this many bytes
constexpr uint64_t LIST_BUDGET = 256ull << 20;
constexpr uint64_t LIST_PAIR_BYTES = 12;

inline uint64_t list_sat_mul(uint64_t a, uint64_t b) { return (a && b > ~0ull / a) ? ~0ull : a * b; }

// lists per sub-chunk when a list has kp rows: as many as the budget holds, at least 1, at most `rows` (so 1 for rows == 0)
inline uint64_t list_sub_chunk(uint64_t rows, uint64_t kp, uint64_t budget = LIST_BUDGET) {
    return std::max<uint64_t>(1, std::min(rows, budget / list_sat_mul(std::max<uint64_t>(kp, 1), LIST_PAIR_BYTES)));
}
// list length of a round: `want` clamped to the longest allowed set among its queries, at least 1 (max_m == 0: nothing is allowed -- one
// slot is still asked for so that every buffer has a size)
inline uint64_t list_len(uint64_t want, uint64_t max_m) { return std::max<uint64_t>(1, std::min(want, max_m)); }

}  // namespace vdb
