// vote_plan.hpp -- the host arithmetic of the k-NN label vote (Index::flat_knn_vote_device / Index::vote_lists_device, k_vote.hip: which
// values of one label column the k nearest rows of a query carry, and how strongly): the argument check with a code per refusal, the
// capacity and the place of the kernel's hash table, its scratch bytes and the sub-chunks of queries that bound a call's lists.  Host
// only: no HIP and no other header of the library but list_plan.hpp (tests/cpp/vote_plan_asan.cpp builds it on its own).
// docs/DESIGN_flat.md 4.1ag.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "list_plan.hpp"

namespace vdb {

constexpr int VOTE_UNIFORM = 0;  // VDB_VOTE_UNIFORM: every vote weighs 1.0f
constexpr int VOTE_INVERSE = 1;  // VDB_VOTE_INVERSE: a vote weighs 1.0f / (d + eps)
constexpr uint64_t VOTE_MAX_K = 4096;
constexpr uint32_t VOTE_LABEL_COLUMNS = 16;  // = LABEL_COLUMNS (kernels.hpp asserts it)
constexpr uint32_t VOTE_TILE = 64;           // list positions per step (one wave)
constexpr uint32_t VOTE_MIN_LG = 7;
// per slot: code, score, votes, first (4 B each) and half a u64 sort key
constexpr uint32_t VOTE_SLOT_BYTES = 20;
// 20 B x 2^11 = 40 KiB: four one-wave workgroups -- one per SIMD -- share the 160 KiB of LDS of a gfx950 CU, and lists of up to 1024
// rows stay in LDS.  One step further (80 KiB) would leave half the SIMDs of a CU without a query.
constexpr uint32_t VOTE_LDS_MAX_LG = 11;

enum VoteBad : int {
    VOTE_OK = 0,
    VOTE_BAD_K = 1,       // k < 1 or k > VOTE_MAX_K
    VOTE_BAD_C = 2,       // c < 1 or c > k
    VOTE_BAD_MODE = 3,    // neither VOTE_UNIFORM nor VOTE_INVERSE
    VOTE_BAD_EPS = 4,     // VOTE_INVERSE: eps not > 0 or not finite
    VOTE_BAD_COLUMN = 5,  // column >= VOTE_LABEL_COLUMNS
};

inline const char *vote_bad_text(int code) {
    switch (code) {
    case VOTE_OK: return nullptr;
    case VOTE_BAD_K: return "vote: k must be in 1 .. 4096 (a longer list is refused, never truncated)";
    case VOTE_BAD_C: return "vote: c must be in 1 .. k";
    case VOTE_BAD_MODE: return "vote: mode must be VDB_VOTE_UNIFORM or VDB_VOTE_INVERSE";
    case VOTE_BAD_EPS: return "vote: eps must be positive and finite with VDB_VOTE_INVERSE";
    case VOTE_BAD_COLUMN: return "vote: column must be below VDB_LABEL_COLUMNS";
    }
    return "vote: bad arguments";
}

// VOTE_OK when the arguments describe a call, otherwise the first thing wrong with them, in the order of VoteBad.  (k is the list length
// ld in the list form.)
inline int vote_check_args(uint64_t k, uint64_t c, int mode, float eps, uint32_t column) {
    if (k < 1 || k > VOTE_MAX_K) return VOTE_BAD_K;
    if (c < 1 || c > k) return VOTE_BAD_C;
    if (mode != VOTE_UNIFORM && mode != VOTE_INVERSE) return VOTE_BAD_MODE;
    if (mode == VOTE_INVERSE && !(eps > 0.0f && eps <= 3.402823466e38f)) return VOTE_BAD_EPS;
    if (column >= VOTE_LABEL_COLUMNS) return VOTE_BAD_COLUMN;
    return VOTE_OK;
}

// log2 of the table's capacity for lists of kp rows: a list entry opens at most one value, so twice kp rounded up to a power of two
// keeps the load at or under one half.  At least 2^VOTE_MIN_LG; 2^13 at kp = VOTE_MAX_K.
inline uint32_t vote_table_lg(uint64_t kp) {
    const uint64_t need = 2 * std::min<uint64_t>(std::max<uint64_t>(kp, 1), VOTE_MAX_K);
    uint32_t lg = VOTE_MIN_LG;
    while ((1ull << lg) < need) lg++;
    return lg;
}
inline bool vote_in_lds(uint32_t lg) { return lg <= VOTE_LDS_MAX_LG; }
// bytes of one query's table and sort keys, in LDS or in the scratch buffer
inline size_t vote_table_bytes(uint32_t lg) { return size_t(VOTE_SLOT_BYTES) << lg; }
// device scratch of a launch over nq queries: none while the table lives in LDS
inline size_t vote_scratch_bytes(uint64_t nq, uint32_t lg) { return vote_in_lds(lg) ? 0 : size_t(nq) * vote_table_bytes(lg); }
// where a code starts probing in a table of 2^lg slots (Fibonacci hashing; the device restates it in k_vote.hip)
inline uint32_t vote_hash(uint32_t code, uint32_t lg) { return (code * 2654435761u) >> (32 - lg); }

// Queries per sub-chunk with lists of kp rows: as many as keep the lists (search form only) and the scratch tables under the budget
inline uint64_t vote_sub_chunk(uint64_t nq, uint64_t kp, bool search = true, uint64_t budget = LIST_BUDGET) {
    if (nq == 0) return 0;
    uint64_t fit = search ? list_sub_chunk(nq, kp, budget) : nq;
    const uint32_t lg = vote_table_lg(kp);
    if (!vote_in_lds(lg)) fit = std::min<uint64_t>(fit, budget / vote_table_bytes(lg));
    return std::max<uint64_t>(1, fit);
}

}  // namespace vdb
