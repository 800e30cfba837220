// mmr_plan.hpp -- the host arithmetic of the diversified Flat k-NN (Index::flat_knn_mmr_device / Index::mmr_select_device, k_mmr.hip:
// greedy maximal-marginal-relevance selection over a query's candidate list): the argument check, the LDS bytes of the kernel's state
// and the sub-chunks of queries that bound a call's candidate lists.  Host only: no HIP and no other header of the library
// (tests/cpp/mmr_plan_asan.cpp builds it on its own).  docs/DESIGN_flat.md 4.1u.
//
// A call is ONE round: the exact sorted list of min(m, fetch_k) rows per query from the existing search, then k_mmr_select, one
// workgroup per query, picks min(k, list length) of them.  fetch_k changes the answer, so it is an argument and not a parameter.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "list_plan.hpp"

namespace vdb {

constexpr uint64_t MMR_MAX_FETCH = 4096;          // longest candidate list: fetch_k of the search form, ld of the list form
constexpr uint32_t MMR_STAGE_FLOATS = 2048;       // floats of the row selected last that LDS holds at a time: a longer row goes through in pieces
constexpr uint32_t MMR_SMALL_THREADS = 64;        // a list of up to 64 positions: one wave
constexpr uint32_t MMR_THREADS = 256;             // every longer list: four waves
constexpr uint32_t MMR_MAX_WAVES = MMR_THREADS / 64;

// nullptr when (k, fetch_k, lambda) is a call the selection accepts, otherwise what is wrong with it.  The list form passes its ld as
// fetch_k: k <= ld <= MMR_MAX_FETCH.  (!(lambda >= 0 && lambda <= 1) refuses NaN too.)
inline const char *mmr_check_args(uint64_t k, uint64_t fetch_k, float lambda) {
    if (!(lambda >= 0.0f && lambda <= 1.0f)) return "mmr: lambda must be a number in [0, 1]";
    if (fetch_k < k) return "mmr: fetch_k (the list length) must be at least k";
    if (fetch_k > MMR_MAX_FETCH) return "mmr: fetch_k (the list length) must be at most 4096";
    return nullptr;
}

// threads of the workgroup that selects from lists of ld positions
inline uint32_t mmr_threads(uint64_t ld) { return ld <= MMR_SMALL_THREADS ? MMR_SMALL_THREADS : MMR_THREADS; }
// list positions the LDS arrays are laid out for: ld rounded up to a multiple of 4, at least 4 (so the staged row starts 16-byte aligned)
inline uint32_t mmr_positions(uint64_t ld) { return (uint32_t)((std::max<uint64_t>(ld, 1) + 3) & ~3ull); }
// floats of the staging buffer for rows of dim floats: dim rounded up to a multiple of 4, at most MMR_STAGE_FLOATS
inline uint32_t mmr_stage_floats(uint64_t dim) { return (uint32_t)std::min<uint64_t>((std::max<uint64_t>(dim, 1) + 3) & ~3ull, MMR_STAGE_FLOATS); }
// LDS bytes of k_mmr_select for lists of ld (<= MMR_MAX_FETCH) positions over rows of dim floats: per position d_p, m_p and the fold's
// carried sum (f32 each), the staged row, a (score, position) pair per wave for the argmin, and a selected byte per position.
// At most 3 x 16 KiB + 8 KiB + 32 B + 4 KiB = 61472 bytes: under the 64 KiB a launch gets without asking for more.
inline size_t mmr_lds_bytes(uint64_t ld, uint64_t dim) {
    const size_t fp = mmr_positions(ld);
    return fp * 3 * sizeof(float) + size_t(mmr_stage_floats(dim)) * sizeof(float) + MMR_MAX_WAVES * 2 * sizeof(uint32_t) + fp;
}
// queries per sub-chunk of a call with lists of kp rows, and the list length of the call's one round: fetch_k clamped (list_plan.hpp)
inline uint64_t mmr_sub_chunk(uint64_t nq, uint64_t kp, uint64_t budget = LIST_BUDGET) { return list_sub_chunk(nq, kp, budget); }
inline uint64_t mmr_list_len(uint64_t fetch_k, uint64_t max_m) { return list_len(fetch_k, max_m); }

}  // namespace vdb
