// fuse_plan.hpp -- the host arithmetic of the fused multi-query Flat search (Index::flat_knn_fused_device / Index::fuse_lists_device,
// k_fuse.hip: several sorted lists per question joined into one top-k by reciprocal rank fusion or by the smallest distance): the
// argument check with a code per refusal, the longest fused query, the size and the place of the kernel's hash table, its scratch bytes
// and the sub-chunks of fused queries that bound a call's lists.  Host only: no HIP and no other header of the library
// (tests/cpp/fuse_plan_asan.cpp builds it on its own).  docs/DESIGN_flat.md 4.1w.
//
// A call is ONE round: the exact sorted list of min(m_s, fetch_k) rows of every sub-query from the existing search, then k_fuse_lists,
// one workgroup per fused query.  fetch_k changes the answer, so it is an argument and not a parameter.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "list_plan.hpp"

namespace vdb {

constexpr int FUSE_RRF = 0, FUSE_MIN = 1;        // VDB_FUSE_RRF / VDB_FUSE_MIN
constexpr uint64_t FUSE_MAX_LISTS = 32;          // sub-queries (lists) of one fused query
constexpr uint64_t FUSE_MAX_FETCH = 4096;        // longest list: fetch_k of the search forms, ld of the list form
constexpr uint64_t FUSE_MAX_ENTRIES = 16384;     // lists x list length of one fused query
constexpr uint64_t FUSE_MAX_SUBQ = 16384;        // sub-queries one list call of the search forms takes
constexpr uint32_t FUSE_THREADS = 256;           // the workgroup of k_fuse_lists; a tile of a list is that many positions
constexpr uint32_t FUSE_MIN_LG = 6, FUSE_LDS_MAX_LG = 13;  // the table has 2^lg slots; up to 2^13 of them live in LDS (128 KiB)
constexpr uint32_t FUSE_SLOT_BYTES = 16;         // per slot: key, accumulator, stamp (4 B each) and half a u64 sort key
constexpr uint32_t FUSE_EMPTY = 0xFFFFFFFFu;     // the key of a free slot (no row: n < 2^32)

// what fuse_check_args refuses, in the order it looks
enum FuseBad : int {
    FUSE_OK = 0,
    FUSE_BAD_MODE = 1,
    FUSE_BAD_LIMS_NULL = 2,
    FUSE_BAD_LIMS_START = 3,
    FUSE_BAD_LIMS_DESCEND = 4,
    FUSE_BAD_NO_LIST = 5,
    FUSE_BAD_TOO_MANY_LISTS = 6,
    FUSE_BAD_FETCH_BELOW_K = 7,
    FUSE_BAD_FETCH_ABOVE_CAP = 8,
    FUSE_BAD_ENTRIES = 9,
    FUSE_BAD_WEIGHTS_WITH_MIN = 10,
    FUSE_BAD_WEIGHT = 11,
    FUSE_BAD_C = 12,
};

inline const char *fuse_bad_text(int code) {
    switch (code) {
    case FUSE_OK: return nullptr;
    case FUSE_BAD_MODE: return "fuse: mode must be VDB_FUSE_RRF or VDB_FUSE_MIN";
    case FUSE_BAD_LIMS_NULL: return "fuse: null list limits";
    case FUSE_BAD_LIMS_START: return "fuse: list limits must start at 0";
    case FUSE_BAD_LIMS_DESCEND: return "fuse: list limits must not decrease";
    case FUSE_BAD_NO_LIST: return "fuse: every fused query needs at least one sub-query";
    case FUSE_BAD_TOO_MANY_LISTS: return "fuse: at most 32 sub-queries per fused query";
    case FUSE_BAD_FETCH_BELOW_K: return "fuse: fetch_k must be at least k";
    case FUSE_BAD_FETCH_ABOVE_CAP: return "fuse: fetch_k (the list length) must be at most 4096";
    case FUSE_BAD_ENTRIES: return "fuse: sub-queries x fetch_k (the list length) must be at most 16384 per fused query";
    case FUSE_BAD_WEIGHTS_WITH_MIN: return "fuse: weights belong to VDB_FUSE_RRF only";
    case FUSE_BAD_WEIGHT: return "fuse: every weight must be a finite number above 0";
    case FUSE_BAD_C: return "fuse: rrf_c must be a finite number, at least 0";
    }
    return "fuse: bad argument";
}

inline bool fuse_finite(float v) { return v - v == 0.0f; }  // (NaN and +-inf give NaN)

// FUSE_OK when the arguments describe a call, otherwise the first thing wrong with them.  lims [nq + 1] (nq == 0: lims[0] is still
// read); weights [lims[nq]] or nullptr.  list_form: fetch_k is the ld of caller-supplied lists, which k may exceed.
inline int fuse_check_args(int mode, const uint64_t *lims, uint64_t nq, uint64_t k, uint64_t fetch_k, const float *weights, float rrf_c,
                           bool list_form = false) {
    if (mode != FUSE_RRF && mode != FUSE_MIN) return FUSE_BAD_MODE;
    if (!lims) return FUSE_BAD_LIMS_NULL;
    if (lims[0] != 0) return FUSE_BAD_LIMS_START;
    for (uint64_t q = 0; q < nq; q++)
        if (lims[q + 1] < lims[q]) return FUSE_BAD_LIMS_DESCEND;
    uint64_t s_max = 0;
    for (uint64_t q = 0; q < nq; q++) {
        const uint64_t s = lims[q + 1] - lims[q];
        if (s == 0) return FUSE_BAD_NO_LIST;
        if (s > FUSE_MAX_LISTS) return FUSE_BAD_TOO_MANY_LISTS;
        s_max = std::max(s_max, s);
    }
    if (!list_form && fetch_k < k) return FUSE_BAD_FETCH_BELOW_K;
    if (fetch_k > FUSE_MAX_FETCH) return FUSE_BAD_FETCH_ABOVE_CAP;
    if (s_max * fetch_k > FUSE_MAX_ENTRIES) return FUSE_BAD_ENTRIES;  // (<= 32 x 4096: no overflow)
    if (weights) {
        if (mode == FUSE_MIN) return FUSE_BAD_WEIGHTS_WITH_MIN;
        for (uint64_t j = 0; j < lims[nq]; j++)
            if (!(weights[j] > 0.0f) || !fuse_finite(weights[j])) return FUSE_BAD_WEIGHT;
    }
    if (!(rrf_c >= 0.0f) || !fuse_finite(rrf_c)) return FUSE_BAD_C;
    return FUSE_OK;
}

// the most lists of one fused query; the limits have passed fuse_check_args
inline uint64_t fuse_s_max(const uint64_t *lims, uint64_t nq) {
    uint64_t s = 0;
    for (uint64_t q = 0; q < nq; q++) s = std::max(s, lims[q + 1] - lims[q]);
    return s;
}

// list length of the search forms' one round: fetch_k clamped to the longest allowed set among the sub-queries (list_plan.hpp)
inline uint64_t fuse_list_len(uint64_t fetch_k, uint64_t max_m) { return list_len(fetch_k, max_m); }

// The table of a launch whose fused queries hold up to s_max lists of ld positions: 2^lg slots, the smallest power of two that keeps the
// load at or under one half, at least 2^FUSE_MIN_LG.  s_max x ld <= FUSE_MAX_ENTRIES: lg <= 15.
inline uint32_t fuse_table_lg(uint64_t s_max, uint64_t ld) {
    const uint64_t entries = std::min<uint64_t>(s_max * ld, FUSE_MAX_ENTRIES);
    uint32_t lg = FUSE_MIN_LG;
    while ((1ull << lg) < 2 * entries) lg++;
    return lg;
}
inline bool fuse_in_lds(uint32_t lg) { return lg <= FUSE_LDS_MAX_LG; }
// bytes of one fused query's table and sort keys, in LDS or in the scratch buffer
inline size_t fuse_table_bytes(uint32_t lg) { return size_t(FUSE_SLOT_BYTES) << lg; }
// device scratch of a launch over nq fused queries: none while the table lives in LDS
inline size_t fuse_scratch_bytes(uint64_t nq, uint32_t lg) { return fuse_in_lds(lg) ? 0 : size_t(nq) * fuse_table_bytes(lg); }
// where the table starts probing for a LOCAL row (the tests build colliding ids from it)
inline uint32_t fuse_hash(uint32_t row, uint32_t lg) { return (row * 2654435761u) >> (32 - lg); }

// Fused queries per sub-chunk: as many as keep the lists (s_max x kp pairs each) and the scratch under LIST_BUDGET and the sub-queries of
// one list call at or under FUSE_MAX_SUBQ; at least 1, at most nq (0 for nq == 0).  search == false (the list form): only the scratch counts.
inline uint64_t fuse_sub_chunk(uint64_t nq, uint64_t s_max, uint64_t kp, bool search = true, uint64_t budget = LIST_BUDGET) {
    if (nq == 0) return 0;
    const uint64_t sm = std::min<uint64_t>(std::max<uint64_t>(s_max, 1), FUSE_MAX_LISTS), kk = std::min<uint64_t>(std::max<uint64_t>(kp, 1), FUSE_MAX_FETCH);
    uint64_t fit = nq;
    if (search) fit = std::min(list_sub_chunk(fit, sm * kk, budget), FUSE_MAX_SUBQ / sm);  // (its floor of 1 is the one below)
    const uint32_t lg = fuse_table_lg(sm, kk);
    if (!fuse_in_lds(lg)) fit = std::min<uint64_t>(fit, budget / fuse_table_bytes(lg));
    return std::max<uint64_t>(1, fit);
}

}  // namespace vdb
