// fuse_groups_plan.hpp -- the host arithmetic of the document-level fused Flat search (Index::flat_knn_fused_groups_device /
// Index::fuse_groups_device, k_fuse_groups.hip: the lists of several sub-queries joined into one top-k of GROUPS, the rows that share a
// value of one label column, by reciprocal rank fusion over group ranks, by the smallest distance or by the late-interaction sum): the
// argument check with a code per refusal, the size and the place of the kernel's hash table, its scratch bytes and the sub-chunks of
// fused queries that bound a call's lists.  Host only: no HIP; it builds on fuse_plan.hpp (the limits, the refusal codes 0 .. 12 and the
// table's load are those of the row-level fusion) and tests/cpp/fuse_groups_plan_asan.cpp builds it on its own.
// docs/DESIGN_flat.md 4.1z.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "fuse_plan.hpp"

namespace vdb {

constexpr int FUSE_SUM = 2;                      // VDB_FUSE_SUM: the sum over the lists of the group's nearest distance (late interaction)
constexpr uint32_t FUSEG_LABEL_COLUMNS = 16;     // = LABEL_COLUMNS (kernels.hpp asserts it)
// per slot: a 64-bit key (bit 32 set: an unlabelled row, a group of its own; clear: a label code), accumulator, stamp, representative
// row and its distance (4 B each) and half a u64 sort key
constexpr uint32_t FUSEG_SLOT_BYTES = 28;
// 28 B x 2^12 = 112 KiB is the largest power of two of slots under the 160 KiB of LDS of a gfx950 CU (2^13 would take 224 KiB)
constexpr uint32_t FUSEG_LDS_MAX_LG = 12;
constexpr uint64_t FUSEG_EMPTY = ~0ull;          // the key of a free slot (no key has bits above bit 32)
constexpr uint64_t FUSEG_ROW_TAG = 1ull << 32;   // the key of an unlabelled row: FUSEG_ROW_TAG | LOCAL row

// what fuse_groups_check_args refuses beyond FuseBad, in the order it looks
enum FuseGroupsBad : int {
    FUSEG_BAD_WEIGHTS_WITH_SUM = 13,
    FUSEG_BAD_COLUMN = 14,
};

inline const char *fuse_groups_bad_text(int code) {
    switch (code) {
    case FUSE_BAD_MODE: return "fuse groups: mode must be VDB_FUSE_RRF, VDB_FUSE_MIN or VDB_FUSE_SUM";
    case FUSEG_BAD_WEIGHTS_WITH_SUM: return "fuse groups: weights belong to VDB_FUSE_RRF only (no weighted VDB_FUSE_SUM)";
    case FUSEG_BAD_COLUMN: return "fuse groups: column must be below VDB_LABEL_COLUMNS";
    }
    return fuse_bad_text(code);
}

// FUSE_OK when the arguments describe a call, otherwise the first thing wrong with them: the codes of fuse_check_args in its order
// (FUSE_SUM is a mode here), FUSEG_BAD_WEIGHTS_WITH_SUM where FUSE_BAD_WEIGHTS_WITH_MIN stands, FUSEG_BAD_COLUMN last.
inline int fuse_groups_check_args(int mode, const uint64_t *lims, uint64_t nq, uint64_t k, uint64_t fetch_k, const float *weights, float rrf_c,
                                  uint32_t column, bool list_form = false) {
    if (mode != FUSE_RRF && mode != FUSE_MIN && mode != FUSE_SUM) return FUSE_BAD_MODE;
    const int shape = fuse_check_args(FUSE_RRF, lims, nq, k, fetch_k, nullptr, 0.0f, list_form);  // the limits, the lengths, the entries
    if (shape != FUSE_OK) return shape;
    if (weights) {
        if (mode == FUSE_MIN) return FUSE_BAD_WEIGHTS_WITH_MIN;
        if (mode == FUSE_SUM) return FUSEG_BAD_WEIGHTS_WITH_SUM;
        for (uint64_t j = 0; j < lims[nq]; j++)
            if (!(weights[j] > 0.0f) || !fuse_finite(weights[j])) return FUSE_BAD_WEIGHT;
    }
    if (!(rrf_c >= 0.0f) || !fuse_finite(rrf_c)) return FUSE_BAD_C;
    if (column >= FUSEG_LABEL_COLUMNS) return FUSEG_BAD_COLUMN;
    return FUSE_OK;
}

// The table: 2^lg slots, lg = fuse_table_lg(s_max, ld) -- a list entry opens at most one group, so the load stays at or under one half.
inline bool fuse_groups_in_lds(uint32_t lg) { return lg <= FUSEG_LDS_MAX_LG; }
// bytes of one fused query's table and sort keys, in LDS or in the scratch buffer
inline size_t fuse_groups_table_bytes(uint32_t lg) { return size_t(FUSEG_SLOT_BYTES) << lg; }
// device scratch of a launch over nq fused queries: none while the table lives in LDS
inline size_t fuse_groups_scratch_bytes(uint64_t nq, uint32_t lg) { return fuse_groups_in_lds(lg) ? 0 : size_t(nq) * fuse_groups_table_bytes(lg); }
// where the table starts probing for a key: the low word alone (the tests build colliding labels from it; an unlabelled row and the
// label code of the same number share a probe path and differ in bit 32 of the key)
inline uint32_t fuse_groups_hash(uint32_t key_low, uint32_t lg) { return fuse_hash(key_low, lg); }

// Fused queries per sub-chunk: fuse_sub_chunk with this kernel's table
inline uint64_t fuse_groups_sub_chunk(uint64_t nq, uint64_t s_max, uint64_t kp, bool search = true, uint64_t budget = LIST_BUDGET) {
    if (nq == 0) return 0;
    const uint64_t sm = std::min<uint64_t>(std::max<uint64_t>(s_max, 1), FUSE_MAX_LISTS), kk = std::min<uint64_t>(std::max<uint64_t>(kp, 1), FUSE_MAX_FETCH);
    uint64_t fit = nq;
    if (search) fit = std::min(list_sub_chunk(fit, sm * kk, budget), FUSE_MAX_SUBQ / sm);  // (its floor of 1 is the one below)
    const uint32_t lg = fuse_table_lg(sm, kk);
    if (!fuse_groups_in_lds(lg)) fit = std::min<uint64_t>(fit, budget / fuse_groups_table_bytes(lg));
    return std::max<uint64_t>(1, fit);
}

}  // namespace vdb
