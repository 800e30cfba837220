// rescore_plan.hpp -- the host arithmetic of the exact late-interaction rescoring of candidate documents (Index::rescore_groups_device,
// flat_rescore.hip, k_rescore.hip; docs/DESIGN_flat.md 4.1ak): the argument check with a code per refusal, the layout of a call -- the
// entry list of a question padded to whole tiles of 64 candidate rows, the table of per-(group slot, sub-query) minima -- and the
// sub-chunks of questions that keep both under a scratch budget.  Host only: no HIP; it builds on fuse_plan.hpp (the limits of a fused
// query and the mode codes are those of the fused searches).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "fuse_groups_plan.hpp"

namespace vdb {

constexpr uint64_t RESCORE_TILE = 64;          // candidate rows of one work item of k_rescore_pairs: a row per lane
constexpr uint64_t RESCORE_MAX_LD = 4096;      // candidates of one question (the sort of k_rescore_finish lives in LDS)
constexpr uint64_t RESCORE_ENTRY_BYTES = 8;    // an entry: (group slot << 32) | LOCAL row
constexpr uint64_t RESCORE_MIN_BYTES = 8;      // a minimum: (order key of the distance << 32) | LOCAL row
constexpr uint64_t RESCORE_ENTRY_PAD = ~0ull;  // the entry of a padding lane (no row: n < 2^32)

// what rescore_check_args refuses, in the order it looks
enum RescoreBad : int {
    RESCORE_OK = 0,
    RESCORE_BAD_MODE = 1,
    RESCORE_BAD_COLUMN = 2,
    RESCORE_BAD_LIMS_NULL = 3,
    RESCORE_BAD_LIMS_START = 4,
    RESCORE_BAD_LIMS_DESCEND = 5,
    RESCORE_BAD_NO_LIST = 6,
    RESCORE_BAD_TOO_MANY_LISTS = 7,
    RESCORE_BAD_LD = 8,
    RESCORE_BAD_K = 9,
    RESCORE_BAD_COUNT = 10,
};

inline const char *rescore_bad_text(int code) {
    switch (code) {
    case RESCORE_OK: return nullptr;
    case RESCORE_BAD_MODE: return "rescore groups: mode must be VDB_FUSE_SUM or VDB_FUSE_MIN";
    case RESCORE_BAD_COLUMN: return "rescore groups: column must be below VDB_LABEL_COLUMNS";
    case RESCORE_BAD_LIMS_NULL: return "rescore groups: null sub-query limits";
    case RESCORE_BAD_LIMS_START: return "rescore groups: sub-query limits must start at 0";
    case RESCORE_BAD_LIMS_DESCEND: return "rescore groups: sub-query limits must not decrease";
    case RESCORE_BAD_NO_LIST: return "rescore groups: every question needs at least one sub-query";
    case RESCORE_BAD_TOO_MANY_LISTS: return "rescore groups: at most 32 sub-queries per question";
    case RESCORE_BAD_LD: return "rescore groups: ld (the candidates of a question) must be at most 4096";
    case RESCORE_BAD_K: return "rescore groups: k must be at most ld";
    case RESCORE_BAD_COUNT: return "rescore groups: a cand_count is above ld";
    }
    return "rescore groups: bad argument";
}

// RESCORE_OK when the arguments describe a call, otherwise the first thing wrong with them.  lims [nq + 1] (nq == 0: lims[0] is still
// read); cand_count [nq] or nullptr (the device form checks its counts after reading them back).
inline int rescore_check_args(int mode, const uint64_t *lims, uint64_t nq, uint64_t k, uint64_t ld, uint32_t column, const uint64_t *cand_count) {
    if (mode != FUSE_SUM && mode != FUSE_MIN) return RESCORE_BAD_MODE;
    if (column >= FUSEG_LABEL_COLUMNS) return RESCORE_BAD_COLUMN;
    if (!lims) return RESCORE_BAD_LIMS_NULL;
    if (lims[0] != 0) return RESCORE_BAD_LIMS_START;
    for (uint64_t q = 0; q < nq; q++)
        if (lims[q + 1] < lims[q]) return RESCORE_BAD_LIMS_DESCEND;
    for (uint64_t q = 0; q < nq; q++) {
        const uint64_t s = lims[q + 1] - lims[q];
        if (s == 0) return RESCORE_BAD_NO_LIST;
        if (s > FUSE_MAX_LISTS) return RESCORE_BAD_TOO_MANY_LISTS;
    }
    if (ld > RESCORE_MAX_LD) return RESCORE_BAD_LD;
    if (k > ld) return RESCORE_BAD_K;
    if (cand_count)
        for (uint64_t q = 0; q < nq; q++)
            if (cand_count[q] > ld) return RESCORE_BAD_COUNT;
    return RESCORE_OK;
}

// tiles of one question whose candidate groups hold `rows` rows together
// (constexpr: k_rescore_prepare pads with it)
constexpr uint64_t rescore_tiles(uint64_t rows) { return (rows + RESCORE_TILE - 1) / RESCORE_TILE; }
// scratch of one question: its padded entry list and its [slots][s] minima
inline uint64_t rescore_question_bytes(uint64_t rows, uint64_t slots, uint64_t s) {
    return rescore_tiles(rows) * RESCORE_TILE * RESCORE_ENTRY_BYTES + slots * s * RESCORE_MIN_BYTES;
}

struct RescoreLayout {
    uint64_t tiles = 0;          // work items of k_rescore_pairs over the whole call
    uint64_t sub_chunk = 0;      // questions per sub-chunk: as many as keep the largest question's scratch x sub_chunk under the budget
    uint64_t scratch_bytes = 0;  // entries + minima of the largest sub-chunk
};

// rows [nq]: the rows of the candidate groups of each question; slots [nq]: its distinct candidate groups (nullptr: `ld` each, the
// most a question can have).  budget 0: LIST_BUDGET.  At least one question per sub-chunk, whatever the budget.
inline RescoreLayout rescore_layout(const uint64_t *lims, uint64_t nq, const uint64_t *rows, const uint64_t *slots, uint64_t ld, uint64_t budget = 0) {
    RescoreLayout l;
    if (nq == 0) return l;
    const uint64_t bud = budget ? budget : LIST_BUDGET;
    uint64_t worst = 0;
    for (uint64_t q = 0; q < nq; q++) {
        l.tiles += rescore_tiles(rows[q]);
        worst = std::max(worst, rescore_question_bytes(rows[q], slots ? slots[q] : ld, lims[q + 1] - lims[q]));
    }
    l.sub_chunk = worst ? std::min<uint64_t>(nq, std::max<uint64_t>(1, bud / worst)) : nq;
    for (uint64_t c0 = 0; c0 < nq; c0 += l.sub_chunk) {
        uint64_t bytes = 0;
        for (uint64_t q = c0; q < std::min(nq, c0 + l.sub_chunk); q++)
            bytes += rescore_question_bytes(rows[q], slots ? slots[q] : ld, lims[q + 1] - lims[q]);
        l.scratch_bytes = std::max(l.scratch_bytes, bytes);
    }
    return l;
}

// the open-addressing table of the wanted label codes of a call with `slots` candidate groups in all: 2^lg entries, load at most 1/2
inline uint32_t rescore_table_lg(uint64_t slots) {
    uint32_t lg = 6;
    while ((1ull << lg) < 2 * slots) lg++;
    return lg;
}
// the LDS table that dedupes the candidates of ONE question (at most ld <= 4096 of them): 12 B per entry, 96 KiB at most
inline uint32_t rescore_dedupe_lg(uint64_t ld) { return rescore_table_lg(std::min(ld, RESCORE_MAX_LD)); }

}  // namespace vdb
