// lookup_plan.hpp -- the host part of the key lookup over ONE label column (Index::label_lookup / k_label_lookup: for each code of a
// list the number of rows that carry it and the lowest such row, from one read of the column): checks the code list of
// vdb_index_label_lookup and decides how a lane resolves its row's code to a position of the list.  Host only: no HIP and no other
// header of the library but mask_partition.hpp, which is host only too (tests/cpp/lookup_plan_asan.cpp builds it on its own).
// docs/DESIGN_flat.md 4.1aa.
//
// The code rules are mask_partition.hpp's: DISTINCT codes in any order, arbitrarily sparse, PART_LABEL_NONE (the rows without a value)
// among them.  Two routes:
//   LOOKUP_SORTED  any codes, in chunks of PART_MAX_CHUNK: the chunk's sorted table in LDS, binary search (mask_partition_layout /
//                  mask_partition_find), counts and firsts in LDS; one read of the column per chunk.
//   LOOKUP_DIRECT  many codes of a dense dictionary: a table slot_of[code - base] of `span` u32 in device scratch (LOOKUP_NO_SLOT where
//                  the list has no such code), one gather per row; ONE read of the column whatever n_codes is.  PART_LABEL_NONE never
//                  enters the table -- base and span are taken over the other codes, and its slot travels by value.  Taken when
//                  n_codes > PART_MAX_CHUNK and 4 B x span <= table_bytes (a cap on scratch memory; 0: never).
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "mask_partition.hpp"

namespace vdb {

constexpr int LOOKUP_SORTED = 0, LOOKUP_DIRECT = 1;
constexpr uint32_t LOOKUP_NO_SLOT = 0xFFFFFFFFu;                 // slot_of: the list does not hold this code
constexpr uint32_t LOOKUP_ROW_NONE32 = 0xFFFFFFFFu;              // the device's "no row yet" (an index has fewer than 2^32 rows)
constexpr uint64_t LOOKUP_ROW_NONE = ~uint64_t(0);               // = VDB_ROW_NONE
constexpr uint64_t LOOKUP_TABLE_BYTES_DEFAULT = 64ull << 20;     // "label_lookup_table_bytes"
constexpr uint64_t LOOKUP_TABLE_BYTES_MAX = 4ull << 30;          // what vdb_set_param accepts

struct LookupPlan {
    int route = LOOKUP_SORTED;
    uint32_t base = 0;       // the lowest code other than PART_LABEL_NONE (0 when there is none)
    uint64_t span = 0;       // highest - lowest + 1 over those codes (0 when there is none): at most 2^32 - 1
    uint64_t chunks = 0;     // reads of the column: ceil(n_codes / PART_MAX_CHUNK) sorted, 1 direct, 0 without codes
    uint64_t none_at = ~uint64_t(0);  // the position of PART_LABEL_NONE in the list; ~0: not named
};

// base, span and the position of PART_LABEL_NONE; reads codes[0 .. n_codes)
inline LookupPlan label_lookup_extent(const uint32_t *codes, uint64_t n_codes) {
    LookupPlan p;
    uint32_t lo = 0xFFFFFFFFu, hi = 0;
    bool any = false;
    for (uint64_t j = 0; j < n_codes; j++) {
        const uint32_t c = codes[j];
        if (c == PART_LABEL_NONE) {
            p.none_at = j;
            continue;
        }
        lo = std::min(lo, c);
        hi = std::max(hi, c);
        any = true;
    }
    if (any) {
        p.base = lo;
        p.span = uint64_t(hi) - lo + 1;
    }
    return p;
}

// mask_partition_check's rules and wording.  A dense list is tested for a duplicate with a bitmap over its span, in O(n_codes), before
// the sort that names the code: the ingestion case hands over a million distinct codes, and sorting them costs more than the lookup.
inline std::string label_lookup_check(uint32_t column, const uint32_t *codes, uint64_t n_codes) {
    if (column >= PART_LABEL_COLUMNS || n_codes == 0 || n_codes >= (1ull << 28) || !codes) return mask_partition_check(column, codes, n_codes);
    const LookupPlan e = label_lookup_extent(codes, n_codes);
    if (e.span <= 64 * n_codes) {
        std::vector<uint64_t> seen((e.span + 63) / 64, 0);
        bool none = false, dup = false;
        for (uint64_t j = 0; j < n_codes && !dup; j++) {
            const uint32_t c = codes[j];
            if (c == PART_LABEL_NONE) {
                dup = none;
                none = true;
                continue;
            }
            const uint64_t off = uint64_t(c) - e.base;
            dup = (seen[off >> 6] >> (off & 63)) & 1;
            seen[off >> 6] |= 1ull << (off & 63);
        }
        if (!dup) return "";
    }
    return mask_partition_check(column, codes, n_codes);
}

// the plan of a CHECKED list
inline LookupPlan label_lookup_plan(const uint32_t *codes, uint64_t n_codes, uint64_t table_bytes) {
    LookupPlan p = label_lookup_extent(codes, n_codes);
    const bool direct = n_codes > PART_MAX_CHUNK && p.span >= 1 && p.span <= table_bytes / sizeof(uint32_t);
    p.route = direct ? LOOKUP_DIRECT : LOOKUP_SORTED;
    p.chunks = n_codes == 0 ? 0 : direct ? 1 : mask_partition_chunks(n_codes, PART_MAX_CHUNK);
    return p;
}

}  // namespace vdb
