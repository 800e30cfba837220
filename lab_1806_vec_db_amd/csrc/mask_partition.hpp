// mask_partition.hpp -- the host part of the single-pass grouping of ONE label column by code (Index::masks_partition /
// k_mask_partition: the masks of many values of the column in one read of it; Index::label_counts / k_label_counts: the number of rows
// per value): checks the code list of vdb_mask_create_partition / vdb_index_label_counts, cuts it into chunks and lays out, per chunk,
// the sorted codes the device searches and the permutation back to the caller's order.  Host only: no HIP and no other header of the
// library (tests/cpp/mask_partition_asan.cpp builds it on its own).  docs/DESIGN_flat.md 4.1p.
//
// The codes of a call are DISTINCT -- that is what makes the masks of a call disjoint, so that a row belongs to at most one of them and
// the allow-lists of a chunk hold at most n entries together -- in any order, arbitrarily sparse, PART_LABEL_NONE (the rows without a
// value) among them.  Chunk c holds the codes [c * chunk, min((c + 1) * chunk, n_codes)) of the caller's list, at most PART_MAX_CHUNK
// of them (the device keeps a chunk's table in LDS); within a chunk `sorted` is ascending and slot[i] is the position, inside the chunk,
// of sorted[i] in the caller's order.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <string>
#include <vector>

namespace vdb {

constexpr uint32_t PART_LABEL_COLUMNS = 16;         // = LABEL_COLUMNS (kernels.hpp asserts it)
constexpr uint32_t PART_LABEL_NONE = 0xFFFFFFFFu;   // = LABEL_NONE
constexpr uint32_t PART_MAX_CHUNK = 1024;           // codes per kernel launch: 2 x 4 KiB of LDS
constexpr uint32_t PART_NO_SLOT = 0xFFFFFFFFu;      // mask_partition_find: the value is not in the table

// Checks everything both calls state about (column, codes, n_codes).  Empty string: fine; otherwise the message.  n_codes is tested
// before codes is read; a duplicate is found by sorting a copy, wherever its two positions are.
inline std::string mask_partition_check(uint32_t column, const uint32_t *codes, uint64_t n_codes) {
    if (column >= PART_LABEL_COLUMNS)
        return "label partition: column " + std::to_string(column) + ", an index has " + std::to_string(PART_LABEL_COLUMNS);
    if (n_codes == 0) return "";
    if (n_codes >= (1ull << 28)) return "too many codes for one call";
    if (!codes) return "null argument";
    std::vector<uint32_t> s(codes, codes + n_codes);
    std::sort(s.begin(), s.end());
    const auto dup = std::adjacent_find(s.begin(), s.end());
    if (dup != s.end()) return "label partition: code " + std::to_string(*dup) + " is named twice (the codes of a call are distinct)";
    return "";
}

// number of chunks of `chunk` (1 .. PART_MAX_CHUNK) codes that n_codes codes make
inline uint64_t mask_partition_chunks(uint64_t n_codes, uint64_t chunk) { return chunk ? (n_codes + chunk - 1) / chunk : 0; }

// The table of the nb (<= PART_MAX_CHUNK) codes codes[0 .. nb) of one chunk: sorted ascending, slot[i] = the index in [0, nb) that
// sorted[i] has in `codes`.
inline void mask_partition_layout(const uint32_t *codes, uint32_t nb, std::vector<uint32_t> &sorted, std::vector<uint32_t> &slot) {
    slot.resize(nb);
    std::iota(slot.begin(), slot.end(), 0u);
    std::sort(slot.begin(), slot.end(), [&](uint32_t a, uint32_t b) { return codes[a] < codes[b]; });
    sorted.resize(nb);
    for (uint32_t i = 0; i < nb; i++) sorted[i] = codes[slot[i]];
}

// The position of v in sorted[0 .. nb), PART_NO_SLOT when it is not there: the binary search a lane of k_mask_partition /
// k_label_counts runs over the table in LDS, statement for statement (the CPU test checks this one by brute force).  At most 11 steps
// for nb <= 1024; every probe lies in [0, nb).
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t mask_partition_find(const uint32_t *sorted, uint32_t nb, uint32_t v) {
    uint32_t lo = 0, hi = nb;  // the first position whose code is >= v lies in [lo, hi]
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (sorted[mid] < v)
            lo = mid + 1;
        else
            hi = mid;
    }
    return (lo < nb && sorted[lo] == v) ? lo : PART_NO_SLOT;
}

}  // namespace vdb
