// multi_plan.hpp -- the work list of a filtered k-NN call that carries one row mask per query (Index::flat_knn_masked_multi_device).
// Host only: no HIP, no other header of the library (tests/cpp/multi_plan_asan.cpp builds it on its own).
//
// The queries of the call are bucketed by their mask.  The buckets of the GROUPED masks (short allow-lists, see vdbhip.h) are laid out
// bucket after bucket -- masks ascending, the queries of a bucket in call order -- as SLOTS; the slot sequence is cut into chunks of at
// most `qch` slots, and a chunk is what one launch of k_scan_gather_grouped, one selection pass and one finalize serve:
//  - slot s of a chunk owns row s of the chunk's dense matrix, whose leading dimension `ld` is the largest m among the masks the chunk
//    holds, rounded up to 64 (`max_m` itself is what the selection scans);
//  - one work item = (mask g, up to MULTI_BQ consecutive slots of g's bucket inside the chunk, one tile of MULTI_TILE allowed rows);
//  - the items of one (mask, tile) are adjacent -- the query groups that read the same 256 rows run next to each other and find them
//    in L2 -- and a mask with m == 0 has slots (its queries are finalized to count 0) but no items.
// qch keeps the dense matrix (ld_all * 4 bytes per slot, ld_all = the call's largest grouped m rounded up to 64) and the selection's
// lists (`list_bytes` per slot, the caller's figure for that m) inside `budget` each; it is a multiple of 8, at least 8, at most 32768.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace vdb {

constexpr uint32_t MULTI_BQ = 8;      // queries per work item
constexpr uint32_t MULTI_TILE = 256;  // allowed rows per work item

struct MultiItem {
    uint32_t mask;  // index into the call's mask array
    uint32_t tile;  // allowed rows [tile * MULTI_TILE, min(m, (tile + 1) * MULTI_TILE))
    uint32_t slot;  // first slot, relative to the chunk
    uint32_t nb;    // 1..MULTI_BQ slots
};

struct MultiChunk {
    uint64_t slot0 = 0, nslots = 0;  // slots [slot0, slot0 + nslots) of the plan
    uint64_t item0 = 0, nitems = 0;  // items [item0, item0 + nitems)
    uint64_t max_m = 0, ld = 0;      // largest m among the chunk's masks; that rounded up to 64
    uint64_t rows = 0;               // sum over the items of their tile's rows (what the scan fetches)
};

struct MultiPlan {
    uint64_t qch = 0;                  // slots per chunk
    std::vector<uint32_t> slot_query;  // slot -> query of the call
    std::vector<uint32_t> slot_mask;   // slot -> its mask
    std::vector<MultiItem> items;
    std::vector<MultiChunk> chunks;
};

// the largest m among the grouped masks that at least one query uses (0: none)
inline uint64_t multi_plan_max_m(const uint64_t *m_of, const uint8_t *grouped, uint64_t n_masks, const uint32_t *mask_of, uint64_t nq) {
    uint64_t mx = 0;
    for (uint64_t q = 0; q < nq; q++)
        if (mask_of[q] < n_masks && grouped[mask_of[q]]) mx = std::max(mx, m_of[mask_of[q]]);
    return mx;
}

inline uint64_t multi_plan_chunk(uint64_t budget, uint64_t max_m, uint64_t list_bytes) {
    const uint64_t ld = (max_m + 63) & ~63ull;
    auto chunk_of = [&](uint64_t row_bytes) { return std::max<uint64_t>(8, std::min<uint64_t>(budget / std::max<uint64_t>(row_bytes, 1), 32768) & ~7ull); };
    return std::min(chunk_of(ld * sizeof(float)), chunk_of(list_bytes));
}

// m_of[g] = allowed rows of mask g (< 2^32), grouped[g] != 0: mask g takes the grouped path; mask_of[q] < n_masks for every q (checked
// by the caller); nq < 2^32.  Queries of the other masks get no slot.
inline void multi_plan(const uint64_t *m_of, const uint8_t *grouped, uint64_t n_masks, const uint32_t *mask_of, uint64_t nq, uint64_t budget,
                       uint64_t list_bytes, MultiPlan &out) {
    out = MultiPlan{};
    // counting sort of the grouped queries by mask: stable, so a bucket keeps the call's order
    std::vector<uint64_t> start(n_masks + 1, 0);
    for (uint64_t q = 0; q < nq; q++)
        if (grouped[mask_of[q]]) start[mask_of[q] + 1]++;
    for (uint64_t g = 0; g < n_masks; g++) start[g + 1] += start[g];
    const uint64_t ns = start[n_masks];
    out.slot_query.resize(ns);
    out.slot_mask.resize(ns);
    {
        std::vector<uint64_t> at(start.begin(), start.end() - 1);
        for (uint64_t q = 0; q < nq; q++) {
            const uint32_t g = mask_of[q];
            if (!grouped[g]) continue;
            out.slot_query[at[g]] = (uint32_t)q;
            out.slot_mask[at[g]] = g;
            at[g]++;
        }
    }
    out.qch = multi_plan_chunk(budget, multi_plan_max_m(m_of, grouped, n_masks, mask_of, nq), list_bytes);
    for (uint64_t s0 = 0; s0 < ns; s0 += out.qch) {
        MultiChunk c;
        c.slot0 = s0;
        c.nslots = std::min(out.qch, ns - s0);
        c.item0 = out.items.size();
        // the runs of equal mask inside the chunk
        for (uint64_t a = s0; a < s0 + c.nslots;) {
            const uint32_t g = out.slot_mask[a];
            uint64_t b = a;
            while (b < s0 + c.nslots && out.slot_mask[b] == g) b++;
            const uint64_t m = m_of[g];
            c.max_m = std::max(c.max_m, m);
            for (uint64_t t = 0; t * MULTI_TILE < m; t++) {
                const uint64_t rows = std::min<uint64_t>(MULTI_TILE, m - t * MULTI_TILE);
                for (uint64_t s = a; s < b; s += MULTI_BQ) {
                    out.items.push_back({g, (uint32_t)t, (uint32_t)(s - s0), (uint32_t)std::min<uint64_t>(MULTI_BQ, b - s)});
                    c.rows += rows;
                }
            }
            a = b;
        }
        c.ld = (c.max_m + 63) & ~63ull;
        c.nitems = out.items.size() - c.item0;
        out.chunks.push_back(c);
    }
}

}  // namespace vdb
