// multi_plan_asan.cpp -- csrc/multi_plan.hpp against a brute-force restatement of what the plan promises, built with
// -fsanitize=address,undefined by tests/test_multi_plan_cpu.py and run as a program of its own.
//   every (grouped query, allowed row of its mask) pair is covered by exactly one work item; a query of another mask by none;
//   the slots are a permutation of the grouped queries, a bucket in call order; a slot's mask is its query's;
//   no item holds more than 8 slots or reaches past its mask's rows; the items of one (mask, tile) are adjacent;
//   a chunk's ld is its largest m rounded up to 64, and its dense matrix and lists stay inside the budget (or it is the 8-slot minimum).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <utility>
#include <vector>

#include "multi_plan.hpp"

using namespace vdb;

static uint64_t rng_state = 0x1806;
static uint64_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return rng_state >> 33;
}

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

static void check_case(const std::vector<uint64_t> &m_of, const std::vector<uint8_t> &grouped, const std::vector<uint32_t> &mask_of, uint64_t budget,
                       uint64_t list_bytes) {
    const uint64_t n_masks = m_of.size(), nq = mask_of.size();
    MultiPlan p;
    multi_plan(m_of.data(), grouped.data(), n_masks, mask_of.data(), nq, budget, list_bytes, p);
    // slots: a permutation of the grouped queries, buckets ascending by mask, call order inside a bucket
    uint64_t n_grouped = 0;
    for (uint64_t q = 0; q < nq; q++) n_grouped += grouped[mask_of[q]] ? 1 : 0;
    CHECK(p.slot_query.size() == n_grouped && p.slot_mask.size() == n_grouped);
    std::set<uint32_t> seen;
    for (uint64_t s = 0; s < n_grouped; s++) {
        const uint32_t q = p.slot_query[s];
        CHECK(q < nq && grouped[mask_of[q]] && p.slot_mask[s] == mask_of[q]);
        CHECK(seen.insert(q).second);
        if (s) {
            CHECK(p.slot_mask[s - 1] <= p.slot_mask[s]);
            if (p.slot_mask[s - 1] == p.slot_mask[s]) CHECK(p.slot_query[s - 1] < q);
        }
    }
    // chunks tile the slots and the items
    CHECK(p.qch >= 8 && p.qch % 8 == 0 && p.qch <= 32768);
    uint64_t max_m_all = 0;
    for (uint64_t q = 0; q < nq; q++)
        if (grouped[mask_of[q]]) max_m_all = std::max(max_m_all, m_of[mask_of[q]]);
    const uint64_t ld_all = (max_m_all + 63) & ~63ull;
    CHECK(p.qch == 8 || (p.qch * ld_all * 4 <= budget && p.qch * list_bytes <= budget));
    uint64_t s_next = 0, i_next = 0;
    std::map<std::pair<uint32_t, uint64_t>, uint32_t> cover;  // (query, column of its mask) -> times covered
    for (const MultiChunk &c : p.chunks) {
        CHECK(c.slot0 == s_next && c.item0 == i_next && c.nslots >= 1 && c.nslots <= p.qch);
        s_next += c.nslots;
        i_next += c.nitems;
        uint64_t mx = 0, rows = 0;
        for (uint64_t s = c.slot0; s < c.slot0 + c.nslots; s++) mx = std::max(mx, m_of[p.slot_mask[s]]);
        CHECK(c.max_m == mx && c.ld == ((mx + 63) & ~63ull) && c.ld <= ld_all);
        std::set<std::pair<uint32_t, uint32_t>> closed;  // (mask, tile) runs already left
        for (uint64_t i = c.item0; i < c.item0 + c.nitems; i++) {
            const MultiItem &it = p.items[i];
            CHECK(it.mask < n_masks && grouped[it.mask]);
            CHECK(it.nb >= 1 && it.nb <= MULTI_BQ && uint64_t(it.slot) + it.nb <= c.nslots);
            const uint64_t m = m_of[it.mask], j0 = uint64_t(it.tile) * MULTI_TILE;
            CHECK(j0 < m);
            const uint64_t j1 = std::min<uint64_t>(m, j0 + MULTI_TILE);
            CHECK(j1 - j0 <= MULTI_TILE && j1 <= c.ld);
            rows += j1 - j0;
            if (i > c.item0) {
                const MultiItem &pr = p.items[i - 1];
                if (pr.mask != it.mask || pr.tile != it.tile) CHECK(closed.insert({pr.mask, pr.tile}).second);
            }
            CHECK(!closed.count({it.mask, it.tile}));
            for (uint32_t b = 0; b < it.nb; b++) {
                const uint64_t s = c.slot0 + it.slot + b;
                CHECK(p.slot_mask[s] == it.mask);
                for (uint64_t j = j0; j < j1; j++) cover[{p.slot_query[s], j}]++;
            }
        }
        CHECK(rows == c.rows);
    }
    CHECK(s_next == n_grouped && i_next == p.items.size());
    uint64_t want = 0;
    for (uint64_t q = 0; q < nq; q++) {
        if (!grouped[mask_of[q]]) continue;
        for (uint64_t j = 0; j < m_of[mask_of[q]]; j++) {
            auto f = cover.find({(uint32_t)q, j});
            CHECK(f != cover.end() && f->second == 1);
        }
        want += m_of[mask_of[q]];
    }
    CHECK(cover.size() == want);
}

int main() {
    const uint64_t BUDGET = 256ull << 20;
    // the boundaries by hand: m = 0, 1, 255, 256, 257, 512, 513; buckets of 1, 7, 8, 9, 15, 16, 17; a mask no query uses; a mask on the other route
    {
        std::vector<uint64_t> m_of = {0, 1, 255, 256, 257, 512, 513, 700, 3000, 100};
        std::vector<uint8_t> grouped = {1, 1, 1, 1, 1, 1, 1, 1, 0, 1};  // mask 8 takes the other route, mask 9 has no query
        const uint32_t sizes[9] = {3, 1, 7, 8, 9, 15, 16, 17, 5};
        std::vector<uint32_t> mask_of;
        for (uint32_t round = 0; round < 17; round++)  // interleaved, not sorted
            for (uint32_t g = 0; g < 9; g++)
                if (round < sizes[g]) mask_of.push_back(g);
        check_case(m_of, grouped, mask_of, BUDGET, 8192);
        check_case(m_of, grouped, mask_of, 8 * 768 * 4, 64);     // a tiny budget: the 8-slot minimum, buckets cut by chunk ends
        check_case(m_of, grouped, mask_of, 24 * 768 * 4, 512 * 8);  // 24 slots by the matrix, fewer by the lists
        check_case(m_of, grouped, {}, BUDGET, 64);               // no query
        check_case({}, {}, {}, BUDGET, 64);                      // no mask
        check_case({0, 0}, {1, 1}, {1, 0, 1}, BUDGET, 64);       // nothing allowed anywhere
        check_case({5}, {0}, {0, 0, 0}, BUDGET, 64);             // nothing grouped
    }
    for (int rep = 0; rep < 300; rep++) {
        const uint64_t n_masks = 1 + rnd() % 12, nq = rnd() % 120;
        std::vector<uint64_t> m_of(n_masks);
        std::vector<uint8_t> grouped(n_masks);
        for (uint64_t g = 0; g < n_masks; g++) {
            const uint64_t kind = rnd() % 6;
            m_of[g] = kind == 0 ? 0 : kind == 1 ? 256 * (1 + rnd() % 3) + (rnd() % 3) - 1 : rnd() % 900;
            grouped[g] = rnd() % 5 != 0;
        }
        std::vector<uint32_t> mask_of(nq);
        for (auto &g : mask_of) g = (uint32_t)(rnd() % n_masks);
        const uint64_t budget = rep % 3 == 0 ? BUDGET : 4096 * (1 + rnd() % 64);
        check_case(m_of, grouped, mask_of, budget, 64 * 8 * (1 + rnd() % 16));
    }
    std::printf("multi_plan ok\n");
    return 0;
}
