// Stand-alone check of csrc/mask_partition.hpp (host only), meant to be built with -fsanitize=address,undefined
// (tests/test_mask_partition_plan_cpu.py): the argument check of vdb_mask_create_partition / vdb_index_label_counts -- duplicates at
// adjacent and at distant positions, LABEL_NONE in the list, the column and count limits, a null array -- the sorted table and its
// permutation for 0, 1, 1024, 1025 and 2049 codes cut into chunks, and mask_partition_find (the host twin of the device's binary search)
// against a linear search for present, absent, smallest and largest codes.  Every array is a heap vector of exactly the documented
// length, so a read past it is an ASan report.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "mask_partition.hpp"

static const uint32_t NONE = vdb::PART_LABEL_NONE;

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

static bool has(const std::string &s, const char *what) { return s.find(what) != std::string::npos; }

// n distinct codes in a shuffled order: sparse values, 0, 0xFFFFFFFE and LABEL_NONE among them when n allows
static std::vector<uint32_t> distinct_codes(uint64_t n, std::mt19937 &rng) {
    std::set<uint32_t> seen;
    const uint32_t fixed[] = {NONE, 0u, 0xFFFFFFFEu, 1u << 31, 7u};
    for (uint32_t f : fixed)
        if (seen.size() < n) seen.insert(f);
    while (seen.size() < n) seen.insert((uint32_t)rng());
    std::vector<uint32_t> v(seen.begin(), seen.end());
    std::shuffle(v.begin(), v.end(), rng);
    return v;
}

static uint32_t linear_find(const std::vector<uint32_t> &sorted, uint32_t v) {
    for (uint32_t i = 0; i < sorted.size(); i++)
        if (sorted[i] == v) return i;
    return vdb::PART_NO_SLOT;
}

static void check_chunks(uint64_t n, uint64_t chunk, std::mt19937 &rng) {
    const std::vector<uint32_t> codes = distinct_codes(n, rng);
    CHECK(vdb::mask_partition_check(3, codes.data(), n).empty());
    const uint64_t nchunks = vdb::mask_partition_chunks(n, chunk);
    CHECK(nchunks == (n + chunk - 1) / chunk);
    std::vector<uint8_t> covered(n, 0);
    for (uint64_t c = 0; c < nchunks; c++) {
        const uint64_t g0 = c * chunk;
        const uint32_t nb = (uint32_t)std::min<uint64_t>(chunk, n - g0);
        CHECK(nb >= 1 && nb <= vdb::PART_MAX_CHUNK);
        const std::vector<uint32_t> piece(codes.begin() + g0, codes.begin() + g0 + nb);  // (exactly nb entries: a read past them is reported)
        std::vector<uint32_t> sorted, slot;
        vdb::mask_partition_layout(piece.data(), nb, sorted, slot);
        CHECK(sorted.size() == nb && slot.size() == nb);
        std::vector<uint8_t> used(nb, 0);
        for (uint32_t i = 0; i < nb; i++) {
            CHECK(i == 0 || sorted[i - 1] < sorted[i]);          // ascending, strictly
            CHECK(slot[i] < nb && !used[slot[i]]);               // a permutation
            used[slot[i]] = 1;
            CHECK(piece[slot[i]] == sorted[i]);                  // back to the caller's order
            covered[g0 + slot[i]] += 1;
        }
        // the lookup: every present code, the smallest and the largest, and absent ones below, between and above
        for (uint32_t i = 0; i < nb; i++) CHECK(vdb::mask_partition_find(sorted.data(), nb, sorted[i]) == i);
        CHECK(vdb::mask_partition_find(sorted.data(), nb, sorted.front()) == 0);
        CHECK(vdb::mask_partition_find(sorted.data(), nb, sorted.back()) == nb - 1);
        const uint32_t probes[] = {0u, 1u, 6u, 7u, 8u, (1u << 31) - 1, 1u << 31, (1u << 31) + 1, 0xFFFFFFFDu, 0xFFFFFFFEu, NONE};
        for (uint32_t v : probes) CHECK(vdb::mask_partition_find(sorted.data(), nb, v) == linear_find(sorted, v));
        for (int t = 0; t < 2000; t++) {
            const uint32_t v = (t & 1) ? (uint32_t)rng() : sorted[rng() % nb] + (uint32_t)(rng() % 3) - 1;
            CHECK(vdb::mask_partition_find(sorted.data(), nb, v) == linear_find(sorted, v));
        }
    }
    for (uint64_t j = 0; j < n; j++) CHECK(covered[j] == 1);  // every input position is the slot of exactly one table entry
}

int main() {
    std::mt19937 rng(1806);
    // ---- the argument check
    CHECK(vdb::mask_partition_check(0, nullptr, 0).empty());   // no codes: nothing is read
    CHECK(vdb::mask_partition_check(15, nullptr, 0).empty());
    CHECK(has(vdb::mask_partition_check(16, nullptr, 0), "column 16"));
    CHECK(has(vdb::mask_partition_check(0xFFFFFFFFu, nullptr, 0), "column"));
    CHECK(has(vdb::mask_partition_check(0, nullptr, 5), "null argument"));
    CHECK(has(vdb::mask_partition_check(0, nullptr, 1ull << 28), "too many codes"));  // (tested before the array is looked at)
    CHECK(has(vdb::mask_partition_check(0, nullptr, ~0ull), "too many codes"));
    {
        const std::vector<uint32_t> one{42};
        CHECK(vdb::mask_partition_check(0, one.data(), 1).empty());
        const std::vector<uint32_t> none{NONE};
        CHECK(vdb::mask_partition_check(0, none.data(), 1).empty());
        const std::vector<uint32_t> ok{5, NONE, 0, 0xFFFFFFFEu, 1u << 31};
        CHECK(vdb::mask_partition_check(2, ok.data(), ok.size()).empty());
        const std::vector<uint32_t> adjacent{1, 9, 9, 3};
        CHECK(has(vdb::mask_partition_check(0, adjacent.data(), adjacent.size()), "code 9 is named twice"));
        const std::vector<uint32_t> two_none{NONE, 4, NONE};
        CHECK(has(vdb::mask_partition_check(0, two_none.data(), two_none.size()), "named twice"));
        std::vector<uint32_t> distant = distinct_codes(3000, rng);  // the two positions lie in different chunks
        distant[2999] = distant[0];
        CHECK(has(vdb::mask_partition_check(0, distant.data(), distant.size()), "named twice"));
        distant[2999] = distant[1500];
        CHECK(has(vdb::mask_partition_check(0, distant.data(), distant.size()), "named twice"));
        CHECK(has(vdb::mask_partition_check(16, adjacent.data(), adjacent.size()), "column 16"));  // (the column is judged first)
    }
    // ---- chunks, tables, lookups
    CHECK(vdb::mask_partition_chunks(0, 1024) == 0);
    {
        std::vector<uint32_t> sorted{1}, slot{1};
        vdb::mask_partition_layout(nullptr, 0, sorted, slot);  // an empty chunk reads nothing
        CHECK(sorted.empty() && slot.empty());
        CHECK(vdb::mask_partition_find(nullptr, 0, 5) == vdb::PART_NO_SLOT);
    }
    for (uint64_t n : {1ull, 2ull, 1024ull, 1025ull, 2049ull}) check_chunks(n, vdb::PART_MAX_CHUNK, rng);
    for (uint64_t chunk : {1ull, 7ull, 42ull}) check_chunks(100, chunk, rng);  // (a large index narrows the chunk)
    std::printf("mask_partition ok\n");
    return 0;
}
