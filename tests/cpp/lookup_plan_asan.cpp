// Stand-alone check of csrc/lookup_plan.hpp (host only) against a restatement, meant to be built with -fsanitize=address,undefined
// (tests/test_lookup_plan_asan_cpu.py): random code lists -- dense, sparse, with and without LABEL_NONE, shuffled -- around the chunk
// size and the table cap, the edge shapes, and every refused list.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <set>
#include <vector>

#include "lookup_plan.hpp"

static int check(const std::vector<uint32_t> &codes, uint64_t table_bytes) {
    const uint64_t m = codes.size();
    // (exactly m elements on the heap: a read past the list is the sanitizer's to find)
    if (!vdb::label_lookup_check(3, codes.data(), m).empty()) return 1;
    uint64_t lo = ~uint64_t(0), hi = 0, none_at = ~uint64_t(0);
    for (uint64_t j = 0; j < m; j++) {
        if (codes[j] == vdb::PART_LABEL_NONE) {
            none_at = j;
            continue;
        }
        lo = std::min<uint64_t>(lo, codes[j]);
        hi = std::max<uint64_t>(hi, codes[j]);
    }
    const bool any = lo != ~uint64_t(0);
    const uint64_t span = any ? hi - lo + 1 : 0;
    const bool direct = m > 1024 && any && span * 4 <= table_bytes;
    const vdb::LookupPlan p = vdb::label_lookup_plan(codes.data(), m, table_bytes);
    if (p.route != (direct ? vdb::LOOKUP_DIRECT : vdb::LOOKUP_SORTED)) return 2;
    if (p.base != (any ? lo : 0) || p.span != span) return 3;
    if (p.chunks != (m == 0 ? 0 : direct ? 1 : (m + 1023) / 1024)) return 4;
    if (p.none_at != none_at) return 5;
    return 0;
}

int main() {
    std::mt19937_64 rng(1806);
    uint64_t cases = 0;
    for (int it = 0; it < 600; it++) {
        const uint64_t picks[8] = {0, 1, 2, 1023, 1024, 1025, 2049, 1 + rng() % 4000};
        const uint64_t m = picks[rng() % 8];
        std::set<uint32_t> s;
        const uint32_t base = it % 3 == 0 ? 0 : (uint32_t)(rng() % 0xFFFF0000ull);
        const uint64_t width = it % 2 ? m + rng() % (m + 2) : (uint64_t(1) << (8 + rng() % 24));  // dense, or spread over up to 2^31
        while (s.size() < m) {
            s.insert((uint32_t)((base + rng() % std::max<uint64_t>(width, m)) % 0xFFFFFFFFull));  // (never LABEL_NONE)
        }
        std::vector<uint32_t> codes(s.begin(), s.end());
        if (it % 4 == 1 && !codes.empty()) codes[rng() % codes.size()] = vdb::PART_LABEL_NONE;
        std::shuffle(codes.begin(), codes.end(), rng);
        const uint64_t span_bytes = 4 * (codes.empty() ? 1 : uint64_t(*std::max_element(s.begin(), s.end())) - *s.begin() + 1);
        const uint64_t caps[6] = {0, span_bytes - 1, span_bytes, span_bytes + 1, 64ull << 20, ~uint64_t(0)};
        const int e = check(codes, caps[rng() % 6]);
        if (e) {
            std::printf("FAILED: code %d at m = %zu\n", e, codes.size());
            return 1;
        }
        cases++;
    }
    // the edges: LABEL_NONE alone; 0 and 0xFFFFFFFE together (4 B x span passes 32 bits) alone and in a long list
    std::vector<uint32_t> wide = {0, 0xFFFFFFFEu};
    if (check({vdb::PART_LABEL_NONE}, 64ull << 20) || check(wide, 64ull << 20)) {
        std::printf("FAILED: edge lists\n");
        return 1;
    }
    for (uint32_t c = 1; c < 1100; c++) wide.push_back(c);
    const vdb::LookupPlan pw = vdb::label_lookup_plan(wide.data(), wide.size(), 0xFFFFFFFFull);
    if (check(wide, 64ull << 20) || check(wide, 0xFFFFFFFFull) || check(wide, 1ull << 34) || pw.route != vdb::LOOKUP_SORTED || pw.span != 0xFFFFFFFFull) {
        std::printf("FAILED: a span whose bytes pass 32 bits\n");
        return 1;
    }
    // refused: a column at 16, a duplicate (dense list, sparse list, LABEL_NONE twice), a null list with codes, 2^28 codes; accepted:
    // no codes with or without a list
    std::vector<uint32_t> dense(2000), sparse = {5, 1u << 31, 9, 1u << 31}, none2 = {vdb::PART_LABEL_NONE, 1, vdb::PART_LABEL_NONE};
    for (uint32_t i = 0; i < 2000; i++) dense[i] = i;
    dense[1999] = 3;
    if (vdb::label_lookup_check(16, wide.data(), 2).empty() || vdb::label_lookup_check(0, dense.data(), dense.size()).empty() ||
        vdb::label_lookup_check(0, sparse.data(), sparse.size()).empty() || vdb::label_lookup_check(0, none2.data(), none2.size()).empty() ||
        vdb::label_lookup_check(0, nullptr, 3).empty() || vdb::label_lookup_check(0, wide.data(), 1ull << 28).empty() ||
        !vdb::label_lookup_check(15, nullptr, 0).empty() || !vdb::label_lookup_check(0, wide.data(), 0).empty() ||
        vdb::label_lookup_check(0, dense.data(), dense.size()).find(" 3 ") == std::string::npos) {
        std::printf("FAILED: list validation\n");
        return 1;
    }
    std::printf("lookup_plan ok: %llu cases\n", (unsigned long long)cases);
    return 0;
}
