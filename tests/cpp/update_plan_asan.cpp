// Stand-alone check of csrc/update_plan.hpp (host only) against a std::set of rows / 16, meant to be built with
// -fsanitize=address,undefined (tests/test_update_plan_asan_cpu.py): random (n, R) with n <= 300 in shuffled order, the edge shapes included.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "update_plan.hpp"

static int check(uint64_t n, const std::vector<uint64_t> &rows) {
    const uint64_t m = rows.size();
    if (vdb::update_plan_check(n, rows.data(), m)) return 1;
    std::set<uint32_t> want;
    for (uint64_t r : rows) want.insert(uint32_t(r / 16));
    std::vector<uint32_t> tiles(3, 77u);  // (stale contents must not survive)
    vdb::update_plan(n, rows.data(), m, tiles);
    if (tiles.size() != want.size()) return 2;
    if (!std::equal(tiles.begin(), tiles.end(), want.begin())) return 3;  // ascending and distinct, like the set
    for (uint32_t t : tiles)
        if (uint64_t(t) * 16 >= n) return 4;
    return 0;
}

int main() {
    std::mt19937_64 rng(1806);
    uint64_t cases = 0;
    auto run = [&](uint64_t n, std::vector<uint64_t> rows) {
        std::shuffle(rows.begin(), rows.end(), rng);  // order is free
        const int e = check(n, rows);
        if (e) {
            std::printf("FAILED: code %d at n = %llu, m = %zu\n", e, (unsigned long long)n, rows.size());
            std::exit(1);
        }
        cases++;
    };
    for (int it = 0; it < 4000; it++) {
        const uint64_t n = rng() % 301;
        std::vector<uint64_t> all(n), rows;
        for (uint64_t i = 0; i < n; i++) all[i] = i;
        std::shuffle(all.begin(), all.end(), rng);
        const uint64_t m = n ? rng() % (n + 1) : 0;
        switch (it % 6) {
        case 0: rows.assign(all.begin(), all.begin() + m); break;  // random
        case 1: break;                                             // nothing
        case 2: rows = all; break;                                 // everything
        case 3: if (n) rows.push_back(rng() % n); break;           // one row
        case 4:                                                    // the rows around every tile boundary
            for (uint64_t r : std::initializer_list<uint64_t>{15, 16, 17, 31, 32, 33})
                if (r < n) rows.push_back(r);
            break;
        default: {                                                 // one contiguous block, the ragged last tile included
            const uint64_t a = n ? rng() % n : 0;
            for (uint64_t i = a; i < n; i++) rows.push_back(i);
        }
        }
        run(n, rows);
    }
    // refused lists: a duplicate (adjacent or not), a row at n, null rows with m > 0, more ids than rows; accepted: any order, m == 0
    const uint64_t dup[] = {2, 5, 2}, adj[] = {4, 4}, far[] = {9, 1}, ok[] = {7, 0, 3};
    if (!vdb::update_plan_check(8, dup, 3) || !vdb::update_plan_check(8, adj, 2) || !vdb::update_plan_check(9, far, 2) ||
        !vdb::update_plan_check(8, nullptr, 1) || !vdb::update_plan_check(2, dup, 3) || vdb::update_plan_check(10, far, 2) ||
        vdb::update_plan_check(8, ok, 3) || vdb::update_plan_check(0, nullptr, 0) || vdb::update_plan_check(8, ok, 0)) {
        std::printf("FAILED: list validation\n");
        return 1;
    }
    std::printf("update_plan ok: %llu cases\n", (unsigned long long)cases);
    return 0;
}
