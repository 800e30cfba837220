// Stand-alone check of csrc/fetch_plan.hpp (host only) against a restatement, meant to be built with -fsanitize=address,undefined
// (tests/test_fetch_plan_asan_cpu.py): random (n, R) with n <= 300 -- random lists with repeats, runs, runs with one row disturbed, the
// edge shapes -- under random row and chunk sizes, and the refused lists.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "fetch_plan.hpp"

static int check(uint64_t n, const std::vector<uint64_t> &rows, uint64_t row_bytes, uint64_t chunk_bytes) {
    const uint64_t m = rows.size();
    // (exactly m elements on the heap: a read past the list is the sanitizer's to find)
    if (vdb::fetch_plan_check(n, rows.data(), m, row_bytes)) return 1;
    bool run = m >= 1;
    for (uint64_t j = 0; j < m; j++) run = run && rows[j] == rows[0] + j;
    const uint64_t cr = chunk_bytes / row_bytes ? chunk_bytes / row_bytes : 1;
    const vdb::FetchPlan p = vdb::fetch_plan(rows.data(), m, row_bytes, chunk_bytes);
    if (p.route != (run ? vdb::FETCH_DIRECT : vdb::FETCH_GATHER)) return 2;
    if (p.chunk_rows != cr) return 3;
    if (p.n_chunks != m / cr + (m % cr ? 1 : 0)) return 4;
    const vdb::FetchPlan c = vdb::fetch_plan_chunks(m, row_bytes, chunk_bytes);
    if (c.chunk_rows != p.chunk_rows || c.n_chunks != p.n_chunks || c.route != vdb::FETCH_GATHER) return 5;
    return 0;
}

int main() {
    std::mt19937_64 rng(1806);
    uint64_t cases = 0;
    for (int it = 0; it < 6000; it++) {
        const uint64_t n = 1 + rng() % 300;
        std::vector<uint64_t> rows;
        switch (it % 6) {
        case 0: {  // random, repeats allowed, m may pass n
            const uint64_t m = rng() % (2 * n + 1);
            for (uint64_t j = 0; j < m; j++) rows.push_back(rng() % n);
            break;
        }
        case 1: break;  // nothing
        case 2:         // every row, ascending
            for (uint64_t i = 0; i < n; i++) rows.push_back(i);
            break;
        case 3: rows.push_back(rng() % n); break;  // one row
        case 4: {                                  // a run
            const uint64_t a = rng() % n, len = rng() % (n - a + 1);
            for (uint64_t i = 0; i < len; i++) rows.push_back(a + i);
            break;
        }
        default: {  // a run with one row disturbed: a swap, a duplicate, a gap or a row far away
            const uint64_t a = rng() % n;
            for (uint64_t i = a; i < n; i++) rows.push_back(i);
            if (rows.size() > 1) rows[1 + rng() % (rows.size() - 1)] = rng() % n;
        }
        }
        const uint64_t row_bytes = 1 + rng() % 5000;
        const uint64_t picks[5] = {1, row_bytes, row_bytes + 1, 7 * row_bytes, ~uint64_t(0)};
        const uint64_t chunk_bytes = it % 2 ? picks[rng() % 5] : 1 + rng() % 20000;
        const int e = check(n, rows, row_bytes, chunk_bytes);
        if (e) {
            std::printf("FAILED: code %d at n = %llu, m = %zu\n", e, (unsigned long long)n, rows.size());
            return 1;
        }
        cases++;
    }
    // refused: a row at n, any row of an empty table, a null list with m > 0, a result whose size wraps; accepted: repeats, any order,
    // m > n, m == 0 (with or without a list)
    const uint64_t at_n[] = {1, 8}, rep[] = {2, 5, 2, 2, 0, 7, 7, 7, 1, 1}, zero[] = {0};
    if (!vdb::fetch_plan_check(8, at_n, 2) || !vdb::fetch_plan_check(0, zero, 1) || !vdb::fetch_plan_check(8, nullptr, 1) ||
        !vdb::fetch_plan_check(8, rep, 10, ~uint64_t(0) / 9) || vdb::fetch_plan_check(8, rep, 10, ~uint64_t(0) / 10) ||
        vdb::fetch_plan_check(9, at_n, 2) || vdb::fetch_plan_check(8, rep, 10) || vdb::fetch_plan_check(0, nullptr, 0) ||
        vdb::fetch_plan_check(8, rep, 0)) {
        std::printf("FAILED: list validation\n");
        return 1;
    }
    // sizes at the edge of 64 bits: the chunk count does not wrap
    const vdb::FetchPlan big = vdb::fetch_plan_chunks(~uint64_t(0), 1, 2);
    if (big.chunk_rows != 2 || big.n_chunks != (uint64_t(1) << 63)) {
        std::printf("FAILED: chunk count at 2^64 - 1 rows\n");
        return 1;
    }
    std::printf("fetch_plan ok: %llu cases\n", (unsigned long long)cases);
    return 0;
}
