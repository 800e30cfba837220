// Stand-alone check of csrc/labels_scatter_plan.hpp (host only, with update_plan.hpp's row check behind it) against a restatement,
// meant to be built with -fsanitize=address,undefined (tests/test_labels_scatter_plan_asan_cpu.py): random (n, rows, columns) with
// n <= 300 -- valid lists, lists with one row or one column disturbed -- and the refused argument shapes.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <set>
#include <vector>

#include "labels_scatter_plan.hpp"

// the restatement: is the call valid?
static bool valid(uint64_t n, const std::vector<uint64_t> &rows, const std::vector<uint32_t> &cols) {
    if (cols.size() > 16 || (cols.empty() && !rows.empty())) return false;
    std::set<uint32_t> cs(cols.begin(), cols.end());
    if (cs.size() != cols.size()) return false;
    for (uint32_t c : cols)
        if (c >= 16) return false;
    std::set<uint64_t> rs(rows.begin(), rows.end());
    if (rs.size() != rows.size()) return false;
    for (uint64_t r : rows)
        if (r >= n) return false;
    return true;
}

int main() {
    std::mt19937_64 rng(1806);
    uint64_t cases = 0, refused = 0;
    for (int it = 0; it < 6000; it++) {
        const uint64_t n = 1 + rng() % 300;
        // (exactly m / n_cols elements on the heap: a read past a list is the sanitizer's to find)
        std::vector<uint64_t> all(n), rows;
        for (uint64_t i = 0; i < n; i++) all[i] = i;
        std::shuffle(all.begin(), all.end(), rng);
        rows.assign(all.begin(), all.begin() + rng() % (n + 1));
        std::vector<uint32_t> perm(16), cols;
        for (uint32_t c = 0; c < 16; c++) perm[c] = c;
        std::shuffle(perm.begin(), perm.end(), rng);
        cols.assign(perm.begin(), perm.begin() + 1 + rng() % 16);
        switch (it % 6) {
        case 1:  // a duplicate row
            if (rows.size() > 1) rows[rng() % rows.size()] = rows[rng() % rows.size()];
            break;
        case 2:  // a row at or past n
            if (!rows.empty()) rows[rng() % rows.size()] = n + rng() % 3;
            break;
        case 3:  // a column out of range, or named twice
            cols[rng() % cols.size()] = rng() % 2 ? 16 + uint32_t(rng() % 3) : cols[rng() % cols.size()];
            break;
        case 4:  // too many columns, or none
            if (rng() % 2)
                cols.assign(17, 0);
            else
                cols.clear();
            break;
        default: break;  // valid as drawn
        }
        const uint64_t m = rows.size();
        const bool want = valid(n, rows, cols);
        const char *why = vdb::labels_scatter_check(n, rows.data(), m, cols.data(), cols.size());
        if ((why == nullptr) != want) {
            std::printf("FAILED: check says %s, want %d at n = %llu, m = %llu, n_cols = %zu\n", why ? why : "ok", int(want), (unsigned long long)n,
                        (unsigned long long)m, cols.size());
            return 1;
        }
        if (want) {
            std::vector<uint32_t> ids(m);
            vdb::labels_scatter_ids(rows.data(), m, ids.data());
            for (uint64_t j = 0; j < m; j++)
                if (ids[j] != rows[j]) {
                    std::printf("FAILED: id %llu\n", (unsigned long long)j);
                    return 1;
                }
        } else {
            refused++;
        }
        cases++;
    }
    // the row check has two routes (a bitmap over the table, a sort of the list): short lists over a large table take the sort
    const uint64_t big = uint64_t(1) << 20, dup[] = {5, 7, 5}, far[] = {big - 1, 0, 77}, past[] = {5, big};
    const uint32_t col3[] = {3};
    if (!vdb::labels_scatter_check(big, dup, 3, col3, 1) || vdb::labels_scatter_check(big, far, 3, col3, 1) ||
        !vdb::labels_scatter_check(big, past, 2, col3, 1) || !vdb::labels_scatter_check(2, dup, 3, col3, 1)) {
        std::printf("FAILED: the sort route of the row check\n");
        return 1;
    }
    const uint64_t two[] = {1, 2};
    const uint32_t col0[] = {0};
    if (!vdb::labels_scatter_check(8, nullptr, 2, col0, 1) || !vdb::labels_scatter_check(8, two, 2, nullptr, 1) ||
        !vdb::labels_scatter_check(8, two, 2, nullptr, 0) || !vdb::labels_scatter_check(0, two, 1, col0, 1) ||
        vdb::labels_scatter_check(8, nullptr, 0, nullptr, 0) || vdb::labels_scatter_check(0, nullptr, 0, col0, 1) ||
        vdb::labels_scatter_check(8, two, 2, col0, 1) || !vdb::update_plan_check(8, nullptr, 2) || vdb::update_plan_check(8, two, 2)) {
        std::printf("FAILED: argument validation\n");
        return 1;
    }
    // labels_scatter_ids is the narrowing of every host id list: nothing (no read, no write), one id, the largest id a shard can hold
    // (exactly m elements on the heap on both sides: a step past either list is the sanitizer's to find)
    for (uint64_t m : {uint64_t(0), uint64_t(1), uint64_t(3)}) {
        std::vector<uint64_t> rows(m);
        for (uint64_t j = 0; j < m; j++) rows[j] = j ? 0xFFFFFFFFull - (j - 1) : 7;  // 7, 2^32 - 1, 2^32 - 2
        std::vector<uint32_t> ids(m, 77u);
        vdb::labels_scatter_ids(rows.data(), m, ids.data());
        for (uint64_t j = 0; j < m; j++)
            if (uint64_t(ids[j]) != rows[j]) {
                std::printf("FAILED: labels_scatter_ids at m = %llu, j = %llu\n", (unsigned long long)m, (unsigned long long)j);
                return 1;
            }
    }
    vdb::labels_scatter_ids(nullptr, 0, nullptr);
    std::printf("labels_scatter_plan ok: %llu cases, %llu refused\n", (unsigned long long)cases, (unsigned long long)refused);
    return 0;
}
