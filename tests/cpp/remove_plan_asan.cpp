// Stand-alone check of csrc/remove_plan.hpp (host only) against the naive replay of swap_remove in descending order, meant to be built
// with -fsanitize=address,undefined (tests/test_remove_plan_asan_cpu.py): random (n, R) with n <= 300, the edge shapes included.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "remove_plan.hpp"

static int check(uint64_t n, const std::vector<uint64_t> &rows) {
    const uint64_t m = rows.size(), n1 = n - m;
    if (vdb::remove_plan_check(n, rows.data(), m)) return 1;
    std::vector<uint64_t> naive(n), fast(n), dst, src;
    for (uint64_t i = 0; i < n; i++) naive[i] = fast[i] = i;
    for (uint64_t j = m; j-- > 0;) {  // VecSet::swap_remove, descending
        naive[rows[j]] = naive.back();
        naive.pop_back();
    }
    vdb::remove_plan(n, rows.data(), m, dst, src);
    if (dst.size() != src.size() || dst.size() != vdb::remove_plan_count(n, rows.data(), m)) return 2;
    uint64_t below = 0;
    for (uint64_t r : rows) below += r < n1;
    if (dst.size() != below) return 3;
    for (size_t j = 0; j < dst.size(); j++) {
        if (!(src[j] >= n1 && src[j] < n && dst[j] < n1)) return 4;
        if (std::binary_search(rows.begin(), rows.end(), src[j])) return 5;
        if (j && dst[j] >= dst[j - 1]) return 6;
        fast[dst[j]] = src[j];  // (sources are never destinations: the original value of fast[src] is still there)
    }
    fast.resize(n1);
    return fast == naive ? 0 : 7;
}

int main() {
    std::mt19937_64 rng(1806);
    uint64_t cases = 0;
    auto run = [&](uint64_t n, std::vector<uint64_t> rows) {
        std::sort(rows.begin(), rows.end());
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
        case 0: rows.assign(all.begin(), all.begin() + m); break;              // random
        case 1: break;                                                         // nothing
        case 2: rows = all; break;                                             // everything
        case 3: for (uint64_t i = n - m / 2; i < n; i++) rows.push_back(i); break;  // the end of the table (inside the tail)
        case 4: {                                                              // all below n'
            const uint64_t mm = std::min(m, n / 2);
            for (uint64_t i = 0; i < mm; i++) rows.push_back(i * ((n - mm) / std::max<uint64_t>(mm, 1)));
            std::sort(rows.begin(), rows.end());
            rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
            while (!rows.empty() && rows.back() >= n - rows.size()) rows.pop_back();
            break;
        }
        default: {                                                             // one contiguous block
            const uint64_t a = n ? rng() % n : 0, len = n ? rng() % (n - a + 1) : 0;
            for (uint64_t i = a; i < a + len; i++) rows.push_back(i);
        }
        }
        run(n, rows);
    }
    // refused lists
    const uint64_t unsorted[] = {3, 1}, dup[] = {2, 2}, far[] = {1, 9};
    if (!vdb::remove_plan_check(8, unsorted, 2) || !vdb::remove_plan_check(8, dup, 2) || !vdb::remove_plan_check(9, far, 2) ||
        vdb::remove_plan_check(10, far, 2)) {
        std::printf("FAILED: list validation\n");
        return 1;
    }
    std::printf("remove_plan ok: %llu cases\n", (unsigned long long)cases);
    return 0;
}
