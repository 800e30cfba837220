// Stand-alone check of csrc/dup_plan.hpp (host only) against a restatement, meant to be built with -fsanitize=address,undefined
// (tests/test_dup_plan_asan_cpu.py): random table sizes, chunk sizes and allowed-row counts around the chunk boundaries, both element
// types, with and without a mask, and every refused argument.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>

#include "dup_plan.hpp"

static int check(uint64_t n, uint64_t dim, bool u8, bool masked, uint64_t m, uint64_t chunk) {
    if (!vdb::dup_check_args(n, m, masked, 0.25f, chunk).empty()) return 1;
    const vdb::DupPlan p = vdb::dup_plan(n, dim, u8, masked, m, chunk);
    const uint64_t calls = m / chunk + (m % chunk ? 1 : 0);
    if (p.m != m || p.n_chunks != calls) return 2;
    if (p.last_len != (m ? m - (calls - 1) * chunk : 0)) return 3;
    if (m && (p.last_len < 1 || p.last_len > chunk)) return 4;
    if (p.gather != (masked || u8)) return 5;
    const uint64_t ql = m < chunk ? m : chunk;
    if (p.chunk_len != ql) return 6;
    if (p.scratch_bytes != 8 * n + 4 * ql + 8 * (ql + 1) + 64 + (p.gather ? ql * dim * 4 : 0)) return 7;
    return 0;
}

int main() {
    std::mt19937_64 rng(1806);
    uint64_t cases = 0;
    const uint64_t chunks[7] = {1, 2, 64, 1024, 4096, 16384, vdb::DUP_CHUNK_MAX};
    for (int it = 0; it < 4000; it++) {
        const uint64_t chunk = it % 5 == 0 ? 1 + rng() % vdb::DUP_CHUNK_MAX : chunks[rng() % 7];
        const uint64_t around[6] = {0, 1, chunk - 1, chunk, chunk + 1, 3 * chunk + rng() % chunk};
        const uint64_t n = it % 7 == 0 ? (1ull << 32) - 1 - rng() % 3 : it % 3 == 0 ? rng() % 2000000 : around[rng() % 6];
        const bool masked = rng() & 1, u8 = rng() & 2;
        const uint64_t m = masked ? (n ? rng() % (n + 1) : 0) : n;
        const int e = check(n, 1 + rng() % 2048, u8, masked, m, chunk);
        if (e) {
            std::printf("FAILED: code %d at n = %llu, m = %llu, chunk = %llu\n", e, (unsigned long long)n, (unsigned long long)m, (unsigned long long)chunk);
            return 1;
        }
        cases++;
    }
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    // refused: a NaN radius, chunk 0 and past the cap, more allowed rows than rows, fewer without a mask, 2^32 rows; accepted: +-inf, < 0
    if (vdb::dup_check_args(10, 10, false, nan, 4).empty() || vdb::dup_check_args(10, 10, false, 0.5f, 0).empty() ||
        vdb::dup_check_args(10, 10, false, 0.5f, vdb::DUP_CHUNK_MAX + 1).empty() || vdb::dup_check_args(10, 11, true, 0.5f, 4).empty() ||
        vdb::dup_check_args(10, 9, false, 0.5f, 4).empty() || vdb::dup_check_args(1ull << 32, 1ull << 32, false, 0.5f, 4).empty() ||
        !vdb::dup_check_args(10, 10, false, inf, 4).empty() || !vdb::dup_check_args(10, 10, false, -inf, 4).empty() ||
        !vdb::dup_check_args(10, 0, true, -1.0f, 4).empty() || !vdb::dup_check_args(0, 0, false, 0.0f, vdb::DUP_CHUNK_MAX).empty() ||
        vdb::dup_check_args(10, 10, false, nan, 4).find("NaN") == std::string::npos) {
        std::printf("FAILED: argument validation\n");
        return 1;
    }
    std::printf("dup_plan ok: %llu cases\n", (unsigned long long)cases);
    return 0;
}
