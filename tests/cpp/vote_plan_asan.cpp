// Stand-alone check of csrc/vote_plan.hpp (the host arithmetic of the k-NN label vote) for tests/test_vote_plan_cpu.py: every refusal in
// its order, the table capacities at hand-written list lengths, the LDS / scratch boundary, the sub-chunks and the hash.  Built with
// -fsanitize=address,undefined; no HIP, no other header of the library but list_plan.hpp.
#include <cmath>
#include <cstdio>
#include <limits>

#include "vote_plan.hpp"

using namespace vdb;

#define CHECK(x)                                                 \
    do {                                                         \
        if (!(x)) {                                              \
            std::printf("vote_plan FAILED line %d: %s\n", __LINE__, #x); \
            return 1;                                            \
        }                                                        \
    } while (0)

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
    CHECK(vote_check_args(10, 1, VOTE_UNIFORM, 0.0f, 0) == VOTE_OK);  // eps plays no part in UNIFORM
    CHECK(vote_check_args(4096, 4096, VOTE_INVERSE, 1e-6f, 15) == VOTE_OK);
    CHECK(vote_check_args(0, 1, VOTE_UNIFORM, 1.0f, 0) == VOTE_BAD_K);
    CHECK(vote_check_args(4097, 1, 7, 0.0f, 99) == VOTE_BAD_K);  // the first thing wrong
    CHECK(vote_check_args(10, 0, VOTE_UNIFORM, 1.0f, 0) == VOTE_BAD_C);
    CHECK(vote_check_args(10, 11, 7, 1.0f, 0) == VOTE_BAD_C);
    CHECK(vote_check_args(10, 10, 2, 1.0f, 0) == VOTE_BAD_MODE);
    CHECK(vote_check_args(10, 10, -1, 1.0f, 0) == VOTE_BAD_MODE);
    CHECK(vote_check_args(10, 1, VOTE_INVERSE, 0.0f, 0) == VOTE_BAD_EPS);
    CHECK(vote_check_args(10, 1, VOTE_INVERSE, -1.0f, 0) == VOTE_BAD_EPS);
    CHECK(vote_check_args(10, 1, VOTE_INVERSE, inf, 0) == VOTE_BAD_EPS);
    CHECK(vote_check_args(10, 1, VOTE_INVERSE, nan, 16) == VOTE_BAD_EPS);
    CHECK(vote_check_args(10, 1, VOTE_UNIFORM, nan, 16) == VOTE_BAD_COLUMN);
    for (int code = 0; code <= 6; code++) CHECK((vote_bad_text(code) == nullptr) == (code == VOTE_OK));

    CHECK(vote_table_lg(0) == 7 && vote_table_lg(1) == 7 && vote_table_lg(64) == 7 && vote_table_lg(65) == 8);
    CHECK(vote_table_lg(1024) == 11 && vote_table_lg(1025) == 12 && vote_table_lg(4096) == 13 && vote_table_lg(~0ull) == 13);
    CHECK(vote_in_lds(11) && !vote_in_lds(12));
    CHECK(vote_table_bytes(7) == 2560 && vote_table_bytes(11) == 40960 && vote_table_bytes(13) == 163840);
    CHECK(vote_scratch_bytes(1000, 11) == 0 && vote_scratch_bytes(3, 12) == 3 * 81920 && vote_scratch_bytes(0, 13) == 0);
    CHECK(vote_hash(0, 7) == 0 && vote_hash(1, 7) == (2654435761u >> 25) && vote_hash(0xFFFFFFFEu, 13) < (1u << 13));
    for (uint32_t lg = 7; lg <= 13; lg++) CHECK(vote_hash(12345, lg) == vote_hash(12345, 13) >> (13 - lg));  // a prefix of one hash

    CHECK(vote_sub_chunk(0, 10) == 0);
    CHECK(vote_sub_chunk(1000, 10) == 1000);                        // everything fits
    CHECK(vote_sub_chunk(1000, 10, true, 1200) == 10);              // lists: 120 B a query
    CHECK(vote_sub_chunk(1000, 10, true, 1) == 1);                  // never 0
    CHECK(vote_sub_chunk(1000, 4096, true, 1u << 20) == 6);         // 1 MiB / 160 KiB of scratch = 6 < 1 MiB / 48 KiB of lists = 21
    CHECK(vote_sub_chunk(1000, 4096, false, 1u << 20) == 6);
    CHECK(vote_sub_chunk(1000, 1024, false, 1) == 1000);            // the list form in LDS: no budget applies
    CHECK(vote_sub_chunk(~0ull, ~0ull) >= 1);
    std::printf("vote_plan ok\n");
    return 0;
}
