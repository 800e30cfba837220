// Stand-alone driver of csrc/mmr_plan.hpp (the host arithmetic of the diversified Flat k-NN) for tests/test_mmr_plan_cpu.py: reads cases
// from the file named on the command line, one per line, and prints what the header computes for each; the test compares the output
// with its own restatement.  Built with -fsanitize=address,undefined; no HIP, no other header of the library.
//   A k fetch_k lambda_bits     -> "A" and 0 (accepted) or 1 (lambda), 2 (fetch_k < k), 3 (fetch_k too large): the first check that fails
//   L ld dim                    -> "L" threads, positions, staged floats, LDS bytes
//   S nq kp budget              -> "S" and the queries per sub-chunk
//   F fetch_k max_m             -> "F" and the list length of the call's round
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "mmr_plan.hpp"

using namespace vdb;

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    if (!in) return 2;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        char op = 0;
        ls >> op;
        if (op == 'A') {
            uint64_t k, fk;
            uint32_t bits;
            ls >> k >> fk >> bits;
            float lambda;
            std::memcpy(&lambda, &bits, sizeof(lambda));
            const char *bad = mmr_check_args(k, fk, lambda);
            int code = 0;
            if (bad) code = std::strstr(bad, "lambda") ? 1 : std::strstr(bad, "at least k") ? 2 : 3;
            std::cout << "A " << code << '\n';
        } else if (op == 'L') {
            uint64_t ld, dim;
            ls >> ld >> dim;
            std::cout << "L " << mmr_threads(ld) << ' ' << mmr_positions(ld) << ' ' << mmr_stage_floats(dim) << ' ' << mmr_lds_bytes(ld, dim) << '\n';
        } else if (op == 'S') {
            uint64_t nq, kp, budget;
            ls >> nq >> kp >> budget;
            std::cout << "S " << mmr_sub_chunk(nq, kp, budget) << '\n';
        } else if (op == 'F') {
            uint64_t fk, m;
            ls >> fk >> m;
            std::cout << "F " << mmr_list_len(fk, m) << '\n';
        } else if (op) {
            return 3;
        }
    }
    std::cout << "mmr_plan ok\n";
    return 0;
}
