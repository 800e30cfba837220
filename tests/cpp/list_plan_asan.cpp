// Stand-alone driver of csrc/list_plan.hpp (the host arithmetic the Flat list re-rankers share) for tests/test_list_plan_cpu.py: reads cases
// from the file named on the command line, one per line, and prints what the header computes for each; the test compares the output
// with its own restatement.  Built with -fsanitize=address,undefined; no HIP, no other header of the library.
//   S rows kp budget            -> "S" and the lists per sub-chunk
//   L want max_m                -> "L" and the list length of a round
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "list_plan.hpp"

using namespace vdb;

static_assert(LIST_BUDGET == 268435456ull && LIST_PAIR_BYTES == 12, "the budget and the bytes of a pair the tests restate");

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    if (!in) return 2;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        char op = 0;
        ls >> op;
        if (op == 'S') {
            uint64_t rows, kp, budget;
            ls >> rows >> kp >> budget;
            std::cout << "S " << list_sub_chunk(rows, kp, budget) << '\n';
        } else if (op == 'L') {
            uint64_t want, m;
            ls >> want >> m;
            std::cout << "L " << list_len(want, m) << '\n';
        } else if (op) {
            return 3;
        }
    }
    std::cout << "list_plan ok\n";
    return 0;
}
