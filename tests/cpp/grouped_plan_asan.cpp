// Stand-alone driver of csrc/grouped_plan.hpp (the host arithmetic of the grouped Flat k-NN) for tests/test_grouped_plan_cpu.py: reads
// cases from the file named on the command line, one per line, and prints what the header computes for each; the test compares the
// output with its own restatement.  Built with -fsanitize=address,undefined; no HIP, no other header of the library.
//   K k oversample m            -> "K" and the list length of every round until it reaches m (at most 64 rounds)
//   S nq kp budget              -> "S" and the queries per sub-chunk
//   T k ld                      -> "T" and log2 of the table capacity
//   H label lg                  -> "H" and the first probe position
//   C kp n  m_0 d_0 .. m_n-1 d_n-1   (the active queries are 0, 2, 4, ..: query 2 i has m_i allowed rows and done byte d_i)
//                               -> "C" exhausted, longest open set, the open queries
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "grouped_plan.hpp"

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
        if (op == 'K') {
            uint64_t k, ov, m;
            ls >> k >> ov >> m;
            uint64_t kp = grouped_first_k(k, ov, m);
            std::cout << "K " << kp;
            for (int r = 0; r < 64 && !grouped_exhausts(kp, m); r++) {
                kp = grouped_next_k(kp, m);
                std::cout << ' ' << kp;
            }
            std::cout << '\n';
        } else if (op == 'S') {
            uint64_t nq, kp, budget;
            ls >> nq >> kp >> budget;
            std::cout << "S " << grouped_sub_chunk(nq, kp, budget) << '\n';
        } else if (op == 'T') {
            uint64_t k, ld;
            ls >> k >> ld;
            std::cout << "T " << grouped_table_lg(k, ld) << '\n';
        } else if (op == 'H') {
            uint64_t label, lg;
            ls >> label >> lg;
            std::cout << "H " << grouped_hash((uint32_t)label, (uint32_t)lg) << '\n';
        } else if (op == 'C') {
            uint64_t kp, n;
            ls >> kp >> n;
            std::vector<uint64_t> active(n), m_of(2 * n + 1, 0), next{99, 98};  // (next starts dirty: the call clears it)
            std::vector<uint8_t> done(n);
            for (uint64_t i = 0; i < n; i++) {
                uint64_t m, d;
                ls >> m >> d;
                active[i] = 2 * i;
                m_of[2 * i] = m;
                done[i] = (uint8_t)d;
            }
            uint64_t exhausted = 0;
            const uint64_t open_m = grouped_compact(active, done.data(), m_of.data(), kp, next, exhausted);
            std::cout << "C " << exhausted << ' ' << open_m;
            for (uint64_t q : next) std::cout << ' ' << q;
            std::cout << '\n';
        } else if (op) {
            return 3;
        }
    }
    std::cout << "grouped_plan ok\n";
    return 0;
}
