// Stand-alone driver of csrc/like_plan.hpp (the host arithmetic of the search by example rows) for tests/test_like_plan_cpu.py: reads cases
// from the file named on the command line, one per line, and prints what the header computes for each; the test compares the output
// with its own restatement.  Built with -fsanitize=address,undefined; no HIP, no other header of the library.
//   C nq has_neg pos_lims[nq + 1] (neg_lims[nq + 1])  -> "C" and 0 (accepted) or 1 (start), 2 (descent), 3 (no positive), 4 (too many): the
//                                                        first check that fails; accepted: e_max behind it
//   D nq lims[nq + 1]                                 -> "D" and 0 / 1 / 2 / 4 for the list form's limits
//   N                                                 -> "N" and the code of NULL positive limits
//   K k e_max exclude max_m                           -> "K" and the list length of the call's round
//   S nq kp budget                                    -> "S" and the queries per sub-chunk
// The limit arrays are heap vectors of exactly nq + 1 entries: a read past them is AddressSanitizer's to report.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "like_plan.hpp"

using namespace vdb;

static int code_of(const char *bad) {
    if (!bad) return 0;
    if (std::strstr(bad, "start at 0")) return 1;
    if (std::strstr(bad, "not decrease")) return 2;
    if (std::strstr(bad, "at least one positive")) return 3;
    if (std::strstr(bad, "at most 1024")) return 4;
    return 5;  // (null limits)
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    if (!in) return 2;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        char op = 0;
        ls >> op;
        if (op == 'C') {
            uint64_t nq;
            int has_neg;
            ls >> nq >> has_neg;
            std::vector<uint64_t> pl(nq + 1), nl(has_neg ? nq + 1 : 0);
            for (auto &v : pl) ls >> v;
            for (auto &v : nl) ls >> v;
            const uint64_t *np = has_neg ? nl.data() : nullptr;
            const int code = code_of(like_check_lims(pl.data(), np, nq));
            std::cout << "C " << code;
            if (code == 0) std::cout << ' ' << like_e_max(pl.data(), np, nq);
            std::cout << '\n';
        } else if (op == 'D') {
            uint64_t nq;
            ls >> nq;
            std::vector<uint64_t> dl(nq + 1);
            for (auto &v : dl) ls >> v;
            std::cout << "D " << code_of(like_check_drop_lims(dl.data(), nq)) << '\n';
        } else if (op == 'N') {
            std::cout << "N " << code_of(like_check_lims(nullptr, nullptr, 3)) << '\n';
        } else if (op == 'K') {
            uint64_t k, e, ex, m;
            ls >> k >> e >> ex >> m;
            std::cout << "K " << like_list_len(k, e, ex != 0, m) << '\n';
        } else if (op == 'S') {
            uint64_t nq, kp, budget;
            ls >> nq >> kp >> budget;
            std::cout << "S " << like_sub_chunk(nq, kp, budget) << '\n';
        } else if (op) {
            return 3;
        }
    }
    std::cout << "like_plan ok\n";
    return 0;
}
