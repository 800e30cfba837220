// Stand-alone driver of csrc/fuse_plan.hpp (the host arithmetic of the fused multi-query search) for tests/test_fuse_plan_cpu.py: reads cases
// from the file named on the command line, one per line, and prints what the header computes for each; the test compares the output
// with its own restatement.  Built with -fsanitize=address,undefined; no HIP, no other header of the library.
//   C mode list_form nq k fetch_k c has_w lims[nq + 1] (weights[lims[nq]])  -> "C" and the refusal code (0: accepted); accepted: S_max behind it
//   N                                                                       -> "N" and the code of NULL limits
//   T s_max ld                                                              -> "T" lg, in LDS (1 / 0), scratch bytes of 3 fused queries
//   K fetch_k max_m                                                         -> "K" and the list length of the call's round
//   S nq s_max kp search budget                                             -> "S" and the fused queries per sub-chunk
//   H row lg                                                                -> "H" and the slot the probe starts at
// c and the weights come as the hexadecimal bit patterns of f32 values.  The arrays are heap vectors of exactly the sizes above: a read
// past them is AddressSanitizer's to report.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "fuse_plan.hpp"

using namespace vdb;

static float f32_of(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
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
            int mode, list_form, has_w;
            uint64_t nq, k, fetch_k;
            uint32_t cbits;
            ls >> mode >> list_form >> nq >> k >> fetch_k >> std::hex >> cbits >> std::dec >> has_w;
            std::vector<uint64_t> lims(nq + 1);
            for (auto &v : lims) ls >> v;
            std::vector<float> w;
            if (has_w) {
                uint32_t u;
                while (ls >> std::hex >> u) w.push_back(f32_of(u));
            }
            const int code = fuse_check_args(mode, lims.data(), nq, k, fetch_k, has_w ? w.data() : nullptr, f32_of(cbits), list_form != 0);
            std::cout << "C " << code;
            if (code == FUSE_OK) std::cout << ' ' << fuse_s_max(lims.data(), nq);
            if ((code == FUSE_OK) != (fuse_bad_text(code) == nullptr)) return 4;
            std::cout << '\n';
        } else if (op == 'N') {
            std::cout << "N " << fuse_check_args(FUSE_RRF, nullptr, 3, 1, 1, nullptr, 60.0f) << '\n';
        } else if (op == 'T') {
            uint64_t s_max, ld;
            ls >> s_max >> ld;
            const uint32_t lg = fuse_table_lg(s_max, ld);
            std::cout << "T " << lg << ' ' << (fuse_in_lds(lg) ? 1 : 0) << ' ' << fuse_scratch_bytes(3, lg) << '\n';
        } else if (op == 'K') {
            uint64_t f, m;
            ls >> f >> m;
            std::cout << "K " << fuse_list_len(f, m) << '\n';
        } else if (op == 'S') {
            uint64_t nq, s_max, kp, search, budget;
            ls >> nq >> s_max >> kp >> search >> budget;
            std::cout << "S " << fuse_sub_chunk(nq, s_max, kp, search != 0, budget) << '\n';
        } else if (op == 'H') {
            uint64_t row, lg;
            ls >> row >> lg;
            std::cout << "H " << fuse_hash((uint32_t)row, (uint32_t)lg) << '\n';
        } else if (op) {
            return 3;
        }
    }
    std::cout << "fuse_plan ok\n";
    return 0;
}
