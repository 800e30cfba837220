// Stand-alone driver of csrc/fuse_groups_plan.hpp (the host arithmetic of the document-level fused search) for
// tests/test_fuse_groups_plan_cpu.py: reads cases from the file named on the command line, one per line, and prints what the header
// computes for each; the test compares the output with its own restatement.  Built with -fsanitize=address,undefined; no HIP, only the
// plan header (which builds on fuse_plan.hpp).
//   C mode list_form nq k fetch_k c column has_w lims[nq + 1] (weights[lims[nq]])  -> "C" and the refusal code (0: accepted); accepted: S_max behind it
//   N                                                                              -> "N" and the code of NULL limits
//   T s_max ld                                                                     -> "T" lg, in LDS (1 / 0), scratch bytes of 3 fused queries, table bytes
//   S nq s_max kp search budget                                                    -> "S" and the fused queries per sub-chunk
//   H key_low lg                                                                   -> "H" and the slot the probe starts at
// c and the weights come as the hexadecimal bit patterns of f32 values.  The arrays are heap vectors of exactly the sizes above: a read
// past them is AddressSanitizer's to report.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "fuse_groups_plan.hpp"

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
            uint64_t nq, k, fetch_k, column;
            uint32_t cbits;
            ls >> mode >> list_form >> nq >> k >> fetch_k >> std::hex >> cbits >> std::dec >> column >> has_w;
            std::vector<uint64_t> lims(nq + 1);
            for (auto &v : lims) ls >> v;
            std::vector<float> w;
            if (has_w) {
                uint32_t u;
                while (ls >> std::hex >> u) w.push_back(f32_of(u));
            }
            const int code = fuse_groups_check_args(mode, lims.data(), nq, k, fetch_k, has_w ? w.data() : nullptr, f32_of(cbits), (uint32_t)column,
                                                    list_form != 0);
            std::cout << "C " << code;
            if (code == FUSE_OK) std::cout << ' ' << fuse_s_max(lims.data(), nq);
            if ((code == FUSE_OK) != (fuse_groups_bad_text(code) == nullptr)) return 4;
            std::cout << '\n';
        } else if (op == 'N') {
            std::cout << "N " << fuse_groups_check_args(FUSE_SUM, nullptr, 3, 1, 1, nullptr, 60.0f, 0) << '\n';
        } else if (op == 'T') {
            uint64_t s_max, ld;
            ls >> s_max >> ld;
            const uint32_t lg = fuse_table_lg(s_max, ld);
            std::cout << "T " << lg << ' ' << (fuse_groups_in_lds(lg) ? 1 : 0) << ' ' << fuse_groups_scratch_bytes(3, lg) << ' '
                      << fuse_groups_table_bytes(lg) << '\n';
        } else if (op == 'S') {
            uint64_t nq, s_max, kp, search, budget;
            ls >> nq >> s_max >> kp >> search >> budget;
            std::cout << "S " << fuse_groups_sub_chunk(nq, s_max, kp, search != 0, budget) << '\n';
        } else if (op == 'H') {
            uint64_t key, lg;
            ls >> key >> lg;
            std::cout << "H " << fuse_groups_hash((uint32_t)key, (uint32_t)lg) << '\n';
        } else if (op) {
            return 3;
        }
    }
    std::cout << "fuse_groups_plan ok\n";
    return 0;
}
