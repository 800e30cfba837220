// Stand-alone check of mask_terms_check in csrc/mask_sets.hpp (host only), meant to be built with -fsanitize=address,undefined
// (tests/test_mask_terms_plan_cpu.py): every rejection vdb_mask_create_where_many documents, with the whole message and in the order
// the call detects them, and the accepted forms at the edges -- eight terms, column 15, no masks at all.  All arrays are heap vectors of
// exactly the documented lengths, so a read past what the limits allow is an ASan report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "mask_sets.hpp"

struct Call {
    std::vector<uint64_t> term_lims{0};
    std::vector<uint32_t> col, code;
    bool no_lims = false, no_cols = false, no_codes = false, no_out = false;
    void term(uint32_t c, uint32_t v) {
        col.push_back(c);
        code.push_back(v);
    }
    void end_mask() { term_lims.push_back(col.size()); }
    std::string check(uint64_t *nt = nullptr) const {
        static int out;  // only tested for null
        uint64_t a = 7;
        const std::string r = vdb::mask_terms_check(no_lims ? nullptr : term_lims.data(), no_cols ? nullptr : col.data(), no_codes ? nullptr : code.data(),
                                                    term_lims.size() - 1, no_out ? nullptr : &out, &a);
        if (nt) *nt = a;
        return r;
    }
};

static void refused(const Call &c, const char *want, const char *what) {
    uint64_t nt = 7;
    const std::string r = c.check(&nt);
    if (r != want || nt != 0) {
        std::printf("FAILED: %s: got \"%s\" (%llu terms), wanted \"%s\"\n", what, r.c_str(), (unsigned long long)nt, want);
        std::exit(1);
    }
}
static void accepted(const Call &c, uint64_t want_nt, const char *what) {
    uint64_t nt = 7;
    const std::string r = c.check(&nt);
    if (!r.empty() || nt != want_nt) {
        std::printf("FAILED: %s: \"%s\" (%llu terms)\n", what, r.c_str(), (unsigned long long)nt);
        std::exit(1);
    }
}
static Call one_mask(int n_terms, uint32_t column = 0) {
    Call c;
    for (int t = 0; t < n_terms; t++) c.term(column, uint32_t(t));
    c.end_mask();
    return c;
}

int main() {
    // ---- the caps: eight terms and column 15 pass, nine and column 16 are refused ----
    accepted(one_mask(8), 8, "eight terms");
    refused(one_mask(9), "mask terms: mask 0 has 9 terms, at most 8 are supported", "nine terms");
    accepted(one_mask(1, 15), 1, "column 15");
    refused(one_mask(1, 16), "mask terms: column 16 (term 0), an index has 16", "column 16");
    {
        Call c = one_mask(8);  // the cap is per mask: a second mask of eight terms is fine, a ninth term in it is not
        for (int t = 0; t < 8; t++) c.term(1, 0);
        c.end_mask();
        accepted(c, 16, "two masks of eight terms");
        c.term_lims.pop_back();
        c.term(1, 0);
        c.end_mask();
        refused(c, "mask terms: mask 1 has 9 terms, at most 8 are supported", "the second mask over the cap");
        Call d = one_mask(2);
        d.term(3, 0);
        d.term(0xFFFFFFFFu, 0);
        d.end_mask();
        refused(d, "mask terms: column 4294967295 (term 3), an index has 16", "the column of a later term");
    }
    // ---- limits ----
    {
        const std::vector<uint64_t> start{1};  // (one entry: nothing behind a wrong start is read)
        int out = 0;
        uint64_t nt = 7;
        const std::string r = vdb::mask_terms_check(start.data(), nullptr, nullptr, 1, &out, &nt);
        if (r != "mask terms: term_lims[0] must be 0" || nt) {
            std::printf("FAILED: term_lims start: got \"%s\"\n", r.c_str());
            return 1;
        }
        Call d;
        d.term(0, 0);
        d.term(0, 0);
        d.term_lims = {0, 2, 1};
        refused(d, "mask terms: term_lims must not decrease (mask 1)", "term_lims order");
    }
    // ---- null arguments, in the order the call finds them ----
    {
        Call c = one_mask(1);
        c.no_lims = true;
        refused(c, "null argument", "null term_lims");
        Call d = one_mask(1);
        d.no_out = true;
        refused(d, "null argument", "null out");
        Call e = one_mask(9, 16);  // the limits are judged before the term arrays are missed, those before a column is read
        e.no_cols = true;
        refused(e, "mask terms: mask 0 has 9 terms, at most 8 are supported", "limits before null columns");
        Call f = one_mask(1, 16);
        f.no_codes = true;
        refused(f, "null argument", "null codes before the column range");
        f.no_codes = false;
        f.no_cols = true;
        refused(f, "null argument", "null columns");
        Call g = one_mask(1);
        g.term_lims[0] = 1;
        g.no_out = true;
        refused(g, "null argument", "null out before the limits");
    }
    {
        // too many masks: judged after the null pointers and before term_lims is read -- one entry stands for 2^28 + 1
        std::vector<uint64_t> lims{5};
        int out = 0;
        uint64_t nt = 7;
        if (vdb::mask_terms_check(lims.data(), nullptr, nullptr, 1ull << 28, &out, &nt) != "too many masks for one call" || nt) {
            std::printf("FAILED: too many masks\n");
            return 1;
        }
        if (vdb::mask_terms_check(nullptr, nullptr, nullptr, 1ull << 28, &out, &nt) != "null argument") {
            std::printf("FAILED: null term_lims before too many masks\n");
            return 1;
        }
    }
    // ---- legal edge forms: no masks, masks without terms ----
    {
        uint64_t nt = 7;
        if (!vdb::mask_terms_check(nullptr, nullptr, nullptr, 0, nullptr, &nt).empty() || nt) {
            std::printf("FAILED: n_masks == 0\n");
            return 1;
        }
        Call c;
        c.end_mask();
        c.end_mask();
        c.no_cols = c.no_codes = true;  // no terms: the term arrays are not looked at
        accepted(c, 0, "masks without terms");
        Call d;
        d.end_mask();
        d.term(15, 0xFFFFFFFFu);  // LABEL_NONE is a legal code
        d.end_mask();
        accepted(d, 1, "an empty mask before a term");
    }
    std::printf("mask_terms ok\n");
    return 0;
}
