// Stand-alone check of csrc/mask_any.hpp (host only), meant to be built with -fsanitize=address,undefined
// (tests/test_mask_any_plan_cpu.py): every accepted and every refused argument shape of vdb_mask_create_where_any_many -- the limits at
// their caps, non-monotone limits, bitmaps that do not fit their span, masks without clauses and clauses without terms -- the laid-out
// clause table and buffer offsets, and a brute-force comparison of mask_any_match with a restatement written here over every label
// value of small spans.  All arrays are heap vectors of exactly the documented lengths, so a read past what the limits allow is an
// ASan report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "mask_any.hpp"

using vdb::SetTerm;
static const uint32_t NONE = 0xFFFFFFFFu;

struct Call {
    std::vector<uint64_t> mask_lims{0}, clause_lims{0};
    std::vector<uint32_t> col, lo, hi, flags;
    std::vector<uint64_t> set_lims{0}, words;
    bool no_set_lims = false, no_clause_lims = false;
    void term(uint32_t c, uint32_t l, uint32_t h, uint32_t f, std::vector<uint64_t> bitmap = {}) {
        col.push_back(c);
        lo.push_back(l);
        hi.push_back(h);
        flags.push_back(f);
        words.insert(words.end(), bitmap.begin(), bitmap.end());
        set_lims.push_back(words.size());
    }
    void end_clause() { clause_lims.push_back(col.size()); }
    void end_mask() { mask_lims.push_back(clause_lims.size() - 1); }
    std::string check(uint64_t *nc = nullptr, uint64_t *nt = nullptr, uint64_t *nw = nullptr) const {
        uint64_t a = 0, b = 0, c = 0;
        const std::string r = vdb::mask_any_check(mask_lims.data(), no_clause_lims ? nullptr : clause_lims.data(), col.data(), lo.data(), hi.data(),
                                                  flags.data(), no_set_lims ? nullptr : set_lims.data(), words.data(), mask_lims.size() - 1, &a, &b, &c);
        if (nc) *nc = a;
        if (nt) *nt = b;
        if (nw) *nw = c;
        return r;
    }
};

static void fail(const char *what) {
    std::printf("FAILED: %s\n", what);
    std::exit(1);
}
static void refused(const Call &c, const char *needle, const char *what) {
    uint64_t nc = 7, nt = 7, nw = 7;
    const std::string r = c.check(&nc, &nt, &nw);
    if (r.find(needle) == std::string::npos) {
        std::printf("FAILED: %s: got \"%s\", wanted \"%s\"\n", what, r.c_str(), needle);
        std::exit(1);
    }
    if (nc || nt || nw) fail("a refused call reports no sizes");
}
static void accepted(const Call &c, uint64_t want_nc, uint64_t want_nt, uint64_t want_nw, const char *what) {
    uint64_t nc = 0, nt = 0, nw = 0;
    const std::string r = c.check(&nc, &nt, &nw);
    if (!r.empty() || nc != want_nc || nt != want_nt || nw != want_nw) {
        std::printf("FAILED: %s: \"%s\" (%llu clauses, %llu terms, %llu words)\n", what, r.c_str(), (unsigned long long)nc, (unsigned long long)nt,
                    (unsigned long long)nw);
        std::exit(1);
    }
}
static Call clauses_of(int n_clauses, int terms_each) {
    Call c;
    for (int k = 0; k < n_clauses; k++) {
        for (int t = 0; t < terms_each; t++) c.term(uint32_t(t), 0, 5, 0);
        c.end_clause();
    }
    c.end_mask();
    return c;
}

int main() {
    // ---- the caps: 64 clauses and 8 terms pass, 65 and 9 are refused ----
    accepted(clauses_of(64, 8), 64, 512, 0, "64 clauses of 8 terms");
    refused(clauses_of(65, 1), "65 clauses", "more than 64 clauses in a mask");
    refused(clauses_of(1, 9), "9 terms", "more than 8 terms in a clause");
    {
        Call c = clauses_of(64, 1);  // the cap is per mask: a second mask of 64 clauses is fine, a 65th clause in it is not
        for (int k = 0; k < 64; k++) {
            c.term(1, 0, 0, 0);
            c.end_clause();
        }
        c.end_mask();
        accepted(c, 128, 128, 0, "two masks of 64 clauses");
        c.mask_lims.pop_back();
        c.term(1, 0, 0, 0);
        c.end_clause();
        c.end_mask();
        refused(c, "mask 1 has 65 clauses", "the second mask over the cap");
    }
    // ---- limits ----
    {
        Call c = clauses_of(2, 1);
        c.mask_lims[0] = 1;
        refused(c, "mask_lims[0] must be 0", "mask_lims start");
        Call d = clauses_of(2, 1);
        d.mask_lims = {0, 2, 1};
        refused(d, "mask_lims must not decrease", "mask_lims order");
        Call e = clauses_of(2, 1);
        e.clause_lims[0] = 1;
        refused(e, "clause_lims[0] must be 0", "clause_lims start");
        Call f = clauses_of(3, 1);
        f.clause_lims = {0, 2, 1, 3};
        refused(f, "clause_lims must not decrease", "clause_lims order");
        Call g = clauses_of(2, 1);
        g.no_clause_lims = true;
        refused(g, "null argument", "clauses without clause_lims");
        uint64_t a, b, c3;
        if (vdb::mask_any_check(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, &a, &b, &c3) != "null argument") fail("null mask_lims");
    }
    // ---- the limits check the four callers share (mask_lims_check): the equality form, the conjunction form, the masks and the clauses
    // of this form.  Each is driven through its own check function with limits that start wrong, descend, or pass the cap by one in
    // group 1; the messages are compared whole with the texts the library has always given.  A limits vector ends where the check
    // must stop reading. ----
    {
        struct Variant {
            const char *who;
            uint64_t cap;
            const char *start, *order, *over;
        };
        const Variant variants[4] = {
            {"equality terms", 8, "mask terms: term_lims[0] must be 0", "mask terms: term_lims must not decrease (mask 1)",
             "mask terms: mask 1 has 9 terms, at most 8 are supported"},
            {"set terms", 8, "mask terms: term_lims[0] must be 0", "mask terms: term_lims must not decrease (mask 1)",
             "mask terms: mask 1 has 9 terms, at most 8 are supported"},
            {"clauses of a mask", 64, "mask clauses: mask_lims[0] must be 0", "mask clauses: mask_lims must not decrease (mask 1)",
             "mask clauses: mask 1 has 65 clauses, at most 64 are supported"},
            {"terms of a clause", 8, "mask clauses: clause_lims[0] must be 0", "mask clauses: clause_lims must not decrease (clause 1)",
             "mask clauses: clause 1 has 9 terms, at most 8 are supported"},
        };
        const std::vector<uint64_t> two_clauses{0, 2};
        int dummy_out = 0;
        for (int v = 0; v < 4; v++) {
            const Variant &V = variants[v];
            const std::vector<uint64_t> cases[3] = {{1}, {0, 2, 1}, {0, 1, 1 + V.cap + 1}};
            const char *want[3] = {V.start, V.order, V.over};
            for (int k = 0; k < 3; k++) {
                const uint64_t *lims = cases[k].data();
                uint64_t a = 0, b = 0, c = 0;
                std::string got;
                if (v == 0) got = vdb::mask_terms_check(lims, nullptr, nullptr, 2, &dummy_out, &a);
                if (v == 1) got = vdb::mask_sets_check(lims, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 2, &a, &b);
                if (v == 2) got = vdb::mask_any_check(lims, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 2, &a, &b, &c);
                if (v == 3) got = vdb::mask_any_check(two_clauses.data(), lims, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, &a, &b, &c);
                if (got != want[k] || a || b || c) {
                    std::printf("FAILED: limits of the %s, case %d: got \"%s\", wanted \"%s\"\n", V.who, k, got.c_str(), want[k]);
                    std::exit(1);
                }
            }
        }
        const std::vector<uint64_t> fine{0, 8, 8, 16};  // the cap itself, an empty group
        if (!vdb::mask_lims_check(fine.data(), 3, 8, "w", "l", "g", "e").empty()) fail("limits at the cap");
    }
    // ---- every argument error of the conjunction call, through the clause layer ----
    {
        Call c;
        c.term(16, 0, 0, 0);
        c.end_clause();
        c.end_mask();
        refused(c, "column 16", "column out of range");
        Call d;
        d.term(0, 0, 0, 4);
        d.end_clause();
        d.end_mask();
        refused(d, "unknown flag bits", "flag bits");
        Call e;
        e.term(0, 0, 5, 0);
        e.end_clause();
        e.end_mask();
        e.set_lims[0] = e.set_lims[1] = 1;
        refused(e, "set_lims[0] must be 0", "set_lims start");
        Call f;
        f.term(0, 0, 63, 0, {1});
        f.end_clause();
        f.term(0, 0, 5, 0);
        f.end_clause();
        f.end_mask();
        f.set_lims[2] = 0;
        refused(f, "set_lims must not decrease", "set_lims order");
        Call g;
        g.term(0, 0, 64, 0, {1});  // 65 codes need 2 words
        g.end_clause();
        g.end_mask();
        refused(g, "need 2", "bitmap too short");
        Call h;
        h.term(0, 0, 63, 0, {1, 1});  // 64 codes need 1 word
        h.end_clause();
        h.end_mask();
        refused(h, "need 1", "bitmap too long");
        Call i;
        i.term(0, 5, 4, 0, {1});
        i.end_clause();
        i.end_mask();
        refused(i, "lo > hi", "a bitmap on an empty range");
        Call j;
        j.term(0, 0, 0xFFFFFFFFu, 0, {1});
        j.end_clause();
        j.end_mask();
        refused(j, "need 67108864", "span computed in 64 bits");
    }
    {
        // more than MASK_MAX_SET_BITS in one call: 9 one-term clauses of 2^18 bitmap words each pass the cap of 2^21 words, 8 are exactly
        // it.  (set_words is never read by the check: a one-word vector stands in for it.)
        Call c;
        for (int k = 0; k < 9; k++) {
            c.col.push_back(0);
            c.lo.push_back(0);
            c.hi.push_back((1u << 24) - 1);
            c.flags.push_back(0);
            c.set_lims.push_back(c.set_lims.back() + (1ull << 18));
            c.end_clause();
        }
        c.end_mask();
        c.words.assign(1, 0);
        refused(c, "bitmap words in one call", "the cap on bitmap bits");
        Call d;
        for (int k = 0; k < 8; k++) {
            d.col.push_back(0);
            d.lo.push_back(0);
            d.hi.push_back((1u << 24) - 1);
            d.flags.push_back(0);
            d.set_lims.push_back(d.set_lims.back() + (1ull << 18));
            d.end_clause();
        }
        d.end_mask();
        d.words.assign(1, 0);
        accepted(d, 8, 8, 1ull << 21, "exactly the cap");
    }
    // ---- legal edge forms: no masks, a mask without clauses, clauses without terms ----
    {
        uint64_t a = 1, b = 1, c3 = 1;
        if (!vdb::mask_any_check(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &a, &b, &c3).empty() || a || b || c3) fail("n_masks == 0");
        Call c;
        c.end_mask();  // a mask without clauses, alone: neither clause_lims nor a term array is read
        c.no_clause_lims = c.no_set_lims = true;
        accepted(c, 0, 0, 0, "one mask without clauses");
        Call d;
        d.end_mask();    // no clauses
        d.end_clause();  // a clause without terms
        d.end_mask();
        d.end_clause();
        d.term(3, 9, 2, vdb::TERM_NEGATE | vdb::TERM_NONE);
        d.term(15, 0, 0xFFFFFFFFu, 0);
        d.end_clause();
        d.end_mask();
        accepted(d, 3, 2, 0, "empty masks and clauses among others");
        d.no_set_lims = true;
        accepted(d, 3, 2, 0, "null set_lims");
        Call e;  // only clauses without terms: the term arrays are not read
        e.end_clause();
        e.end_clause();
        e.end_mask();
        e.no_set_lims = true;
        accepted(e, 2, 0, 0, "clauses without terms alone");
        std::vector<uint32_t> tab;
        vdb::mask_any_layout(e.clause_lims.data(), 2, tab);
        if (tab != std::vector<uint32_t>{0, 0, 0}) fail("clause table of empty clauses");
        vdb::mask_any_layout(nullptr, 0, tab);
        if (tab != std::vector<uint32_t>{0}) fail("clause table without clauses");
        const vdb::AnyLayout L0 = vdb::mask_any_buffer(0, 0, 0);
        if (L0.clause_off != sizeof(SetTerm) || L0.sets_off != L0.clause_off + 8 || L0.total != L0.sets_off) fail("buffer of an empty call");
    }
    // ---- layout and brute-force match ----
    std::mt19937_64 rng(1806);
    const uint32_t SPACE = 40;  // labels 0 .. 39 and NONE in each of three columns; a "row" is one combination of them
    std::vector<uint32_t> colv[3];
    for (uint32_t a = 0; a <= SPACE; a += 3)
        for (uint32_t b = 0; b <= SPACE; b += 5)
            for (uint32_t c = 0; c <= SPACE; c += 7) {
                colv[0].push_back(a == SPACE - 1 ? NONE : a);
                colv[1].push_back(b == SPACE ? NONE : b);
                colv[2].push_back(c == SPACE - 5 ? NONE : c);
            }
    const uint64_t n_rows = colv[0].size();
    const uint32_t *col_ptrs[16];
    for (int c = 0; c < 16; c++) col_ptrs[c] = c < 3 ? colv[c].data() : nullptr;  // columns 3 .. 15 were never written
    uint64_t masks_checked = 0, allowed = 0;
    for (int it = 0; it < 300; it++) {
        Call c;
        std::vector<std::set<uint32_t>> sets;
        const int n_masks = 1 + int(rng() % 4);
        for (int g = 0; g < n_masks; g++) {
            const int ncl = int(rng() % 5);
            for (int k = 0; k < ncl; k++) {
                const int nt = int(rng() % 4);
                for (int t = 0; t < nt; t++) {
                    uint32_t lo = uint32_t(rng() % SPACE), hi = uint32_t(rng() % SPACE);
                    const uint32_t f = uint32_t(rng() % 4);
                    std::vector<uint64_t> bm;
                    std::set<uint32_t> codes;
                    const int kind = int(rng() % 4);
                    if (!(kind == 0 && lo > hi)) {  // (else: an empty range, kept)
                        if (lo > hi) std::swap(lo, hi);
                        if (kind == 1) hi = 0xFFFFFFFFu;
                        if (kind >= 2) {
                            bm.assign(vdb::mask_sets_span_words(lo, hi), 0);
                            for (uint32_t v = lo; v <= hi; v++)
                                if (rng() % 2) {
                                    codes.insert(v);
                                    bm[(v - lo) >> 6] |= 1ull << ((v - lo) & 63);
                                }
                        }
                    }
                    c.term(uint32_t(rng() % 5), lo, hi, f, bm);
                    sets.push_back(codes);
                }
                c.end_clause();
            }
            c.end_mask();
        }
        uint64_t nc = 0, nt = 0, nw = 0;
        if (!c.check(&nc, &nt, &nw).empty() || nc != c.clause_lims.size() - 1 || nt != c.col.size() || nw != c.words.size()) fail("a legal random call was refused");
        const vdb::AnyLayout L = vdb::mask_any_buffer(nc, nt, nw);
        if (L.clause_off % 8 || L.sets_off % 8 || L.clause_off < nt * sizeof(SetTerm) || L.sets_off < L.clause_off + (nc + 1) * 4 ||
            L.total != L.sets_off + nw * 8)
            fail("buffer offsets");
        std::vector<uint64_t> dev(c.words);  // the packed block "on the device": exactly nw words
        std::vector<SetTerm> terms;
        std::vector<uint32_t> tab;
        vdb::mask_sets_layout(c.col.data(), c.lo.data(), c.hi.data(), c.flags.data(), c.set_lims.data(), nt, col_ptrs, dev.data(), terms);
        vdb::mask_any_layout(c.clause_lims.data(), nc, tab);
        if (tab.size() != nc + 1 || tab[nc] != nt) fail("clause table size");
        for (int g = 0; g < n_masks; g++) {
            const uint32_t c0 = uint32_t(c.mask_lims[g]), c1 = uint32_t(c.mask_lims[g + 1]);
            for (uint64_t r = 0; r < n_rows; r++) {
                bool want = false;  // the rule, written out from the call's own arrays
                for (uint32_t k = c0; k < c1; k++) {
                    bool okc = true;
                    for (uint64_t t = c.clause_lims[k]; t < c.clause_lims[k + 1]; t++) {
                        const uint32_t v = c.col[t] < 3 ? colv[c.col[t]][r] : NONE;
                        bool m;
                        if (v == NONE)
                            m = (c.flags[t] & 2u) != 0;
                        else {
                            const bool has = c.set_lims[t + 1] > c.set_lims[t];
                            const bool inside = c.lo[t] <= v && v <= c.hi[t] && (!has || sets[t].count(v));
                            m = inside != ((c.flags[t] & 1u) != 0);
                        }
                        okc = okc && m;
                    }
                    want = want || okc;
                }
                if (vdb::mask_any_match(terms.data(), tab.data(), c0, c1, r) != want) fail("match(row)");
                allowed += want;
            }
            masks_checked++;
        }
    }
    if (allowed == 0 || allowed == masks_checked * n_rows) fail("the random masks are degenerate");
    std::printf("mask_any ok: %llu masks over %llu rows\n", (unsigned long long)masks_checked, (unsigned long long)n_rows);
    return 0;
}
