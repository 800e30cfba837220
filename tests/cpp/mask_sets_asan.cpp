// Stand-alone check of csrc/mask_sets.hpp (host only), meant to be built with -fsanitize=address,undefined
// (tests/test_mask_sets_plan_cpu.py): every rejection vdb_mask_create_where_sets_many documents, the laid-out bitmap offsets, and for
// every term it builds a brute-force match(v) over a small code space against a restatement written here.  All arrays are heap
// vectors of exactly the documented lengths, so a read past what the limits allow is an ASan report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "mask_sets.hpp"

using vdb::SetTerm;
static const uint32_t NONE = 0xFFFFFFFFu;

struct Call {
    std::vector<uint64_t> term_lims{0};
    std::vector<uint32_t> col, lo, hi, flags;
    std::vector<uint64_t> set_lims{0}, words;
    bool no_set_lims = false;
    void term(uint32_t c, uint32_t l, uint32_t h, uint32_t f, std::vector<uint64_t> bitmap = {}) {
        col.push_back(c);
        lo.push_back(l);
        hi.push_back(h);
        flags.push_back(f);
        words.insert(words.end(), bitmap.begin(), bitmap.end());
        set_lims.push_back(words.size());
    }
    void end_mask() { term_lims.push_back(col.size()); }
    std::string check(uint64_t *nt = nullptr, uint64_t *nw = nullptr) const {
        uint64_t a = 0, b = 0;
        const std::string r = vdb::mask_sets_check(term_lims.data(), col.data(), lo.data(), hi.data(), flags.data(),
                                                   no_set_lims ? nullptr : set_lims.data(), words.data(), term_lims.size() - 1, &a, &b);
        if (nt) *nt = a;
        if (nw) *nw = b;
        return r;
    }
};

static void fail(const char *what) {
    std::printf("FAILED: %s\n", what);
    std::exit(1);
}
static void refused(const Call &c, const char *needle, const char *what) {
    const std::string r = c.check();
    if (r.find(needle) == std::string::npos) {
        std::printf("FAILED: %s: got \"%s\", wanted \"%s\"\n", what, r.c_str(), needle);
        std::exit(1);
    }
}

int main() {
    // ---- rejections ----
    {
        Call c;
        for (int i = 0; i < 9; i++) c.term(0, 0, 0, 0);
        c.end_mask();
        refused(c, "9 terms", "more than 8 terms in a mask");
    }
    {
        Call c;
        c.term(16, 0, 0, 0);
        c.end_mask();
        refused(c, "column 16", "column out of range");
    }
    {
        Call c;
        c.term(0, 0, 0, 4);
        c.end_mask();
        refused(c, "unknown flag bits", "flag bits");
    }
    {
        Call c;
        c.term(0, 0, 5, 0);
        c.end_mask();
        c.set_lims[0] = 1;
        c.set_lims[1] = 1;
        refused(c, "set_lims[0] must be 0", "set_lims start");
    }
    {
        Call c;
        c.term(0, 0, 63, 0, {1});
        c.term(0, 0, 5, 0);
        c.end_mask();
        c.set_lims[2] = 0;
        refused(c, "set_lims must not decrease", "set_lims order");
    }
    {
        Call c;
        c.term(0, 0, 64, 0, {1});  // 65 codes need 2 words
        c.end_mask();
        refused(c, "need 2", "bitmap too short");
        Call d;
        d.term(0, 0, 63, 0, {1, 1});  // 64 codes need 1 word
        d.end_mask();
        refused(d, "need 1", "bitmap too long");
    }
    {
        Call c;
        c.term(0, 5, 4, 0, {1});
        c.end_mask();
        refused(c, "lo > hi", "a bitmap on an empty range");
    }
    {
        Call c;  // the full u32 span: 2^26 words are needed; a 32-bit hi - lo + 1 would wrap to 0
        c.term(0, 0, 0xFFFFFFFFu, 0, {1});
        c.end_mask();
        refused(c, "need 67108864", "span computed in 64 bits");
        if (vdb::mask_sets_span_words(0, 0xFFFFFFFFu) != (1ull << 26) || vdb::mask_sets_span_words(7, 7) != 1 ||
            vdb::mask_sets_span_words(1, 64) != 1 || vdb::mask_sets_span_words(1, 65) != 2)
            fail("span words");
    }
    {
        // more than MASK_MAX_SET_BITS in one call: 2^21 words is the cap; 9 terms of 2^18 words each pass it.  (Lengths match the
        // spans; set_words itself is never read by the check, so a one-word vector stands in for it.)
        Call c;
        const uint32_t span_hi = (1u << 24) - 1;  // 2^24 codes = 2^18 words
        for (int g = 0; g < 9; g++) {
            c.col.push_back(0);
            c.lo.push_back(0);
            c.hi.push_back(span_hi);
            c.flags.push_back(0);
            c.set_lims.push_back(c.set_lims.back() + (1ull << 18));
            c.end_mask();
        }
        c.words.assign(1, 0);
        refused(c, "bitmap words in one call", "the cap on bitmap bits");
        Call d = c;  // 8 of them are exactly the cap: fine
        d.col.pop_back(), d.lo.pop_back(), d.hi.pop_back(), d.flags.pop_back(), d.set_lims.pop_back(), d.term_lims.pop_back();
        uint64_t nt = 0, nw = 0;
        if (!d.check(&nt, &nw).empty() || nt != 8 || nw != (1ull << 21)) fail("exactly the cap is legal");
    }
    {
        Call c;
        c.term(0, 0, 0, 0);
        c.end_mask();
        c.term_lims[0] = 1;
        refused(c, "term_lims[0] must be 0", "term_lims start");
        Call d;
        d.term(0, 0, 0, 0);
        d.term(0, 0, 0, 0);
        d.term_lims = {0, 2, 1};
        refused(d, "term_lims must not decrease", "term_lims order");
    }
    // ---- legal edge forms ----
    {
        Call c;
        c.end_mask();  // a mask without terms
        c.term(3, 9, 2, 0);  // the empty range
        c.term(3, 9, 2, vdb::TERM_NEGATE | vdb::TERM_NONE);
        c.term(15, 0, 0xFFFFFFFFu, 0);  // hi = 0xFFFFFFFF without a bitmap
        c.end_mask();
        uint64_t nt = 0, nw = 0;
        if (!c.check(&nt, &nw).empty() || nt != 3 || nw != 0) fail("legal edge forms");
        c.no_set_lims = true;  // set_lims == NULL: no term has a bitmap
        if (!c.check(&nt, &nw).empty() || nt != 3 || nw != 0) fail("null set_lims");
        uint64_t a, b;
        if (!vdb::mask_sets_check(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &a, &b).empty()) fail("n_masks == 0");
    }
    // ---- layout and brute-force match ----
    std::mt19937_64 rng(1806);
    const uint32_t SPACE = 300;  // labels 0 .. 299 and NONE
    std::vector<uint32_t> fake_cols(16);
    const uint32_t *col_ptrs[16];
    for (int c = 0; c < 16; c++) col_ptrs[c] = (c % 3 == 1) ? nullptr : &fake_cols[c];
    uint64_t terms_checked = 0;
    for (int it = 0; it < 400; it++) {
        Call c;
        std::vector<std::set<uint32_t>> sets;  // the codes of every term with a bitmap
        const int n_masks = 1 + int(rng() % 4);
        for (int g = 0; g < n_masks; g++) {
            const int nt = int(rng() % 9);
            for (int t = 0; t < nt; t++) {
                uint32_t lo = uint32_t(rng() % SPACE), hi = uint32_t(rng() % SPACE);
                const uint32_t f = uint32_t(rng() % 4);
                std::vector<uint64_t> bm;
                std::set<uint32_t> codes;
                const int kind = int(rng() % 4);
                if (kind == 0 && lo > hi) {
                    // an empty range, kept
                } else {
                    if (lo > hi) std::swap(lo, hi);
                    if (kind == 1) hi = 0xFFFFFFFFu;  // open above, no bitmap
                    if (kind >= 2) {
                        bm.assign(vdb::mask_sets_span_words(lo, hi), 0);
                        for (uint32_t v = lo; v <= hi; v++)
                            if (kind == 2 ? (v == lo || v == hi) : (rng() % 3 == 0)) {
                                codes.insert(v);
                                bm[(v - lo) >> 6] |= 1ull << ((v - lo) & 63);
                            }
                        if ((hi - lo + 1) % 64) bm.back() |= ~0ull << ((hi - lo + 1) % 64);  // bits past hi - lo are ignored
                    }
                }
                c.term(uint32_t(rng() % 16), lo, hi, f, bm);
                sets.push_back(codes);
            }
            c.end_mask();
        }
        uint64_t nt = 0, nw = 0;
        if (!c.check(&nt, &nw).empty() || nt != c.col.size() || nw != c.words.size()) fail("a legal random call was refused");
        // the packed block "on the device": a copy of exactly nw words, so an offset past it is an ASan report
        std::vector<uint64_t> dev(c.words);
        std::vector<SetTerm> tab;
        vdb::mask_sets_layout(c.col.data(), c.lo.data(), c.hi.data(), c.flags.data(), c.set_lims.data(), nt, col_ptrs, dev.data(), tab);
        if (tab.size() != nt) fail("table size");
        for (uint64_t t = 0; t < nt; t++) {
            const SetTerm &tm = tab[t];
            const bool has = c.set_lims[t + 1] > c.set_lims[t];
            if (tm.col != col_ptrs[c.col[t]] || tm.lo != c.lo[t] || tm.hi != c.hi[t] || tm.flags != c.flags[t]) fail("term fields");
            if (has ? tm.bitmap != dev.data() + c.set_lims[t] : tm.bitmap != nullptr) fail("bitmap offset");
            for (uint32_t v = 0; v <= SPACE; v++) {
                const uint32_t label = v == SPACE ? NONE : v;
                bool want;
                if (label == NONE)
                    want = (c.flags[t] & 2u) != 0;
                else {
                    const bool inside = c.lo[t] <= label && label <= c.hi[t] && (!has || sets[t].count(label));
                    want = inside != ((c.flags[t] & 1u) != 0);
                }
                if (vdb::mask_sets_match(tm, label) != want) fail("match(v)");
            }
            terms_checked++;
        }
        // with set_lims == NULL the same ranges carry no bitmap
        std::vector<SetTerm> plain;
        vdb::mask_sets_layout(c.col.data(), c.lo.data(), c.hi.data(), c.flags.data(), nullptr, nt, col_ptrs, nullptr, plain);
        for (const SetTerm &tm : plain)
            if (tm.bitmap) fail("null set_lims layout");
    }
    // the two documented equivalences of the equality terms
    {
        SetTerm eq{}, none{};
        eq.lo = eq.hi = 7;
        none.lo = 1, none.hi = 0, none.flags = vdb::TERM_NONE;
        for (uint32_t v = 0; v <= SPACE; v++) {
            const uint32_t label = v == SPACE ? NONE : v;
            if (vdb::mask_sets_match(eq, label) != (label == 7) || vdb::mask_sets_match(none, label) != (label == NONE)) fail("equality equivalences");
        }
    }
    std::printf("mask_sets ok: %llu terms\n", (unsigned long long)terms_checked);
    return 0;
}
