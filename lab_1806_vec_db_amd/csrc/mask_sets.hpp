// mask_sets.hpp -- the host part of the label predicates of one conjunction per mask: checks the arguments of the equality terms
// (vdb_mask_create_where*; Index::masks_where, MaskEq) and of the set / range terms (vdb_mask_create_where_sets*; Index::masks_where_sets,
// MaskAll) and lays out the device term table over the packed bitmap block.  Host only: no HIP, no other header of the library
// (tests/cpp/mask_terms_asan.cpp and mask_sets_asan.cpp build it on its own).  docs/DESIGN_flat.md 4.1l, 4.1m.
//
// A term is {column, lo, hi, flags, bitmap}.  A row whose label in the column is v matches it
//  - when v == LABEL_NONE (no value, or a column never written): iff flags has TERM_NONE -- TERM_NEGATE never inverts this case;
//  - otherwise: inside = lo <= v <= hi and (no bitmap or bit (v - lo) of the bitmap); the row matches iff inside != (flags has TERM_NEGATE).
// The bitmaps of a call arrive packed back to back in `set_words`; term t's is words [set_lims[t], set_lims[t + 1]) and is absent when
// that range is empty.  The packed block is uploaded as it is, so a term's device bitmap is `bitmap_base + set_lims[t]`.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace vdb {

constexpr uint32_t TERM_NEGATE = 1u;                  // VDB_TERM_NEGATE
constexpr uint32_t TERM_NONE = 2u;                    // VDB_TERM_NONE
constexpr uint64_t MASK_MAX_SET_BITS = 1ull << 27;    // VDB_MASK_MAX_SET_BITS: bitmap bits per call (16 MiB)
constexpr uint32_t SETS_LABEL_COLUMNS = 16;           // = LABEL_COLUMNS (kernels.hpp asserts it)
constexpr uint32_t SETS_LABEL_NONE = 0xFFFFFFFFu;     // = LABEL_NONE
constexpr uint32_t SETS_MAX_TERMS = 8;                // = MASK_MAX_TERMS

struct SetTerm {            // one entry of the device term table (32 B)
    const uint32_t *col;    // the term's column, nullptr: never written (every row reads LABEL_NONE)
    const uint64_t *bitmap; // bit j = code lo + j is in the set; nullptr: the whole range [lo, hi]
    uint32_t lo, hi, flags, pad;
};

// 64-bit words of a bitmap over the codes [lo, hi] (lo <= hi): up to 2^26, so never in 32-bit arithmetic
inline uint64_t mask_sets_span_words(uint32_t lo, uint32_t hi) { return (uint64_t(hi) - uint64_t(lo) + 1 + 63) / 64; }

// The check every limits array of the mask calls gets: lims[0 .. n_groups] starts at 0, does not decrease, and no group
// [lims[g], lims[g + 1]) has more than `cap` entries.  Empty string: fine; otherwise "<what>: ..." with the array's name and the nouns
// of a group and of its entries.  Reads lims[g + 1] only after lims[g] passed.
inline std::string mask_lims_check(const uint64_t *lims, uint64_t n_groups, uint64_t cap, const char *what, const char *name, const char *group,
                                   const char *entries) {
    const std::string w = std::string(what) + ": ";
    if (lims[0] != 0) return w + name + "[0] must be 0";
    for (uint64_t g = 0; g < n_groups; g++) {
        if (lims[g + 1] < lims[g]) return w + name + " must not decrease (" + group + " " + std::to_string(g) + ")";
        if (lims[g + 1] - lims[g] > cap)
            return w + group + " " + std::to_string(g) + " has " + std::to_string(lims[g + 1] - lims[g]) + " " + entries + ", at most " +
                   std::to_string(cap) + " are supported";
    }
    return "";
}

// Checks everything vdb_mask_create_where_many states about its arguments (`out` = where the masks go, only tested for null).  Empty
// string: fine, and *n_terms_out holds the number of terms of the call; otherwise the message.  term_lims is read before the term arrays,
// those up to term_lims[n_masks], `codes` never.
inline std::string mask_terms_check(const uint64_t *term_lims, const uint32_t *columns, const uint32_t *codes, uint64_t n_masks, const void *out,
                                    uint64_t *n_terms_out) {
    *n_terms_out = 0;
    if (n_masks == 0) return "";
    if (!term_lims || !out) return "null argument";
    if (n_masks >= (1ull << 28)) return "too many masks for one call";
    const std::string bad = mask_lims_check(term_lims, n_masks, SETS_MAX_TERMS, "mask terms", "term_lims", "mask", "terms");
    if (!bad.empty()) return bad;
    const uint64_t n_terms = term_lims[n_masks];
    if (n_terms && (!columns || !codes)) return "null argument";
    for (uint64_t t = 0; t < n_terms; t++)
        if (columns[t] >= SETS_LABEL_COLUMNS)
            return "mask terms: column " + std::to_string(columns[t]) + " (term " + std::to_string(t) + "), an index has " +
                   std::to_string(SETS_LABEL_COLUMNS);
    *n_terms_out = n_terms;
    return "";
}

// Checks everything vdb_mask_create_where_sets_many states about its arguments.  Empty string: fine, and *n_terms_out / *set_words_out
// hold the number of terms and of bitmap words of the call; otherwise the message.  Reads nothing past what the limits allow: term_lims
// before the term arrays, set_lims entry by entry, set_words never.
inline std::string mask_sets_check(const uint64_t *term_lims, const uint32_t *columns, const uint32_t *lo, const uint32_t *hi,
                                   const uint32_t *flags, const uint64_t *set_lims, const uint64_t *set_words, uint64_t n_masks,
                                   uint64_t *n_terms_out, uint64_t *set_words_out) {
    *n_terms_out = *set_words_out = 0;
    if (n_masks == 0) return "";
    if (!term_lims) return "null argument";
    if (n_masks >= (1ull << 28)) return "too many masks for one call";
    const std::string bad = mask_lims_check(term_lims, n_masks, SETS_MAX_TERMS, "mask terms", "term_lims", "mask", "terms");
    if (!bad.empty()) return bad;
    const uint64_t n_terms = term_lims[n_masks];
    if (n_terms == 0) return "";
    if (!columns || !lo || !hi || !flags) return "null argument";
    for (uint64_t t = 0; t < n_terms; t++) {
        if (columns[t] >= SETS_LABEL_COLUMNS)
            return "mask terms: column " + std::to_string(columns[t]) + " (term " + std::to_string(t) + "), an index has " +
                   std::to_string(SETS_LABEL_COLUMNS);
        if (flags[t] & ~(TERM_NEGATE | TERM_NONE))
            return "mask terms: unknown flag bits " + std::to_string(flags[t]) + " (term " + std::to_string(t) + ")";
    }
    uint64_t words = 0;
    if (set_lims) {
        if (set_lims[0] != 0) return "mask terms: set_lims[0] must be 0";
        for (uint64_t t = 0; t < n_terms; t++) {
            if (set_lims[t + 1] < set_lims[t]) return "mask terms: set_lims must not decrease (term " + std::to_string(t) + ")";
            const uint64_t len = set_lims[t + 1] - set_lims[t];
            if (len == 0) continue;  // no bitmap: a plain range, which may be empty
            if (lo[t] > hi[t]) return "mask terms: term " + std::to_string(t) + " has a bitmap and lo > hi";
            const uint64_t want = mask_sets_span_words(lo[t], hi[t]);
            if (len != want)
                return "mask terms: the bitmap of term " + std::to_string(t) + " has " + std::to_string(len) + " words, the codes " +
                       std::to_string(lo[t]) + " .. " + std::to_string(hi[t]) + " need " + std::to_string(want);
        }
        words = set_lims[n_terms];
        if (words > MASK_MAX_SET_BITS / 64)
            return "mask terms: " + std::to_string(words) + " bitmap words in one call, at most " + std::to_string(MASK_MAX_SET_BITS / 64) +
                   " (VDB_MASK_MAX_SET_BITS bits) are supported";
        if (words && !set_words) return "null argument";
    }
    *n_terms_out = n_terms;
    *set_words_out = words;
    return "";
}

// The device term table of a checked call: col_ptrs[c] = the device column c or nullptr, bitmap_base = where the packed block
// set_words[0 .. set_lims[n_terms]) lies on the device.  No pointer is formed for a term without a bitmap.
inline void mask_sets_layout(const uint32_t *columns, const uint32_t *lo, const uint32_t *hi, const uint32_t *flags, const uint64_t *set_lims,
                             uint64_t n_terms, const uint32_t *const *col_ptrs, const uint64_t *bitmap_base, std::vector<SetTerm> &out) {
    out.assign(n_terms, SetTerm{});
    for (uint64_t t = 0; t < n_terms; t++) {
        SetTerm &tm = out[t];
        tm.col = col_ptrs[columns[t]];
        tm.bitmap = (set_lims && set_lims[t + 1] > set_lims[t]) ? bitmap_base + set_lims[t] : nullptr;
        tm.lo = lo[t];
        tm.hi = hi[t];
        tm.flags = flags[t];
    }
}

// The match of one laid-out term against a label value, as set_term_match of k_labels.hip evaluates it with `bitmap` readable on the
// host (the restatement the CPU test checks by brute force; the kernel has its own copy of these four lines).
inline bool mask_sets_match(const SetTerm &tm, uint32_t v) {
    if (v == SETS_LABEL_NONE) return (tm.flags & TERM_NONE) != 0;
    bool inside = tm.lo <= v && v <= tm.hi;
    if (inside && tm.bitmap) inside = (tm.bitmap[(v - tm.lo) >> 6] >> ((v - tm.lo) & 63)) & 1;
    return inside != ((tm.flags & TERM_NEGATE) != 0);
}

}  // namespace vdb
