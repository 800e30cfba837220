// mask_any.hpp -- the host part of the OR-of-conjunctions masks over label columns (Index::masks_where_any, MaskAny of k_labels.hip): checks the
// arguments of vdb_mask_create_where_any* and lays out the clause table over the term table of mask_sets.hpp.  Host only: no HIP, no
// other header of the library but mask_sets.hpp for SetTerm (tests/cpp/mask_any_asan.cpp builds it on its own).  docs/DESIGN_flat.md 4.1o.
//
// A mask is the OR of its clauses, clauses [mask_lims[g], mask_lims[g + 1]) of the call, at most MASK_MAX_CLAUSES of them; a clause is
// the AND of its terms, terms [clause_lims[c], clause_lims[c + 1]), at most SETS_MAX_TERMS of them; a term is the set / range term of
// mask_sets.hpp with the same match.  A mask without clauses allows NO row; a clause without terms allows EVERY row.
//
// On the device the call is one buffer: the SetTerm table, then the clause limits as u32 (n_clauses + 1 entries, padded to 8 bytes),
// then the packed bitmap block as it arrived.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "mask_sets.hpp"

namespace vdb {

constexpr uint32_t MASK_MAX_CLAUSES = 64;  // VDB_MASK_MAX_CLAUSES

// Checks everything vdb_mask_create_where_any_many states about its arguments.  Empty string: fine, and the three outputs hold the
// clauses, terms and bitmap words of the call; otherwise the message.  The limits are read before what they index: mask_lims, then
// clause_lims, then (mask_sets_check, with the clauses as its conjunctions) the term arrays and set_lims; set_words never.
inline std::string mask_any_check(const uint64_t *mask_lims, const uint64_t *clause_lims, const uint32_t *columns, const uint32_t *lo,
                                  const uint32_t *hi, const uint32_t *flags, const uint64_t *set_lims, const uint64_t *set_words,
                                  uint64_t n_masks, uint64_t *n_clauses_out, uint64_t *n_terms_out, uint64_t *set_words_out) {
    *n_clauses_out = *n_terms_out = *set_words_out = 0;
    if (n_masks == 0) return "";
    if (!mask_lims) return "null argument";
    if (n_masks >= (1ull << 28)) return "too many masks for one call";
    std::string bad = mask_lims_check(mask_lims, n_masks, MASK_MAX_CLAUSES, "mask clauses", "mask_lims", "mask", "clauses");
    if (!bad.empty()) return bad;
    const uint64_t n_clauses = mask_lims[n_masks];
    if (n_clauses == 0) return "";  // every mask is empty: nothing else is read
    if (n_clauses >= (1ull << 28)) return "too many clauses for one call";  // (so a term index fits 32 bits)
    if (!clause_lims) return "null argument";
    bad = mask_lims_check(clause_lims, n_clauses, SETS_MAX_TERMS, "mask clauses", "clause_lims", "clause", "terms");
    if (!bad.empty()) return bad;
    bad = mask_sets_check(clause_lims, columns, lo, hi, flags, set_lims, set_words, n_clauses, n_terms_out, set_words_out);
    if (!bad.empty()) return bad;
    *n_clauses_out = n_clauses;
    return "";
}

struct AnyLayout {  // byte offsets of the three parts of the device buffer of a checked call
    size_t clause_off, sets_off, total;
};
// clause_entries u32 behind the term table: 0 for a masks_where_sets call, whose bitmaps follow the terms directly
inline AnyLayout mask_terms_buffer(uint64_t n_terms, uint64_t clause_entries, uint64_t n_set_words) {
    AnyLayout L;
    L.clause_off = size_t(n_terms ? n_terms : 1) * sizeof(SetTerm);  // (a multiple of 8)
    L.sets_off = L.clause_off + (size_t(clause_entries) * sizeof(uint32_t) + 7) / 8 * 8;
    L.total = L.sets_off + size_t(n_set_words) * sizeof(uint64_t);
    return L;
}
inline AnyLayout mask_any_buffer(uint64_t n_clauses, uint64_t n_terms, uint64_t n_set_words) {
    return mask_terms_buffer(n_terms, n_clauses + 1, n_set_words);
}
// the clause table: out[c] = first term of clause c, out[n_clauses] = n_terms (the term table itself is mask_sets_layout's)
inline void mask_any_layout(const uint64_t *clause_lims, uint64_t n_clauses, std::vector<uint32_t> &out) {
    out.assign(n_clauses + 1, 0);
    for (uint64_t c = 0; n_clauses && c <= n_clauses; c++) out[c] = (uint32_t)clause_lims[c];
}

// The match of row `row` against clauses [c0, c1) of a laid-out call, as the kernel (MaskAny, k_labels.hip) evaluates it with the columns and bitmaps
// readable on the host (the restatement the CPU test checks by brute force).
inline bool mask_any_match(const SetTerm *terms, const uint32_t *clause_tab, uint32_t c0, uint32_t c1, uint64_t row) {
    bool any = false;
    for (uint32_t c = c0; c < c1 && !any; c++) {
        bool okc = true;
        for (uint32_t t = clause_tab[c]; t < clause_tab[c + 1]; t++) okc = okc && mask_sets_match(terms[t], terms[t].col ? terms[t].col[row] : SETS_LABEL_NONE);
        any = okc;
    }
    return any;
}

}  // namespace vdb
