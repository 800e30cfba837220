// index_masks.hip -- the row masks Index builds on the device from its label columns (k_labels.hip; docs/DESIGN_flat.md 4.1l/m/o/p/y):
// masks_where, masks_where_sets, masks_where_any, mask_combine, masks_partition, and label_counts and label_lookup (4.1aa) beside them.  All five builders have
// one second half, masks_finish; the three predicate forms also have one first half behind their argument checks, masks_from_table.
#include <algorithm>
#include <array>

#include "index.hpp"

namespace vdb {

namespace {

// Where the bit words or the allow-lists of a chunk's masks go: views into ONE allocation that the masks share (RowMask::slab_bits /
// slab_ids; every view starts at a multiple of DEVBUF_ALIGN), or an allocation per mask.
struct MaskPlacer {
    std::shared_ptr<DevBuf> slab;  // null: an allocation per mask
    size_t at = 0;
    explicit MaskPlacer(bool slabs) : slab(slabs ? std::make_shared<DevBuf>() : nullptr) {}
    void reserve(size_t total) {  // (the sum of devbuf_align_up(bytes) over the chunk, before the first place)
        if (slab) slab->reserve(total);
    }
    void place(DevBuf &buf, std::shared_ptr<DevBuf> &hold, size_t bytes) {
        if (slab) {
            hold = slab;
            buf.view(slab->as<char>() + at, devbuf_align_up(bytes));
            at += devbuf_align_up(bytes);
        } else {
            buf.reserve(bytes);
        }
    }
};

// one part of a call's table buffer (its terms, its clause table, its bitmaps): `bytes` from `src` (host) to offset `off`; 0: nothing
struct TablePart {
    size_t off = 0;
    const void *src = nullptr;
    size_t bytes = 0;
};
using TableParts = std::array<TablePart, 3>;

// The table buffer of a checked call of set / range terms, with a clause table (clause_entries = clauses + 1, masks_where_any) or without
// one (0, masks_where_sets), at mask_terms_buffer's offsets L.  `lay` builds the host side against the buffer's device address.
struct SetTables {
    AnyLayout L;
    std::vector<SetTerm> terms;
    std::vector<uint32_t> clims;
    TableParts lay(const Index &ix, char *base, const uint64_t *clause_lims, uint64_t clause_entries, const uint32_t *columns, const uint32_t *lo,
                   const uint32_t *hi, const uint32_t *flags, const uint64_t *set_lims, const uint64_t *set_words, uint64_t n_terms,
                   uint64_t n_set_words) {
        const uint32_t *col_ptrs[LABEL_COLUMNS];
        for (uint32_t c = 0; c < LABEL_COLUMNS; c++) col_ptrs[c] = ix.label_col(c);
        mask_sets_layout(columns, lo, hi, flags, set_lims, n_terms, col_ptrs, reinterpret_cast<const uint64_t *>(base + L.sets_off), terms);
        if (clause_entries) mask_any_layout(clause_lims, clause_entries - 1, clims);
        return {{{0, terms.data(), n_terms * sizeof(SetTerm)},
                 {L.clause_off, clims.data(), clims.size() * sizeof(uint32_t)},
                 {L.sets_off, set_words, n_set_words * sizeof(uint64_t)}}};
    }
};

// The second half of all five builders.  `launch(g0, nb)` enqueues the bit-word kernel and k_mask_scan for masks [g0, g0 + nb) of the
// call (jobs in ws.keys_b, block counts in ws.flags, totals in ws.misc; the caller's tables in ws.keys_a); lims[g] .. lims[g + 1] = the
// range a job carries (nullptr: none); bytes(g0, nb) = what the launch reads, for the profile entry `prof`.  Per chunk of masks:
// headers and jobs, launch, ONE read-back of the totals (the only synchronisation before the allow-lists can be allocated), k_mask_ids,
// synchronise.  The chunk bounds grid.y and the block-count scratch (at most 1024 masks and 64 MiB of counts).  slabs
// (masks_partition): bit words and allow-lists of a chunk are views into one allocation each instead of one per mask and list.
template <class Bytes, class Launch>
void masks_finish(Index &ix, Workspace &ws, const uint64_t *lims, uint64_t n_masks, RowMask *const *out, const char *prof, Bytes bytes, Launch launch,
                  bool slabs = false) {
    hipStream_t s = ws.stream;
    const uint64_t n = ix.n;
    slabs = slabs && !devbuf_efence();  // (a mask's own end stays fenced: per-mask allocations)
    const uint64_t nw = (n + 63) / 64;
    const uint32_t nblocks = mask_where_blocks(n);
    const uint64_t gen = ix.write_gen.load();
    const uint64_t chunk = nblocks ? std::min<uint64_t>({n_masks, 1024, std::max<uint64_t>((64ull << 20) / (sizeof(uint32_t) * nblocks), 1)}) : n_masks;
    std::vector<MaskJob> h_jobs(chunk);
    std::vector<uint32_t *> h_ids(chunk);
    if (nblocks) {  // (contents not preserved by reserve: everything a chunk needs is sized here, once)
        ws.keys_b.reserve(chunk * sizeof(MaskJob));
        ws.keys_c.reserve(chunk * sizeof(uint32_t *));
        ws.flags.reserve(chunk * nblocks * sizeof(uint32_t));
        ws.misc.reserve(chunk * sizeof(uint32_t));
    }
    const size_t bits_bytes = std::max<uint64_t>(nw, 1) * sizeof(uint64_t);
    for (uint64_t g0 = 0; g0 < n_masks; g0 += chunk) {
        const uint64_t nb = std::min(chunk, n_masks - g0);
        MaskPlacer bits(slabs), ids(slabs);
        bits.reserve(nb * devbuf_align_up(bits_bytes));
        for (uint64_t j = 0; j < nb; j++) {
            RowMask &m = *out[g0 + j];
            m.owner = &ix;
            m.device = ix.device;
            m.gen = gen;
            m.n_rows = n;
            m.m = 0;
            bits.place(m.d_bits, m.slab_bits, bits_bytes);
            h_jobs[j] = {m.d_bits.as<uint64_t>(), lims ? (uint32_t)lims[g0 + j] : 0u, lims ? (uint32_t)lims[g0 + j + 1] : 0u};
        }
        if (!nblocks) {  // an empty index: masks with m = 0
            ids.reserve(nb * devbuf_align_up(sizeof(uint32_t)));
            for (uint64_t j = 0; j < nb; j++) ids.place(out[g0 + j]->d_ids, out[g0 + j]->slab_ids, sizeof(uint32_t));
            continue;
        }
        uint32_t *h_tot = static_cast<uint32_t *>(ws.pinned(chunk * sizeof(uint32_t)));
        VDB_HIP(hipMemcpyAsync(ws.keys_b.p, h_jobs.data(), nb * sizeof(MaskJob), hipMemcpyHostToDevice, s));
        ix.prof_begin(ws, prof, bytes(g0, nb) + double(nb) * double(nw) * sizeof(uint64_t));
        launch(g0, nb);
        ix.prof_end(ws);
        VDB_HIP(hipMemcpyAsync(h_tot, ws.misc.p, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        VDB_SYNC(s);
        uint64_t sum_m = 0;
        size_t total = 0;  // the lists back to back, each start rounded up to DEVBUF_ALIGN
        for (uint64_t j = 0; j < nb; j++) {
            out[g0 + j]->m = h_tot[j];
            sum_m += h_tot[j];
            total += devbuf_align_up(std::max<uint64_t>(h_tot[j], 1) * sizeof(uint32_t));
        }
        ids.reserve(total);
        for (uint64_t j = 0; j < nb; j++) {
            RowMask &m = *out[g0 + j];
            ids.place(m.d_ids, m.slab_ids, std::max<uint64_t>(m.m, 1) * sizeof(uint32_t));
            h_ids[j] = m.d_ids.as<uint32_t>();
        }
        VDB_HIP(hipMemcpyAsync(ws.keys_c.p, h_ids.data(), nb * sizeof(uint32_t *), hipMemcpyHostToDevice, s));
        ix.prof_begin(ws, prof, double(nb) * double(nw) * sizeof(uint64_t) + double(sum_m) * sizeof(uint32_t));
        launch_mask_ids(ws.keys_b.as<MaskJob>(), ws.keys_c.as<uint32_t *>(), (uint32_t)nb, n, ws.flags.as<uint32_t>(), s);
        ix.prof_end(ws);
        VDB_SYNC(s);
        ix.prof_collect(ws);
    }
}

// What the three predicate forms do behind their argument checks: lease a workspace, reserve the call's table buffer in keys_a and
// upload it ONCE before the first chunk -- tables(base) lays the host side out against the buffer's device address and names its parts;
// reserve does not preserve contents, so nothing else sizes keys_a -- then masks_finish with k_mask_rows over pred(base), and the masks
// are counted.  An empty index uploads nothing and launches nothing.
template <class Tables, class MakePred, class Bytes>
void masks_from_table(Index &ix, const uint64_t *lims, uint64_t n_masks, RowMask *const *out, const char *prof, std::atomic<uint64_t> &counter,
                      size_t table_bytes, Tables tables, MakePred pred, Bytes bytes) {
    ix.use_device();
    WsLease ws(ix);
    hipStream_t s = ws->stream;
    if (ix.n) {
        ws->keys_a.reserve(table_bytes);
        char *base = ws->keys_a.as<char>();
        for (const TablePart &p : tables(base))
            if (p.bytes) VDB_HIP(hipMemcpyAsync(base + p.off, p.src, p.bytes, hipMemcpyHostToDevice, s));
    }
    masks_finish(ix, *ws, lims, n_masks, out, prof, bytes, [&](uint64_t, uint64_t nb) {
        launch_mask_rows(pred(ws->keys_a.as<char>()), ws->keys_b.as<MaskJob>(), (uint32_t)nb, ix.n, ws->flags.as<uint32_t>(), ws->misc.as<uint32_t>(), s);
    });
    counter += n_masks;
}

}  // namespace

// A conjunction of equality terms per mask (mask_sets.hpp: mask_terms_check; MaskEq evaluates).
void Index::masks_where(const uint64_t *term_lims, const uint32_t *columns, const uint32_t *codes, uint64_t n_masks, RowMask *const *out) {
    uint64_t n_terms = 0;
    const std::string bad = mask_terms_check(term_lims, columns, codes, n_masks, out, &n_terms);
    VDB_REQUIRE(bad.empty(), bad);
    if (n_masks == 0) return;
    std::vector<MaskTerm> h_terms(std::max<uint64_t>(n_terms, 1));
    for (uint64_t t = 0; t < n_terms; t++) h_terms[t] = {label_col(columns[t]), codes[t]};
    masks_from_table(
        *this, term_lims, n_masks, out, "mask_where", mask_where_masks, h_terms.size() * sizeof(MaskTerm),
        [&](char *) { return TableParts{{{0, h_terms.data(), h_terms.size() * sizeof(MaskTerm)}}}; },
        [](char *base) { return MaskEq{reinterpret_cast<const MaskTerm *>(base)}; },
        [&](uint64_t g0, uint64_t nb) { return double(term_lims[g0 + nb] - term_lims[g0]) * double(n) * sizeof(uint32_t); });
}

// A conjunction of set / range terms per mask (mask_sets.hpp checks and lays out; MaskAll evaluates).
void Index::masks_where_sets(const uint64_t *term_lims, const uint32_t *columns, const uint32_t *lo, const uint32_t *hi, const uint32_t *flags,
                             const uint64_t *set_lims, const uint64_t *set_words, uint64_t n_masks, RowMask *const *out) {
    VDB_REQUIRE(n_masks == 0 || out, "null argument");
    uint64_t n_terms = 0, n_set_words = 0;
    const std::string bad = mask_sets_check(term_lims, columns, lo, hi, flags, set_lims, set_words, n_masks, &n_terms, &n_set_words);
    VDB_REQUIRE(bad.empty(), bad);
    if (n_masks == 0) return;
    SetTables T{mask_terms_buffer(n_terms, 0, n_set_words)};
    masks_from_table(
        *this, term_lims, n_masks, out, "mask_where_sets", mask_where_set_masks, T.L.total,
        [&](char *base) { return T.lay(*this, base, nullptr, 0, columns, lo, hi, flags, set_lims, set_words, n_terms, n_set_words); },
        [](char *base) { return MaskAll{reinterpret_cast<const SetTerm *>(base)}; },
        [&](uint64_t g0, uint64_t nb) { return double(term_lims[g0 + nb] - term_lims[g0]) * double(n) * sizeof(uint32_t); });
}

// An OR of conjunctions per mask (mask_any.hpp checks and lays out; MaskAny evaluates).
void Index::masks_where_any(const uint64_t *mask_lims, const uint64_t *clause_lims, const uint32_t *columns, const uint32_t *lo, const uint32_t *hi,
                            const uint32_t *flags, const uint64_t *set_lims, const uint64_t *set_words, uint64_t n_masks, RowMask *const *out) {
    VDB_REQUIRE(n_masks == 0 || out, "null argument");
    uint64_t n_clauses = 0, n_terms = 0, n_set_words = 0;
    const std::string bad = mask_any_check(mask_lims, clause_lims, columns, lo, hi, flags, set_lims, set_words, n_masks, &n_clauses, &n_terms, &n_set_words);
    VDB_REQUIRE(bad.empty(), bad);
    if (n_masks == 0) return;
    SetTables T{mask_any_buffer(n_clauses, n_terms, n_set_words)};
    masks_from_table(
        *this, mask_lims, n_masks, out, "mask_where_any", mask_where_any_masks, T.L.total,
        [&](char *base) { return T.lay(*this, base, clause_lims, n_clauses + 1, columns, lo, hi, flags, set_lims, set_words, n_terms, n_set_words); },
        [&](char *base) { return MaskAny{reinterpret_cast<const SetTerm *>(base), reinterpret_cast<const uint32_t *>(base + T.L.clause_off)}; },
        [&](uint64_t g0, uint64_t nb) {  // 4 B x terms x rows over all clauses of the chunk
            const uint64_t c0 = mask_lims[g0], c1 = mask_lims[g0 + nb];
            return c1 > c0 ? double(clause_lims[c1] - clause_lims[c0]) * double(n) * sizeof(uint32_t) : 0.0;
        });
}

// AND / OR / NOT of finished masks (k_mask_combine): one output mask through the same second half.
void Index::mask_combine(int op, const RowMask *const *in, const uint8_t *invert, uint64_t n_in, RowMask &out) {
    VDB_REQUIRE(op == MASK_OP_AND || op == MASK_OP_OR, "mask combine: unknown op " + std::to_string(op));
    VDB_REQUIRE(n_in >= 1 && n_in <= MASK_COMBINE_MAX, "mask combine: " + std::to_string(n_in) + " inputs, 1 .. " + std::to_string(MASK_COMBINE_MAX) + " are supported");
    VDB_REQUIRE(in, "null argument");
    for (uint64_t i = 0; i < n_in; i++) VDB_REQUIRE(in[i], "null mask");
    for (uint64_t i = 0; i < n_in; i++) check_mask(*in[i]);
    use_device();
    WsLease ws(*this);
    MaskCombine a{};
    a.n_in = (uint32_t)n_in;
    a.op = op;
    for (uint64_t i = 0; i < n_in; i++) {
        a.in[i] = in[i]->d_bits.as<uint64_t>();
        if (invert && invert[i]) a.invert |= 1u << i;
    }
    RowMask *outp = &out;
    masks_finish(
        *this, *ws, nullptr, 1, &outp, "mask_combine", [&](uint64_t, uint64_t) { return double(n_in) * double((n + 63) / 64) * sizeof(uint64_t); },
        [&](uint64_t, uint64_t) { launch_mask_combine(a, out.d_bits.as<uint64_t>(), n, ws->flags.as<uint32_t>(), ws->misc.as<uint32_t>(), ws->stream); });
    mask_combine_masks += 1;
}

// ONE column grouped by code (mask_partition.hpp checks the codes and lays out a chunk's table; k_mask_partition reads the column once
// per chunk).  masks_finish cuts the call into chunks and places every chunk's masks in two slabs; per chunk the launch clears the bit
// words and the block counts, uploads the chunk's table and runs the kernel -- all of it inside the profile entry.
void Index::masks_partition(uint32_t column, const uint32_t *codes, uint64_t n_codes, RowMask *const *out) {
    const std::string bad = mask_partition_check(column, codes, n_codes);
    VDB_REQUIRE(bad.empty(), bad);
    VDB_REQUIRE(n_codes == 0 || out, "null argument");
    if (n_codes == 0) return;
    use_device();
    WsLease ws(*this);
    hipStream_t s = ws->stream;
    const uint32_t *col = label_col(column);
    const uint32_t nblocks = mask_where_blocks(n);
    const size_t bits_bytes = std::max<uint64_t>((n + 63) / 64, 1) * sizeof(uint64_t);
    std::vector<uint32_t> h_sorted, h_slot, h_table;  // (alive until masks_finish has synchronised the chunk that reads them)
    if (n) ws->keys_a.reserve(2 * size_t(PART_MAX_CHUNK) * sizeof(uint32_t));
    masks_finish(
        *this, *ws, nullptr, n_codes, out, "mask_partition", [&](uint64_t, uint64_t nb) { return double(n) * sizeof(uint32_t) + double(nb) * double(nblocks) * sizeof(uint32_t); },
        [&](uint64_t g0, uint64_t nb) {
            if (out[g0]->slab_bits) {  // the chunk's masks are one slab: one clear
                VDB_HIP(hipMemsetAsync(out[g0]->slab_bits->p, 0, nb * out[g0]->d_bits.cap, s));
            } else {
                for (uint64_t j = 0; j < nb; j++) VDB_HIP(hipMemsetAsync(out[g0 + j]->d_bits.p, 0, bits_bytes, s));
            }
            VDB_HIP(hipMemsetAsync(ws->flags.p, 0, nb * size_t(nblocks) * sizeof(uint32_t), s));
            mask_partition_layout(codes + g0, (uint32_t)nb, h_sorted, h_slot);
            h_table.assign(h_sorted.begin(), h_sorted.end());
            h_table.insert(h_table.end(), h_slot.begin(), h_slot.end());
            VDB_HIP(hipMemcpyAsync(ws->keys_a.p, h_table.data(), h_table.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
            launch_mask_partition(col, ws->keys_a.as<uint32_t>(), (uint32_t)nb, ws->keys_b.as<MaskJob>(), n, ws->flags.as<uint32_t>(), ws->misc.as<uint32_t>(), s);
        },
        true);
    mask_partition_masks += n_codes;
}

// Rows per code of one column, over all rows or under a mask (k_label_counts): per chunk of PART_MAX_CHUNK codes one launch over the
// column, the counters read back in the table's order and handed out in the caller's.
void Index::label_counts(uint32_t column, const RowMask *mask, const uint32_t *codes, uint64_t n_codes, uint64_t *out_counts) {
    const std::string bad = mask_partition_check(column, codes, n_codes);
    VDB_REQUIRE(bad.empty(), bad);
    VDB_REQUIRE(n_codes == 0 || out_counts, "null argument");
    if (mask) check_mask(*mask);
    label_count_calls += 1;
    if (n_codes == 0) return;
    std::fill(out_counts, out_counts + n_codes, uint64_t(0));
    if (n == 0) return;
    use_device();
    WsLease ws(*this);
    hipStream_t s = ws->stream;
    const uint32_t *col = label_col(column);
    const uint64_t *bits = mask ? mask->d_bits.as<uint64_t>() : nullptr;
    std::vector<uint32_t> h_sorted, h_slot;
    ws->keys_a.reserve(size_t(PART_MAX_CHUNK) * sizeof(uint32_t));
    ws->misc.reserve(size_t(PART_MAX_CHUNK) * sizeof(uint32_t));
    uint32_t *h_cnt = static_cast<uint32_t *>(ws->pinned(size_t(PART_MAX_CHUNK) * sizeof(uint32_t)));
    for (uint64_t g0 = 0; g0 < n_codes; g0 += PART_MAX_CHUNK) {
        const uint32_t nb = (uint32_t)std::min<uint64_t>(PART_MAX_CHUNK, n_codes - g0);
        mask_partition_layout(codes + g0, nb, h_sorted, h_slot);
        VDB_HIP(hipMemcpyAsync(ws->keys_a.p, h_sorted.data(), nb * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        prof_begin(*ws, "label_counts", double(n) * sizeof(uint32_t) + (bits ? double((n + 63) / 64) * sizeof(uint64_t) : 0.0));
        VDB_HIP(hipMemsetAsync(ws->misc.p, 0, nb * sizeof(uint32_t), s));
        launch_label_counts(col, ws->keys_a.as<uint32_t>(), nb, bits, n, ws->misc.as<uint32_t>(), num_cu, s);
        prof_end(*ws);
        VDB_HIP(hipMemcpyAsync(h_cnt, ws->misc.p, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        VDB_SYNC(s);
        prof_collect(*ws);
        for (uint32_t i = 0; i < nb; i++) out_counts[g0 + h_slot[i]] = h_cnt[i];
    }
}

// Rows per code and the lowest row of each (k_lookup.hip; lookup_plan.hpp checks the list and picks the route).  Both routes keep
// [counts | firsts] of all n_codes entries in ws.misc, prepared by two fills, and read them back ONCE.  Sorted: the tables of all
// chunks are uploaded together (keys_a) and chunk c's launch writes entries [c * PART_MAX_CHUNK, ...) in its table's order; the host
// hands them out in the caller's.  Direct: the codes go up as they are (keys_a), k_lookup_table scatters their positions into slot_of
// (keys_b, span u32) and one launch over the column writes the entries in the caller's order.
void Index::label_lookup(uint32_t column, const uint32_t *codes, uint64_t n_codes, uint64_t *out_first, uint64_t *out_counts) {
    const std::string bad = label_lookup_check(column, codes, n_codes);
    VDB_REQUIRE(bad.empty(), bad);
    VDB_REQUIRE(n_codes == 0 || (out_first && out_counts), "null argument");
    const LookupPlan plan = label_lookup_plan(codes, n_codes, label_lookup_table_bytes);
    uint64_t passes = 0;
    if (n_codes && n) {
        use_device();
        WsLease ws(*this);
        hipStream_t s = ws->stream;
        const uint32_t *col = label_col(column);
        ws->keys_a.reserve(n_codes * sizeof(uint32_t));
        ws->misc.reserve(2 * n_codes * sizeof(uint32_t));
        uint32_t *d_cnt = ws->misc.as<uint32_t>(), *d_first = d_cnt + n_codes;
        uint32_t *h_out = static_cast<uint32_t *>(ws->pinned(2 * n_codes * sizeof(uint32_t)));
        std::vector<uint32_t> h_table, h_slot, c_sorted, c_slot;  // (alive until the stream has been synchronised)
        prof_begin(*ws, "label_lookup", double(plan.chunks) * double(n) * sizeof(uint32_t) + (plan.route == LOOKUP_DIRECT ? double(plan.span) * sizeof(uint32_t) : 0.0));
        VDB_HIP(hipMemsetAsync(d_cnt, 0, n_codes * sizeof(uint32_t), s));
        VDB_HIP(hipMemsetAsync(d_first, 0xFF, n_codes * sizeof(uint32_t), s));
        if (plan.route == LOOKUP_DIRECT) {
            ws->keys_b.reserve(plan.span * sizeof(uint32_t));
            VDB_HIP(hipMemcpyAsync(ws->keys_a.p, codes, n_codes * sizeof(uint32_t), hipMemcpyHostToDevice, s));
            VDB_HIP(hipMemsetAsync(ws->keys_b.p, 0xFF, plan.span * sizeof(uint32_t), s));
            launch_lookup_table(ws->keys_a.as<uint32_t>(), n_codes, plan.base, (uint32_t)plan.span, ws->keys_b.as<uint32_t>(), num_cu, s);
            launch_label_lookup_direct(col, ws->keys_b.as<uint32_t>(), plan.base, (uint32_t)plan.span,
                                       plan.none_at == ~uint64_t(0) ? LOOKUP_NO_SLOT : (uint32_t)plan.none_at, n, d_cnt, d_first, num_cu,
                                       label_lookup_max_blocks, s);
            passes = 1;
        } else {
            h_table.resize(n_codes);
            h_slot.resize(n_codes);
            for (uint64_t g0 = 0; g0 < n_codes; g0 += PART_MAX_CHUNK) {
                const uint32_t nb = (uint32_t)std::min<uint64_t>(PART_MAX_CHUNK, n_codes - g0);
                mask_partition_layout(codes + g0, nb, c_sorted, c_slot);
                std::copy(c_sorted.begin(), c_sorted.end(), h_table.begin() + g0);
                std::copy(c_slot.begin(), c_slot.end(), h_slot.begin() + g0);
            }
            VDB_HIP(hipMemcpyAsync(ws->keys_a.p, h_table.data(), n_codes * sizeof(uint32_t), hipMemcpyHostToDevice, s));
            for (uint64_t g0 = 0; g0 < n_codes; g0 += PART_MAX_CHUNK) {
                const uint32_t nb = (uint32_t)std::min<uint64_t>(PART_MAX_CHUNK, n_codes - g0);
                launch_label_lookup(col, ws->keys_a.as<uint32_t>() + g0, nb, n, d_cnt + g0, d_first + g0, num_cu, label_lookup_max_blocks, s);
                passes++;
            }
        }
        prof_end(*ws);
        VDB_HIP(hipMemcpyAsync(h_out, d_cnt, 2 * n_codes * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        VDB_SYNC(s);
        prof_collect(*ws);
        for (uint64_t i = 0; i < n_codes; i++) {
            const uint64_t j = plan.route == LOOKUP_DIRECT ? i : (i / PART_MAX_CHUNK) * PART_MAX_CHUNK + h_slot[i];
            out_counts[j] = h_out[i];
            out_first[j] = h_out[n_codes + i] == LOOKUP_ROW_NONE32 ? LOOKUP_ROW_NONE : uint64_t(h_out[n_codes + i]);
        }
    } else if (n_codes) {  // an empty index: no row carries anything
        std::fill(out_counts, out_counts + n_codes, uint64_t(0));
        std::fill(out_first, out_first + n_codes, LOOKUP_ROW_NONE);
    }
    label_lookup_calls += 1;
    label_lookup_codes += n_codes;
    label_lookup_direct += passes && plan.route == LOOKUP_DIRECT ? 1 : 0;
    label_lookup_passes += passes;
}

}  // namespace vdb
