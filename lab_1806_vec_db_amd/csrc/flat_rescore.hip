// flat_rescore.hip -- the driver of the exact late-interaction rescoring of candidate documents (Index::rescore_groups_device; kernels:
// k_rescore.hip, host arithmetic: rescore_plan.hpp; docs/DESIGN_flat.md 4.1ak).
//
// The second stage behind the document-level fused search: that call ranks documents by a lower bound (every list is cut at fetch_k);
// this one takes its representatives as candidates and scores their documents over ALL their rows.  One call:
//   1  the ids are checked on the device (one flag read back);
//   2  collect, part one, for the whole call: group slots per question, the table of wanted codes, ONE counting pass over the label
//      column; the counts [n_slots | rows] come back (8 B per question) and size the layout -- tiles, offsets, sub-chunks;
//   3  per sub-chunk of questions: collect, part two (minima cleared, unlabelled candidates, ONE appending pass over the label column),
//      pairs, finish.
// Buffers: grp_aux [flag | lims | coff | mask bit pointers], grp_ids / grp_dist the slots' keys / rows, grp_cnt [n_slots | rows | cursors],
// grp_table the code table, grp_q [ent_off | tab_off | items], lists the entries, dense the minima, qsq the query norms.  Every buffer of a
// phase is reserved before its first launch; the read-back between the phases has synchronised.
#include <algorithm>
#include <cstring>
#include <vector>

#include "index.hpp"

namespace vdb {

void Index::rescore_groups_device(Workspace &ws, const float *d_q, const uint64_t *lims, uint64_t nq, const uint64_t *d_cand, const uint64_t *d_cand_cnt,
                                  const uint64_t *h_cand_cnt, uint64_t ld, uint64_t k, int mode, uint32_t column, const RowMask *const *masks,
                                  uint64_t n_masks, const uint32_t *mask_of, uint64_t *d_idx, float *d_dist, uint64_t *d_cnt) {
    hipStream_t s = ws.stream;
    require_f32_rows(*this);
    VDB_REQUIRE(rescore_check_args(mode, lims, nq, k, ld, column, h_cand_cnt) == RESCORE_OK, "rescore groups: bad arguments");
    VDB_REQUIRE(n < (1ull << 32) && nq < (1ull << 31), "rescore groups: too many rows or questions");
    if (nq == 0) return;
    const uint64_t nl = lims[nq];
    // ---- the upload: [flag u64 | lims | coff | mask bit pointers] ------------------------------------------------------------------------
    const size_t off_l = sizeof(uint64_t), off_c = off_l + (nq + 1) * sizeof(uint64_t), off_b = off_c + (nq + 1) * sizeof(uint64_t);
    std::vector<char> blob(off_b + (n_masks ? nl * sizeof(uint64_t *) : 0), 0);
    uint64_t *h_lims = reinterpret_cast<uint64_t *>(blob.data() + off_l), *h_coff = reinterpret_cast<uint64_t *>(blob.data() + off_c);
    for (uint64_t q = 0; q <= nq; q++) h_lims[q] = lims[q];
    for (uint64_t q = 0; q < nq; q++) h_coff[q + 1] = h_coff[q] + h_cand_cnt[q];
    const uint64_t n_cand = h_coff[nq];
    if (n_masks) {
        const uint64_t **h_bits = reinterpret_cast<const uint64_t **>(blob.data() + off_b);
        for (uint64_t j = 0; j < nl; j++) h_bits[j] = masks[mask_of[j]]->d_bits.as<uint64_t>();
    }
    const uint32_t glg = rescore_table_lg(n_cand);
    const uint64_t gcap = 1ull << glg;
    ws.grp_aux.reserve(blob.size());
    ws.grp_ids.reserve(std::max<uint64_t>(n_cand, 1) * sizeof(uint64_t));
    ws.grp_dist.reserve(std::max<uint64_t>(n_cand, 1) * sizeof(uint32_t));
    ws.grp_cnt.reserve(3 * nq * sizeof(uint32_t));
    ws.grp_table.reserve(gcap * (sizeof(uint64_t) + sizeof(uint32_t)));
    VDB_HIP(hipMemcpyAsync(ws.grp_aux.p, blob.data(), blob.size(), hipMemcpyHostToDevice, s));
    char *aux = ws.grp_aux.as<char>();
    const uint64_t *u_lims = reinterpret_cast<const uint64_t *>(aux + off_l), *u_coff = reinterpret_cast<const uint64_t *>(aux + off_c);
    const uint64_t *const *u_bits = n_masks ? reinterpret_cast<const uint64_t *const *>(aux + off_b) : nullptr;
    if (ld)
        ids_ok(
            ws, s, ws.grp_aux.as<uint32_t>(), "rescore groups: a candidate id is no row of this index (id - id_offset must be below len)",
            [&](uint32_t *d_flag) { launch_list_check(d_cand, d_cand_cnt, nq, ld, n, id_offset, d_flag, s); }, true);  // (the upload's first word: zero)
    rescore_calls++;
    rescore_questions += nq;
    if (k == 0) {  // nothing is ranked and no pair is evaluated
        VDB_HIP(hipMemsetAsync(d_cnt, 0, nq * sizeof(uint64_t), s));
        VDB_SYNC(s);
        return;
    }
    // ---- collect, part one -------------------------------------------------------------------------------------------------------------
    uint64_t *slot_key = ws.grp_ids.as<uint64_t>(), *tkey = ws.grp_table.as<uint64_t>();
    uint32_t *slot_row = ws.grp_dist.as<uint32_t>(), *tslot = reinterpret_cast<uint32_t *>(tkey + gcap);
    uint32_t *d_slots = ws.grp_cnt.as<uint32_t>(), *d_rows_cnt = d_slots + nq, *d_cur = d_rows_cnt + nq;
    const uint32_t *col = label_col(column);
    prof_begin(ws, "rescore_collect", double(n_cand) * sizeof(uint64_t) + (col ? double(n) * sizeof(uint32_t) : 0.0));
    launch_rescore_fill64(tkey, gcap, FUSEG_EMPTY, s);
    launch_rescore_slots(d_cand, d_cand_cnt, nq, ld, u_coff, col, id_offset, slot_key, slot_row, d_slots, d_rows_cnt, tkey, tslot, glg, s);
    launch_rescore_match(col, n, tkey, tslot, glg, false, 0, nq, d_rows_cnt, nullptr, nullptr, nullptr, s);
    prof_end(ws);
    uint32_t *h_back = static_cast<uint32_t *>(ws.pinned(2 * nq * sizeof(uint32_t)));
    VDB_HIP(hipMemcpyAsync(h_back, d_slots, 2 * nq * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    VDB_SYNC(s);
    // ---- the layout --------------------------------------------------------------------------------------------------------------------
    std::vector<uint64_t> rows(nq), slots(nq);
    uint64_t rows_all = 0;
    for (uint64_t q = 0; q < nq; q++) {
        slots[q] = h_back[q];
        rows[q] = h_back[nq + q];
        rows_all += rows[q];
    }
    rescore_rows += rows_all;
    const RescoreLayout lay = rescore_layout(lims, nq, rows.data(), slots.data(), ld);
    const size_t off_t = nq * sizeof(uint64_t), off_i = 2 * off_t;
    std::vector<char> blob2(off_i + lay.tiles * sizeof(uint2));
    uint64_t *h_ent = reinterpret_cast<uint64_t *>(blob2.data()), *h_tab = reinterpret_cast<uint64_t *>(blob2.data() + off_t);
    uint2 *h_items = reinterpret_cast<uint2 *>(blob2.data() + off_i);
    uint64_t ent_max = 0, tab_max = 0, item = 0;
    for (uint64_t c0 = 0; c0 < nq; c0 += lay.sub_chunk) {  // offsets from the start of each sub-chunk's buffers
        uint64_t ent = 0, tab = 0;
        for (uint64_t q = c0; q < std::min(nq, c0 + lay.sub_chunk); q++) {
            h_ent[q] = ent;
            h_tab[q] = tab;
            for (uint64_t t = 0; t < rescore_tiles(rows[q]); t++) h_items[item++] = make_uint2((uint32_t)q, (uint32_t)t);
            ent += rescore_tiles(rows[q]) * RESCORE_TILE;
            tab += slots[q] * (lims[q + 1] - lims[q]);
        }
        ent_max = std::max(ent_max, ent);
        tab_max = std::max(tab_max, tab);
    }
    ws.grp_q.reserve(blob2.size());
    ws.lists.reserve(std::max<uint64_t>(ent_max, 1) * RESCORE_ENTRY_BYTES);
    ws.dense.reserve(std::max<uint64_t>(tab_max, 1) * RESCORE_MIN_BYTES);
    const int metric = dist == 0 ? MET_L2_DIRECT : MET_COSINE;
    if (metric == MET_COSINE) {
        ws.qsq.reserve(nl * sizeof(float));
        launch_row_sqnorm(d_q, nl, (uint32_t)dim, ws.qsq.as<float>(), s);
    }
    VDB_HIP(hipMemcpyAsync(ws.grp_q.p, blob2.data(), blob2.size(), hipMemcpyHostToDevice, s));
    const uint64_t *u_ent = ws.grp_q.as<uint64_t>(), *u_tab = u_ent + nq;
    const uint2 *u_items = reinterpret_cast<const uint2 *>(ws.grp_q.as<char>() + off_i);
    uint64_t *entries = ws.lists.as<uint64_t>(), *mins = ws.dense.as<uint64_t>();
    // ---- per sub-chunk: collect part two, pairs, finish ----------------------------------------------------------------------------------
    uint64_t item0 = 0;
    for (uint64_t c0 = 0; c0 < nq; c0 += lay.sub_chunk) {
        const uint64_t nb = std::min(lay.sub_chunk, nq - c0);
        uint64_t tiles = 0, c_rows = 0;
        for (uint64_t q = c0; q < c0 + nb; q++) {
            tiles += rescore_tiles(rows[q]);
            c_rows += rows[q];
        }
        prof_begin(ws, "rescore_collect", double(c_rows) * RESCORE_ENTRY_BYTES + (col ? double(n) * sizeof(uint32_t) : 0.0));
        launch_rescore_prepare(c0, nb, u_lims, u_coff, slot_key, slot_row, d_slots, d_rows_cnt, u_ent, u_tab, entries, mins, d_cur, s);
        launch_rescore_match(col, n, tkey, tslot, glg, true, c0, nb, d_rows_cnt, d_cur, u_ent, entries, s);
        prof_end(ws);
        prof_begin(ws, "rescore_pairs", double(c_rows) * dim * sizeof(float));
        launch_rescore_pairs(d_rows.as<float>(), (uint32_t)dim, d_q, u_lims, u_items + item0, tiles, entries, u_ent, mins, u_tab, metric, d_sq.as<float>(),
                             ws.qsq.as<float>(), u_bits, s);
        prof_end(ws);
        prof_begin(ws, "rescore_finish", double(nb) * k * (sizeof(uint64_t) + sizeof(float)));
        launch_rescore_finish(c0, nb, u_lims, u_coff, slot_row, d_slots, mins, u_tab, mode, id_offset, (uint32_t)k, d_idx, d_dist, d_cnt, s);
        prof_end(ws);
        item0 += tiles;
    }
    VDB_SYNC(s);  // (`blob` and `blob2` are pageable memory: alive until here)
    prof_collect(ws);
}

}  // namespace vdb
