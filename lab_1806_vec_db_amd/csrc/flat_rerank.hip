// flat_rerank.hip -- the Flat list re-rankers of Index: grouped k-NN, diversified k-NN (MMR), search by example rows and the fused
// multi-query search -- by row and by document, the value of a label column --, each as a search form and as a list form over
// caller-supplied lists (docs/DESIGN_flat.md 4.1x and 4.1q/u/v/w/z).
//
// All of them have one shape.  A search form fetches the exact sorted list of K' rows per query -- flat_knn_device, or
// flat_knn_masked_multi_device when the call has masks -- for a sub-chunk of queries whose lists fit LIST_BUDGET (list_plan.hpp) and runs
// ONE small kernel over those lists; a list form checks the ids of the caller's lists (ids_ok, index.hpp) and runs that kernel alone.  The
// kernels differ; what stands around them is here once: zero_counts, max_allowed, reserve_lists / fetch_lists, sub_chunk_loop, end_call.
#include <algorithm>
#include <cstring>

#include "index.hpp"

namespace vdb {

namespace {

// the masks of a call or round (n_masks == 0: unfiltered, masks / mask_of not read)
struct Allowed {
    const RowMask *const *masks;
    uint64_t n_masks;
    const uint32_t *mask_of;
};
// the candidate lists of a sub-chunk, [..][kp] in the workspace
struct Lists {
    uint64_t *ids;
    float *dist;
    uint64_t *cnt;
    uint64_t kp;
};
// a sub-chunk: the queries c0 .. c0 + nb of the call and their lists j0 .. j0 + nj (one each, j0 == c0, unless the call is a fused one)
struct Chunk {
    uint64_t c0, nb, j0, nj;
};

// the answer of every call with k == 0
void zero_counts(Workspace &ws, uint64_t *d_cnt, uint64_t nq) {
    VDB_HIP(hipMemsetAsync(d_cnt, 0, nq * sizeof(uint64_t), ws.stream));
    VDB_SYNC(ws.stream);
}

// the longest allowed set among the first `count` entries of mask_of
uint64_t max_allowed(const Index &ix, const Allowed &a, uint64_t count) {
    if (!a.n_masks) return ix.n;
    uint64_t m = 0;
    for (uint64_t q = 0; q < count; q++) m = std::max<uint64_t>(m, a.masks[a.mask_of[q]]->m);
    return m;
}

// The list buffers of a call (of a round of the grouped call) for sub-chunks of `rows` lists of kp rows, and the one count of that call
// (round) among the calls with a mask per query.  Every buffer of a call is reserved before its first launch: a later, larger reserve
// would free a buffer in use.
Lists reserve_lists(Index &ix, Workspace &ws, uint64_t rows, uint64_t kp, uint64_t n_masks) {
    ws.grp_ids.reserve(rows * kp * sizeof(uint64_t));
    ws.grp_dist.reserve(rows * kp * sizeof(float));
    ws.grp_cnt.reserve(rows * sizeof(uint64_t));
    if (n_masks) ix.filtered_multi_calls++;
    return {ws.grp_ids.as<uint64_t>(), ws.grp_dist.as<float>(), ws.grp_cnt.as<uint64_t>(), kp};
}

// the exact sorted lists of the nj queries at Q, which are entries off .. off + nj of the call's mask_of
void fetch_lists(Index &ix, Workspace &ws, const float *Q, uint64_t nj, const Allowed &a, uint64_t off, const Lists &l) {
    if (a.n_masks)
        ix.flat_knn_masked_multi_device(ws, Q, nj, l.kp, a.masks, a.n_masks, a.mask_of + off, l.ids, l.dist, l.cnt);
    else
        ix.flat_knn_device(ws, Q, nj, l.kp, l.ids, l.dist, l.cnt);
}

// The loop of every form: the nq queries in sub-chunks of `sub`; per sub-chunk fetch(c) -- no_fetch in the list forms --, then launch(c)
// timed as `name` with bytes(c) bytes.  lims (HOST, nq + 1 entries, any base; nullptr: a list per query) gives the lists of a fused query.
template <class Fetch, class Bytes, class Launch>
void sub_chunk_loop(Index &ix, Workspace &ws, uint64_t nq, uint64_t sub, const uint64_t *lims, const char *name, Fetch &&fetch, Bytes &&bytes,
                    Launch &&launch) {
    for (uint64_t c0 = 0; c0 < nq; c0 += sub) {
        const uint64_t nb = std::min(sub, nq - c0);
        const uint64_t j0 = lims ? lims[c0] - lims[0] : c0, nj = lims ? lims[c0 + nb] - lims[c0] : nb;
        const Chunk c{c0, nb, j0, nj};
        fetch(c);
        ix.prof_begin(ws, name, bytes(c));
        launch(c);
        ix.prof_end(ws);
    }
}
constexpr auto no_fetch = [](const Chunk &) {};

// ends a call (a round): everything enqueued has run, the profile entries are in
void end_call(Index &ix, Workspace &ws) {
    VDB_SYNC(ws.stream);
    ix.prof_collect(ws);
}

}  // namespace

// ---- Flat: grouped k-NN, at most g hits per value of one label column (k_group.hip, grouped_plan.hpp; docs/DESIGN_flat.md 4.1q) ----------
// Whether a row is kept depends only on the rows before it in the query's order, so the capped walk of a PREFIX of that order gives a
// prefix of the answer: a round fetches the exact sorted list of K' rows and walks it, and a query that neither filled its k slots nor
// saw its whole allowed set goes round again with a longer list, walked again from its start (the walk is cheap beside the search that
// made the list, and nothing is carried between rounds but the list of open queries).  Round 0 runs on the call's own query block and
// mask_of; later rounds on a compacted block.  A round's queries are cut into sub-chunks whose lists stay under LIST_BUDGET; its
// done bytes are read back once, at its end.
void Index::flat_knn_grouped_device(Workspace &ws, const float *d_q, uint64_t nq, uint64_t k, uint32_t column, uint64_t g, const RowMask *const *masks,
                                    uint64_t n_masks, const uint32_t *mask_of, uint64_t *d_idx, float *d_dist, uint64_t *d_cnt) {
    hipStream_t s = ws.stream;
    require_f32_rows(*this);
    VDB_REQUIRE(column < LABEL_COLUMNS && g >= 1, "grouped k-NN: bad column or group size");
    if (nq == 0) return;
    VDB_REQUIRE(nq < (1ull << 32) && k <= (1ull << 30) - GROUPED_TILE, "flat knn: too many queries or k too large");  // (the walk's table: 2^31 entries at most)
    grouped_queries += nq;
    if (k == 0) return zero_counts(ws, d_cnt, nq);
    std::vector<uint64_t> m_of(nq);
    for (uint64_t q = 0; q < nq; q++) m_of[q] = n_masks ? masks[mask_of[q]]->m : n;
    const uint32_t *col = label_live[column] ? d_labels[column].as<uint32_t>() : nullptr;
    const uint32_t g32 = (uint32_t)std::min<uint64_t>(g, 0xFFFFFFFFull);
    std::vector<uint64_t> active(nq), next;
    for (uint64_t q = 0; q < nq; q++) active[q] = q;
    std::vector<uint32_t> slot, mo;
    uint64_t kp = grouped_first_k(k, flat_grouped_oversample, max_allowed(*this, {masks, n_masks, mask_of}, nq));
    uint64_t exhausted = 0, rounds = 0;
    for (bool first = true; !active.empty(); first = false) {
        const uint64_t na = active.size();
        uint64_t sub = grouped_sub_chunk(na, kp);
        const size_t table1 = group_cap_scratch_bytes(1, k, kp);
        if (table1) sub = std::max<uint64_t>(1, std::min<uint64_t>(sub, LIST_BUDGET / table1));
        // every buffer of the round before its first launch; the round before has synchronised
        const size_t off_slot = na * sizeof(uint64_t), off_done = off_slot + na * sizeof(uint32_t);
        const Lists l = reserve_lists(*this, ws, sub, kp, n_masks);
        ws.grp_aux.reserve(off_done + na);
        if (table1) ws.grp_table.reserve(sub * table1);
        char *aux = ws.grp_aux.as<char>();
        const uint32_t *d_slot = nullptr;
        uint8_t *d_done = reinterpret_cast<uint8_t *>(aux + off_done);
        const float *Q = d_q;
        Allowed open{masks, n_masks, mask_of};
        if (!first) {  // the open queries as a block of their own: rows, the map back to the call's positions, their masks
            ws.grp_q.reserve(na * dim * sizeof(float));
            slot.resize(na);
            for (uint64_t i = 0; i < na; i++) slot[i] = (uint32_t)active[i];
            VDB_HIP(hipMemcpyAsync(aux, active.data(), na * sizeof(uint64_t), hipMemcpyHostToDevice, s));
            VDB_HIP(hipMemcpyAsync(aux + off_slot, slot.data(), na * sizeof(uint32_t), hipMemcpyHostToDevice, s));
            launch_gather_rows_f32(d_q, reinterpret_cast<const uint64_t *>(aux), na, (uint32_t)dim, ws.grp_q.as<float>(), s);
            d_slot = reinterpret_cast<const uint32_t *>(aux + off_slot);
            Q = ws.grp_q.as<float>();
            if (n_masks) {
                mo.resize(na);
                for (uint64_t i = 0; i < na; i++) mo[i] = mask_of[active[i]];
                open.mask_of = mo.data();
            }
        }
        sub_chunk_loop(
            *this, ws, na, sub, nullptr, "group_cap", [&](const Chunk &c) { fetch_lists(*this, ws, Q + c.c0 * dim, c.nb, open, c.c0, l); },
            [&](const Chunk &c) { return double(c.nb) * kp * (LIST_PAIR_BYTES + sizeof(uint32_t)); },
            [&](const Chunk &c) {
                if (first)
                    launch_group_cap(l.ids, l.dist, l.cnt, c.nb, kp, col, n, id_offset, (uint32_t)k, g32, ws.grp_table.as<uint32_t>(), nullptr, d_idx + c.c0 * k,
                                     d_dist + c.c0 * k, d_cnt + c.c0, d_done + c.c0, s);
                else
                    launch_group_cap(l.ids, l.dist, l.cnt, c.nb, kp, col, n, id_offset, (uint32_t)k, g32, ws.grp_table.as<uint32_t>(), d_slot + c.c0, d_idx,
                                     d_dist, d_cnt, d_done + c.c0, s);
            });
        uint8_t *h_done = static_cast<uint8_t *>(ws.pinned(na));  // (the list calls have synchronised: their use of the block is over)
        VDB_HIP(hipMemcpyAsync(h_done, d_done, na, hipMemcpyDeviceToHost, s));
        end_call(*this, ws);  // (ends the round: the host arrays uploaded above are free again)
        rounds++;
        const uint64_t open_m = grouped_compact(active, h_done, m_of.data(), kp, next, exhausted);
        active.swap(next);
        if (!active.empty()) kp = grouped_next_k(kp, open_m);
    }
    grouped_rounds += rounds;
    grouped_exhausted += exhausted;
}

void Index::group_cap_device(Workspace &ws, const uint64_t *d_ids, const float *d_dists, const uint64_t *d_counts, uint64_t nq, uint64_t ld, uint64_t k,
                             uint32_t column, uint64_t g, uint64_t *d_idx, float *d_dist, uint64_t *d_cnt) {
    hipStream_t s = ws.stream;
    VDB_REQUIRE(column < LABEL_COLUMNS && g >= 1, "grouped k-NN: bad column or group size");
    if (nq == 0) return;
    VDB_REQUIRE(nq < (1ull << 32) && k < (1ull << 31), "flat knn: too many queries or k too large");
    VDB_REQUIRE(std::min(k, ld) <= (1ull << 30) - GROUPED_TILE, "grouped k-NN: k too large");
    const size_t table1 = group_cap_scratch_bytes(1, k, ld);
    const uint64_t sub = table1 ? std::max<uint64_t>(1, std::min<uint64_t>(nq, LIST_BUDGET / table1)) : nq;
    ws.grp_aux.reserve(sizeof(uint32_t) + nq);  // [flag | done]
    if (table1) ws.grp_table.reserve(sub * table1);
    uint8_t *d_done = ws.grp_aux.as<uint8_t>() + sizeof(uint32_t);
    ids_ok(ws, s, ws.grp_aux.as<uint32_t>(), "group cap: a list holds an id that is no row of this index (id - id_offset must be below len)",
           [&](uint32_t *d_flag) { launch_list_check(d_ids, d_counts, nq, ld, n, id_offset, d_flag, s); });
    const uint32_t *col = label_live[column] ? d_labels[column].as<uint32_t>() : nullptr;
    const uint32_t g32 = (uint32_t)std::min<uint64_t>(g, 0xFFFFFFFFull);
    sub_chunk_loop(
        *this, ws, nq, sub, nullptr, "group_cap", no_fetch, [&](const Chunk &c) { return double(c.nb) * ld * (LIST_PAIR_BYTES + sizeof(uint32_t)); },
        [&](const Chunk &c) {
            launch_group_cap(d_ids + c.c0 * ld, d_dists + c.c0 * ld, d_counts + c.c0, c.nb, ld, col, n, id_offset, (uint32_t)k, g32, ws.grp_table.as<uint32_t>(),
                             nullptr, d_idx + c.c0 * k, d_dist + c.c0 * k, d_cnt + c.c0, d_done + c.c0, s);
        });
    end_call(*this, ws);
}

// ---- Flat: diversified k-NN, maximal marginal relevance over the fetch_k nearest allowed rows (k_mmr.hip, mmr_plan.hpp; 4.1u) ------------
// The candidates of a query are a PREFIX of its order of fixed length, so one round is the whole call: the exact sorted list of
// kp = min(fetch_k, longest allowed set) rows per query (a query with fewer allowed rows gets a shorter count), then the selection.
void Index::flat_knn_mmr_device(Workspace &ws, const float *d_q, uint64_t nq, uint64_t k, uint64_t fetch_k, float lambda, const RowMask *const *masks,
                                uint64_t n_masks, const uint32_t *mask_of, uint64_t *d_idx, float *d_dist, uint64_t *d_cnt) {
    hipStream_t s = ws.stream;
    require_f32_rows(*this);
    VDB_REQUIRE(mmr_check_args(k, fetch_k, lambda) == nullptr, "mmr: bad k, fetch_k or lambda");
    if (nq == 0) return;
    VDB_REQUIRE(nq < (1ull << 31), "flat knn: too many queries");
    mmr_queries += nq;
    if (k == 0) return zero_counts(ws, d_cnt, nq);
    const Allowed all{masks, n_masks, mask_of};
    const uint64_t kp = mmr_list_len(fetch_k, max_allowed(*this, all, nq));
    const uint64_t sub = mmr_sub_chunk(nq, kp);
    const Lists l = reserve_lists(*this, ws, sub, kp, n_masks);
    sub_chunk_loop(
        *this, ws, nq, sub, nullptr, "mmr_select", [&](const Chunk &c) { fetch_lists(*this, ws, d_q + c.c0 * dim, c.nb, all, c.c0, l); },
        [&](const Chunk &c) { return double(c.nb) * kp * (LIST_PAIR_BYTES + dim * sizeof(float)); },
        [&](const Chunk &c) {
            launch_mmr_select(l.ids, l.dist, l.cnt, c.nb, kp, d_rows.as<float>(), d_sq.as<float>(), n, (uint32_t)dim, dist != 0, id_offset, (uint32_t)k, lambda,
                              nullptr, d_idx + c.c0 * k, d_dist + c.c0 * k, d_cnt + c.c0, s);
        });
    end_call(*this, ws);
}

void Index::mmr_select_device(Workspace &ws, const uint64_t *d_ids, const float *d_dists, const uint64_t *d_counts, uint64_t nq, uint64_t ld, uint64_t k,
                              float lambda, uint64_t *d_idx, float *d_dist, uint64_t *d_cnt) {
    hipStream_t s = ws.stream;
    require_f32_rows(*this);
    VDB_REQUIRE(mmr_check_args(k, ld, lambda) == nullptr, "mmr: bad k, ld or lambda");
    if (nq == 0) return;
    VDB_REQUIRE(nq < (1ull << 31), "flat knn: too many queries");
    if (k == 0) return zero_counts(ws, d_cnt, nq);  // (ld == 0 implies it)
    ws.grp_aux.reserve(sizeof(uint32_t));
    ids_ok(ws, s, ws.grp_aux.as<uint32_t>(), "mmr select: a list holds an id that is no row of this index (id - id_offset must be below len)",
           [&](uint32_t *d_flag) { launch_list_check(d_ids, d_counts, nq, ld, n, id_offset, d_flag, s); });
    sub_chunk_loop(
        *this, ws, nq, nq, nullptr, "mmr_select", no_fetch, [&](const Chunk &c) { return double(c.nb) * ld * (LIST_PAIR_BYTES + dim * sizeof(float)); },
        [&](const Chunk &) {
            launch_mmr_select(d_ids, d_dists, d_counts, nq, ld, d_rows.as<float>(), d_sq.as<float>(), n, (uint32_t)dim, dist != 0, id_offset, (uint32_t)k, lambda,
                              nullptr, d_idx, d_dist, d_cnt, s);
        });
    end_call(*this, ws);
}

// ---- Flat: search by example rows (k_like.hip, like_plan.hpp; 4.1v) ----------------------------------------------------------------------
// The answer of a query is a prefix of its order with the examples taken out, and a list of k + e_max rows always holds it: one round is
// the whole call.  The query vectors of a sub-chunk live in grp_q; the caller keeps the example lists in grp_table and the flag of the id
// check is in grp_aux -- none of which the list calls touch.
void Index::like_queries_device(Workspace &ws, const LikeLists &ll, uint64_t q0, uint64_t nq, float *d_out) {
    require_f32_rows(*this);
    if (nq == 0) return;
    prof_begin(ws, "like_build", double(nq) * dim * sizeof(float));
    launch_like_build(ll.pos_ids, ll.pos_lims + q0, ll.neg_ids, ll.neg_lims ? ll.neg_lims + q0 : nullptr, ll.global_ids, nq, d_rows.as<float>(), n,
                      (uint32_t)dim, id_offset, d_out, ws.stream);
    prof_end(ws);
}

void Index::flat_knn_like_device(Workspace &ws, const LikeLists &ll, uint64_t q0, uint64_t nq, uint64_t k, bool exclude, const RowMask *const *masks,
                                 uint64_t n_masks, const uint32_t *mask_of, uint64_t *d_idx, float *d_dist, uint64_t *d_cnt) {
    hipStream_t s = ws.stream;
    require_f32_rows(*this);
    if (nq == 0) return;
    VDB_REQUIRE(nq < (1ull << 31) && k < (1ull << 31), "flat knn: too many queries or k too large");
    like_queries += nq;
    if (k == 0) return zero_counts(ws, d_cnt, nq);
    const Allowed all{masks, n_masks, mask_of};
    const uint64_t kp = like_list_len(k, ll.e_max, exclude, max_allowed(*this, all, nq));
    const uint64_t sub = like_sub_chunk(nq, kp);
    ws.grp_q.reserve(sub * dim * sizeof(float));
    const Lists l = reserve_lists(*this, ws, sub, kp, n_masks);
    float *l_q = ws.grp_q.as<float>();
    sub_chunk_loop(
        *this, ws, nq, sub, nullptr, "like_drop",
        [&](const Chunk &c) {
            like_queries_device(ws, ll, q0 + c.c0, c.nb, l_q);
            fetch_lists(*this, ws, l_q, c.nb, all, c.c0, l);
        },
        [&](const Chunk &c) { return double(c.nb) * kp * LIST_PAIR_BYTES; },
        [&](const Chunk &c) {
            const uint64_t *pl = exclude ? ll.pos_lims + q0 + c.c0 : nullptr;
            const uint64_t *nl = exclude && ll.neg_lims ? ll.neg_lims + q0 + c.c0 : nullptr;
            launch_like_drop(l.ids, l.dist, l.cnt, c.nb, kp, ll.pos_ids, pl, ll.neg_ids, nl, ll.global_ids, id_offset, (uint32_t)k, d_idx + c.c0 * k,
                             d_dist + c.c0 * k, d_cnt + c.c0, s);
        });
    end_call(*this, ws);
}

void Index::like_check_ids_device(Workspace &ws, const uint64_t *d_a, uint64_t ma, const uint64_t *d_b, uint64_t mb) {
    if (ma + mb == 0) return;
    hipStream_t s = ws.stream;
    ws.grp_aux.reserve(sizeof(uint32_t));
    ids_ok(ws, s, ws.grp_aux.as<uint32_t>(), "like: a list holds an id that is no row of this index (id - id_offset must be below len)", [&](uint32_t *d_flag) {
        launch_fetch_check(d_a, ma, n, id_offset, d_flag, num_cu, s);
        launch_fetch_check(d_b, mb, n, id_offset, d_flag, num_cu, s);
    });
}

void Index::drop_listed_device(Workspace &ws, const uint64_t *d_ids, const float *d_dists, const uint64_t *d_counts, uint64_t nq, uint64_t ld, uint64_t k,
                               const uint64_t *d_drop_lims, const uint64_t *d_drop_ids, uint64_t n_drop, uint64_t *d_idx, float *d_dist,
                               uint64_t *d_cnt) {
    hipStream_t s = ws.stream;
    if (nq == 0) return;
    VDB_REQUIRE(nq < (1ull << 31) && k < (1ull << 31), "drop listed: too many queries or k too large");
    if (k == 0) return zero_counts(ws, d_cnt, nq);
    ws.grp_aux.reserve(sizeof(uint32_t));
    ids_ok(ws, s, ws.grp_aux.as<uint32_t>(), "drop listed: a list holds an id that is no row of this index (id - id_offset must be below len)",
           [&](uint32_t *d_flag) {
               launch_list_check(d_ids, d_counts, nq, ld, n, id_offset, d_flag, s);
               if (n_drop) launch_fetch_check(d_drop_ids, n_drop, n, id_offset, d_flag, num_cu, s);
           });
    sub_chunk_loop(*this, ws, nq, nq, nullptr, "like_drop", no_fetch, [&](const Chunk &c) { return double(c.nb) * ld * LIST_PAIR_BYTES; }, [&](const Chunk &) {
        launch_like_drop(d_ids, d_dists, d_counts, nq, ld, d_drop_ids, d_drop_lims, nullptr, nullptr, true, id_offset, (uint32_t)k, d_idx, d_dist, d_cnt, s);
    });
    end_call(*this, ws);
}

// ---- Flat: fused multi-query search, several lists per question joined on the device (k_fuse.hip, fuse_plan.hpp; 4.1w) --------------------
// The candidates of a sub-query are a PREFIX of its order of fixed length, so one round is the whole call: the exact sorted lists of
// kp = min(fetch_k, longest allowed set) rows of every sub-query of a sub-chunk from ONE list call, then ONE fusion launch.  The kernel's
// scratch lives in grp_table, [flag | limits | weights] in grp_aux -- which the list calls do not touch.
struct FuseUpload {
    const uint64_t *lims;
    const float *weights;
};
// [u64 flag word | lims rebased to 0 | weights] into ws.grp_aux with one copy out of `blob`, which the caller keeps until the stream has been
// waited for
static FuseUpload fuse_upload(Workspace &ws, std::vector<char> &blob, const uint64_t *lims, uint64_t nq, const float *weights) {
    const uint64_t nl = lims[nq] - lims[0];
    const size_t off_l = sizeof(uint64_t), off_w = off_l + (nq + 1) * sizeof(uint64_t);
    blob.assign(off_w + (weights ? nl * sizeof(float) : 0), 0);
    uint64_t *hl = reinterpret_cast<uint64_t *>(blob.data() + off_l);
    for (uint64_t q = 0; q <= nq; q++) hl[q] = lims[q] - lims[0];
    if (weights) std::memcpy(blob.data() + off_w, weights, nl * sizeof(float));
    ws.grp_aux.reserve(blob.size());
    VDB_HIP(hipMemcpyAsync(ws.grp_aux.p, blob.data(), blob.size(), hipMemcpyHostToDevice, ws.stream));
    char *d = ws.grp_aux.as<char>();
    return {reinterpret_cast<const uint64_t *>(d + off_l), weights ? reinterpret_cast<const float *>(d + off_w) : nullptr};
}

void Index::flat_knn_fused_device(Workspace &ws, const float *d_q, const uint64_t *lims, uint64_t nq, uint64_t k, uint64_t fetch_k, int mode,
                                  const float *weights, float rrf_c, const RowMask *const *masks, uint64_t n_masks, const uint32_t *mask_of,
                                  uint64_t *d_idx, float *d_dist, uint64_t *d_cnt) {
    hipStream_t s = ws.stream;
    require_f32_rows(*this);
    if (nq == 0) return;
    const uint64_t nl = lims[nq] - lims[0];
    fused_queries += nq;
    fused_lists += nl;
    if (k == 0) return zero_counts(ws, d_cnt, nq);
    const Allowed all{masks, n_masks, mask_of};
    const uint64_t s_max = fuse_s_max(lims, nq);
    const uint64_t kp = fuse_list_len(fetch_k, max_allowed(*this, all, nl));
    const uint32_t lg = fuse_table_lg(s_max, kp);
    const uint64_t sub = fuse_sub_chunk(nq, s_max, kp);
    const Lists l = reserve_lists(*this, ws, std::min(nl, sub * s_max), kp, n_masks);
    if (const size_t tb = fuse_scratch_bytes(sub, lg)) ws.grp_table.reserve(tb);
    std::vector<char> blob;
    const FuseUpload up = fuse_upload(ws, blob, lims, nq, weights);
    sub_chunk_loop(
        *this, ws, nq, sub, lims, "fuse_lists", [&](const Chunk &c) { fetch_lists(*this, ws, d_q + c.j0 * dim, c.nj, all, c.j0, l); },
        [&](const Chunk &c) { return double(c.nj) * kp * LIST_PAIR_BYTES; },
        [&](const Chunk &c) {
            launch_fuse_lists(l.ids, l.dist, l.cnt, c.nb, kp, up.lims + c.c0, c.j0, up.weights, mode, rrf_c, id_offset, (uint32_t)k, lg,
                              ws.grp_table.as<uint32_t>(), d_idx + c.c0 * k, d_dist + c.c0 * k, d_cnt + c.c0, s);
        });
    end_call(*this, ws);  // (`blob` is pageable memory: alive until here)
}

void Index::fuse_lists_device(Workspace &ws, const uint64_t *d_ids, const float *d_dists, const uint64_t *d_counts, const uint64_t *lims, uint64_t nq,
                              uint64_t ld, uint64_t k, int mode, const float *weights, float rrf_c, uint64_t *d_idx, float *d_dist, uint64_t *d_cnt) {
    hipStream_t s = ws.stream;
    require_f32_rows(*this);
    if (nq == 0) return;
    VDB_REQUIRE(nq < (1ull << 31) && k < (1ull << 31), "fuse lists: too many fused queries or k too large");
    if (k == 0 || ld == 0) {
        if (k) {
            VDB_HIP(hipMemsetAsync(d_idx, 0, nq * k * sizeof(uint64_t), s));
            VDB_HIP(hipMemsetAsync(d_dist, 0, nq * k * sizeof(float), s));
        }
        return zero_counts(ws, d_cnt, nq);
    }
    const uint64_t s_max = fuse_s_max(lims, nq);
    const uint32_t lg = fuse_table_lg(s_max, ld);
    const uint64_t sub = fuse_sub_chunk(nq, s_max, ld, false);
    if (const size_t tb = fuse_scratch_bytes(sub, lg)) ws.grp_table.reserve(tb);
    std::vector<char> blob;
    const FuseUpload up = fuse_upload(ws, blob, lims, nq, weights);
    ids_ok(
        ws, s, ws.grp_aux.as<uint32_t>(), "fuse lists: a list holds an id that is no row of this index (id - id_offset must be below len)",
        [&](uint32_t *d_flag) { launch_list_check(d_ids, d_counts, lims[nq], ld, n, id_offset, d_flag, s); }, true);  // (the upload's first word: zero)
    sub_chunk_loop(
        *this, ws, nq, sub, lims, "fuse_lists", no_fetch, [&](const Chunk &c) { return double(c.nj) * ld * LIST_PAIR_BYTES; },
        [&](const Chunk &c) {
            launch_fuse_lists(d_ids, d_dists, d_counts, c.nb, ld, up.lims + c.c0, 0, up.weights, mode, rrf_c, id_offset, (uint32_t)k, lg,
                              ws.grp_table.as<uint32_t>(), d_idx + c.c0 * k, d_dist + c.c0 * k, d_cnt + c.c0, s);
        });
    end_call(*this, ws);
}

// ---- Flat: document-level fused search, the lists joined by the value of a label column (k_fuse_groups.hip, fuse_groups_plan.hpp; 4.1z) ---
// The fused search with another kernel behind the same list call: the table is keyed by the row's GROUP, its slot is wider, so the
// sub-chunk and the scratch come from fuse_groups_plan.hpp.  k == 0: nothing is fetched or ranked -- zero counts, zero `exact`.
static void zero_exact(Workspace &ws, uint8_t *d_exact, uint64_t nq) {
    if (d_exact) VDB_HIP(hipMemsetAsync(d_exact, 0, nq, ws.stream));
}

void Index::flat_knn_fused_groups_device(Workspace &ws, const float *d_q, const uint64_t *lims, uint64_t nq, uint64_t k, uint64_t fetch_k, int mode,
                                         const float *weights, float rrf_c, uint32_t column, const RowMask *const *masks, uint64_t n_masks,
                                         const uint32_t *mask_of, uint64_t *d_idx, float *d_dist, uint64_t *d_cnt, uint8_t *d_exact) {
    hipStream_t s = ws.stream;
    require_f32_rows(*this);
    VDB_REQUIRE(column < LABEL_COLUMNS, "fuse groups: bad column");
    if (nq == 0) return;
    const uint64_t nl = lims[nq] - lims[0];
    fused_groups_queries += nq;
    fused_groups_lists += nl;
    if (k == 0) {
        zero_exact(ws, d_exact, nq);
        return zero_counts(ws, d_cnt, nq);
    }
    const Allowed all{masks, n_masks, mask_of};
    const uint64_t s_max = fuse_s_max(lims, nq);
    const uint64_t max_m = max_allowed(*this, all, nl);
    const uint64_t kp = fuse_list_len(fetch_k, max_m);
    // a list of fetch_k entries may have left rows behind -- unless fetch_k reaches the longest allowed set: every list is whole then
    const uint64_t trunc_len = fetch_k >= max_m ? kp + 1 : fetch_k;
    const uint32_t lg = fuse_table_lg(s_max, kp);
    const uint64_t sub = fuse_groups_sub_chunk(nq, s_max, kp);
    const Lists l = reserve_lists(*this, ws, std::min(nl, sub * s_max), kp, n_masks);
    if (const size_t tb = fuse_groups_scratch_bytes(sub, lg)) ws.grp_table.reserve(tb);
    std::vector<char> blob;
    const FuseUpload up = fuse_upload(ws, blob, lims, nq, weights);
    const uint32_t *col = label_live[column] ? d_labels[column].as<uint32_t>() : nullptr;
    sub_chunk_loop(
        *this, ws, nq, sub, lims, "fuse_groups", [&](const Chunk &c) { fetch_lists(*this, ws, d_q + c.j0 * dim, c.nj, all, c.j0, l); },
        [&](const Chunk &c) { return double(c.nj) * kp * (LIST_PAIR_BYTES + sizeof(uint32_t)); },
        [&](const Chunk &c) {
            launch_fuse_groups(l.ids, l.dist, l.cnt, c.nb, kp, up.lims + c.c0, c.j0, up.weights, col, n, mode, rrf_c, id_offset, trunc_len, (uint32_t)k, lg,
                               ws.grp_table.as<uint32_t>(), d_idx + c.c0 * k, d_dist + c.c0 * k, d_cnt + c.c0, d_exact ? d_exact + c.c0 : nullptr, s);
        });
    end_call(*this, ws);  // (`blob` is pageable memory: alive until here)
}

void Index::fuse_groups_device(Workspace &ws, const uint64_t *d_ids, const float *d_dists, const uint64_t *d_counts, const uint64_t *lims, uint64_t nq,
                               uint64_t ld, uint64_t k, int mode, const float *weights, float rrf_c, uint32_t column, uint64_t trunc_len,
                               uint64_t *d_idx, float *d_dist, uint64_t *d_cnt, uint8_t *d_exact) {
    hipStream_t s = ws.stream;
    require_f32_rows(*this);
    VDB_REQUIRE(column < LABEL_COLUMNS && trunc_len >= 1, "fuse groups: bad column or trunc_len");
    if (nq == 0) return;
    VDB_REQUIRE(nq < (1ull << 31) && k < (1ull << 31), "fuse groups: too many fused queries or k too large");
    if (k == 0) {
        zero_exact(ws, d_exact, nq);
        return zero_counts(ws, d_cnt, nq);
    }
    const uint64_t s_max = fuse_s_max(lims, nq);
    const uint32_t lg = fuse_table_lg(s_max, ld);
    const uint64_t sub = fuse_groups_sub_chunk(nq, s_max, ld, false);
    if (const size_t tb = fuse_groups_scratch_bytes(sub, lg)) ws.grp_table.reserve(tb);
    std::vector<char> blob;
    const FuseUpload up = fuse_upload(ws, blob, lims, nq, weights);
    if (ld)
        ids_ok(
            ws, s, ws.grp_aux.as<uint32_t>(), "fuse groups: a list holds an id that is no row of this index (id - id_offset must be below len)",
            [&](uint32_t *d_flag) { launch_list_check(d_ids, d_counts, lims[nq], ld, n, id_offset, d_flag, s); }, true);  // (the upload's first word: zero)
    const uint32_t *col = label_live[column] ? d_labels[column].as<uint32_t>() : nullptr;
    sub_chunk_loop(
        *this, ws, nq, sub, lims, "fuse_groups", no_fetch, [&](const Chunk &c) { return double(c.nj) * ld * (LIST_PAIR_BYTES + sizeof(uint32_t)); },
        [&](const Chunk &c) {  // (ld == 0: every list is empty and nothing of d_ids / d_dists is read)
            launch_fuse_groups(d_ids, d_dists, d_counts, c.nb, ld, up.lims + c.c0, 0, up.weights, col, n, mode, rrf_c, id_offset, trunc_len, (uint32_t)k, lg,
                               ws.grp_table.as<uint32_t>(), d_idx + c.c0 * k, d_dist + c.c0 * k, d_cnt + c.c0, d_exact ? d_exact + c.c0 : nullptr, s);
        });
    end_call(*this, ws);
}

}  // namespace vdb
