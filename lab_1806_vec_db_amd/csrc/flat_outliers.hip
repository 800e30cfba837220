// flat_outliers.hip -- the k-NN self-join of an index's own rows and the outlier scores on its graph (docs/DESIGN_flat.md 4.1ah): the drivers
// Index::flat_knn_graph_device and Index::flat_outliers_device, and the score stages alone over a caller's graph, Index::lof_lists_device.
// outlier_plan.hpp states the rule, checks the arguments and lays the chunks out; k_outlier.hip holds the kernels.
// The walk is the range self-join's (self_join.hpp) with the k-NN search in the place of the range search: the allowed rows are the
// queries, a chunk at a time in ascending row order, where they lie or gathered into ws.grp_q under a mask.  Per chunk ONE call of the
// existing search at kp = min(k + 1, m) -- flat_knn_device, or flat_knn_masked_device under the call's mask, whose counters advance as for
// that call -- into ws.grp_ids / grp_dist / grp_cnt, which the search does not touch, then ONE k_knn_self_pack launch on the same stream.
// The graph stays resident for the two score launches: 8 B x m x k (160 MB at 1M x 20).
#include <algorithm>

#include "index.hpp"
#include "outlier_plan.hpp"

namespace vdb {

namespace {

// where k_knn_self_pack writes: all [m][k] / [m] by position but kdist, [n] by row; nullptr: not wanted (nd always is)
struct GraphOut {
    uint32_t *nbr = nullptr;
    uint64_t *ids = nullptr;
    float *nd = nullptr;
    uint32_t *cnt32 = nullptr;
    uint64_t *cnt64 = nullptr;
    float *kdist = nullptr;
};

void walk_knn_graph(Index &ix, Workspace &ws, const OutlierPlan &plan, uint64_t k, const RowMask *mask, const GraphOut &g) {
    hipStream_t s = ws.stream;
    const uint64_t dim = ix.dim, kp = plan.kp;
    if (plan.m == 0) return;
    // every buffer of the walk before its first launch: a later, larger reserve would free a buffer in use
    ws.grp_ids.reserve(plan.chunk_len * kp * sizeof(uint64_t));
    ws.grp_dist.reserve(plan.chunk_len * kp * sizeof(float));
    ws.grp_cnt.reserve(plan.chunk_len * sizeof(uint64_t));
    if (plan.gather) ws.grp_q.reserve(plan.chunk_len * dim * sizeof(float));
    uint64_t *l_ids = ws.grp_ids.as<uint64_t>(), *l_cnt = ws.grp_cnt.as<uint64_t>();
    float *l_dist = ws.grp_dist.as<float>();
    for (uint64_t c = 0; c < plan.n_chunks; c++) {
        const uint64_t a = c * plan.chunk_len, nb = c + 1 == plan.n_chunks ? plan.last_len : plan.chunk_len;
        const uint32_t *src32 = mask ? mask->d_ids.as<uint32_t>() + a : nullptr;
        if (mask) {
            launch_rows_gather(ix.d_rows.p, dim * sizeof(float), src32, false, 0, ws.grp_q.p, nb, ix.num_cu, s);
            ix.flat_knn_masked_device(ws, ws.grp_q.as<float>(), nb, kp, *mask, l_ids, l_dist, l_cnt);
        } else
            ix.flat_knn_device(ws, ix.d_rows.as<float>() + a * dim, nb, kp, l_ids, l_dist, l_cnt);  // the rows are the queries, where they lie
        ix.prof_begin(ws, "knn_self_pack", double(nb) * (kp * LIST_PAIR_BYTES + k * 2 * sizeof(uint32_t)));
        launch_knn_self_pack(l_ids, l_dist, l_cnt, nb, kp, src32, a, ix.id_offset, (uint32_t)k, (uint32_t)plan.kk, g.nbr, g.ids, g.nd, g.cnt32, g.cnt64,
                             g.kdist, ix.num_cu, s);
        ix.prof_end(ws);
    }
    VDB_SYNC(s);  // (the lists of the last chunk are free again)
}

OutlierPlan checked_plan(const Index &ix, uint64_t k, const RowMask *mask) {
    if (mask) ix.check_mask(*mask);
    const uint64_t m = mask ? mask->m : ix.n;
    const std::string bad = outlier_check_args(ix.n, m, mask != nullptr, ix.elem_u8, k, ix.dup_chunk);
    VDB_REQUIRE(bad.empty(), bad);
    return outlier_plan(ix.n, ix.dim, mask != nullptr, m, k, ix.dup_chunk);
}

// stages 2 and 3 over a resident graph: lrd64 is reserved here; kdist [rows] is the caller's
void score_graph(Index &ix, Workspace &ws, const uint32_t *nbr, const float *nd, const uint32_t *cnt, const uint32_t *src32, uint64_t m, uint64_t k,
                 uint64_t rows, const float *kdist, float *d_kdist, float *d_lrd, float *d_lof) {
    DevBuf lrd64;
    lrd64.reserve(std::max<uint64_t>(rows, 1) * sizeof(double));
    ix.prof_begin(ws, "lof_stages", double(m) * k * (2 * sizeof(uint32_t) + sizeof(float) + (d_lof ? sizeof(uint32_t) + sizeof(double) : 0)));
    launch_lof_stages(nbr, nd, cnt, src32, m, (uint32_t)k, kdist, lrd64.as<double>(), d_kdist, d_lrd, d_lof, ix.num_cu, ws.stream);
    ix.prof_end(ws);
    VDB_SYNC(ws.stream);  // (lrd64 goes out of scope)
}

}  // namespace

void Index::flat_knn_graph_device(Workspace &ws, uint64_t k, const RowMask *mask, uint64_t *d_ids, float *d_dists, uint64_t *d_counts) {
    const OutlierPlan plan = checked_plan(*this, k, mask);
    GraphOut g;
    g.ids = d_ids, g.nd = d_dists, g.cnt64 = d_counts;
    walk_knn_graph(*this, ws, plan, k, mask, g);
    knn_graph_calls += 1;
    knn_graph_chunks += plan.n_chunks;
}

void Index::flat_outliers_device(Workspace &ws, uint64_t k, const RowMask *mask, float *d_kdist, float *d_lrd, float *d_lof) {
    const OutlierPlan plan = checked_plan(*this, k, mask);
    if (plan.m == 0) {
        knn_graph_calls += 1;
        return;
    }
    DevBuf nbr, nd, cnt, kdist;
    nbr.reserve(plan.m * k * sizeof(uint32_t));
    nd.reserve(plan.m * k * sizeof(float));
    cnt.reserve(plan.m * sizeof(uint32_t));
    kdist.reserve(n * sizeof(float));
    GraphOut g;
    g.nbr = nbr.as<uint32_t>(), g.nd = nd.as<float>(), g.cnt32 = cnt.as<uint32_t>(), g.kdist = kdist.as<float>();
    walk_knn_graph(*this, ws, plan, k, mask, g);
    score_graph(*this, ws, g.nbr, g.nd, g.cnt32, mask ? mask->d_ids.as<uint32_t>() : nullptr, plan.m, k, n, g.kdist, d_kdist, d_lrd, d_lof);
    knn_graph_calls += 1;
    knn_graph_chunks += plan.n_chunks;
}

void Index::lof_lists_device(Workspace &ws, const uint32_t *d_nbr, const float *d_nd, const uint32_t *d_cnt, uint64_t m, uint64_t k, float *d_kdist,
                             float *d_lrd, float *d_lof) {
    hipStream_t s = ws.stream;
    const std::string bad = outlier_check_k(k);
    VDB_REQUIRE(bad.empty(), bad);
    VDB_REQUIRE(m < (1ull << 32), "lof lists: too many lists for one call");
    if (m == 0) return;
    VDB_REQUIRE(d_nbr && d_nd && d_cnt, "lof lists: null argument");
    DevBuf kdist;  // [flag | kdist f32 x m]
    kdist.reserve(DEVBUF_ALIGN + m * sizeof(float));
    ids_ok(ws, s, kdist.as<uint32_t>(), "lof lists: a count passes k, or a list holds an id that is no list of the call (it must be below m)",
           [&](uint32_t *d_flag) { launch_lof_check(d_nbr, d_cnt, m, (uint32_t)k, m, d_flag, num_cu, s); });
    float *kd = reinterpret_cast<float *>(kdist.as<char>() + DEVBUF_ALIGN);
    launch_lof_kdist(d_nd, d_cnt, m, (uint32_t)k, kd, num_cu, s);
    score_graph(*this, ws, d_nbr, d_nd, d_cnt, nullptr, m, k, m, kd, d_kdist, d_lrd, d_lof);
}

}  // namespace vdb
