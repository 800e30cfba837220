// flat_silhouette.hip -- silhouette scoring of an index's labelled rows (docs/DESIGN_flat.md 4.1aj): Index::flat_silhouette_device.  The rule
// is stated once in include/vdbhip.h; silhouette_plan.hpp checks the arguments and lays out tiles and scratch, k_silhouette.hip holds the
// kernels.  The (code, row) order is made on the HOST from one read-back of the candidates' codes (4 B per candidate, LABEL_NONE where the
// row is not scored): O(m log m) against the O(m^2 dim) pair pass, and it gives the cluster count before any output is written.  No
// pairwise arithmetic happens on the host.  Everything else is one chain of launches on the workspace's stream.
#include <algorithm>
#include <string>
#include <vector>

#include "index.hpp"

namespace vdb {

void Index::flat_silhouette_device(Workspace &ws, uint32_t col, const RowMask *mask, uint32_t flags, float *d_out_s, double *d_out_mean, uint64_t *out_m,
                                   uint64_t *out_clusters) {
    hipStream_t s = ws.stream;
    if (mask) check_mask(*mask);
    const uint64_t cand = mask ? mask->m : n;
    const bool cosine = dist != 0;
    const std::string bad = sil_check_args(n, dim, elem_u8, cosine, flags, col, col < LABEL_COLUMNS && label_live[col], mask != nullptr, cand);
    VDB_REQUIRE(bad.empty(), bad);
    const uint32_t *ids = mask ? mask->d_ids.as<uint32_t>() : nullptr;
    const float *X = d_rows.as<float>();
    DevBuf key, nrm;
    std::vector<uint64_t> order;  // (code << 32 | candidate) of the scored rows, ascending: the candidates ascend with the rows
    if (cand) {
        key.reserve(cand * sizeof(uint32_t));
        nrm.reserve(cand * sizeof(double));
        uint32_t *h_key = static_cast<uint32_t *>(ws.pinned(cand * sizeof(uint32_t)));
        prof_begin(ws, "sil_prepare", double(cand) * (dim + 1) * sizeof(float));
        launch_sil_prepare(X, ids, label_col(col), cand, (uint32_t)dim, cosine, key.as<uint32_t>(), nrm.as<double>(), s);
        prof_end(ws);
        VDB_HIP(hipMemcpyAsync(h_key, key.p, cand * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        VDB_SYNC(s);
        for (uint64_t p = 0; p < cand; p++)
            if (h_key[p] != LABEL_NONE) order.push_back(uint64_t(h_key[p]) << 32 | p);
        std::sort(order.begin(), order.end());
    }
    std::vector<uint64_t> sizes;
    for (size_t i = 0; i < order.size(); i++) {
        if (i == 0 || (order[i] >> 32) != (order[i - 1] >> 32)) sizes.push_back(0);
        sizes.back() += 1;
    }
    const std::string few = sil_check_clusters(order.size(), sizes.size());
    VDB_REQUIRE(few.empty(), few);
    const SilPlan p = sil_plan(sizes.data(), sizes.size(), dim, cand);
    std::vector<uint32_t> h_ord(p.padded, LABEL_NONE), h_tile_cl(p.tiles), h_size(p.clusters);
    for (uint64_t c = 0, at = 0; c < p.clusters; c++) {
        h_size[c] = (uint32_t)sizes[c];
        for (uint64_t i = 0; i < sizes[c]; i++) h_ord[p.first_tile[c] * SIL_TILE + i] = (uint32_t)order[at++];
        for (uint64_t t = p.first_tile[c]; t < p.first_tile[c + 1]; t++) h_tile_cl[t] = (uint32_t)c;
    }
    DevBuf ord, orow, onorm, tile_cl, cl_size, sum_a, min_b, s64;
    ord.reserve(p.padded * sizeof(uint32_t));
    orow.reserve(p.padded * sizeof(uint32_t));
    onorm.reserve(p.padded * sizeof(double));
    tile_cl.reserve(p.tiles * sizeof(uint32_t));
    cl_size.reserve(p.clusters * sizeof(uint32_t));
    sum_a.reserve(p.padded * sizeof(double));
    min_b.reserve(p.padded * sizeof(double));
    s64.reserve(p.padded * sizeof(double));
    VDB_HIP(hipMemcpyAsync(ord.p, h_ord.data(), p.padded * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    VDB_HIP(hipMemcpyAsync(tile_cl.p, h_tile_cl.data(), p.tiles * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    VDB_HIP(hipMemcpyAsync(cl_size.p, h_size.data(), p.clusters * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    prof_begin(ws, "sil_prepare", double(p.padded) * 24.0 + double(n) * sizeof(float));  // (the stage's second half: gather and NaN fill)
    launch_sil_gather(ord.as<uint32_t>(), ids, nrm.as<double>(), p.padded, orow.as<uint32_t>(), onorm.as<double>(), d_out_s, n, s);
    prof_end(ws);
    prof_begin(ws, "sil_pairs", double(p.tiles) * double(p.padded + SIL_TILE) * dim * sizeof(float));  // a row block reads itself and every tile
    launch_sil_pairs(X, (uint32_t)dim, cosine, (flags & SIL_EUCLIDEAN) != 0, p, orow.as<uint32_t>(), onorm.as<double>(), tile_cl.as<uint32_t>(),
                     cl_size.as<uint32_t>(), sum_a.as<double>(), min_b.as<double>(), s);
    prof_end(ws);
    prof_begin(ws, "sil_finish", double(p.padded) * 36.0);
    launch_sil_finish(p, orow.as<uint32_t>(), tile_cl.as<uint32_t>(), cl_size.as<uint32_t>(), sum_a.as<double>(), min_b.as<double>(), d_out_s,
                      s64.as<double>(), d_out_mean, s);
    prof_end(ws);
    VDB_SYNC(s);
    *out_m = p.m;
    *out_clusters = p.clusters;
    silhouette_calls += 1;
    silhouette_rows += p.m;
}

}  // namespace vdb
