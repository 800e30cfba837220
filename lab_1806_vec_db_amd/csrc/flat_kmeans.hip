// flat_kmeans.hip -- k-means clustering of an index's own rows (docs/DESIGN_flat.md 4.1ad): the Lloyd driver Index::flat_kmeans_device and the
// assignment step alone, Index::kmeans_assign_device.  The rule, stated once in include/vdbhip.h: rows go to the centroid with the smallest
// (strict-fold pair distance, centroid id); a centroid becomes the f64 mean of its members, summed in ascending row order, rounded to f32
// once; a cluster without members keeps its centroid.  kmeans_plan.hpp checks the arguments and lays out the scratch, k_kmeans.hip holds
// the kernels.  One iteration is one chain of launches on the workspace's stream and ONE read-back: rows that changed cluster, inertia,
// rows the matrix pass left to the exact fold.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "index.hpp"
#include "pq_hnsw.hpp"

namespace vdb {

namespace {

// the device state of one call (kmeans_plan's scratch_bytes)
struct KmState {
    DevBuf planes, csq, cent, unsure, prev, best, count, offsets, sizes, tmp, members, hist, partial, counters;
    uint64_t *cnt() const { return counters.as<uint64_t>(); }
    void reserve(const Index &ix, uint64_t m, uint64_t c) {
        const KmeansPlan p = kmeans_plan(ix.n, ix.dim, m, c);
        const uint64_t m1 = std::max<uint64_t>(m, 1), n1 = std::max<uint64_t>(ix.n, 1);
        planes.reserve(p.plane_bytes);
        csq.reserve(p.cent_tiles * KM_CENT_TILE * sizeof(float));
        cent.reserve(c * ix.dim * sizeof(float));
        unsure.reserve(m1 * sizeof(uint32_t));
        prev.reserve(n1 * sizeof(uint32_t));
        best.reserve(n1 * sizeof(float));
        count.reserve(c * sizeof(uint32_t));
        offsets.reserve((c + 1) * sizeof(uint32_t));
        sizes.reserve(c * sizeof(uint64_t));
        tmp.reserve(m1 * sizeof(uint32_t));
        members.reserve(m1 * sizeof(uint32_t));
        hist.reserve(256 * std::max<uint64_t>(p.order_blocks, 1) * sizeof(uint32_t));
        partial.reserve(std::max<uint64_t>((m + KM_REDUCE_CHUNK - 1) / KM_REDUCE_CHUNK, 1) * sizeof(double));
        counters.reserve(KM_COUNTERS * sizeof(uint64_t));
    }
};

// the assignment of every position to st.cent, exact: assign[row] and, when want_best, the exact best[row] (else best is scratch of the
// matrix pass); enqueued; counters word 0 = the unsure rows
void km_assign(Index &ix, Workspace &ws, KmState &st, const RowMask *mask, uint64_t m, uint32_t c, uint32_t *assign, float *best, bool want_best) {
    hipStream_t s = ws.stream;
    const uint32_t dim = (uint32_t)ix.dim;
    const bool cosine = ix.dist == 1;
    const uint32_t *ids = mask ? mask->d_ids.as<uint32_t>() : nullptr;
    const float *X = ix.d_rows.as<float>(), *xsq = ix.d_sq.as<float>();
    uint32_t *cmax = reinterpret_cast<uint32_t *>(st.cnt() + 3);
    VDB_HIP(hipMemsetAsync(st.counters.p, 0, KM_COUNTERS * sizeof(uint64_t), s));
    ix.prof_begin(ws, "kmeans_assign", double(m) * dim * sizeof(float));
    launch_kmeans_prep(st.cent.as<float>(), c, dim, st.planes.as<uint4>(), st.csq.as<float>(), cmax, s);
    launch_kmeans_assign(X, xsq, ids, m, dim, c, st.planes.as<uint4>(), st.csq.as<float>(), cmax, cosine, assign, best, st.unsure.as<uint32_t>(), st.cnt(),
                         s);
    ix.prof_end(ws);
    ix.prof_begin(ws, "kmeans_resolve", double(m) * dim * sizeof(float));
    launch_kmeans_resolve(X, xsq, ids, m, dim, st.cent.as<float>(), st.csq.as<float>(), c, cosine, st.unsure.as<uint32_t>(), st.cnt(), assign, best,
                          ix.num_cu, s);
    if (want_best) launch_kmeans_best(X, xsq, ids, m, dim, st.cent.as<float>(), st.csq.as<float>(), c, cosine, assign, best, s);
    ix.prof_end(ws);
}

// the rows outside a mask read KM_LABEL_NONE / NaN (all bits set, both)
void km_blank(const Index &ix, const RowMask *mask, uint32_t *assign, float *best, hipStream_t s) {
    if (!mask || ix.n == 0) return;
    if (assign) VDB_HIP(hipMemsetAsync(assign, 0xFF, ix.n * sizeof(uint32_t), s));
    if (best) VDB_HIP(hipMemsetAsync(best, 0xFF, ix.n * sizeof(float), s));
}

// min(m, 64 c) allowed rows drawn by a splitmix64 stream from `seed`, fetched by the bulk row fetch, seeded by host_kmeans with max_iter = 0
std::vector<float> km_seed(Index &ix, const RowMask *mask, uint64_t m, uint64_t c, uint64_t seed) {
    const uint64_t ns = std::min(m, KM_SEED_PER_CLUSTER * c);
    uint64_t rng = seed;
    std::vector<uint64_t> rows(ns);
    if (ns == m) {
        for (uint64_t i = 0; i < ns; i++) rows[i] = i;
    } else {  // the first ns places of a Fisher-Yates shuffle of the positions (VecSet::random_sample's walk, pq_build)
        std::vector<uint32_t> perm(m);
        for (uint64_t i = 0; i < m; i++) perm[i] = (uint32_t)i;
        for (uint64_t i = 0; i < ns; i++) {
            std::swap(perm[i], perm[i + host_splitmix64(rng) % (m - i)]);
            rows[i] = perm[i];
        }
    }
    if (mask) {
        std::vector<uint32_t> ids(m);
        VDB_HIP(hipMemcpy(ids.data(), mask->d_ids.p, m * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (auto &r : rows) r = ids[r];
    }
    std::vector<float> sample(ns * ix.dim), cent(c * ix.dim);
    ix.get_rows(rows.data(), ns, sample.data(), true);
    host_kmeans(sample.data(), ns, ix.dim, 0, ix.dim, c, /*max_iter=*/0, 0.0f, ix.dist, host_splitmix64(rng), cent.data());
    return cent;
}

}  // namespace

void Index::kmeans_assign_device(Workspace &ws, const float *d_cent, uint64_t c, const RowMask *mask, uint32_t *d_assign, float *d_best, uint64_t *unsure) {
    hipStream_t s = ws.stream;
    if (mask) check_mask(*mask);
    const uint64_t m = mask ? mask->m : n;
    const std::string bad = kmeans_check_args(n, dim, elem_u8, mask != nullptr, m, c);
    VDB_REQUIRE(bad.empty(), bad);
    *unsure = 0;
    if (m == 0) {
        km_blank(*this, mask, d_assign, d_best, s);
        VDB_SYNC(s);
        return;
    }
    KmState st;
    st.reserve(*this, m, c);
    VDB_HIP(hipMemcpyAsync(st.cent.p, d_cent, c * dim * sizeof(float), hipMemcpyDeviceToDevice, s));
    km_blank(*this, mask, d_assign, d_best, s);
    km_assign(*this, ws, st, mask, m, (uint32_t)c, d_assign, d_best ? d_best : st.best.as<float>(), d_best != nullptr);
    uint64_t *h = static_cast<uint64_t *>(ws.pinned(KM_COUNTERS * sizeof(uint64_t)));
    VDB_HIP(hipMemcpyAsync(h, st.counters.p, KM_COUNTERS * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    VDB_SYNC(s);
    *unsure = h[0];
    kmeans_rows_assigned += m;
    kmeans_unsure_rows += h[0];
}

void Index::flat_kmeans_device(Workspace &ws, uint64_t c, uint64_t max_iter, float tol, uint64_t seed, const float *init, const RowMask *mask,
                               float *d_cent, uint32_t *d_assign, uint64_t *d_sizes, uint64_t *iters, double *inertia) {
    hipStream_t s = ws.stream;
    if (mask) check_mask(*mask);
    const uint64_t m = mask ? mask->m : n;
    std::string bad = kmeans_check_args(n, dim, elem_u8, mask != nullptr, m, c);
    if (bad.empty()) bad = kmeans_check_fit(m, c);
    VDB_REQUIRE(bad.empty(), bad);
    std::vector<float> seeded;
    if (!init) {
        seeded = km_seed(*this, mask, m, c, seed);
        init = seeded.data();
    }
    KmState st;
    st.reserve(*this, m, c);
    const uint32_t *ids = mask ? mask->d_ids.as<uint32_t>() : nullptr;
    VDB_HIP(hipMemcpyAsync(st.cent.p, init, c * dim * sizeof(float), hipMemcpyHostToDevice, s));
    VDB_HIP(hipMemsetAsync(st.prev.p, 0xFF, n * sizeof(uint32_t), s));  // no row has a cluster yet
    km_blank(*this, mask, d_assign, nullptr, s);
    uint64_t *h = static_cast<uint64_t *>(ws.pinned(KM_COUNTERS * sizeof(uint64_t)));
    uint64_t done = 0, steps = 0, unsure_rows = 0;
    double now = 0.0, before = 0.0;
    for (uint64_t t = 0;; t++) {
        km_assign(*this, ws, st, mask, m, (uint32_t)c, d_assign, st.best.as<float>(), true);
        prof_begin(ws, "kmeans_update", double(m) * dim * sizeof(float));
        VDB_HIP(hipMemsetAsync(st.count.p, 0, c * sizeof(uint32_t), s));
        launch_kmeans_order(d_assign, ids, m, (uint32_t)c, st.count.as<uint32_t>(), st.offsets.as<uint32_t>(), st.sizes.as<uint64_t>(),
                            st.hist.as<uint32_t>(), st.tmp.as<uint32_t>(), st.members.as<uint32_t>(), s);
        launch_kmeans_reduce(d_assign, st.prev.as<uint32_t>(), st.best.as<float>(), ids, m, st.partial.as<double>(), st.cnt() + 1,
                             reinterpret_cast<double *>(st.cnt() + 2), s);
        VDB_HIP(hipMemcpyAsync(h, st.counters.p, KM_COUNTERS * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        VDB_SYNC(s);  // the iteration's one read-back
        steps += 1;
        unsure_rows += h[0];
        before = now;
        std::memcpy(&now, &h[2], sizeof(double));
        const bool stop = t == max_iter || (t > 0 && (h[1] == 0 || std::fabs(now - before) <= double(tol) * before));
        if (!stop) {
            launch_kmeans_update(d_rows.as<float>(), ids, (uint32_t)dim, (uint32_t)c, st.offsets.as<uint32_t>(), st.members.as<uint32_t>(),
                                 st.cent.as<float>(), s);
            VDB_HIP(hipMemcpyAsync(st.prev.p, d_assign, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
            done += 1;
        }
        prof_end(ws);
        if (stop) break;
    }
    VDB_HIP(hipMemcpyAsync(d_cent, st.cent.p, c * dim * sizeof(float), hipMemcpyDeviceToDevice, s));
    VDB_HIP(hipMemcpyAsync(d_sizes, st.sizes.p, c * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    VDB_SYNC(s);
    *iters = done;
    *inertia = now;
    kmeans_calls += 1;
    kmeans_iterations += done;
    kmeans_rows_assigned += steps * m;
    kmeans_unsure_rows += unsure_rows;
}

}  // namespace vdb
