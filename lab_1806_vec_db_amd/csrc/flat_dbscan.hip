// flat_dbscan.hip -- density clustering (DBSCAN) of an index's own rows (docs/DESIGN_flat.md 4.1ae): the driver
// Index::flat_dbscan_device over the range self-join's chunk walk (self_join.hpp, shared with flat_dups.hip) and the stage alone over a
// caller's lists, Index::dbscan_pairs_device.  dbscan_plan.hpp states the rule and checks the arguments, k_dbscan.hip holds the kernels.
// Per chunk of queries: the limits are uploaded once (by the walk), then k_dbscan_core and k_dbscan_link on the call's stream; one
// stream sync per chunk, where the range result goes out of scope, and one at the end.  ONE pass over the chunks is enough because the
// exact pair distances are symmetric bit for bit (L2Sqr: (a - b)^2 == (b - a)^2; Cosine: the dot product and the product of the norms
// commute): a pair whose other end lies in a later chunk is left to that chunk, where the kinds of both ends are final.
#include <algorithm>
#include <cstring>

#include "index.hpp"
#include "self_join.hpp"

namespace vdb {

namespace {

// the device state of one call: parent u32 [n], border u64 [n], kind u8 [n], counters [8] u64
struct DensityState {
    DevBuf parent, border, kind, counters;
    uint64_t *cnt() const { return counters.as<uint64_t>(); }
    void start(const Index &ix, const uint64_t *bits, hipStream_t s) {
        parent.reserve(ix.n * sizeof(uint32_t));
        border.reserve(ix.n * sizeof(uint64_t));
        kind.reserve(ix.n);
        counters.reserve(DBSCAN_COUNTER_BYTES);
        launch_dbscan_init(bits, ix.n, parent.as<uint32_t>(), border.as<uint64_t>(), kind.as<uint8_t>(), cnt(), ix.num_cu, s);
    }
    void chunk(Index &ix, Workspace &ws, const uint64_t *src64, const uint32_t *src32, uint64_t src_base, const uint64_t *d_lims, const uint64_t *d_ids,
               const float *d_dists, uint64_t nq, uint64_t total, uint64_t min_samples, bool more_chunks) {
        ix.prof_begin(ws, "dbscan_link", double(total) * (sizeof(uint64_t) + sizeof(float)));
        launch_dbscan_chunk(src64, src32, src_base, d_lims, d_ids, d_dists, nq, ix.id_offset, min_samples, more_chunks, kind.as<uint8_t>(),
                            parent.as<uint32_t>(), border.as<uint64_t>(), cnt(), ix.num_cu, ws.stream);
        ix.prof_end(ws);
    }
    // labels + counts, label / kind to the outputs, the five counters to stats; returns synchronised
    void finish(Index &ix, Workspace &ws, uint64_t *d_label, uint8_t *d_kind, uint64_t *stats) {
        hipStream_t s = ws.stream;
        ix.prof_begin(ws, "dbscan_labels", double(ix.n) * (sizeof(uint32_t) + 2 * sizeof(uint64_t) + 2));
        launch_dbscan_labels(parent.as<uint32_t>(), kind.as<uint8_t>(), border.as<uint64_t>(), ix.n, ix.id_offset, d_label, d_kind, cnt(), ix.num_cu, s);
        ix.prof_end(ws);
        uint64_t *h = static_cast<uint64_t *>(ws.pinned(DBSCAN_STATS * sizeof(uint64_t)));
        VDB_HIP(hipMemcpyAsync(h, counters.p, DBSCAN_STATS * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        VDB_SYNC(s);
        std::memcpy(stats, h, DBSCAN_STATS * sizeof(uint64_t));
    }
};

}  // namespace

void Index::flat_dbscan_device(Workspace &ws, float eps, uint64_t min_samples, const RowMask *mask, uint64_t *d_label, uint8_t *d_kind,
                               uint64_t *stats) {
    hipStream_t s = ws.stream;
    if (mask) check_mask(*mask);
    const uint64_t m = mask ? mask->m : n;
    const std::string bad = dbscan_check_args(n, m, mask != nullptr, eps, min_samples, dup_chunk);
    VDB_REQUIRE(bad.empty(), bad);
    if (n == 0) {
        std::fill(stats, stats + DBSCAN_STATS, uint64_t(0));
        dbscan_calls += 1;
        return;
    }
    const DbscanPlan plan = dbscan_plan(n, dim, elem_u8, mask != nullptr, m, dup_chunk);
    DensityState st;
    walk_self_join(
        *this, ws, plan.walk, dup_chunk, eps, 0, mask, [&] { st.start(*this, mask ? mask->d_bits.as<uint64_t>() : nullptr, s); },
        [&](const SelfJoinChunk &ch) {
            // the queries ascend by row: the kinds are final up to the chunk's last query row
            st.chunk(*this, ws, nullptr, ch.src32, ch.a, ch.d_lims, ch.r.idx.as<uint64_t>(), ch.r.dist.as<float>(), ch.nb, ch.total, min_samples, true);
        });
    uint64_t h_stats[DBSCAN_STATS];
    st.finish(*this, ws, d_label, d_kind, h_stats);
    std::memcpy(stats, h_stats, sizeof(h_stats));
    dbscan_calls += 1;
    dbscan_chunks += plan.walk.n_chunks;
    dbscan_pairs += h_stats[4];
}

void Index::dbscan_pairs_device(Workspace &ws, const uint64_t *d_src, const uint64_t *d_lims, const uint64_t *d_ids, const float *d_dists, uint64_t nq,
                                uint64_t min_samples, uint64_t *d_label, uint8_t *d_kind, uint64_t *stats) {
    hipStream_t s = ws.stream;
    const std::string bad = dbscan_check_min_samples(min_samples);
    VDB_REQUIRE(bad.empty(), bad);
    VDB_REQUIRE(nq < (1ull << 32), "dbscan pairs: too many lists for one call");
    VDB_REQUIRE(n < (1ull << 32), "dbscan pairs: an index of 2^32 rows or more");
    VDB_REQUIRE(nq == 0 || (d_src && d_lims && d_ids && d_dists), "dbscan pairs: null argument");
    VDB_REQUIRE(n == 0 || (d_label && d_kind), "dbscan pairs: null argument");
    VDB_REQUIRE(stats, "dbscan pairs: null argument");
    DensityState st;
    st.counters.reserve(DBSCAN_COUNTER_BYTES);
    uint64_t total = 0;
    if (nq) {  // limits, source ids and listed ids: the check of link_pairs_device; the sources distinct; one read-back of [flags | pairs]
        uint64_t *d_chk = st.cnt() + 6;
        VDB_HIP(hipMemsetAsync(d_chk, 0, 2 * sizeof(uint64_t), s));
        launch_pairs_check(d_src, d_lims, d_ids, nq, n, id_offset, d_chk, num_cu, s);
        const size_t seen_bytes = (n + 31) / 32 * sizeof(uint32_t);  // the sources' bit set, in `border` before the state is set up
        st.border.reserve(std::max<size_t>(n * sizeof(uint64_t), 8));  // (n x 8 B hold the ceil(n / 32) words)
        if (seen_bytes) VDB_HIP(hipMemsetAsync(st.border.p, 0, seen_bytes, s));
        launch_dbscan_sources(d_src, nq, n, id_offset, st.border.as<uint32_t>(), d_chk, num_cu, s);
        uint64_t *h = static_cast<uint64_t *>(ws.pinned(2 * sizeof(uint64_t)));
        VDB_HIP(hipMemcpyAsync(h, d_chk, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        VDB_SYNC(s);
        VDB_REQUIRE((h[0] & 1) == 0, "dbscan pairs: the limits do not ascend from 0, or a list holds an id that is no row of this index (id - "
                                     "id_offset must be below len)");
        VDB_REQUIRE(h[0] == 0, "dbscan pairs: two lists have the same source row");
        total = h[1];
    }
    if (n == 0) {
        std::fill(stats, stats + DBSCAN_STATS, uint64_t(0));
        return;
    }
    st.start(*this, nullptr, s);
    // all lists are one chunk: no row is left to a later one
    if (total) st.chunk(*this, ws, d_src, nullptr, 0, d_lims, d_ids, d_dists, nq, total, min_samples, false);
    uint64_t h_stats[DBSCAN_STATS];
    st.finish(*this, ws, d_label, d_kind, h_stats);
    std::memcpy(stats, h_stats, sizeof(h_stats));
}

}  // namespace vdb
