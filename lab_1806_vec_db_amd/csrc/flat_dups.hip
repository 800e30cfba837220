// flat_dups.hip -- near-duplicate grouping of an index's own rows (docs/DESIGN_flat.md 4.1ab): the range self-join driver
// Index::flat_dup_groups_device and the component stage alone, Index::link_pairs_device.  The rule: for every allowed row i the list
// flat_range_device returns for query = row i (radius, limit, mask) names its neighbours; every j != i on it is an undirected edge;
// the groups are the connected components of the allowed rows under these edges -- SINGLE LINKAGE at the radius: A-B and B-C put A and
// C together even when D(A, C) > radius -- and a group is named by its lowest row.  dup_plan.hpp checks and lays out the chunks,
// self_join.hpp walks them (shared with flat_dbscan.hip), k_components.hip holds the union-find.
#include <algorithm>
#include <cstring>
#include <vector>

#include "index.hpp"
#include "self_join.hpp"

namespace vdb {

namespace {

// the device state of one call: parent | size [n] u32 each, counters [4] u64 (+ the list check's two words behind them)
struct Components {
    DevBuf parent, size, counters;
    uint64_t *cnt() const { return counters.as<uint64_t>(); }
    void start(const Index &ix, hipStream_t s) {
        parent.reserve(std::max<uint64_t>(ix.n, 1) * sizeof(uint32_t));
        size.reserve(std::max<uint64_t>(ix.n, 1) * sizeof(uint32_t));
        counters.reserve(DUP_COUNTER_BYTES);
        VDB_HIP(hipMemsetAsync(counters.p, 0, DUP_COUNTER_BYTES, s));
        launch_comp_init(parent.as<uint32_t>(), size.as<uint32_t>(), ix.n, ix.num_cu, s);
    }
    // flatten + count, the group ids to d_group, the four counters to stats; returns synchronised
    void finish(Index &ix, Workspace &ws, const uint64_t *bits, uint64_t *d_group, uint64_t *stats) {
        hipStream_t s = ws.stream;
        ix.prof_begin(ws, "dup_flatten", double(ix.n) * (3 * sizeof(uint32_t) + sizeof(uint64_t)));
        launch_comp_flatten(parent.as<uint32_t>(), bits, ix.n, ix.id_offset, d_group, size.as<uint32_t>(), cnt(), ix.num_cu, s);
        ix.prof_end(ws);
        uint64_t *h = static_cast<uint64_t *>(ws.pinned(DUP_STATS * sizeof(uint64_t)));
        VDB_HIP(hipMemcpyAsync(h, counters.p, DUP_STATS * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        VDB_SYNC(s);
        std::memcpy(stats, h, DUP_STATS * sizeof(uint64_t));
    }
};

}  // namespace

void Index::flat_dup_groups_device(Workspace &ws, float radius, uint64_t limit, const RowMask *mask, uint64_t *d_group, uint64_t *stats) {
    hipStream_t s = ws.stream;
    if (mask) check_mask(*mask);
    const std::string bad = dup_check_args(n, mask ? mask->m : n, mask != nullptr, radius, dup_chunk);
    VDB_REQUIRE(bad.empty(), bad);
    if (n == 0) {
        std::fill(stats, stats + DUP_STATS, uint64_t(0));
        dup_calls += 1;
        return;
    }
    const DupPlan plan = dup_plan(n, dim, elem_u8, mask != nullptr, mask ? mask->m : n, dup_chunk);
    Components cc;
    walk_self_join(
        *this, ws, plan, dup_chunk, radius, limit, mask, [&] { cc.start(*this, s); },
        [&](const SelfJoinChunk &ch) {
            prof_begin(ws, "dup_hook", double(ch.total) * sizeof(uint64_t));
            launch_comp_hook(nullptr, ch.src32, ch.a, ch.d_lims, ch.r.idx.as<uint64_t>(), ch.nb, ch.total, id_offset, limit, cc.parent.as<uint32_t>(),
                             cc.cnt(), num_cu, s);
            prof_end(ws);
        });
    uint64_t h_stats[DUP_STATS];
    cc.finish(*this, ws, mask ? mask->d_bits.as<uint64_t>() : nullptr, d_group, h_stats);
    std::memcpy(stats, h_stats, sizeof(h_stats));
    dup_calls += 1;
    dup_chunks += plan.n_chunks;
    dup_pairs += h_stats[2];
}

void Index::link_pairs_device(Workspace &ws, const uint64_t *d_src, const uint64_t *d_lims, const uint64_t *d_ids, uint64_t nq, uint64_t *d_group,
                              uint64_t *stats) {
    hipStream_t s = ws.stream;
    VDB_REQUIRE(nq < (1ull << 32), "link pairs: too many lists for one call");
    VDB_REQUIRE(n < (1ull << 32), "link pairs: an index of 2^32 rows or more");
    VDB_REQUIRE(nq == 0 || (d_src && d_lims), "link pairs: null argument");
    VDB_REQUIRE(n == 0 || d_group, "link pairs: null argument");
    VDB_REQUIRE(stats, "link pairs: null argument");
    Components cc;
    cc.counters.reserve(DUP_COUNTER_BYTES);
    uint64_t total = 0;
    if (nq) {  // limits, source ids and listed ids: one kernel, one read-back of [flag | pairs]
        uint64_t *d_chk = cc.cnt() + DUP_STATS;
        VDB_HIP(hipMemsetAsync(d_chk, 0, 2 * sizeof(uint64_t), s));
        launch_pairs_check(d_src, d_lims, d_ids, nq, n, id_offset, d_chk, num_cu, s);
        uint64_t *h = static_cast<uint64_t *>(ws.pinned(2 * sizeof(uint64_t)));
        VDB_HIP(hipMemcpyAsync(h, d_chk, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        VDB_SYNC(s);
        VDB_REQUIRE(h[0] == 0, "link pairs: the limits do not ascend from 0, or a list holds an id that is no row of this index (id - id_offset must be "
                               "below len)");
        total = h[1];
    }
    if (n == 0) {
        std::fill(stats, stats + DUP_STATS, uint64_t(0));
        return;
    }
    cc.start(*this, s);
    if (total) {
        prof_begin(ws, "dup_hook", double(total) * sizeof(uint64_t));
        launch_comp_hook(d_src, nullptr, 0, d_lims, d_ids, nq, total, id_offset, 0, cc.parent.as<uint32_t>(), cc.cnt(), num_cu, s);
        prof_end(ws);
    }
    uint64_t h_stats[DUP_STATS];
    cc.finish(*this, ws, nullptr, d_group, h_stats);
    std::memcpy(stats, h_stats, sizeof(h_stats));
}

}  // namespace vdb
