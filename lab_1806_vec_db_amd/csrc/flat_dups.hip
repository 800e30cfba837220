// flat_dups.hip -- near-duplicate grouping of an index's own rows (docs/DESIGN_flat.md 4.1ab): the range self-join driver
// Index::flat_dup_groups_device and the component stage alone, Index::link_pairs_device.  The rule: for every allowed row i the list
// flat_range_device returns for query = row i (radius, limit, mask) names its neighbours; every j != i on it is an undirected edge;
// the groups are the connected components of the allowed rows under these edges -- SINGLE LINKAGE at the radius: A-B and B-C put A and
// C together even when D(A, C) > radius -- and a group is named by its lowest row.  dup_plan.hpp checks and lays out the chunks,
// k_components.hip holds the union-find.
#include <algorithm>
#include <cstring>
#include <vector>

#include "index.hpp"

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
    // every buffer of the call before its first launch: the range calls use the workspace's other buffers
    Components cc;
    DevBuf aux;  // [radii f32 x chunk_len | limits u64 x (chunk_len + 1)]
    const size_t lims_off = (plan.chunk_len * sizeof(float) + 7) & ~size_t(7);
    aux.reserve(lims_off + (plan.chunk_len + 1) * sizeof(uint64_t));
    if (plan.gather) ws.grp_q.reserve(std::max<uint64_t>(plan.chunk_len, 1) * dim * sizeof(float));
    const std::vector<float> h_radius(plan.chunk_len, radius);  // (alive until the call has synchronised)
    if (plan.chunk_len) VDB_HIP(hipMemcpyAsync(aux.p, h_radius.data(), plan.chunk_len * sizeof(float), hipMemcpyHostToDevice, s));
    cc.start(*this, s);
    VDB_SYNC(s);
    uint64_t *d_lims = reinterpret_cast<uint64_t *>(aux.as<char>() + lims_off);
    for (uint64_t c = 0; c < plan.n_chunks; c++) {
        const uint64_t a = c * dup_chunk, nb = c + 1 == plan.n_chunks ? plan.last_len : dup_chunk;
        const float *Q;
        if (!plan.gather)
            Q = d_rows.as<float>() + a * dim;  // the rows are the queries, where they lie
        else {
            Q = ws.grp_q.as<float>();
            if (mask && elem_u8)
                launch_rows_gather_widen(d_rows.as<uint8_t>(), dim, mask->d_ids.as<uint32_t>() + a, false, 0, ws.grp_q.as<float>(), nb, num_cu, s);
            else if (mask)
                launch_rows_gather(d_rows.p, dim * sizeof(float), mask->d_ids.as<uint32_t>() + a, false, 0, ws.grp_q.p, nb, num_cu, s);
            else
                launch_widen_u8(d_rows.as<uint8_t>() + a * dim, nb * dim, ws.grp_q.as<float>(), s);
        }
        RangeResult r;  // dropped at the end of the chunk: peak memory is one chunk's result
        flat_range_device(ws, Q, nb, aux.as<float>(), limit, r, mask);
        const uint64_t total = r.lims[nb];
        if (total) {
            VDB_HIP(hipMemcpyAsync(d_lims, r.lims.data(), (nb + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
            prof_begin(ws, "dup_hook", double(total) * sizeof(uint64_t));
            launch_comp_hook(nullptr, mask ? mask->d_ids.as<uint32_t>() + a : nullptr, a, d_lims, r.idx.as<uint64_t>(), nb, total, id_offset, limit,
                             cc.parent.as<uint32_t>(), cc.cnt(), num_cu, s);
            prof_end(ws);
            VDB_SYNC(s);  // (r and its limits go out of scope)
        }
    }
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
