// self_join.hpp -- THE walk over the chunks of the range self-join: every allowed row of an index is a query of the exact range search,
// `chunk` of them per flat_range_device call, in ascending row order (dup_plan.hpp lays the chunks out).  Index::flat_dup_groups_device
// (flat_dups.hip) and Index::flat_dbscan_device (flat_dbscan.hip) both call it with a per-chunk callback; there is no second copy.
//   On an unfiltered f32 index a chunk's queries are the rows where they lie; under a mask they are gathered, on a u8 index widened, into
//   ws.grp_q.  ONE flat_range_device call per chunk, whose counters advance as for that call.  A chunk with a non-empty result has its
//   limits uploaded once, is handed to `per_chunk`, and the stream is synchronised where the result goes out of scope.
//   start() runs once after every buffer of the walk is reserved and before the first launch -- the range calls use the workspace's other
//   buffers -- so the caller sets its own state up there; the stream is synchronised behind it.
#pragma once
#include <algorithm>
#include <vector>

#include "index.hpp"

namespace vdb {

struct SelfJoinChunk {
    uint64_t a, nb;           // the chunk's queries: positions [a, a + nb) of the allowed rows
    const uint32_t *src32;    // their rows on the device (the mask's ids + a); nullptr: row = position
    const RangeResult &r;     // the chunk's lists
    const uint64_t *d_lims;   // r.lims on the device
    uint64_t total;           // r.lims[nb] > 0
};

template <class Start, class PerChunk>
void walk_self_join(Index &ix, Workspace &ws, const DupPlan &plan, uint64_t chunk, float radius, uint64_t limit, const RowMask *mask, Start &&start,
                    PerChunk &&per_chunk) {
    hipStream_t s = ws.stream;
    const uint64_t dim = ix.dim;
    DevBuf aux;  // [radii f32 x chunk_len | limits u64 x (chunk_len + 1)]
    const size_t lims_off = (plan.chunk_len * sizeof(float) + 7) & ~size_t(7);
    aux.reserve(lims_off + (plan.chunk_len + 1) * sizeof(uint64_t));
    if (plan.gather) ws.grp_q.reserve(std::max<uint64_t>(plan.chunk_len, 1) * dim * sizeof(float));
    const std::vector<float> h_radius(plan.chunk_len, radius);  // (alive until the walk has synchronised)
    if (plan.chunk_len) VDB_HIP(hipMemcpyAsync(aux.p, h_radius.data(), plan.chunk_len * sizeof(float), hipMemcpyHostToDevice, s));
    start();
    VDB_SYNC(s);
    uint64_t *d_lims = reinterpret_cast<uint64_t *>(aux.as<char>() + lims_off);
    for (uint64_t c = 0; c < plan.n_chunks; c++) {
        const uint64_t a = c * chunk, nb = c + 1 == plan.n_chunks ? plan.last_len : chunk;
        const float *Q;
        if (!plan.gather)
            Q = ix.d_rows.as<float>() + a * dim;  // the rows are the queries, where they lie
        else {
            Q = ws.grp_q.as<float>();
            if (mask && ix.elem_u8)
                launch_rows_gather_widen(ix.d_rows.as<uint8_t>(), dim, mask->d_ids.as<uint32_t>() + a, false, 0, ws.grp_q.as<float>(), nb, ix.num_cu, s);
            else if (mask)
                launch_rows_gather(ix.d_rows.p, dim * sizeof(float), mask->d_ids.as<uint32_t>() + a, false, 0, ws.grp_q.p, nb, ix.num_cu, s);
            else
                launch_widen_u8(ix.d_rows.as<uint8_t>() + a * dim, nb * dim, ws.grp_q.as<float>(), s);
        }
        RangeResult r;  // dropped at the end of the chunk: peak memory is one chunk's result
        ix.flat_range_device(ws, Q, nb, aux.as<float>(), limit, r, mask);
        const uint64_t total = r.lims[nb];
        if (total) {
            VDB_HIP(hipMemcpyAsync(d_lims, r.lims.data(), (nb + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
            per_chunk(SelfJoinChunk{a, nb, mask ? mask->d_ids.as<uint32_t>() + a : nullptr, r, d_lims, total});
            VDB_SYNC(s);  // (r and its limits go out of scope)
        }
    }
}

}  // namespace vdb
