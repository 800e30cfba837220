// k_group.hip -- the capped walk of the grouped Flat k-NN (Index::flat_knn_grouped_device / Index::group_cap_device, grouped_plan.hpp;
// docs/DESIGN_flat.md 4.1q): from a query's candidate list, in the order given, the first k rows of which at most g carry any one
// value of a label column.
//
// k_group_cap: ONE WAVE PER QUERY (a workgroup is that wave).  The wave takes the list in tiles of 64 positions.  A lane loads its id and
// distance and gathers labels[id - id_offset] -- a dependent random 4-byte read, the latency of this kernel -- and the loads of tile t + 1
// are issued before tile t is worked on.  A row without a label (LABEL_NONE, a never-written column, an id that is no row of the index:
// never gathered) is always kept.  State: an open-addressing table label -> rows kept under it so far (saturating at g), linear probing
// from grouped_hash, 2^lg entries with a load of at most one half (grouped_table_lg) -- in LDS up to 2^GROUPED_LDS_MAX_LG entries, beyond
// that the same code on the query's slice of a global scratch buffer; the kernel clears it.  Per tile:
//   look up   every labelled lane probes for its label: the count before this tile (0 when absent)
//   rank      the wave walks its distinct labels as k_mask_partition does: the ballot of "my label is this one" and a prefix popcount give
//             a lane its rank among the tile's rows of that label; the first lane of the label then writes min(g, count + rows) into the
//             table -- once per distinct label, one lane at a time with a workgroup barrier after it, so no two lanes claim one empty slot
//   keep      unlabelled, or count + rank < g; the ballot of that and a prefix popcount give a kept lane its output slot (slots >= k are
//             not written)
// and the walk stops at k kept or at the end of the list.  The walk always starts at position 0 with an empty table: a longer list of a
// later round is walked again from its start (no table or position is carried between launches).  Outputs of query b go to row
// slot_q[b] (nullptr: b) of [..][k] arrays: the kept pairs, zeros behind them, the count, and done[b] = k rows were kept | the list held
// fewer than ld entries (it was everything its maker had).
#include "kernels.hpp"

namespace vdb {

static_assert(GROUPED_TILE == 64, "a tile is one wave");

template <bool IN_LDS>
__global__ __launch_bounds__(64) void k_group_cap(const uint64_t *__restrict__ ids, const float *__restrict__ dists,
                                                  const uint64_t *__restrict__ counts, uint64_t ld, const uint32_t *__restrict__ labels,
                                                  uint64_t n, uint64_t id_offset, uint32_t k, uint32_t g, uint32_t lg, uint32_t *g_table,
                                                  const uint32_t *__restrict__ slot_q, uint64_t *__restrict__ out_idx,
                                                  float *__restrict__ out_dist, uint64_t *__restrict__ out_cnt, uint8_t *__restrict__ done) {
    extern __shared__ uint32_t s_table[];
    const uint32_t lane = threadIdx.x;
    const uint64_t b = blockIdx.x;
    const uint32_t cap = 1u << lg, mask = cap - 1;
    uint32_t *tk = IN_LDS ? s_table : g_table + b * (uint64_t(2) << lg);  // keys (LABEL_NONE: empty), then counts
    uint32_t *tv = tk + cap;
    for (uint32_t i = lane; i < cap; i += 64) tk[i] = LABEL_NONE;
    __syncthreads();

    const uint64_t cnt = counts[b] < ld ? counts[b] : ld;
    const uint64_t *my_ids = ids + b * ld;
    const float *my_d = dists + b * ld;
    const uint64_t o = slot_q ? slot_q[b] : b;
    uint64_t *o_idx = out_idx + o * k;
    float *o_dist = out_dist + o * k;
    const uint64_t lt = (1ull << lane) - 1;

    // tile 0's loads
    uint64_t n_id = 0;
    float n_d = 0.0f;
    uint32_t n_lab = LABEL_NONE;
    if (lane < cnt) {
        n_id = my_ids[lane];
        n_d = my_d[lane];
        const uint64_t row = n_id - id_offset;
        if (labels && n_id >= id_offset && row < n) n_lab = labels[row];
    }
    uint64_t kept = 0;
    for (uint64_t t0 = 0; t0 < cnt && kept < k; t0 += 64) {  // (wave-uniform)
        const bool valid = t0 + lane < cnt;
        const uint64_t id = n_id;
        const float d = n_d;
        const uint32_t lab = n_lab;
        {  // the next tile's loads, in flight while this one is worked on
            const uint64_t p = t0 + 64 + lane;
            n_lab = LABEL_NONE;
            if (p < cnt) {
                n_id = my_ids[p];
                n_d = my_d[p];
                const uint64_t row = n_id - id_offset;
                if (labels && n_id >= id_offset && row < n) n_lab = labels[row];
            }
        }
        const bool labelled = valid && lab != LABEL_NONE;
        // look up
        uint32_t slot = 0, before = 0;
        if (labelled) {
            slot = (lab * 2654435761u) >> (32 - lg);  // grouped_hash
            uint32_t key = tk[slot];
            while (key != lab && key != LABEL_NONE) {
                slot = (slot + 1) & mask;
                key = tk[slot];
            }
            before = key == lab ? tv[slot] : 0;  // (<= g)
        }
        __syncthreads();  // every look-up of the tile before the first update
        // rank, update
        uint32_t rank = 0;
        uint64_t pending = __ballot(labelled);
        while (pending) {  // (wave-uniform; at most 64 rounds)
            const uint32_t lead = (uint32_t)__ffsll((unsigned long long)pending) - 1;
            const uint32_t cur = (uint32_t)__shfl((int)lab, (int)lead);
            const uint64_t same = __ballot(labelled && lab == cur);
            if (labelled && lab == cur) rank = (uint32_t)__popcll(same & lt);
            if (lane == lead) {
                const uint32_t rows = (uint32_t)__popcll(same);
                // `slot` is where the look-up stopped: the label's entry, or the first empty slot then -- which a label updated
                // earlier in this tile may have taken since, so the probe goes on from there
                uint32_t key = tk[slot];
                while (key != cur && key != LABEL_NONE) {
                    slot = (slot + 1) & mask;
                    key = tk[slot];
                }
                tk[slot] = cur;
                tv[slot] = (g - before <= rows) ? g : before + rows;
            }
            __syncthreads();
            pending &= ~same;
        }
        // keep
        const bool keep = valid && (!labelled || rank < g - before);
        const uint64_t kb = __ballot(keep);
        const uint64_t at = kept + (uint64_t)__popcll(kb & lt);
        if (keep && at < k) {
            o_idx[at] = id;
            o_dist[at] = d;
        }
        kept += (uint64_t)__popcll(kb);
    }
    if (kept > k) kept = k;
    for (uint64_t i = kept + lane; i < k; i += 64) {
        o_idx[i] = 0;
        o_dist[i] = 0.0f;
    }
    if (lane == 0) {
        out_cnt[o] = kept;
        done[b] = (kept == k || cnt < ld) ? 1 : 0;
    }
}

size_t group_cap_scratch_bytes(uint64_t nq, uint64_t k, uint64_t ld) {
    const uint32_t lg = grouped_table_lg(k, ld);
    return lg <= GROUPED_LDS_MAX_LG ? 0 : size_t(nq) * (size_t(8) << lg);
}

void launch_group_cap(const uint64_t *ids, const float *dists, const uint64_t *counts, uint64_t nq, uint64_t ld, const uint32_t *labels, uint64_t n,
                      uint64_t id_offset, uint32_t k, uint32_t g, uint32_t *scratch, const uint32_t *slot_q, uint64_t *out_idx, float *out_dist,
                      uint64_t *out_cnt, uint8_t *done, hipStream_t s) {
    if (nq == 0) return;
    const uint32_t lg = grouped_table_lg(k, ld);
    if (lg <= GROUPED_LDS_MAX_LG)
        hipLaunchKernelGGL(k_group_cap<true>, dim3((unsigned)nq), dim3(64), size_t(8) << lg, s, ids, dists, counts, ld, labels, n, id_offset, k, g, lg,
                           (uint32_t *)nullptr, slot_q, out_idx, out_dist, out_cnt, done);
    else
        hipLaunchKernelGGL(k_group_cap<false>, dim3((unsigned)nq), dim3(64), 0, s, ids, dists, counts, ld, labels, n, id_offset, k, g, lg, scratch,
                           slot_q, out_idx, out_dist, out_cnt, done);
}

}  // namespace vdb
