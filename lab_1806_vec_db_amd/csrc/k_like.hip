// k_like.hip -- the two kernels of the search by example rows (Index::flat_knn_like_device / Index::like_queries_device /
// Index::drop_listed_device, like_plan.hpp; docs/DESIGN_flat.md 4.1v): "more like these rows, and not like those".
//
// k_like_build<Id>: one query vector per query from its example rows, element by element in f32 with one rounding per operation (the
// file is compiled with -ffp-contract=off and the pragma below repeats it; the divide is the correctly rounded one):
//     sp = +0.0f; sp = sp + row[j] for every positive in list order (a strict left fold, repeats count);  ap = sp / (float)|P|
//     with negatives: an = the same fold and divide over them, query[j] = (ap + ap) - an;  without: query[j] = ap.
// A thread owns the elements j = blockIdx.x * 256 + tid, + gridDim.x * 256, ..; it walks the query's rows in list order with WAVE-UNIFORM
// ids (one id load per row for the whole wave), so every row is read coalesced across the lanes, 4 bytes per lane: nothing assumes
// dim % 4 == 0 or an aligned output.  Row offsets are 64-bit (id * dim passes 2^32 on a 4.5M x 960 index).  Id = uint32_t LOCAL rows or
// uint64_t GLOBAL ids (row + id_offset).  The callers have checked every id; one that is no row of the index is still never gathered
// (its elements read as NaN).
//
// k_like_drop<Id>: ONE WAVE PER QUERY (a workgroup is that wave), the k_group_cap pattern without its table.  The query's listed ids
// (two lists: positives, negatives; either may be absent) are staged in LDS as global ids.  The wave takes the candidate list in tiles
// of 64 positions; a lane tests its id against the staged ids (every lane reads the same LDS address: a broadcast), the ballot of "not
// listed" and a prefix popcount give a kept lane its output slot, and the walk stops at k kept or at the end of the list.  Order is
// preserved; the kept pairs go to out_idx / out_dist [b][k] with zeros behind them, their number to out_cnt[b].
#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace vdb {

constexpr uint32_t LIKE_BUILD_THREADS = 256;

// the strict left fold of element j over the rows ids[lo .. hi), divided by their number (hi > lo)
template <class Id>
__device__ __forceinline__ float like_mean(const Id *__restrict__ ids, uint64_t lo, uint64_t hi, const float *__restrict__ X, uint64_t n, uint32_t dim,
                                           uint64_t id_offset, uint32_t j) {
    float s = 0.0f;
    for (uint64_t p = lo; p < hi; p++) {  // (wave-uniform: p, the id and the branch)
        const uint64_t id = ids[p];
        const uint64_t row = sizeof(Id) == 8 ? id - id_offset : id;
        const bool ok = row < n && (sizeof(Id) != 8 || id >= id_offset);
        const float v = ok ? X[row * dim + j] : __builtin_nanf("");
        s = s + v;
    }
    const float cnt = (float)(hi - lo);  // (<= LIKE_MAX_EXAMPLES: exact)
    return s / cnt;
}

template <class Id>
__global__ __launch_bounds__(LIKE_BUILD_THREADS) void k_like_build(const Id *__restrict__ pos_ids, const uint64_t *__restrict__ pos_lims,
                                                                   const Id *__restrict__ neg_ids, const uint64_t *__restrict__ neg_lims,
                                                                   const float *__restrict__ X, uint64_t n, uint32_t dim, uint64_t id_offset,
                                                                   float *__restrict__ out) {
    const uint64_t b = blockIdx.y;
    const uint64_t p0 = pos_lims[b], p1 = pos_lims[b + 1];
    const uint64_t g0 = neg_lims ? neg_lims[b] : 0, g1 = neg_lims ? neg_lims[b + 1] : 0;
    float *o = out + b * dim;
    for (uint32_t j = blockIdx.x * LIKE_BUILD_THREADS + threadIdx.x; j < dim; j += gridDim.x * LIKE_BUILD_THREADS) {
        const float ap = p1 > p0 ? like_mean<Id>(pos_ids, p0, p1, X, n, dim, id_offset, j) : __builtin_nanf("");
        float r = ap;
        if (g1 > g0) {
            const float an = like_mean<Id>(neg_ids, g0, g1, X, n, dim, id_offset, j);
            const float twice = ap + ap;
            r = twice - an;
        }
        o[j] = r;
    }
}

template <class Id>
__global__ __launch_bounds__(64) void k_like_drop(const uint64_t *__restrict__ ids, const float *__restrict__ dists,
                                                  const uint64_t *__restrict__ counts, uint64_t ld, const Id *__restrict__ a_ids,
                                                  const uint64_t *__restrict__ a_lims, const Id *__restrict__ b_ids,
                                                  const uint64_t *__restrict__ b_lims, uint64_t id_offset, uint32_t k,
                                                  uint64_t *__restrict__ out_idx, float *__restrict__ out_dist, uint64_t *__restrict__ out_cnt) {
    __shared__ uint64_t s_ex[LIKE_MAX_EXAMPLES];
    const uint32_t lane = threadIdx.x;
    const uint64_t b = blockIdx.x;
    const uint64_t add = sizeof(Id) == 8 ? 0 : id_offset;  // staged ids are global
    // (the host has checked the limits: na + nb <= LIKE_MAX_EXAMPLES; the clamps keep a bad call inside the array all the same)
    const uint64_t a0 = a_lims ? a_lims[b] : 0, b0 = b_lims ? b_lims[b] : 0;
    uint32_t na = a_lims ? (uint32_t)std::min<uint64_t>(a_lims[b + 1] - a0, LIKE_MAX_EXAMPLES) : 0;
    uint32_t nb = b_lims ? (uint32_t)std::min<uint64_t>(b_lims[b + 1] - b0, LIKE_MAX_EXAMPLES - na) : 0;
    for (uint32_t i = lane; i < na; i += 64) s_ex[i] = (uint64_t)a_ids[a0 + i] + add;
    for (uint32_t i = lane; i < nb; i += 64) s_ex[na + i] = (uint64_t)b_ids[b0 + i] + add;
    const uint32_t ne = na + nb;
    __syncthreads();

    const uint64_t cnt = counts[b] < ld ? counts[b] : ld;
    const uint64_t *my_ids = ids + b * ld;
    const float *my_d = dists + b * ld;
    uint64_t *o_idx = out_idx + b * k;
    float *o_dist = out_dist + b * k;
    const uint64_t lt = (1ull << lane) - 1;

    uint64_t kept = 0;
    for (uint64_t t0 = 0; t0 < cnt && kept < k; t0 += 64) {  // (wave-uniform)
        const bool valid = t0 + lane < cnt;
        uint64_t id = 0;
        float d = 0.0f;
        if (valid) {
            id = my_ids[t0 + lane];
            d = my_d[t0 + lane];
        }
        bool listed = false;
        for (uint32_t e = 0; e < ne; e++) listed |= s_ex[e] == id;
        const bool keep = valid && !listed;
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
    if (lane == 0) out_cnt[b] = kept;
}

void launch_like_build(const void *pos_ids, const uint64_t *pos_lims, const void *neg_ids, const uint64_t *neg_lims, bool global_ids, uint64_t nq,
                       const float *X, uint64_t n, uint32_t dim, uint64_t id_offset, float *out, hipStream_t s) {
    if (nq == 0 || dim == 0) return;
    const unsigned gx = (unsigned)std::min<uint64_t>((uint64_t(dim) + LIKE_BUILD_THREADS - 1) / LIKE_BUILD_THREADS, 1024);
    for (uint64_t q0 = 0; q0 < nq; q0 += 32768) {  // (grid.y)
        const uint64_t nb = std::min<uint64_t>(32768, nq - q0);
        const dim3 grid(gx, (unsigned)nb), block(LIKE_BUILD_THREADS);
        const uint64_t *nl = neg_lims ? neg_lims + q0 : nullptr;
        if (global_ids)
            hipLaunchKernelGGL(k_like_build<uint64_t>, grid, block, 0, s, static_cast<const uint64_t *>(pos_ids), pos_lims + q0,
                               static_cast<const uint64_t *>(neg_ids), nl, X, n, dim, id_offset, out + q0 * dim);
        else
            hipLaunchKernelGGL(k_like_build<uint32_t>, grid, block, 0, s, static_cast<const uint32_t *>(pos_ids), pos_lims + q0,
                               static_cast<const uint32_t *>(neg_ids), nl, X, n, dim, id_offset, out + q0 * dim);
    }
}

void launch_like_drop(const uint64_t *ids, const float *dists, const uint64_t *counts, uint64_t nq, uint64_t ld, const void *a_ids,
                      const uint64_t *a_lims, const void *b_ids, const uint64_t *b_lims, bool global_ids, uint64_t id_offset, uint32_t k,
                      uint64_t *out_idx, float *out_dist, uint64_t *out_cnt, hipStream_t s) {
    if (nq == 0) return;
    VDB_REQUIRE(nq < (1ull << 31), "like drop: too many queries");
    const dim3 grid((unsigned)nq), block(64);
    if (global_ids)
        hipLaunchKernelGGL(k_like_drop<uint64_t>, grid, block, 0, s, ids, dists, counts, ld, static_cast<const uint64_t *>(a_ids), a_lims,
                           static_cast<const uint64_t *>(b_ids), b_lims, id_offset, k, out_idx, out_dist, out_cnt);
    else
        hipLaunchKernelGGL(k_like_drop<uint32_t>, grid, block, 0, s, ids, dists, counts, ld, static_cast<const uint32_t *>(a_ids), a_lims,
                           static_cast<const uint32_t *>(b_ids), b_lims, id_offset, k, out_idx, out_dist, out_cnt);
}

}  // namespace vdb
