// k_fuse.hip -- the kernel of the fused multi-query Flat search (Index::flat_knn_fused_device / Index::fuse_lists_device, fuse_plan.hpp;
// docs/DESIGN_flat.md 4.1w): the S lists of a fused query -- one per sub-query, walked as given, position = rank -- joined into one
// top-k by reciprocal rank fusion (score = the strict left fold, over the lists in ascending order, of w_s / ((float)(rank + 1) + c)) or by
// the smallest distance (the bits of the first list that attains it).  f32, one rounding per operation (the file is compiled with
// -ffp-contract=off and the pragma below repeats it; the divide is the correctly rounded one), no float atomic, no order-dependent sum.
//
// k_fuse_lists<IN_LDS>: ONE WORKGROUP (256 threads) PER FUSED QUERY.  State: an open-addressing table keyed by the 32-bit LOCAL row
// (id - id_offset), linear probing from fuse_hash, 2^lg slots with a load of at most one half (fuse_table_lg) -- per slot the key, the
// accumulator and a stamp -- and behind it 2^(lg - 1) u64 sort keys: in LDS up to 2^FUSE_LDS_MAX_LG slots, beyond that the same code on
// the query's slice of a global scratch buffer; the kernel clears it.  Every access to the table is a relaxed atomic (plain LDS
// operations in LDS; in global memory served from the coherence point, so that a plain read never meets a stale line behind an atomic
// of another wave); the barriers order them.
// The lists are taken in ascending s, which is the fold order, a tile of 256 positions at a time, one lane per entry:
//   claim    the lane probes for its row with a compare-and-swap on the key (an empty slot becomes the row's) and reads the slot's stamp:
//            0 = the row is new to this fused query; a stamp of THIS list = an earlier tile held the row already, the lane drops out
//   stamp    atomic max of (s << 16) | (0xFFFF - position) on the slot: a later list beats every earlier one, and inside a list the
//            earliest position wins -- the first-occurrence rule
//   fold     the one lane whose value IS the stamp adds its term to the accumulator (RRF) or takes the minimum under the knn order
//            (MIN: strictly smaller only, so the first list that attains it keeps its bits; a row new to the query takes the distance as
//            it is) with a plain read and write: one writer per slot per list
// with a barrier between the steps; the barrier between claim and stamp of the next tile also separates two lists.  Then the occupied
// slots are compacted into pair keys -- (key of -score, row) for RRF: scores are > 0, descending by score and ascending by row;
// (key of the distance, row) for MIN -- padded with PAIR_NONE to a power of two, sorted by a bitonic network over the workgroup, and the
// first min(k, |U|) go out: the id with id_offset added and the accumulator's own bits, looked up again by row (the key canonicalises
// -0 and NaN, the answer does not).  Zeros behind the count.
#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace vdb {

template <bool IN_LDS>
__device__ __forceinline__ uint32_t fuse_ld(const uint32_t *p) {
    if constexpr (IN_LDS)
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool IN_LDS>
__device__ __forceinline__ void fuse_st(uint32_t *p, uint32_t v) {
    if constexpr (IN_LDS)
        __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else
        __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the slot of `row`: its own, or the first empty one on its probe path, which becomes its own
template <bool IN_LDS>
__device__ __forceinline__ uint32_t fuse_claim(uint32_t *tk, uint32_t row, uint32_t lg, uint32_t mask) {
    uint32_t slot = (row * 2654435761u) >> (32 - lg);  // fuse_hash
    for (;;) {  // (load <= 1/2: an empty slot exists)
        uint32_t seen = FUSE_EMPTY;
        if constexpr (IN_LDS)
            __hip_atomic_compare_exchange_strong(tk + slot, &seen, row, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else
            __hip_atomic_compare_exchange_strong(tk + slot, &seen, row, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (seen == FUSE_EMPTY || seen == row) return slot;
        slot = (slot + 1) & mask;
    }
}
// the slot that holds `row` (it is in the table)
template <bool IN_LDS>
__device__ __forceinline__ uint32_t fuse_find(const uint32_t *tk, uint32_t row, uint32_t lg, uint32_t mask) {
    uint32_t slot = (row * 2654435761u) >> (32 - lg);
    while (fuse_ld<IN_LDS>(tk + slot) != row) slot = (slot + 1) & mask;
    return slot;
}

template <bool IN_LDS>
__global__ __launch_bounds__(FUSE_THREADS) void k_fuse_lists(const uint64_t *__restrict__ ids, const float *__restrict__ dists,
                                                             const uint64_t *__restrict__ counts, uint64_t ld, const uint64_t *__restrict__ lims,
                                                             uint64_t list_base, const float *__restrict__ weights, int mode, float c,
                                                             uint64_t id_offset, uint32_t k, uint32_t lg, uint32_t *g_table,
                                                             uint64_t *__restrict__ out_idx, float *__restrict__ out_dist,
                                                             uint64_t *__restrict__ out_cnt) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_table[];
    __shared__ uint32_t s_used;
    const uint32_t tid = threadIdx.x;
    const uint64_t b = blockIdx.x;
    const uint32_t cap = 1u << lg, mask = cap - 1;
    uint32_t *tk = IN_LDS ? s_table : g_table + b * (uint64_t(FUSE_SLOT_BYTES / 4) << lg);  // keys (FUSE_EMPTY: free), accumulators, stamps
    uint32_t *ta = tk + cap, *ts = ta + cap;
    uint64_t *keys = reinterpret_cast<uint64_t *>(ts + cap);  // cap / 2 sort keys (8-byte aligned: 12 x cap bytes behind an aligned base)
    for (uint32_t i = tid; i < cap; i += FUSE_THREADS) {
        fuse_st<IN_LDS>(tk + i, FUSE_EMPTY);
        fuse_st<IN_LDS>(ta + i, 0u);  // +0.0f
        fuse_st<IN_LDS>(ts + i, 0u);
    }
    if (tid == 0) s_used = 0;
    __syncthreads();

    const uint64_t l0 = lims[b], l1 = lims[b + 1];
    for (uint64_t l = l0; l < l1; l++) {  // (workgroup-uniform)
        const uint32_t s = (uint32_t)(l - l0);
        const uint64_t li = l - list_base;
        const uint64_t cnt = counts[li] < ld ? counts[li] : ld;
        const uint64_t *my_ids = ids + li * ld;
        const float *my_d = dists + li * ld;
        const float w = weights ? weights[l] : 1.0f;
        for (uint64_t t0 = 0; t0 < cnt; t0 += FUSE_THREADS) {
            const uint64_t p = t0 + tid;
            bool live = p < cnt;
            uint32_t slot = 0, mine = 0;
            float d = 0.0f;
            bool fresh = false;
            if (live) {
                const uint32_t row = (uint32_t)(my_ids[p] - id_offset);
                d = my_d[p];
                slot = fuse_claim<IN_LDS>(tk, row, lg, mask);
                const uint32_t prev = fuse_ld<IN_LDS>(ts + slot);
                fresh = prev == 0;
                live = fresh || (prev >> 16) != s;  // (a stamp of this list: an earlier tile holds the row at an earlier position)
                mine = (s << 16) | (0xFFFFu - (uint32_t)p);  // (p < 4096: never 0)
            }
            __syncthreads();  // every stamp of the tile read before the first is raised
            if (live) {
                if constexpr (IN_LDS)
                    __hip_atomic_fetch_max(ts + slot, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                else
                    __hip_atomic_fetch_max(ts + slot, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __syncthreads();
            if (live && fuse_ld<IN_LDS>(ts + slot) == mine) {  // the first occurrence of the row in this list: the slot's one writer
                const float acc = __uint_as_float(fuse_ld<IN_LDS>(ta + slot));
                float r;
                if (mode == FUSE_RRF) {
                    const float den = (float)(uint32_t)(p + 1) + c;
                    const float term = w / den;
                    r = acc + term;
                } else {
                    r = (fresh || f32_orderable(d) < f32_orderable(acc)) ? d : acc;
                }
                fuse_st<IN_LDS>(ta + slot, __float_as_uint(r));
            }
            // (the next tile's claim touches keys and reads stamps only; its first barrier is behind every fold of this one)
        }
    }
    __syncthreads();

    // compact: the occupied slots as pair keys, in any order (the rows are distinct: the sort decides)
    for (uint32_t i = tid; i < cap; i += FUSE_THREADS) {
        const uint32_t row = fuse_ld<IN_LDS>(tk + i);
        if (row != FUSE_EMPTY) {
            const float a = __uint_as_float(fuse_ld<IN_LDS>(ta + i));
            keys[atomicAdd(&s_used, 1u)] = pair_key(mode == FUSE_RRF ? -a : a, row);
        }
    }
    __syncthreads();
    const uint32_t used = s_used;  // (<= cap / 2)
    uint32_t np = 2;
    while (np < used) np <<= 1;  // (<= cap / 2)
    for (uint32_t i = used + tid; i < np; i += FUSE_THREADS) keys[i] = PAIR_NONE;
    __syncthreads();
    for (uint32_t kk = 2; kk <= np; kk <<= 1) {
        for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
            for (uint32_t i = tid; i < (np >> 1); i += FUSE_THREADS) {
                const uint32_t lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
                const uint64_t x = keys[lo], y = keys[hi];
                if ((x > y) == ((lo & kk) == 0)) {
                    keys[lo] = y;
                    keys[hi] = x;
                }
            }
            __syncthreads();
        }
    }
    const uint32_t take = used < k ? used : k;
    uint64_t *o_idx = out_idx + b * k;
    float *o_dist = out_dist + b * k;
    for (uint32_t i = tid; i < k; i += FUSE_THREADS) {
        uint64_t id = 0;
        float v = 0.0f;
        if (i < take) {
            const uint32_t row = (uint32_t)keys[i];
            id = uint64_t(row) + id_offset;
            v = __uint_as_float(fuse_ld<IN_LDS>(ta + fuse_find<IN_LDS>(tk, row, lg, mask)));
        }
        o_idx[i] = id;
        o_dist[i] = v;
    }
    if (tid == 0) out_cnt[b] = take;
}

void launch_fuse_lists(const uint64_t *ids, const float *dists, const uint64_t *counts, uint64_t nq, uint64_t ld, const uint64_t *lims,
                       uint64_t list_base, const float *weights, int mode, float c, uint64_t id_offset, uint32_t k, uint32_t lg, uint32_t *scratch,
                       uint64_t *out_idx, float *out_dist, uint64_t *out_cnt, hipStream_t s) {
    if (nq == 0) return;
    VDB_REQUIRE(lg >= FUSE_MIN_LG && lg <= 15 && ld <= FUSE_MAX_FETCH, "fuse lists: table size or list length");
    if (fuse_in_lds(lg)) {
        func_max_lds(reinterpret_cast<const void *>(&k_fuse_lists<true>), int(fuse_table_bytes(FUSE_LDS_MAX_LG)));
        hipLaunchKernelGGL(k_fuse_lists<true>, dim3((unsigned)nq), dim3(FUSE_THREADS), fuse_table_bytes(lg), s, ids, dists, counts, ld, lims, list_base,
                           weights, mode, c, id_offset, k, lg, (uint32_t *)nullptr, out_idx, out_dist, out_cnt);
    } else {
        hipLaunchKernelGGL(k_fuse_lists<false>, dim3((unsigned)nq), dim3(FUSE_THREADS), 0, s, ids, dists, counts, ld, lims, list_base, weights, mode, c,
                           id_offset, k, lg, scratch, out_idx, out_dist, out_cnt);
    }
    VDB_HIP(hipGetLastError());
}

}  // namespace vdb
