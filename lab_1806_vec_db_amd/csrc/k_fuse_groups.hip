// k_fuse_groups.hip -- the kernel of the document-level fused Flat search (Index::flat_knn_fused_groups_device / Index::fuse_groups_device,
// fuse_groups_plan.hpp; docs/DESIGN_flat.md 4.1z): the S lists of a fused query joined into one top-k of GROUPS -- a group is the rows that
// share a value of one label column; a row without a value is a group of its own.  Per list a group counts once, at its FIRST position
// (in a sorted list its nearest row): its rank among the groups of the list feeds RRF, that row's distance feeds MIN and SUM.  f32, one
// rounding per operation (-ffp-contract=off, the pragma below repeats it; the divide is the correctly rounded one), no float atomic, no
// order-dependent sum.
//
// k_fuse_groups<IN_LDS>: ONE WORKGROUP (256 threads) PER FUSED QUERY, the shape of k_fuse_lists.  State: an open-addressing table keyed by
// the group -- a 64-bit key, the label code, or FUSEG_ROW_TAG | LOCAL row for an unlabelled row: 33 bits of key space, so label code 5 and
// unlabelled row 5 are two groups -- linear probing from fuse_groups_hash, 2^lg slots with a load of at most one half; per slot the key,
// the accumulator, a stamp, the representative row and its distance, and behind them 2^(lg - 1) u64 sort keys: in LDS up to
// 2^FUSEG_LDS_MAX_LG slots, beyond that the same code on the query's slice of a global scratch buffer; the kernel clears it.  Every access
// to the table is a relaxed atomic (see k_fuse.hip); the barriers order them.
// The lists are taken in ascending s, which is the fold order, a tile of 256 positions at a time, one lane per entry; the id, distance
// and label gather of tile t + 1 are issued before tile t is worked on (the gather is a dependent random read: k_group.hip).
//   claim    compare-and-swap on the key; the slot's stamp tells a group new to the query (0) and one an earlier tile of THIS list held
//   stamp    atomic max of (s << 16) | (0xFFFF - position): inside a list the earliest position wins -- the first-occurrence rule
//   rank     the lanes whose value IS the stamp are the tile's first occurrences: wave ballots, prefix popcounts and per-wave sums in LDS
//            give each its 0-based rank among the groups of the list (a running base per list is carried over the tiles)
//   fold     that one lane per slot folds its term in with a plain read and write, and takes the representative when its distance is
//            strictly smaller under the knn order (so the earliest list keeps it; a group new to the query takes it as it is):
//              RRF  acc = acc + w / ((float)(rank + 1) + c)
//              MIN  nothing more: the score is the representative's distance
//              SUM  acc = acc + d, a group new to the query starting from the fold of f_0 .. f_(s-1), the last distances of the
//                   non-empty lists before s (the same bits for every group: every thread carries it)
//   fill     SUM only, after a non-empty list: the occupied slots the list did not stamp add f_s
// Then the occupied slots are compacted into pair keys (key of the score, representative row) -- distinct groups have distinct
// representatives --, sorted by a bitonic network, and the first min(k, |U|) go out: the representative with id_offset added and the
// score's own bits (the slot is found again through the representative's label; a NaN sum goes out as 0x7FC00000).
#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace vdb {

static_assert(FUSEG_LABEL_COLUMNS == LABEL_COLUMNS, "fuse_groups_plan.hpp and kernels.hpp agree");
static_assert((size_t(FUSEG_SLOT_BYTES) << FUSEG_LDS_MAX_LG) + 64 <= 160 * 1024, "the table, its sort keys and the static words fit the LDS of a CU");

template <bool IN_LDS, class T>
__device__ __forceinline__ T fg_ld(const T *p) {
    if constexpr (IN_LDS)
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool IN_LDS, class T>
__device__ __forceinline__ void fg_st(T *p, T v) {
    if constexpr (IN_LDS)
        __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else
        __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the group of LOCAL row `row`, whose label is `lab`
__device__ __forceinline__ uint64_t fg_key(uint32_t row, uint32_t lab) { return lab != LABEL_NONE ? uint64_t(lab) : (FUSEG_ROW_TAG | row); }
// the slot of `key`: its own, or the first empty one on its probe path, which becomes its own (load <= 1/2: an empty slot exists; the
// probe is bounded by the table all the same)
template <bool IN_LDS>
__device__ __forceinline__ uint32_t fg_claim(uint64_t *tk, uint64_t key, uint32_t lg, uint32_t mask) {
    uint32_t slot = ((uint32_t)key * 2654435761u) >> (32 - lg);  // fuse_groups_hash
    for (uint32_t probe = 0; probe < mask; probe++) {
        unsigned long long seen = FUSEG_EMPTY;
        unsigned long long *p = reinterpret_cast<unsigned long long *>(tk + slot);
        if constexpr (IN_LDS)
            __hip_atomic_compare_exchange_strong(p, &seen, (unsigned long long)key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else
            __hip_atomic_compare_exchange_strong(p, &seen, (unsigned long long)key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (seen == FUSEG_EMPTY || seen == key) break;
        slot = (slot + 1) & mask;
    }
    return slot;
}
// the slot that holds `key` (it is in the table)
template <bool IN_LDS>
__device__ __forceinline__ uint32_t fg_find(const uint64_t *tk, uint64_t key, uint32_t lg, uint32_t mask) {
    uint32_t slot = ((uint32_t)key * 2654435761u) >> (32 - lg);
    for (uint32_t probe = 0; probe < mask && fg_ld<IN_LDS>(tk + slot) != key; probe++) slot = (slot + 1) & mask;
    return slot;
}

template <bool IN_LDS>
__global__ __launch_bounds__(FUSE_THREADS) void k_fuse_groups(const uint64_t *__restrict__ ids, const float *__restrict__ dists,
                                                              const uint64_t *__restrict__ counts, uint64_t ld, const uint64_t *__restrict__ lims,
                                                              uint64_t list_base, const float *__restrict__ weights,
                                                              const uint32_t *__restrict__ labels, uint64_t n, int mode, float c, uint64_t id_offset,
                                                              uint64_t trunc_len, uint32_t k, uint32_t lg, uint32_t *g_table,
                                                              uint64_t *__restrict__ out_idx, float *__restrict__ out_dist,
                                                              uint64_t *__restrict__ out_cnt, uint8_t *__restrict__ out_exact) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_table[];
    __shared__ uint32_t s_used;
    __shared__ uint32_t s_wave[FUSE_THREADS / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t b = blockIdx.x;
    const uint32_t cap = 1u << lg, mask = cap - 1;
    uint32_t *base = IN_LDS ? s_table : g_table + b * (uint64_t(FUSEG_SLOT_BYTES / 4) << lg);
    uint64_t *tk = reinterpret_cast<uint64_t *>(base);  // keys (FUSEG_EMPTY: free)
    uint32_t *ta = base + 2 * cap, *ts = ta + cap;      // accumulators, stamps
    uint32_t *tr = ts + cap, *td = tr + cap;            // representative rows and their distances
    uint64_t *keys = reinterpret_cast<uint64_t *>(td + cap);  // cap / 2 sort keys (24 x cap bytes behind an aligned base)
    for (uint32_t i = tid; i < cap; i += FUSE_THREADS) {
        fg_st<IN_LDS>(tk + i, (uint64_t)FUSEG_EMPTY);
        fg_st<IN_LDS>(ta + i, 0u);  // +0.0f
        fg_st<IN_LDS>(ts + i, 0u);
    }
    if (tid == 0) s_used = 0;
    __syncthreads();

    const uint64_t lt = (1ull << lane) - 1;
    const uint64_t l0 = lims[b], l1 = lims[b + 1];
    float prefix = 0.0f;           // SUM: the fold of the last distances of the non-empty lists so far (workgroup-uniform)
    bool truncated = false;        // a list counts at least trunc_len entries (workgroup-uniform)
    uint32_t trunc_key = ~0u;      // the smallest order key of the last distance of a truncated list
    for (uint64_t l = l0; l < l1; l++) {  // (workgroup-uniform)
        const uint32_t s = (uint32_t)(l - l0);
        const uint64_t li = l - list_base;
        const uint64_t cnt = counts[li] < ld ? counts[li] : ld;
        if (cnt == 0) continue;  // a list without a counted entry is skipped in every fold
        const uint64_t *my_ids = ids + li * ld;
        const float *my_d = dists + li * ld;
        const float w = weights ? weights[l] : 1.0f;
        const float f_s = my_d[cnt - 1];
        if (cnt >= trunc_len) {
            truncated = true;
            const uint32_t fk = f32_orderable(f_s);
            trunc_key = fk < trunc_key ? fk : trunc_key;
        }
        uint32_t rank_base = 0;
        // tile 0's loads
        uint32_t n_row = 0, n_lab = LABEL_NONE;
        float n_d = 0.0f;
        if (tid < cnt) {
            const uint64_t id = my_ids[tid], row = id - id_offset;
            n_d = my_d[tid];
            n_row = (uint32_t)row;
            if (labels && id >= id_offset && row < n) n_lab = labels[row];
        }
        for (uint64_t t0 = 0; t0 < cnt; t0 += FUSE_THREADS) {
            const uint64_t p = t0 + tid;
            bool live = p < cnt;
            const uint32_t row = n_row, lab = n_lab;
            const float d = n_d;
            {  // the next tile's loads, in flight while this one is worked on
                const uint64_t pn = p + FUSE_THREADS;
                n_lab = LABEL_NONE;
                if (pn < cnt) {
                    const uint64_t id = my_ids[pn], r = id - id_offset;
                    n_d = my_d[pn];
                    n_row = (uint32_t)r;
                    if (labels && id >= id_offset && r < n) n_lab = labels[r];
                }
            }
            uint32_t slot = 0, mine = 0;
            bool fresh = false;
            if (live) {
                slot = fg_claim<IN_LDS>(tk, fg_key(row, lab), lg, mask);
                const uint32_t prev = fg_ld<IN_LDS>(ts + slot);
                fresh = prev == 0;
                live = fresh || (prev >> 16) != s;  // (a stamp of this list: an earlier tile holds the group at an earlier position)
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
            const bool owner = live && fg_ld<IN_LDS>(ts + slot) == mine;  // the first occurrence of the group in this list
            const uint64_t ob = __ballot(owner);
            if (lane == 0) s_wave[wave] = (uint32_t)__popcll(ob);
            __syncthreads();
            uint32_t before = 0, total = 0;
#pragma unroll
            for (uint32_t v = 0; v < FUSE_THREADS / 64; v++) {
                const uint32_t x = s_wave[v];
                before += v < wave ? x : 0;
                total += x;
            }
            if (owner) {  // the slot's one writer
                const uint32_t rank = rank_base + before + (uint32_t)__popcll(ob & lt);
                if (mode != FUSE_MIN) {
                    const float acc = fresh ? (mode == FUSE_SUM ? prefix : 0.0f) : __uint_as_float(fg_ld<IN_LDS>(ta + slot));
                    float r;
                    if (mode == FUSE_RRF) {
                        const float den = (float)(rank + 1) + c;
                        const float term = w / den;
                        r = acc + term;
                    } else {
                        r = acc + d;
                    }
                    fg_st<IN_LDS>(ta + slot, __float_as_uint(r));
                }
                if (fresh || f32_orderable(d) < f32_orderable(__uint_as_float(fg_ld<IN_LDS>(td + slot)))) {
                    fg_st<IN_LDS>(tr + slot, row);
                    fg_st<IN_LDS>(td + slot, __float_as_uint(d));
                }
            }
            rank_base += total;
            // (the next tile's claim touches keys and reads stamps only, and its two barriers stand before s_wave is written again)
        }
        if (mode == FUSE_SUM) {
            __syncthreads();  // every fold of the list before the fill reads its stamps and accumulators
            for (uint32_t i = tid; i < cap; i += FUSE_THREADS) {
                if (fg_ld<IN_LDS>(tk + i) != FUSEG_EMPTY && (fg_ld<IN_LDS>(ts + i) >> 16) != s) {
                    const float acc = __uint_as_float(fg_ld<IN_LDS>(ta + i));
                    fg_st<IN_LDS>(ta + i, __float_as_uint(acc + f_s));
                }
            }
            prefix = prefix + f_s;
            __syncthreads();  // (a slot belongs to one thread of the fill; the next list claims slots only behind it)
        }
    }
    __syncthreads();

    // compact: the occupied slots as pair keys, in any order (the representatives are distinct: the sort decides)
    for (uint32_t i = tid; i < cap; i += FUSE_THREADS) {
        if (fg_ld<IN_LDS>(tk + i) != FUSEG_EMPTY) {
            const float a = __uint_as_float(fg_ld<IN_LDS>(ta + i)), dm = __uint_as_float(fg_ld<IN_LDS>(td + i));
            const float score = mode == FUSE_RRF ? -a : (mode == FUSE_MIN ? dm : a);
            keys[atomicAdd(&s_used, 1u)] = pair_key(score, fg_ld<IN_LDS>(tr + i));
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
            const uint32_t lab = (labels && row < n) ? labels[row] : LABEL_NONE;
            const uint32_t slot = fg_find<IN_LDS>(tk, fg_key(row, lab), lg, mask);
            id = uint64_t(row) + id_offset;
            v = __uint_as_float(fg_ld<IN_LDS>((mode == FUSE_MIN ? td : ta) + slot));
            if (mode == FUSE_SUM && v != v) v = __uint_as_float(0x7FC00000u);  // (the payload of a NaN sum is the adder's business)
        }
        o_idx[i] = id;
        o_dist[i] = v;
    }
    if (tid == 0) {
        out_cnt[b] = take;
        if (out_exact) {
            bool exact = !truncated;
            // MIN: k groups whose k-th score is strictly before the last distance of every truncated list are the k nearest groups
            if (!exact && mode == FUSE_MIN && k > 0 && take == k) exact = (uint32_t)(keys[k - 1] >> 32) < trunc_key;
            out_exact[b] = exact ? 1 : 0;
        }
    }
}

void launch_fuse_groups(const uint64_t *ids, const float *dists, const uint64_t *counts, uint64_t nq, uint64_t ld, const uint64_t *lims,
                        uint64_t list_base, const float *weights, const uint32_t *labels, uint64_t n, int mode, float c, uint64_t id_offset,
                        uint64_t trunc_len, uint32_t k, uint32_t lg, uint32_t *scratch, uint64_t *out_idx, float *out_dist, uint64_t *out_cnt,
                        uint8_t *out_exact, hipStream_t s) {
    if (nq == 0) return;
    VDB_REQUIRE(lg >= FUSE_MIN_LG && lg <= 15 && ld <= FUSE_MAX_FETCH, "fuse groups: table size or list length");
    if (fuse_groups_in_lds(lg)) {
        func_max_lds(reinterpret_cast<const void *>(&k_fuse_groups<true>), int(fuse_groups_table_bytes(FUSEG_LDS_MAX_LG)));
        hipLaunchKernelGGL(k_fuse_groups<true>, dim3((unsigned)nq), dim3(FUSE_THREADS), fuse_groups_table_bytes(lg), s, ids, dists, counts, ld, lims,
                           list_base, weights, labels, n, mode, c, id_offset, trunc_len, k, lg, (uint32_t *)nullptr, out_idx, out_dist, out_cnt,
                           out_exact);
    } else {
        VDB_REQUIRE(scratch, "fuse groups: no scratch for a table beyond LDS");
        hipLaunchKernelGGL(k_fuse_groups<false>, dim3((unsigned)nq), dim3(FUSE_THREADS), 0, s, ids, dists, counts, ld, lims, list_base, weights, labels,
                           n, mode, c, id_offset, trunc_len, k, lg, scratch, out_idx, out_dist, out_cnt, out_exact);
    }
    VDB_HIP(hipGetLastError());
}

}  // namespace vdb
