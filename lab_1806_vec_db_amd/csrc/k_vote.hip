// k_vote.hip -- the label vote of the k-NN classifier (Index::flat_knn_vote_device / Index::vote_lists_device, vote_plan.hpp;
// docs/DESIGN_flat.md 4.1ag): from a query's hit list, in the order given, the values of one label column its rows carry, each with the
// strict left fold of its voters' weights, its number of voters and the list position of its first voter; the top c by (score
// descending, first ascending).
//
// k_vote_lists: ONE WAVE PER QUERY (a workgroup is that wave).  A list has at most 4096 entries -- 64 tiles -- and the fold of a value is
// serial by its definition, so more waves on one list would only wait for each other at barriers; a call's parallelism is its queries,
// and a one-wave workgroup keeps every barrier of this kernel a wave-local one.  The wave takes the list in tiles of 64 positions.  A lane
// loads its id and distance and gathers labels[id - id_offset] -- a dependent random 4-byte read, the latency of this kernel -- and the
// loads of tile t + 1 are issued before tile t is worked on.  A row without a label (LABEL_NONE, a never-written column, an id that is
// no row of the index: never gathered) does not vote.  State: an open-addressing table code -> {score, votes, first}, linear probing
// from vote_hash, 2^lg slots with a load of at most one half (vote_table_lg) -- in LDS up to 2^VOTE_LDS_MAX_LG slots, beyond that the
// same code on the query's slice of a global scratch buffer; the kernel clears it.  Per tile:
//   weigh     1.0f, or 1.0f / (d + eps) with 0.0f for a NaN d; the tile's weights go to 64 words of LDS
//   claim     every voting lane finds its code's slot or takes the first empty one on its probe path by compare-and-swap on the code word
//   match     the wave walks its distinct codes as k_mask_partition does: the ballot of "my code is this one" is, for every lane of that
//             code, the set of the tile's voters of its value -- one round per distinct code, no memory touched
//   fold      the LOWEST lane of every value -- all of them at once, their slots are distinct -- adds the weights of its set to the slot's
//             score in ascending lane order, adds the set's popcount to the votes and, if the slot had none, sets first
// so a slot has one writer per tile, tiles follow each other behind a barrier, and the fold of a value is the list order whatever the
// other values do.  No float atomic exists in this file.  After the last tile the occupied slots become u64 keys
// (~f32_orderable(score), first, slot), a bitonic sort in the table's own tail orders them, and the first c are written out.
#include "common.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace vdb {

static_assert(VOTE_TILE == 64, "a tile is one wave");
static_assert(VOTE_MAX_K <= (1u << 12) && VOTE_MAX_K * 2 <= (1u << 13), "first and slot share the low word of a sort key");

template <bool IN_LDS>
__device__ __forceinline__ uint32_t vote_ld(const uint32_t *p) {
    if constexpr (IN_LDS)
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool IN_LDS>
__device__ __forceinline__ void vote_st(uint32_t *p, uint32_t v) {
    if constexpr (IN_LDS)
        __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else
        __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the slot of `code`: its own, or the first empty one on its probe path, which becomes its own (load <= 1/2: an empty slot exists)
template <bool IN_LDS>
__device__ __forceinline__ uint32_t vote_claim(uint32_t *tk, uint32_t code, uint32_t lg, uint32_t mask) {
    uint32_t slot = (code * 2654435761u) >> (32 - lg);  // vote_hash
    for (;;) {
        uint32_t seen = LABEL_NONE;
        if constexpr (IN_LDS)
            __hip_atomic_compare_exchange_strong(tk + slot, &seen, code, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else
            __hip_atomic_compare_exchange_strong(tk + slot, &seen, code, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (seen == LABEL_NONE || seen == code) return slot;
        slot = (slot + 1) & mask;
    }
}

template <bool IN_LDS>
__global__ __launch_bounds__(64) void k_vote_lists(const uint64_t *__restrict__ ids, const float *__restrict__ dists,
                                                   const uint64_t *__restrict__ counts, uint64_t ld, const uint32_t *__restrict__ labels,
                                                   uint64_t n, uint64_t id_offset, int mode, float eps, uint32_t c, uint32_t lg, uint32_t *g_table,
                                                   uint32_t *__restrict__ out_code, float *__restrict__ out_score,
                                                   uint32_t *__restrict__ out_votes, uint64_t *__restrict__ out_cnt,
                                                   uint64_t *__restrict__ out_voters) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_vote[];
    __shared__ float s_w[VOTE_TILE];
    __shared__ uint32_t s_used;
    const uint32_t lane = threadIdx.x;
    const uint64_t b = blockIdx.x;
    const uint32_t cap = 1u << lg, mask = cap - 1;
    uint32_t *tk = IN_LDS ? s_vote : g_table + b * (uint64_t(VOTE_SLOT_BYTES / 4) << lg);  // codes (LABEL_NONE: free), scores, votes, firsts
    uint32_t *ts = tk + cap, *tv = ts + cap, *tf = tv + cap;
    uint64_t *keys = reinterpret_cast<uint64_t *>(tf + cap);  // cap / 2 sort keys (8-byte aligned: 16 x cap bytes behind an aligned base)
    for (uint32_t i = lane; i < cap; i += 64) {
        vote_st<IN_LDS>(tk + i, LABEL_NONE);
        vote_st<IN_LDS>(ts + i, 0u);  // +0.0f
        vote_st<IN_LDS>(tv + i, 0u);
    }
    if (lane == 0) s_used = 0;
    __syncthreads();

    const uint64_t cnt = counts[b] < ld ? counts[b] : ld;
    const uint64_t *my_ids = ids + b * ld;
    const float *my_d = dists + b * ld;
    const uint64_t lt = (1ull << lane) - 1;

    // tile 0's loads
    float n_d = 0.0f;
    uint32_t n_lab = LABEL_NONE;
    if (lane < cnt) {
        const uint64_t id = my_ids[lane];
        n_d = my_d[lane];
        const uint64_t row = id - id_offset;
        if (labels && id >= id_offset && row < n) n_lab = labels[row];
    }
    uint64_t voters = 0;
    for (uint64_t t0 = 0; t0 < cnt; t0 += 64) {  // (wave-uniform)
        const float d = n_d;
        const uint32_t lab = n_lab;  // (LABEL_NONE past the end of the list)
        {  // the next tile's loads, in flight while this one is worked on
            const uint64_t p = t0 + 64 + lane;
            n_lab = LABEL_NONE;
            if (p < cnt) {
                const uint64_t id = my_ids[p];
                n_d = my_d[p];
                const uint64_t row = id - id_offset;
                if (labels && id >= id_offset && row < n) n_lab = labels[row];
            }
        }
        const bool voter = lab != LABEL_NONE;
        // weigh
        float w = 1.0f;
        if (mode == VOTE_INVERSE) w = (d != d) ? 0.0f : 1.0f / (d + eps);
        s_w[lane] = w;
        // claim
        uint32_t slot = 0;
        if (voter) slot = vote_claim<IN_LDS>(tk, lab, lg, mask);
        // match
        uint64_t mine = 0;
        const uint64_t all = __ballot(voter);
        for (uint64_t pending = all; pending;) {  // (wave-uniform; at most 64 rounds)
            const uint32_t lead = (uint32_t)__ffsll((unsigned long long)pending) - 1;
            const uint32_t cur = (uint32_t)__shfl((int)lab, (int)lead);
            const uint64_t same = __ballot(voter && lab == cur);
            if (voter && lab == cur) mine = same;
            pending &= ~same;
        }
        voters += (uint64_t)__popcll(all);
        __syncthreads();  // the tile's weights are in LDS
        // fold
        if (voter && (mine & lt) == 0) {  // the first voter of its value in this tile: the slot's one writer
            float acc = __uint_as_float(vote_ld<IN_LDS>(ts + slot));
            for (uint64_t m = mine; m; m &= m - 1) acc = acc + s_w[__ffsll((unsigned long long)m) - 1];
            vote_st<IN_LDS>(ts + slot, __float_as_uint(acc));
            const uint32_t v = vote_ld<IN_LDS>(tv + slot);
            if (v == 0) vote_st<IN_LDS>(tf + slot, (uint32_t)(t0 + lane));
            vote_st<IN_LDS>(tv + slot, v + (uint32_t)__popcll(mine));
        }
        __syncthreads();  // every fold of the tile before the next one's weights and reads
    }

    // compact: the occupied slots as sort keys, in any order (the firsts are distinct: the sort decides)
    for (uint32_t i = lane; i < cap; i += 64) {
        if (vote_ld<IN_LDS>(tk + i) != LABEL_NONE) {
            const float sc = __uint_as_float(vote_ld<IN_LDS>(ts + i));
            const uint32_t first = vote_ld<IN_LDS>(tf + i);
            keys[atomicAdd(&s_used, 1u)] = (uint64_t(~f32_orderable(sc)) << 32) | (uint64_t(first) << 13) | i;
        }
    }
    __syncthreads();
    const uint32_t used = s_used;  // (<= cap / 2)
    uint32_t np = 2;
    while (np < used) np <<= 1;  // (<= cap / 2)
    for (uint32_t i = used + lane; i < np; i += 64) keys[i] = PAIR_NONE;
    __syncthreads();
    for (uint32_t kk = 2; kk <= np; kk <<= 1) {
        for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
            for (uint32_t i = lane; i < (np >> 1); i += 64) {
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
    const uint32_t take = used < c ? used : c;
    for (uint32_t i = lane; i < c; i += 64) {
        uint32_t code = LABEL_NONE, votes = 0;
        float sc = 0.0f;
        if (i < take) {
            const uint32_t slot = (uint32_t)keys[i] & 0x1FFFu;
            code = vote_ld<IN_LDS>(tk + slot);
            sc = __uint_as_float(vote_ld<IN_LDS>(ts + slot));
            votes = vote_ld<IN_LDS>(tv + slot);
        }
        out_code[b * c + i] = code;
        out_score[b * c + i] = sc;
        out_votes[b * c + i] = votes;
    }
    if (lane == 0) {
        out_cnt[b] = take;
        out_voters[b] = voters;
    }
}

void launch_vote_lists(const uint64_t *ids, const float *dists, const uint64_t *counts, uint64_t nq, uint64_t ld, const uint32_t *labels, uint64_t n,
                       uint64_t id_offset, int mode, float eps, uint32_t c, uint32_t *scratch, uint32_t *out_code, float *out_score,
                       uint32_t *out_votes, uint64_t *out_cnt, uint64_t *out_voters, hipStream_t s) {
    if (nq == 0) return;
    // (c may pass ld: the lists of a search under short masks are shorter than the k its c was checked against)
    VDB_REQUIRE(ld >= 1 && ld <= VOTE_MAX_K && c >= 1 && c <= VOTE_MAX_K, "vote lists: list length or c");
    const uint32_t lg = vote_table_lg(ld);
    if (vote_in_lds(lg)) {
        hipLaunchKernelGGL(k_vote_lists<true>, dim3((unsigned)nq), dim3(64), vote_table_bytes(lg), s, ids, dists, counts, ld, labels, n, id_offset, mode,
                           eps, c, lg, (uint32_t *)nullptr, out_code, out_score, out_votes, out_cnt, out_voters);
    } else {
        VDB_REQUIRE(scratch, "vote lists: the table needs scratch");
        hipLaunchKernelGGL(k_vote_lists<false>, dim3((unsigned)nq), dim3(64), 0, s, ids, dists, counts, ld, labels, n, id_offset, mode, eps, c, lg,
                           scratch, out_code, out_score, out_votes, out_cnt, out_voters);
    }
    VDB_HIP(hipGetLastError());
}

}  // namespace vdb
