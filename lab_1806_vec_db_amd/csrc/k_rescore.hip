// k_rescore.hip -- the kernels of the exact late-interaction rescoring of candidate documents (Index::rescore_groups_device,
// flat_rescore.hip, rescore_plan.hpp; docs/DESIGN_flat.md 4.1ak): the groups of a question's candidate rows scored over ALL their rows --
// per sub-query the group's nearest allowed row under the knn order, the scores a strict left fold over the sub-queries (SUM) or their
// smallest (MIN).  f32, one rounding per operation (-ffp-contract=off, the pragma below repeats it; the divide and the square root are
// the correctly rounded ones), no float atomic: a minimum is an INTEGER min of (order key << 32 | row), which does not depend on the order
// of arrival, and the sum is a fold of its own over those minima.
//
// collect   k_rescore_slots: a workgroup per question dedupes its candidates' groups in an LDS table (claim by compare-and-swap, the
//           earliest position by an atomic min; the first occurrences take their slot numbers from wave ballots and prefix popcounts, as
//           k_fuse_groups ranks its groups) and enters every labelled group into ONE table of the call, keyed (question, code) and probed
//           from the hash of the code alone.  k_rescore_match then reads the label column once: a row walks the probe path of its code and
//           meets every question that wants it; the lanes of a wave that hit the same question share one atomic add (ballot, prefix
//           popcount).  Run twice: to count (the host sizes the tiles from the counts) and to append.  k_rescore_prepare clears a
//           question's minima, appends its unlabelled candidates (groups of their own) and pads its last tile.
// pairs     k_rescore_pairs, the hot path: a workgroup of 4 waves per (question, tile of 64 entries).  Lane l of EVERY wave owns row l of
//           the tile; wave w owns the sub-queries w, w + 4, .. (at most 8 accumulators per lane).  The rows are not read lane-per-row
//           from global memory (64 lines per load instruction): the workgroup stages them in slices of 32 dimensions, a half-wave
//           reading the 128 contiguous bytes of one row's slice, into a [64][33] f32 LDS panel (33: lane l reads bank 33 l + j, all
//           distinct) and the question's S x 32 slice into a second panel (read as broadcasts); both are double-buffered -- slice c + 1
//           is in registers while slice c is folded.  The fold is fold1 / epilogue of k_exact.hip, ascending in the dimension; the last
//           dim % 32 elements run element by element.  Then the minima: the lanes of one group in a tile first meet in an LDS table
//           [leader lane][s] (leader: the lowest lane of the tile with the same slot), and the leader alone goes to the global table.
//           LDS: 2 x 8448 + 2 x 4096 + 16384 + 768 = 42240 B, 3 workgroups per CU; registers: see the design note.
// finish    k_rescore_finish: a workgroup per question, a thread per group slot folds the S minima in ascending s (an empty one is
//           +inf), the (score key, representative) pairs are sorted by the bitonic network of k_fuse_groups in LDS and the first k leave.
#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace vdb {

static_assert(RESCORE_TILE == 64, "a tile is a row per lane");
static_assert(FUSEG_ROW_TAG == (1ull << 32) && FUSEG_EMPTY == ~0ull, "the group keys are those of k_fuse_groups");

namespace {

constexpr uint32_t RS_THREADS = 256;
constexpr uint32_t RS_SLICE = 32;            // dimensions of one staged slice
constexpr uint32_t RS_LDX = RS_SLICE + 1;    // the row panel's stride: 33 l mod 64 is a permutation of the banks
constexpr uint32_t RS_PAD_ROW = 0xFFFFFFFFu;  // the row of RESCORE_ENTRY_PAD

enum Fold : int { FOLD_L2 = 0, FOLD_DOT = 1 };

// (k_exact.hip: fold1 / epilogue -- the same statements, so the same roundings)
template <int FOLD>
__device__ __forceinline__ float fold1(float acc, float x, float q) {
    if (FOLD == FOLD_L2) {
        float df = x - q;
        float sq = df * df;
        return acc + sq;
    } else {
        float p = x * q;
        return acc + p;
    }
}
__device__ __forceinline__ float epilogue(int metric, float acc, float xsq, float qsq) {
    if (metric == MET_L2_DIRECT) return acc;
    // distance/mod.rs:60-69: 1 - dot / max(|a|*|b|, 1e-10)
    float den = fmaxf(sqrtf(qsq) * sqrtf(xsq), 1e-10f);
    float r = acc / den;
    return 1.0f - r;
}

__device__ __forceinline__ uint32_t rs_hash(uint32_t key_low, uint32_t lg) { return (key_low * 2654435761u) >> (32 - lg); }
// the group of LOCAL row `row`, whose label is `lab` (k_fuse_groups' fg_key)
__device__ __forceinline__ uint64_t rs_key(uint32_t row, uint32_t lab) { return lab != LABEL_NONE ? uint64_t(lab) : (FUSEG_ROW_TAG | row); }

}  // namespace

__global__ __launch_bounds__(RS_THREADS) void k_rescore_fill64(uint64_t *__restrict__ p, uint64_t count, uint64_t value) {
    for (uint64_t i = uint64_t(blockIdx.x) * RS_THREADS + threadIdx.x; i < count; i += uint64_t(gridDim.x) * RS_THREADS) p[i] = value;
}

void launch_rescore_fill64(uint64_t *p, uint64_t count, uint64_t value, hipStream_t s) {
    if (count == 0) return;
    const unsigned grid = (unsigned)std::min<uint64_t>((count + RS_THREADS - 1) / RS_THREADS, 4096);
    hipLaunchKernelGGL(k_rescore_fill64, dim3(grid), dim3(RS_THREADS), 0, s, p, count, value);
    VDB_HIP(hipGetLastError());
}

// ---- collect: the group slots of a question ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RS_THREADS) void k_rescore_slots(const uint64_t *__restrict__ ids, const uint64_t *__restrict__ counts, uint64_t ld,
                                                              const uint64_t *__restrict__ coff, const uint32_t *__restrict__ labels,
                                                              uint64_t id_offset, uint32_t lg, uint64_t *__restrict__ slot_key,
                                                              uint32_t *__restrict__ slot_row, uint32_t *__restrict__ n_slots,
                                                              uint32_t *__restrict__ rows_cnt, uint64_t *tkey, uint32_t *tslot, uint32_t glg) {
    extern __shared__ __attribute__((aligned(16))) uint64_t s_keys[];  // 2^lg keys, then 2^lg first positions
    __shared__ uint32_t s_wave[RS_THREADS / 64];
    __shared__ uint32_t s_unl;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t b = blockIdx.x;
    const uint32_t cap = 1u << lg, mask = cap - 1, gmask = (1u << glg) - 1;
    uint32_t *s_pos = reinterpret_cast<uint32_t *>(s_keys + cap);
    for (uint32_t i = tid; i < cap; i += RS_THREADS) {
        s_keys[i] = FUSEG_EMPTY;
        s_pos[i] = 0xFFFFFFFFu;
    }
    if (tid == 0) s_unl = 0;
    __syncthreads();
    const uint32_t cnt = (uint32_t)(counts[b] < ld ? counts[b] : ld);
    const uint64_t *my = ids + b * ld;
    // the slot of `key` in the LDS table: its own, or the first empty one on its probe path, which becomes its own (load <= 1/2)
    auto claim = [&](uint64_t key) -> uint32_t {
        uint32_t slot = rs_hash((uint32_t)key, lg);
        for (uint32_t probe = 0; probe < cap; probe++) {
            unsigned long long seen = FUSEG_EMPTY;
            __hip_atomic_compare_exchange_strong(reinterpret_cast<unsigned long long *>(s_keys + slot), &seen, (unsigned long long)key, __ATOMIC_RELAXED,
                                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (seen == FUSEG_EMPTY || seen == key) break;
            slot = (slot + 1) & mask;
        }
        return slot;
    };
    for (uint32_t p = tid; p < cnt; p += RS_THREADS) {
        const uint32_t row = (uint32_t)(my[p] - id_offset);
        const uint32_t slot = claim(rs_key(row, labels ? labels[row] : LABEL_NONE));
        __hip_atomic_fetch_min(s_pos + slot, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    const uint64_t lt = (1ull << lane) - 1;
    uint32_t base = 0;
    for (uint32_t t0 = 0; t0 < cnt; t0 += RS_THREADS) {  // (workgroup-uniform)
        const uint32_t p = t0 + tid;
        uint32_t row = 0, lab = LABEL_NONE;
        bool first = false;
        if (p < cnt) {
            row = (uint32_t)(my[p] - id_offset);
            lab = labels ? labels[row] : LABEL_NONE;
            first = s_pos[claim(rs_key(row, lab))] == p;  // (the key is in the table: claim finds it)
        }
        const uint64_t ob = __ballot(first);
        if (lane == 0) s_wave[wave] = (uint32_t)__popcll(ob);
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t v = 0; v < RS_THREADS / 64; v++) {
            const uint32_t x = s_wave[v];
            before += v < wave ? x : 0;
            total += x;
        }
        if (first) {
            const uint32_t g = base + before + (uint32_t)__popcll(ob & lt);
            slot_key[coff[b] + g] = rs_key(row, lab);
            slot_row[coff[b] + g] = row;
            if (lab == LABEL_NONE) {
                atomicAdd(&s_unl, 1u);
            } else {  // (question, code) is new to the call's table: the question holds the code once
                const unsigned long long key = (b << 32) | lab;
                uint32_t slot = rs_hash(lab, glg);
                for (uint32_t probe = 0; probe <= gmask; probe++) {
                    unsigned long long seen = FUSEG_EMPTY;
                    __hip_atomic_compare_exchange_strong(reinterpret_cast<unsigned long long *>(tkey + slot), &seen, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                         __HIP_MEMORY_SCOPE_AGENT);
                    if (seen == FUSEG_EMPTY) {
                        tslot[slot] = g;
                        break;
                    }
                    slot = (slot + 1) & gmask;
                }
            }
        }
        base += total;
        __syncthreads();  // (s_wave is written again by the next tile)
    }
    if (tid == 0) {
        n_slots[b] = base;
        rows_cnt[b] = s_unl;
    }
}

void launch_rescore_slots(const uint64_t *ids, const uint64_t *counts, uint64_t nq, uint64_t ld, const uint64_t *coff, const uint32_t *labels,
                          uint64_t id_offset, uint64_t *slot_key, uint32_t *slot_row, uint32_t *n_slots, uint32_t *rows_cnt, uint64_t *tkey,
                          uint32_t *tslot, uint32_t glg, hipStream_t s) {
    if (nq == 0) return;
    VDB_REQUIRE(ld <= RESCORE_MAX_LD && nq < (1ull << 31) && glg >= 6 && glg <= 31, "rescore slots: list length, questions or table size");
    const uint32_t lg = rescore_dedupe_lg(ld);
    const size_t lds = size_t(12) << lg;
    func_max_lds(reinterpret_cast<const void *>(&k_rescore_slots), int(size_t(12) << rescore_dedupe_lg(RESCORE_MAX_LD)));
    hipLaunchKernelGGL(k_rescore_slots, dim3((unsigned)nq), dim3(RS_THREADS), lds, s, ids, counts, ld, coff, labels, id_offset, lg, slot_key, slot_row,
                       n_slots, rows_cnt, tkey, tslot, glg);
    VDB_HIP(hipGetLastError());
}

// ---- collect: the rows that carry a wanted code, ONE pass over the label column -----------------------------------------------------------
// Every lane of a wave reaches every ballot and shuffle: the loops below end on wave-uniform conditions only.
template <bool FILL>
__global__ __launch_bounds__(RS_THREADS) void k_rescore_match(const uint32_t *__restrict__ labels, uint64_t n, const uint64_t *__restrict__ tkey,
                                                              const uint32_t *__restrict__ tslot, uint32_t glg, uint32_t q0, uint32_t q1,
                                                              uint32_t *rows_cnt, uint32_t *cur, const uint64_t *__restrict__ ent_off,
                                                              uint64_t *__restrict__ entries) {
    const uint32_t lane = threadIdx.x & 63, gmask = (1u << glg) - 1;
    const uint64_t r = uint64_t(blockIdx.x) * RS_THREADS + threadIdx.x, lt = (1ull << lane) - 1;
    const uint32_t lab = r < n ? labels[r] : LABEL_NONE;
    bool walking = lab != LABEL_NONE;
    uint32_t slot = rs_hash(lab, glg);
    for (uint32_t probe = 0; probe <= gmask; probe++) {
        const uint64_t e = walking ? tkey[slot] : FUSEG_EMPTY;
        walking = walking && e != FUSEG_EMPTY;
        if (__ballot(walking) == 0) break;
        const uint32_t eq = (uint32_t)(e >> 32);
        const bool hit = walking && (uint32_t)e == lab && eq >= q0 && eq < q1;
        uint64_t pend = __ballot(hit);
        while (pend) {  // the lanes that hit the same question share one atomic
            const int leader = __ffsll((unsigned long long)pend) - 1;
            const uint32_t lq = __shfl(eq, leader);
            const bool mine = hit && eq == lq;
            const uint64_t same = __ballot(mine);
            const uint32_t add = (uint32_t)__popcll(same);
            if (FILL) {
                uint32_t at = 0;
                if ((int)lane == leader) at = atomicAdd(cur + lq, add);
                at = __shfl(at, leader) + (uint32_t)__popcll(same & lt);
                if (mine && at < rows_cnt[lq]) entries[ent_off[lq] + at] = (uint64_t(tslot[slot]) << 32) | r;  // (never past the counted rows)
            } else if ((int)lane == leader) {
                atomicAdd(rows_cnt + lq, add);
            }
            pend &= ~same;
        }
        slot = (slot + 1) & gmask;
    }
}

void launch_rescore_match(const uint32_t *labels, uint64_t n, const uint64_t *tkey, const uint32_t *tslot, uint32_t glg, bool fill, uint64_t q0,
                          uint64_t nb, uint32_t *rows_cnt, uint32_t *cur, const uint64_t *ent_off, uint64_t *entries, hipStream_t s) {
    if (n == 0 || nb == 0 || !labels) return;
    VDB_REQUIRE(n < (1ull << 32) && q0 + nb < (1ull << 31), "rescore match: too many rows or questions");
    const dim3 grid((unsigned)((n + RS_THREADS - 1) / RS_THREADS)), block(RS_THREADS);
    if (fill)
        hipLaunchKernelGGL(k_rescore_match<true>, grid, block, 0, s, labels, n, tkey, tslot, glg, (uint32_t)q0, (uint32_t)(q0 + nb), rows_cnt, cur, ent_off,
                           entries);
    else
        hipLaunchKernelGGL(k_rescore_match<false>, grid, block, 0, s, labels, n, tkey, tslot, glg, (uint32_t)q0, (uint32_t)(q0 + nb), rows_cnt, cur, ent_off,
                           entries);
    VDB_HIP(hipGetLastError());
}

// ---- collect: a question's minima, its unlabelled candidates and the padding of its last tile --------------------------------------------
__global__ __launch_bounds__(RS_THREADS) void k_rescore_prepare(uint64_t q0, const uint64_t *__restrict__ lims, const uint64_t *__restrict__ coff,
                                                                const uint64_t *__restrict__ slot_key, const uint32_t *__restrict__ slot_row,
                                                                const uint32_t *__restrict__ n_slots, const uint32_t *__restrict__ rows_cnt,
                                                                const uint64_t *__restrict__ ent_off, const uint64_t *__restrict__ tab_off,
                                                                uint64_t *__restrict__ entries, uint64_t *__restrict__ mins,
                                                                uint32_t *__restrict__ cur) {
    __shared__ uint32_t s_self;
    const uint64_t q = q0 + blockIdx.x;
    const uint32_t tid = threadIdx.x, ns = n_slots[q], rows = rows_cnt[q];
    const uint64_t S = lims[q + 1] - lims[q];
    uint64_t *m = mins + tab_off[q], *ent = entries + ent_off[q];
    for (uint64_t i = tid; i < ns * S; i += RS_THREADS) m[i] = FUSEG_EMPTY;
    // every entry starts as padding, not only the tail of the last tile: a place the appending pass does not reach votes nothing
    for (uint64_t i = tid; i < rescore_tiles(rows) * RESCORE_TILE; i += RS_THREADS) ent[i] = RESCORE_ENTRY_PAD;
    if (tid == 0) s_self = 0;
    __syncthreads();
    for (uint32_t g = tid; g < ns; g += RS_THREADS)
        if (slot_key[coff[q] + g] & FUSEG_ROW_TAG) {  // (at most rows_cnt[q] of them: the slots kernel counted them first)
            const uint32_t at = atomicAdd(&s_self, 1u);
            if (at < rows) ent[at] = (uint64_t(g) << 32) | slot_row[coff[q] + g];
        }
    __syncthreads();
    if (tid == 0) cur[q] = s_self;
}

void launch_rescore_prepare(uint64_t q0, uint64_t nb, const uint64_t *lims, const uint64_t *coff, const uint64_t *slot_key, const uint32_t *slot_row,
                            const uint32_t *n_slots, const uint32_t *rows_cnt, const uint64_t *ent_off, const uint64_t *tab_off, uint64_t *entries,
                            uint64_t *mins, uint32_t *cur, hipStream_t s) {
    if (nb == 0) return;
    hipLaunchKernelGGL(k_rescore_prepare, dim3((unsigned)nb), dim3(RS_THREADS), 0, s, q0, lims, coff, slot_key, slot_row, n_slots, rows_cnt, ent_off, tab_off,
                       entries, mins, cur);
    VDB_HIP(hipGetLastError());
}

// ---- pairs: every (row, sub-query) distance of a tile, the minima per (group slot, sub-query) --------------------------------------------
namespace {

// slice `cols` wide of row `lane` (xp) against NA sub-queries, 4 apart in the query panel (qp: this wave's first)
template <int FOLD, int NA>
__device__ __forceinline__ void rs_fold(float (&acc)[8], const float *xp, const float *qp, uint32_t cols) {
    if (cols == RS_SLICE) {
#pragma unroll
        for (uint32_t j = 0; j < RS_SLICE; j++) {
            const float x = xp[j];
#pragma unroll
            for (int a = 0; a < NA; a++) acc[a] = fold1<FOLD>(acc[a], x, qp[a * 4 * RS_SLICE + j]);
        }
    } else {  // the last dim % 32 elements, one by one
        for (uint32_t j = 0; j < cols; j++) {
            const float x = xp[j];
#pragma unroll
            for (int a = 0; a < NA; a++) acc[a] = fold1<FOLD>(acc[a], x, qp[a * 4 * RS_SLICE + j]);
        }
    }
}

}  // namespace

template <int FOLD>
__global__ __launch_bounds__(RS_THREADS) void k_rescore_pairs(const float *__restrict__ X, uint32_t dim, const float *__restrict__ Q,
                                                              const uint64_t *__restrict__ lims, const uint2 *__restrict__ items,
                                                              const uint64_t *__restrict__ entries, const uint64_t *__restrict__ ent_off,
                                                              uint64_t *mins, const uint64_t *__restrict__ tab_off, int metric,
                                                              const float *__restrict__ xsq, const float *__restrict__ qsq,
                                                              const uint64_t *const *__restrict__ bits) {
    __shared__ float s_x[2][RESCORE_TILE * RS_LDX];
    __shared__ float s_q[2][FUSE_MAX_LISTS * RS_SLICE];
    __shared__ uint64_t s_min[RESCORE_TILE * FUSE_MAX_LISTS];  // [leader lane][s]
    __shared__ uint32_t s_row[RESCORE_TILE], s_slot[RESCORE_TILE], s_lead[RESCORE_TILE];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint2 it = items[blockIdx.x];
    const uint64_t q = it.x, l0 = lims[q];
    const uint32_t S = (uint32_t)(lims[q + 1] - l0);
    if (tid < RESCORE_TILE) {
        const uint64_t e = entries[ent_off[q] + uint64_t(it.y) * RESCORE_TILE + tid];
        s_row[tid] = (uint32_t)e;
        s_slot[tid] = (uint32_t)(e >> 32);
    }
    for (uint32_t i = tid; i < RESCORE_TILE * FUSE_MAX_LISTS; i += RS_THREADS) s_min[i] = FUSEG_EMPTY;
    __syncthreads();
    if (tid < RESCORE_TILE) {  // the lowest lane of the tile that holds the same group
        uint32_t lead = tid;
        const uint32_t mine = s_slot[tid];
        for (uint32_t j = 0; j < RESCORE_TILE; j++)
            if (j < lead && s_row[j] != RS_PAD_ROW && s_slot[j] == mine) lead = j;
        s_lead[tid] = lead;
    }
    const float *Qq = Q + l0 * dim;
    const uint32_t nsl = (dim + RS_SLICE - 1) / RS_SLICE, c32 = tid & 31;
    float xr[8], qr[4];
    auto load_slice = [&](uint32_t c) {
        const uint32_t col = c * RS_SLICE + c32;
#pragma unroll
        for (int i = 0; i < 8; i++) {  // a half-wave per row: 128 contiguous bytes
            const uint32_t row = s_row[(tid >> 5) + 8 * i];
            xr[i] = (row != RS_PAD_ROW && col < dim) ? X[uint64_t(row) * dim + col] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t s = (tid >> 5) + 8 * i;
            qr[i] = (s < S && col < dim) ? Qq[uint64_t(s) * dim + col] : 0.0f;
        }
    };
    auto store_slice = [&](uint32_t buf) {
#pragma unroll
        for (int i = 0; i < 8; i++) s_x[buf][((tid >> 5) + 8 * i) * RS_LDX + c32] = xr[i];
#pragma unroll
        for (int i = 0; i < 4; i++) s_q[buf][((tid >> 5) + 8 * i) * RS_SLICE + c32] = qr[i];
    };
    float acc[8];
#pragma unroll
    for (int a = 0; a < 8; a++) acc[a] = 0.0f;
    const uint32_t na = S > wave ? (S - wave + 3) / 4 : 0;  // this wave's sub-queries: wave, wave + 4, ..
    load_slice(0);
    store_slice(0);
    __syncthreads();
    for (uint32_t c = 0; c < nsl; c++) {
        const uint32_t buf = c & 1;
        if (c + 1 < nsl) load_slice(c + 1);
        const uint32_t cols = dim - c * RS_SLICE < RS_SLICE ? dim - c * RS_SLICE : RS_SLICE;
        const float *xp = &s_x[buf][lane * RS_LDX], *qp = &s_q[buf][wave * RS_SLICE];
        // (wave-uniform; a variant folds up to NA sub-queries, the ones past S against a zero panel row, and they vote nothing)
        if (na > 4)
            rs_fold<FOLD, 8>(acc, xp, qp, cols);
        else if (na > 2)
            rs_fold<FOLD, 4>(acc, xp, qp, cols);
        else if (na == 2)
            rs_fold<FOLD, 2>(acc, xp, qp, cols);
        else if (na == 1)
            rs_fold<FOLD, 1>(acc, xp, qp, cols);
        if (c + 1 < nsl) store_slice(buf ^ 1);  // (the other buffer: every wave left it at the barrier that ended slice c - 1)
        __syncthreads();
    }
    const uint32_t row = s_row[lane], lead = s_lead[lane];
    const bool valid = row != RS_PAD_ROW;
    const float xs = (metric == MET_L2_DIRECT || !valid) ? 0.0f : xsq[row];
#pragma unroll
    for (int a = 0; a < 8; a++) {
        const uint32_t s = wave + 4 * a;
        if (s >= S) break;  // (wave-uniform)
        const float qs = metric == MET_L2_DIRECT ? 0.0f : qsq[l0 + s];
        const float d = epilogue(metric, acc[a], xs, qs);
        bool allowed = valid;
        if (allowed && bits) {
            const uint64_t *bm = bits[l0 + s];
            if (bm) allowed = (bm[row >> 6] >> (row & 63)) & 1ull;
        }
        if (allowed) __hip_atomic_fetch_min(&s_min[lead * FUSE_MAX_LISTS + s], pair_key(d, row), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    if (valid && lead == lane) {  // a group of the tile goes to the question's table once per sub-query
        uint64_t *m = mins + tab_off[q] + uint64_t(s_slot[lane]) * S;
        for (uint32_t s = wave; s < S; s += 4) {
            const uint64_t v = s_min[lane * FUSE_MAX_LISTS + s];
            if (v != FUSEG_EMPTY) __hip_atomic_fetch_min(m + s, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

void launch_rescore_pairs(const float *X, uint32_t dim, const float *Q, const uint64_t *lims, const uint2 *items, uint64_t n_items,
                          const uint64_t *entries, const uint64_t *ent_off, uint64_t *mins, const uint64_t *tab_off, int metric, const float *xsq,
                          const float *qsq, const uint64_t *const *bits, hipStream_t s) {
    if (n_items == 0) return;
    VDB_REQUIRE(metric == MET_L2_DIRECT || metric == MET_COSINE, "rescore pairs: metric");
    VDB_REQUIRE(n_items < (1ull << 31) && dim >= 1, "rescore pairs: too many work items or no dimension");
    const dim3 grid((unsigned)n_items), block(RS_THREADS);
    if (metric == MET_L2_DIRECT)
        hipLaunchKernelGGL(k_rescore_pairs<FOLD_L2>, grid, block, 0, s, X, dim, Q, lims, items, entries, ent_off, mins, tab_off, metric, xsq, qsq, bits);
    else
        hipLaunchKernelGGL(k_rescore_pairs<FOLD_DOT>, grid, block, 0, s, X, dim, Q, lims, items, entries, ent_off, mins, tab_off, metric, xsq, qsq, bits);
    VDB_HIP(hipGetLastError());
}

// ---- finish: scores, representatives, the order ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(RS_THREADS) void k_rescore_finish(uint64_t q0, const uint64_t *__restrict__ lims, const uint64_t *__restrict__ coff,
                                                               const uint32_t *__restrict__ slot_row, const uint32_t *__restrict__ n_slots,
                                                               const uint64_t *__restrict__ mins, const uint64_t *__restrict__ tab_off, int mode,
                                                               uint64_t id_offset, uint32_t k, uint64_t *__restrict__ out_idx,
                                                               float *__restrict__ out_dist, uint64_t *__restrict__ out_cnt) {
    __shared__ uint64_t keys[RESCORE_MAX_LD];
    const uint32_t tid = threadIdx.x;
    const uint64_t q = q0 + blockIdx.x;
    const uint32_t S = (uint32_t)(lims[q + 1] - lims[q]);
    const uint32_t ns = n_slots[q] < RESCORE_MAX_LD ? n_slots[q] : (uint32_t)RESCORE_MAX_LD;
    const uint64_t *m = mins + tab_off[q];
    for (uint32_t g = tid; g < ns; g += RS_THREADS) {
        float acc = 0.0f;
        uint64_t best = FUSEG_EMPTY;  // the smallest (order key, row) over the sub-queries, the first s on a tie of the key
        for (uint32_t s = 0; s < S; s++) {
            const uint64_t v = m[uint64_t(g) * S + s];
            const float d = v == FUSEG_EMPTY ? __uint_as_float(0x7F800000u) : f32_from_orderable((uint32_t)(v >> 32));
            acc = acc + d;
            if (v != FUSEG_EMPTY && (best == FUSEG_EMPTY || (uint32_t)(v >> 32) < (uint32_t)(best >> 32))) best = v;
        }
        const uint32_t rep = best == FUSEG_EMPTY ? slot_row[coff[q] + g] : (uint32_t)best;
        const float score = mode == FUSE_SUM ? acc : (best == FUSEG_EMPTY ? __uint_as_float(0x7F800000u) : f32_from_orderable((uint32_t)(best >> 32)));
        keys[g] = pair_key(score, rep);  // (a NaN sum leaves as 0x7FC00000: the order key holds one NaN)
    }
    uint32_t np = 2;
    while (np < ns) np <<= 1;  // (<= RESCORE_MAX_LD)
    for (uint32_t i = ns + tid; i < np; i += RS_THREADS) keys[i] = PAIR_NONE;
    __syncthreads();
    for (uint32_t kk = 2; kk <= np; kk <<= 1) {
        for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
            for (uint32_t i = tid; i < (np >> 1); i += RS_THREADS) {
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
    const uint32_t take = ns < k ? ns : k;
    for (uint32_t i = tid; i < k; i += RS_THREADS) {
        out_idx[q * k + i] = i < take ? uint64_t((uint32_t)keys[i]) + id_offset : 0;
        out_dist[q * k + i] = i < take ? f32_from_orderable((uint32_t)(keys[i] >> 32)) : 0.0f;
    }
    if (tid == 0) out_cnt[q] = take;
}

void launch_rescore_finish(uint64_t q0, uint64_t nb, const uint64_t *lims, const uint64_t *coff, const uint32_t *slot_row, const uint32_t *n_slots,
                           const uint64_t *mins, const uint64_t *tab_off, int mode, uint64_t id_offset, uint32_t k, uint64_t *out_idx, float *out_dist,
                           uint64_t *out_cnt, hipStream_t s) {
    if (nb == 0) return;
    VDB_REQUIRE(k <= RESCORE_MAX_LD && (mode == FUSE_SUM || mode == FUSE_MIN), "rescore finish: k or mode");
    hipLaunchKernelGGL(k_rescore_finish, dim3((unsigned)nb), dim3(RS_THREADS), 0, s, q0, lims, coff, slot_row, n_slots, mins, tab_off, mode, id_offset, k,
                       out_idx, out_dist, out_cnt);
    VDB_HIP(hipGetLastError());
}

}  // namespace vdb
