// k_lookup.hip -- the key lookup over ONE label column (Index::label_lookup; lookup_plan.hpp; docs/DESIGN_flat.md 4.1aa): for every code
// of a list the number of rows that carry it and the lowest such row, in one read of the column.  The grid is k_label_counts': a wave
// per 64-row word, grid-strided.  A lane loads its row's code once and resolves it to a slot or none -- by binary search over a chunk's
// sorted table in LDS (k_label_lookup) or by one gather from slot_of[code - base] (k_label_lookup_direct).  The wave then walks its
// distinct slots as k_mask_partition does: the slot of the lowest pending lane (uniform), the ballot of "my slot is that one", and that
// lowest lane -- whose row is the lowest of the word that carries the slot -- keeps the popcount; those lanes retire.  After the walk
// the leaders, one lane per distinct slot, add their popcount and take the min with their row, in ONE atomic instruction each: a column
// where most rows share a code makes one atomic per wave, not 64.  Only integer atomicAdd / atomicMin touch the outputs, so the answer
// does not depend on the order of waves.
#include <algorithm>

#include "kernels.hpp"

namespace vdb {

// cnt[slot] += the wave's rows with that slot; first[slot] = min(first[slot], the lowest of them).  `row` fits 32 bits.
__device__ __forceinline__ void lookup_wave(uint32_t slot, uint32_t row, uint32_t lane, uint32_t *cnt, uint32_t *first) {
    uint64_t pending = __ballot(slot != LOOKUP_NO_SLOT);
    uint32_t mine = 0;  // > 0: this lane leads its slot
    while (pending) {   // (wave-uniform)
        const uint32_t lead = (uint32_t)__ffsll((unsigned long long)pending) - 1;
        const uint32_t cur = (uint32_t)__shfl((int)slot, (int)lead);
        const uint64_t w = __ballot(slot == cur);  // (the lead lane is its lowest bit: every lane of this slot is still pending)
        if (lane == lead) mine = (uint32_t)__popcll(w);
        pending &= ~w;
    }
    if (mine) {
        atomicAdd(&cnt[slot], mine);
        atomicMin(&first[slot], row);
    }
}

// Sorted route: table = the chunk's nb (<= PART_MAX_CHUNK) codes ascending.  counts[i] += rows whose code is table[i], first[i] = the
// lowest of them; the caller has set counts to zero and first to LOOKUP_ROW_NONE32.  A workgroup keeps the chunk's counters and firsts
// in LDS and flushes the slots it met, once.  col == nullptr: a column never written, LABEL_NONE in every row without a load.
__global__ __launch_bounds__(256) void k_label_lookup(const uint32_t *__restrict__ col, const uint32_t *__restrict__ table, uint32_t nb, uint64_t n,
                                                      uint32_t nwords, uint32_t *__restrict__ counts, uint32_t *__restrict__ first) {
    __shared__ uint32_t s_code[PART_MAX_CHUNK], s_cnt[PART_MAX_CHUNK], s_first[PART_MAX_CHUNK];
    for (uint32_t i = threadIdx.x; i < nb; i += 256) {
        s_code[i] = table[i];
        s_cnt[i] = 0;
        s_first[i] = LOOKUP_ROW_NONE32;
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t word = blockIdx.x * 4 + wave; word < nwords; word += gridDim.x * 4) {  // (wave-uniform)
        const uint64_t row = uint64_t(word) * 64 + lane;
        const bool in = row < n;
        const uint32_t v = (col && in) ? col[row] : LABEL_NONE;
        const uint32_t pos = mask_partition_find(s_code, nb, v);  // (below nb, or PART_NO_SLOT == LOOKUP_NO_SLOT)
        lookup_wave(in ? pos : LOOKUP_NO_SLOT, (uint32_t)row, lane, s_cnt, s_first);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nb; i += 256) {
        const uint32_t c = s_cnt[i];
        if (c) {
            atomicAdd(&counts[i], c);
            atomicMin(&first[i], s_first[i]);
        }
    }
}

// Direct route: slot_of[code - base] for base <= code < base + span, none_slot for LABEL_NONE (by value; LOOKUP_NO_SLOT: not asked
// for), no slot elsewhere.  A lane gathers 4 bytes only after ITS OWN range test passed, so the index is below span.  counts / first
// [n_codes] in the caller's order, prepared as above; the leaders' atomics go to global memory.
__global__ __launch_bounds__(256) void k_label_lookup_direct(const uint32_t *__restrict__ col, const uint32_t *__restrict__ slot_of, uint32_t base,
                                                             uint32_t span, uint32_t none_slot, uint64_t n, uint32_t nwords,
                                                             uint32_t *__restrict__ counts, uint32_t *__restrict__ first) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t word = blockIdx.x * 4 + wave; word < nwords; word += gridDim.x * 4) {  // (wave-uniform)
        const uint64_t row = uint64_t(word) * 64 + lane;
        const bool in = row < n;
        const uint32_t v = (col && in) ? col[row] : LABEL_NONE;
        const uint32_t off = v - base;
        uint32_t slot = LOOKUP_NO_SLOT;
        if (in) {
            if (v == LABEL_NONE)
                slot = none_slot;
            else if (v >= base && off < span)
                slot = slot_of[off];
        }
        lookup_wave(slot, (uint32_t)row, lane, counts, first);
    }
}

// slot_of[codes[j] - base] = j for the codes other than LABEL_NONE (distinct, inside [base, base + span): lookup_plan.hpp); the caller
// has filled slot_of with LOOKUP_NO_SLOT.
__global__ __launch_bounds__(256) void k_lookup_table(const uint32_t *__restrict__ codes, uint64_t n_codes, uint32_t base, uint32_t span,
                                                      uint32_t *__restrict__ slot_of) {
    const uint64_t stride = uint64_t(gridDim.x) * 256;
    for (uint64_t j = uint64_t(blockIdx.x) * 256 + threadIdx.x; j < n_codes; j += stride) {
        const uint32_t c = codes[j];
        const uint32_t off = c - base;
        if (c != LABEL_NONE && c >= base && off < span) slot_of[off] = (uint32_t)j;
    }
}

static_assert(PART_NO_SLOT == LOOKUP_NO_SLOT, "mask_partition_find's miss is the walk's no-slot");

static unsigned label_lookup_grid(uint64_t n, int num_cu, uint32_t max_blocks) {
    const uint64_t cap = max_blocks ? uint64_t(max_blocks) : uint64_t(std::max(num_cu, 1)) * 8;
    return (unsigned)std::min<uint64_t>(mask_where_blocks(n), cap);
}
void launch_label_lookup(const uint32_t *col, const uint32_t *table, uint32_t nb, uint64_t n, uint32_t *counts, uint32_t *first, int num_cu,
                         uint32_t max_blocks, hipStream_t s) {
    const uint32_t nwords = (uint32_t)((n + 63) / 64);
    if (nb == 0 || nwords == 0) return;
    hipLaunchKernelGGL(k_label_lookup, dim3(label_lookup_grid(n, num_cu, max_blocks)), dim3(256), 0, s, col, table, nb, n, nwords, counts, first);
}
void launch_label_lookup_direct(const uint32_t *col, const uint32_t *slot_of, uint32_t base, uint32_t span, uint32_t none_slot, uint64_t n,
                                uint32_t *counts, uint32_t *first, int num_cu, uint32_t max_blocks, hipStream_t s) {
    const uint32_t nwords = (uint32_t)((n + 63) / 64);
    if (nwords == 0) return;
    hipLaunchKernelGGL(k_label_lookup_direct, dim3(label_lookup_grid(n, num_cu, max_blocks)), dim3(256), 0, s, col, slot_of, base, span, none_slot, n,
                       nwords, counts, first);
}
void launch_lookup_table(const uint32_t *codes, uint64_t n_codes, uint32_t base, uint32_t span, uint32_t *slot_of, int num_cu, hipStream_t s) {
    if (n_codes == 0) return;
    const unsigned grid = (unsigned)std::min<uint64_t>((n_codes + 255) / 256, uint64_t(std::max(num_cu, 1)) * 8);
    hipLaunchKernelGGL(k_lookup_table, dim3(grid), dim3(256), 0, s, codes, n_codes, base, span, slot_of);
}

}  // namespace vdb
