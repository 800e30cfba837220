// k_labels.hip -- label columns (one u32 per row and column, Index::d_labels) and the row masks built from them on the device
// (index_masks.hip): upkeep of the columns under add / swap_remove / remove_rows; k_mask_rows<Pred>, k_mask_scan and k_mask_ids, which turn
// a predicate over the columns into a RowMask's bit words and its ascending allow-list -- Pred = a conjunction of `column == code` terms
// (MaskEq; docs/DESIGN_flat.md 4.1l), of set / range terms (MaskAll, mask_sets.hpp; 4.1m) or an OR of such conjunctions (MaskAny,
// mask_any.hpp; 4.1o) -- and the same for the AND / OR / NOT of finished masks (k_mask_combine; 4.1o); and the two kernels that group ONE column
// by code in a single read of it -- into the masks of many values (Index::masks_partition) or into rows per value (Index::label_counts;
// mask_partition.hpp; 4.1p); and the two kernels that write codes to scattered rows of several columns in one launch -- per row of an id
// list, or one code per column over a mask's rows (Index::labels_scatter, labels_set_mask; labels_scatter_plan.hpp; 4.1t).
#include <algorithm>

#include "kernels.hpp"

namespace vdb {

// ---- upkeep ------------------------------------------------------------------------------------------------------------------------------
// col[r] = LABEL_NONE for r in [r0, r1) of every column of `cols` (blockIdx.y = column)
__global__ __launch_bounds__(256) void k_label_fill(LabelCols cols, uint64_t r0, uint64_t r1) {
    uint32_t *col = cols.col[blockIdx.y];
    const uint64_t stride = uint64_t(gridDim.x) * 256;
    for (uint64_t r = r0 + uint64_t(blockIdx.x) * 256 + threadIdx.x; r < r1; r += stride) col[r] = LABEL_NONE;
}

// col[dst] = col[src] for every move of a removal plan (moves[2 j] = dst, moves[2 j + 1] = src: k_remove.hip) and every column of `cols`
// (blockIdx.y = column).  Every src lies above every dst, so no lane reads what another writes.  moves == nullptr: the one move
// (one_dst, one_src) of swap_remove.
__global__ __launch_bounds__(256) void k_label_move(LabelCols cols, const uint32_t *__restrict__ moves, uint64_t n_moves, uint32_t one_dst,
                                                    uint32_t one_src) {
    uint32_t *col = cols.col[blockIdx.y];
    const uint64_t stride = uint64_t(gridDim.x) * 256;
    for (uint64_t j = uint64_t(blockIdx.x) * 256 + threadIdx.x; j < n_moves; j += stride) {
        const uint32_t dst = moves ? moves[2 * j] : one_dst, src = moves ? moves[2 * j + 1] : one_src;
        col[dst] = col[src];
    }
}

void launch_label_fill(const LabelCols &cols, uint64_t r0, uint64_t r1, int num_cu, hipStream_t s) {
    if (cols.n == 0 || r1 <= r0) return;
    const unsigned grid = (unsigned)std::min<uint64_t>((r1 - r0 + 255) / 256, uint64_t(num_cu) * 8);
    hipLaunchKernelGGL(k_label_fill, dim3(grid, cols.n), dim3(256), 0, s, cols, r0, r1);
}
void launch_label_move(const LabelCols &cols, const uint32_t *moves, uint64_t n_moves, int num_cu, hipStream_t s) {
    if (cols.n == 0 || n_moves == 0) return;
    const unsigned grid = (unsigned)std::min<uint64_t>((n_moves + 255) / 256, uint64_t(num_cu) * 8);
    hipLaunchKernelGGL(k_label_move, dim3(grid, cols.n), dim3(256), 0, s, cols, moves, n_moves, 0u, 0u);
}
void launch_label_move_one(const LabelCols &cols, uint32_t dst, uint32_t src, hipStream_t s) {
    if (cols.n == 0) return;
    hipLaunchKernelGGL(k_label_move, dim3(1, cols.n), dim3(256), 0, s, cols, static_cast<const uint32_t *>(nullptr), uint64_t(1), dst, src);
}

// ---- masks from labels ---------------------------------------------------------------------------------------------------------------------
// One wave = one mask word, one lane = one row: on a 64-lane wave the ballot of "this row matches" IS the word (bit l = row 64 w + l), so
// the bit words need no shuffles, no atomics and no LDS.  Grid (ceil(words / 4), masks of the chunk), 256 threads = 4 waves = 4 words.
// A lane asks the predicate about its row -- rows at and past n are false, so the tail bits of the last word stay clear -- and lane 0
// stores the ballot.  blockcnt[mask][block] = allowed rows of the block's (up to) four words.  Pred (kernels.hpp: MaskEq, MaskAll,
// MaskAny; by value, its tables in scalars) says whether row `row` of the index matches job's range [job.t0, job.t1) of its table;
// `in` = row < n, and a predicate loads nothing of a row that is not in.
template <class Pred>
__global__ __launch_bounds__(256) void k_mask_rows(Pred pred, const MaskJob *__restrict__ jobs, uint64_t n, uint32_t nwords, uint32_t nblocks,
                                                   uint32_t *__restrict__ blockcnt) {
    __shared__ uint32_t s_cnt[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const MaskJob job = jobs[blockIdx.y];
    const uint32_t word = blockIdx.x * 4 + wave;
    const uint64_t row = uint64_t(word) * 64 + lane;
    const bool in = row < n;
    const uint64_t w = __ballot(pred(job, row, in));
    if (lane == 0) {
        if (word < nwords) job.bits[word] = w;
        s_cnt[wave] = (uint32_t)__popcll(w);  // (a word at or past nwords has no row below n: 0)
    }
    __syncthreads();
    if (threadIdx.x == 0) blockcnt[size_t(blockIdx.y) * nblocks + blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// A conjunction of `column == code` terms (docs/DESIGN_flat.md 4.1l).  A lane loads its row's value of every term column (4 B per lane,
// 256 B per wave and term, contiguous) and ANDs the comparisons.  A null column (never written) reads as LABEL_NONE for every row; zero
// terms allow every row.
__device__ __forceinline__ bool MaskEq::operator()(const MaskJob &job, uint64_t row, bool in) const {
    bool ok = in;
    for (uint32_t t = job.t0; t < job.t1; t++) {  // (wave-uniform)
        const MaskTerm tm = terms[t];
        const uint32_t v = (tm.col && in) ? tm.col[row] : LABEL_NONE;
        ok = ok && v == tm.code;
    }
    return ok;
}

// SET / RANGE terms (mask_sets.hpp; docs/DESIGN_flat.md 4.1m): a term is {col, lo, hi, flags, bitmap}.  A row without a value
// (LABEL_NONE, or a null column) matches iff the term has TERM_NONE, whatever TERM_NEGATE says; a labelled row is inside when
// lo <= v <= hi and, with a bitmap, bit (v - lo) of it is set, and matches when inside != TERM_NEGATE.
// Both loads are selects: a lane at or past n reads no column, and a lane reads a bitmap word only after ITS OWN range test passed, so
// (v - lo) >> 6 is below the bitmap's ceil((hi - lo + 1) / 64) words.  The bitmap read is a per-lane gather of one 8-byte word from a
// block of at most a few KiB that every wave of the mask re-reads: it stays in cache, and LDS staging per 256-row workgroup would move
// more bytes than the gather does.
__device__ __forceinline__ bool set_term_match(const SetTerm tm, uint64_t row, bool in) {
    const uint32_t v = (tm.col && in) ? tm.col[row] : LABEL_NONE;
    const bool labelled = v != LABEL_NONE;
    const uint32_t off = v - tm.lo;
    bool inside = labelled && tm.lo <= v && v <= tm.hi;
    const uint64_t bw = (inside && tm.bitmap) ? tm.bitmap[off >> 6] : ~0ull;
    inside = inside && ((bw >> (off & 63)) & 1);
    return labelled ? inside != bool(tm.flags & TERM_NEGATE) : bool(tm.flags & TERM_NONE);
}
// a conjunction of such terms
__device__ __forceinline__ bool MaskAll::operator()(const MaskJob &job, uint64_t row, bool in) const {
    bool ok = in;
    for (uint32_t t = job.t0; t < job.t1; t++) {  // (wave-uniform)
        ok = ok && set_term_match(terms[t], row, in);
    }
    return ok;
}

// An OR of up to MASK_MAX_CLAUSES such conjunctions (mask_any.hpp; docs/DESIGN_flat.md 4.1o): an outer loop over the mask's clauses
// [job.t0, job.t1) of the clause table -- clause c is terms [clims[c], clims[c + 1]).  Both loops are wave-uniform.  okc = in-range AND
// every term of the clause (set_term_match: the loads keep their two rules), any |= okc; rows at and past n are false in every clause,
// so the tail bits stay clear; a mask without clauses is empty, a clause without terms allows every row.  A column that several
// clauses name is re-read from cache.  (A wave-uniform exit from the clause loop once every in-range lane is allowed was measured and
// bought nothing: docs/DESIGN_flat.md 4.1o.)
__device__ __forceinline__ bool MaskAny::operator()(const MaskJob &job, uint64_t row, bool in) const {
    bool any = false;
    for (uint32_t c = job.t0; c < job.t1; c++) {  // (wave-uniform)
        const uint32_t t1 = clims[c + 1];
        bool okc = in;
        for (uint32_t t = clims[c]; t < t1; t++) okc = okc && set_term_match(terms[t], row, in);  // (wave-uniform)
        any = any || okc;
    }
    return any;
}

// AND / OR of up to MASK_COMBINE_MAX finished masks, input i complemented first when bit i of a.invert is set.  One thread per entry of
// blockcnt, i.e. per four output words (32 contiguous bytes of every input): it writes the words and their popcount, which is the
// blockcnt contract of the kernels above, so k_mask_scan and k_mask_ids follow unchanged.  The bits at and past n of the last word are
// cleared after the operation: a complement stays within the index's rows.
__global__ __launch_bounds__(256) void k_mask_combine(MaskCombine a, uint64_t *__restrict__ out, uint64_t n, uint32_t nwords, uint32_t nblocks,
                                                      uint32_t *__restrict__ blockcnt) {
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nblocks) return;
    uint32_t cnt = 0;
    for (uint32_t u = 0; u < 4; u++) {
        const uint32_t word = b * 4 + u;
        if (word >= nwords) break;
        uint64_t acc = a.op == MASK_OP_AND ? ~0ull : 0ull;
        for (uint32_t i = 0; i < a.n_in; i++) {
            const uint64_t w = a.in[i][word] ^ (((a.invert >> i) & 1) ? ~0ull : 0ull);
            acc = a.op == MASK_OP_AND ? acc & w : acc | w;
        }
        if (word == nwords - 1 && (n & 63)) acc &= (1ull << (n & 63)) - 1;
        out[word] = acc;
        cnt += (uint32_t)__popcll(acc);
    }
    blockcnt[b] = cnt;
}

// One workgroup per mask: blockcnt[mask][0 .. nblocks) -> its exclusive prefix sums, in place; totals[mask] = the sum (the mask's m).
// 256 counts per iteration (a shuffle scan inside the wave, the four wave sums through LDS), the running sum carried over iterations.
__global__ __launch_bounds__(256) void k_mask_scan(uint32_t *__restrict__ blockcnt, uint32_t nblocks, uint32_t *__restrict__ totals) {
    __shared__ uint32_t s_wave[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t *cnt = blockcnt + size_t(blockIdx.x) * nblocks;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nblocks; base += 256) {  // (block-uniform trip count)
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < nblocks ? cnt[i] : 0;
        uint32_t incl = v;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t u = 0; u < 4; u++) {
            const uint32_t x = s_wave[u];
            if (u < wave) before += x;
            all += x;
        }
        if (i < nblocks) cnt[i] = carry + before + incl - v;
        carry += all;
        __syncthreads();  // (s_wave is rewritten by the next iteration)
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// Same grid as k_mask_rows.  A wave re-reads its word; the lane whose bit is set writes its row at
//   blockoff[mask][block] + popcounts of the block's earlier words + popcount(word & lanes below):
// positions ascend with the row, so the allow-list is ascending without a sort.  ids[mask] holds exactly totals[mask] entries.
__global__ __launch_bounds__(256) void k_mask_ids(const MaskJob *__restrict__ jobs, uint32_t *const *__restrict__ ids, uint32_t nwords,
                                                  uint32_t nblocks, const uint32_t *__restrict__ blockoff) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t word = blockIdx.x * 4 + wave;
    if (word >= nwords) return;  // (wave-uniform; no barrier below)
    const uint64_t *bits = jobs[blockIdx.y].bits;
    uint32_t *out = ids[blockIdx.y];
    const uint64_t w = bits[word];
    if (w == 0) return;
    uint32_t off = blockoff[size_t(blockIdx.y) * nblocks + blockIdx.x];
    for (uint32_t u = 0; u < wave; u++) off += (uint32_t)__popcll(bits[blockIdx.x * 4 + u]);
    if ((w >> lane) & 1) out[off + (uint32_t)__popcll(w & ((1ull << lane) - 1))] = word * 64 + lane;
}

template <class Pred>
void launch_mask_rows(Pred pred, const MaskJob *jobs, uint32_t n_masks, uint64_t n, uint32_t *blockcnt, uint32_t *totals, hipStream_t s) {
    const uint32_t nwords = (uint32_t)((n + 63) / 64), nblocks = mask_where_blocks(n);
    if (n_masks == 0 || nblocks == 0) return;
    hipLaunchKernelGGL(k_mask_rows<Pred>, dim3(nblocks, n_masks), dim3(256), 0, s, pred, jobs, n, nwords, nblocks, blockcnt);
    hipLaunchKernelGGL(k_mask_scan, dim3(n_masks), dim3(256), 0, s, blockcnt, nblocks, totals);
}
template void launch_mask_rows(MaskEq, const MaskJob *, uint32_t, uint64_t, uint32_t *, uint32_t *, hipStream_t);
template void launch_mask_rows(MaskAll, const MaskJob *, uint32_t, uint64_t, uint32_t *, uint32_t *, hipStream_t);
template void launch_mask_rows(MaskAny, const MaskJob *, uint32_t, uint64_t, uint32_t *, uint32_t *, hipStream_t);
void launch_mask_combine(const MaskCombine &a, uint64_t *out, uint64_t n, uint32_t *blockcnt, uint32_t *totals, hipStream_t s) {
    const uint32_t nwords = (uint32_t)((n + 63) / 64), nblocks = mask_where_blocks(n);
    if (nblocks == 0) return;
    hipLaunchKernelGGL(k_mask_combine, dim3((nblocks + 255) / 256), dim3(256), 0, s, a, out, n, nwords, nblocks, blockcnt);
    hipLaunchKernelGGL(k_mask_scan, dim3(1), dim3(256), 0, s, blockcnt, nblocks, totals);
}
void launch_mask_ids(const MaskJob *jobs, uint32_t *const *ids, uint32_t n_masks, uint64_t n, const uint32_t *blockoff, hipStream_t s) {
    const uint32_t nwords = (uint32_t)((n + 63) / 64), nblocks = mask_where_blocks(n);
    if (n_masks == 0 || nblocks == 0) return;
    hipLaunchKernelGGL(k_mask_ids, dim3(nblocks, n_masks), dim3(256), 0, s, jobs, ids, nwords, nblocks, blockoff);
}

// ---- one column grouped by code (mask_partition.hpp; docs/DESIGN_flat.md 4.1p) -----------------------------------------------------------
// The masks of up to PART_MAX_CHUNK DISTINCT codes of ONE column in one read of it: the grid over words of k_mask_rows with grid.y == 1.
// The workgroup stages the chunk's table -- the codes ascending, and for each the mask (slot) it belongs to -- in LDS; a lane loads its
// row's code once and binary-searches it (mask_partition_find), which gives it one slot or none.  The wave then walks its distinct
// slots: the slot of the first pending lane (uniform), the ballot of "my slot is that one" IS that mask's word, lane 0 stores it and adds
// its popcount to blockcnt[slot][block], and those lanes retire -- at most 64 rounds, usually as many as the wave has distinct codes.
// The bit words and the counts are zero before the launch (launch_mask_partition clears them), so every word no wave writes is already
// right; rows at and past n have no slot, so the tail bits stay clear; a null column is LABEL_NONE in every row without a load.  The
// four waves of a block may add to one count: integer adds, the sum does not depend on their order.  blockcnt then holds what
// k_mask_rows leaves there, so k_mask_scan and k_mask_ids follow unchanged.
__global__ __launch_bounds__(256) void k_mask_partition(const uint32_t *__restrict__ col, const uint32_t *__restrict__ table, uint32_t nb,
                                                        const MaskJob *__restrict__ jobs, uint64_t n, uint32_t nwords, uint32_t nblocks,
                                                        uint32_t *__restrict__ blockcnt) {
    __shared__ uint32_t s_code[PART_MAX_CHUNK], s_slot[PART_MAX_CHUNK];
    for (uint32_t i = threadIdx.x; i < nb; i += 256) {
        s_code[i] = table[i];
        s_slot[i] = table[nb + i];
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t word = blockIdx.x * 4 + wave;
    const uint64_t row = uint64_t(word) * 64 + lane;
    const bool in = row < n;
    const uint32_t v = (col && in) ? col[row] : LABEL_NONE;
    const uint32_t pos = mask_partition_find(s_code, nb, v);
    uint32_t slot = (in && pos != PART_NO_SLOT) ? s_slot[pos] : PART_NO_SLOT;  // (a lane in range makes word < nwords)
    uint64_t pending = __ballot(slot != PART_NO_SLOT);
    while (pending) {  // (wave-uniform)
        const uint32_t cur = (uint32_t)__shfl((int)slot, __ffsll((unsigned long long)pending) - 1);
        const uint64_t w = __ballot(slot == cur);
        if (lane == 0) {
            jobs[cur].bits[word] = w;
            atomicAdd(&blockcnt[size_t(cur) * nblocks + blockIdx.x], (uint32_t)__popcll(w));
        }
        pending &= ~w;
    }
}

// The number of rows per code of the same table, over all rows or under a mask: counts[i] += rows whose code is table[i].  A workgroup
// keeps the chunk's counters in LDS and walks the words grid-strided, a wave per word as above; under a mask the wave reads its 8-byte
// mask word and lanes with a clear bit sit out.  At the end the non-zero counters are flushed with global integer adds (counts is zero
// before the launch).  An index has fewer than 2^32 rows: no counter overflows.
__global__ __launch_bounds__(256) void k_label_counts(const uint32_t *__restrict__ col, const uint32_t *__restrict__ table, uint32_t nb,
                                                      const uint64_t *__restrict__ bits, uint64_t n, uint32_t nwords,
                                                      uint32_t *__restrict__ counts) {
    __shared__ uint32_t s_code[PART_MAX_CHUNK], s_cnt[PART_MAX_CHUNK];
    for (uint32_t i = threadIdx.x; i < nb; i += 256) {
        s_code[i] = table[i];
        s_cnt[i] = 0;
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t word = blockIdx.x * 4 + wave; word < nwords; word += gridDim.x * 4) {  // (wave-uniform)
        const uint64_t row = uint64_t(word) * 64 + lane;
        const uint64_t mw = bits ? bits[word] : ~0ull;
        const bool in = row < n && ((mw >> lane) & 1);
        const uint32_t v = (col && in) ? col[row] : LABEL_NONE;
        const uint32_t pos = mask_partition_find(s_code, nb, v);
        if (in && pos != PART_NO_SLOT) atomicAdd(&s_cnt[pos], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nb; i += 256) {
        const uint32_t c = s_cnt[i];
        if (c) atomicAdd(&counts[i], c);
    }
}

void launch_mask_partition(const uint32_t *col, const uint32_t *table, uint32_t nb, const MaskJob *jobs, uint64_t n, uint32_t *blockcnt,
                           uint32_t *totals, hipStream_t s) {
    const uint32_t nwords = (uint32_t)((n + 63) / 64), nblocks = mask_where_blocks(n);
    if (nb == 0 || nblocks == 0) return;
    hipLaunchKernelGGL(k_mask_partition, dim3(nblocks), dim3(256), 0, s, col, table, nb, jobs, n, nwords, nblocks, blockcnt);
    hipLaunchKernelGGL(k_mask_scan, dim3(nb), dim3(256), 0, s, blockcnt, nblocks, totals);
}
void launch_label_counts(const uint32_t *col, const uint32_t *table, uint32_t nb, const uint64_t *bits, uint64_t n, uint32_t *counts,
                         int num_cu, hipStream_t s) {
    const uint32_t nwords = (uint32_t)((n + 63) / 64), nblocks = mask_where_blocks(n);
    if (nb == 0 || nblocks == 0) return;
    const unsigned grid = (unsigned)std::min<uint64_t>(nblocks, uint64_t(num_cu) * 8);
    hipLaunchKernelGGL(k_label_counts, dim3(grid), dim3(256), 0, s, col, table, nb, bits, n, nwords, counts);
}

// ---- scattered writes (Index::labels_scatter*, labels_set_mask; docs/DESIGN_flat.md 4.1t) ---------------------------------------------------
// col[c][ids[j] - id_offset] = codes[c][j] for every column c of `cols` and every list entry j < m: ONE launch whatever cols.n is.  A
// lane owns entry j, grid-stride: it loads its id once (coalesced), then per column one coalesced load of its code and one plain
// scattered 4-byte store.  The column loop is wave-uniform, the column pointers come from the by-value table.  No atomics, no LDS: the ids
// are distinct (labels_scatter_plan.hpp) or, in the device form, an id named twice gets one of its codes, whole.  Id = u32 local rows
// (id_offset 0) or u64 global ids; the caller checked them (k_fetch_check for the device form), and a row fits 32 bits since an index
// has fewer than 2^32 rows.  codes + c * m is formed in 64 bits: n_cols x m may pass 2^32.
template <class Id>
__global__ __launch_bounds__(256) void k_labels_scatter(LabelCols cols, const Id *__restrict__ ids, uint64_t id_offset,
                                                        const uint32_t *__restrict__ codes, uint64_t m) {
    const uint64_t stride = uint64_t(gridDim.x) * 256;
    for (uint64_t j = uint64_t(blockIdx.x) * 256 + threadIdx.x; j < m; j += stride) {
        const uint32_t row = uint32_t(uint64_t(ids[j]) - id_offset);
        for (uint32_t c = 0; c < cols.n; c++) cols.col[c][row] = codes[uint64_t(c) * m + j];
    }
}

// col[c][ids[j]] = set.code[c] for every (column, code) pair of `set` and every j < m: ids = a RowMask's ascending allow-list (u32 local
// rows).  Pairs and list travel by value / by pointer: nothing is uploaded.
__global__ __launch_bounds__(256) void k_labels_set_mask(LabelSet set, const uint32_t *__restrict__ ids, uint64_t m) {
    const uint64_t stride = uint64_t(gridDim.x) * 256;
    for (uint64_t j = uint64_t(blockIdx.x) * 256 + threadIdx.x; j < m; j += stride) {
        const uint32_t row = ids[j];
        for (uint32_t c = 0; c < set.n; c++) set.col[c][row] = set.code[c];
    }
}

uint64_t labels_scatter_span(int num_cu, uint32_t max_blocks) {
    return (max_blocks ? uint64_t(max_blocks) : uint64_t(std::max(num_cu, 1)) * 8) * 256;
}
static unsigned labels_scatter_grid(uint64_t m, int num_cu, uint32_t max_blocks) {
    return (unsigned)std::min<uint64_t>((m + 255) / 256, labels_scatter_span(num_cu, max_blocks) / 256);
}
void launch_labels_scatter(const LabelCols &cols, const void *ids, bool ids_u64, uint64_t id_offset, const uint32_t *codes, uint64_t m,
                           int num_cu, uint32_t max_blocks, hipStream_t s) {
    if (cols.n == 0 || m == 0) return;
    const unsigned grid = labels_scatter_grid(m, num_cu, max_blocks);
    if (ids_u64)
        hipLaunchKernelGGL(k_labels_scatter<uint64_t>, dim3(grid), dim3(256), 0, s, cols, static_cast<const uint64_t *>(ids), id_offset, codes, m);
    else
        hipLaunchKernelGGL(k_labels_scatter<uint32_t>, dim3(grid), dim3(256), 0, s, cols, static_cast<const uint32_t *>(ids), id_offset, codes, m);
}
void launch_labels_set_mask(const LabelSet &set, const uint32_t *ids, uint64_t m, int num_cu, uint32_t max_blocks, hipStream_t s) {
    if (set.n == 0 || m == 0) return;
    hipLaunchKernelGGL(k_labels_set_mask, dim3(labels_scatter_grid(m, num_cu, max_blocks)), dim3(256), 0, s, set, ids, m);
}

}  // namespace vdb
