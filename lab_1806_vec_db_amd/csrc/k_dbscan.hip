// k_dbscan.hip -- the stage behind the range self-join that turns neighbour lists into density clusters (Index::flat_dbscan_device,
// Index::dbscan_pairs_device; dbscan_plan.hpp states the rule; docs/DESIGN_flat.md 4.1ae).  State of a call, per row of the table:
// parent u32 (the union-find of comp_uf.hpp, over CORE rows only), border u64 (the smallest pair_key(distance, core row) offered to a
// non-core row, PAIR_NONE: none yet) and kind u8.  The lists arrive a chunk of queries at a time, each ascending by (distance, index):
//   init    border = PAIR_NONE, kind = 1 for an allowed row and 0 for the others, the counters zero; parent by k_comp_init.
//   core    a lane per query of the chunk: |N(i)| = lims[q + 1] - lims[q]; kind[i] = 3 when it reaches min_samples, else 1.  After this
//           launch the kind of every row up to the chunk's last query row `hi` is final.
//   link    a WAVE per list.  Row i and kind[i] are read once and are wave-uniform; the list is walked in tiles of 64 with coalesced
//           loads of ids and distances.  A lane drops j == i and every j > hi: j's own list has not been produced yet, and the pair is
//           handled from j's side in j's chunk, where i <= hi' and both kinds are final (the pair distances are symmetric bit for bit,
//           so j in N(i) iff i in N(j)).  Of the rest,
//             core i, core j      comp_link, skipped by the lanes whose root already is the wave's current root of i;
//             core i, other j     atomicMin(border[j], pair_key(d, i));
//             non-core i          the list ascends by (distance, index), so the first core lane of the first tile that has one holds the
//                                 best candidate among the rows seen so far: ballot, find-first-set, ONE atomicMin(border[i],
//                                 pair_key(d, j)) per wave, and the wave leaves the list -- as soon as it has also passed the row's own
//                                 entry, which the pair count needs (a list holds it at most once, at the front under L2Sqr; what is
//                                 left behind it is added to the count unread).
//           A pair inside one chunk is processed from both sides, which is idempotent: link and min commute with themselves.
//   labels  a lane per row after the last chunk: a core row's label is its root, a non-core row with a key in border takes the root of
//           the core row in the key's low half and becomes border, the others are noise; rows outside the mask get DBSCAN_ROW_NONE.  The
//           four counts come from ballots and popcounts over the final kinds; a cluster is counted at the core row that is its own root.
// Integer atomics only (CAS and add on u32 / u64, a 64-bit unsigned min), no float atomics; nothing waits for another thread; every
// racing access to `parent` is an agent-scope relaxed atomic.  min, link and the counts commute, so the answer is a function of the lists
// alone.  counters [8] u64: clusters | core | border | noise | non-self pairs | spare | the two words of the list check.
#include <algorithm>

#include "common.hpp"
#include "comp_uf.hpp"
#include "kernels.hpp"

namespace vdb {

// bits: the allowed rows (nullptr: every row)
__global__ __launch_bounds__(256) void k_dbscan_init(const uint64_t *__restrict__ bits, uint64_t n, uint64_t *__restrict__ border,
                                                     uint8_t *__restrict__ kind, unsigned long long *counters) {
    const uint64_t stride = uint64_t(gridDim.x) * 256;
    for (uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += stride) {
        border[i] = PAIR_NONE;
        kind[i] = !bits || ((bits[i >> 6] >> (i & 63)) & 1) ? DBSCAN_NOISE : DBSCAN_OUTSIDE;
    }
    if (blockIdx.x == 0 && threadIdx.x < 6) counters[threadIdx.x] = 0;
}

// query q's source row: src64[q] - id_offset, else src32[q], else src_base + q
__device__ __forceinline__ uint32_t dbscan_row_of(const uint64_t *__restrict__ src64, const uint32_t *__restrict__ src32, uint64_t src_base,
                                                  uint64_t id_offset, uint32_t q) {
    return src64 ? (uint32_t)(src64[q] - id_offset) : src32 ? src32[q] : (uint32_t)(src_base + q);
}

// The stage-alone entry's sources must be distinct (two lists of one row would race on its kind): bit row of `seen` (ceil(n / 32) words,
// zeroed by the caller) is set for every source row below n; out[0] |= 2 when a bit was set already.  Beside k_pairs_check, one read-back.
__global__ __launch_bounds__(256) void k_dbscan_sources(const uint64_t *__restrict__ src, uint64_t nq, uint64_t n, uint64_t id_offset, uint32_t *seen,
                                                        unsigned long long *out) {
    const uint64_t stride = uint64_t(gridDim.x) * 256;
    bool twice = false;
    for (uint64_t q = uint64_t(blockIdx.x) * 256 + threadIdx.x; q < nq; q += stride) {
        const uint64_t row = src[q] - id_offset;
        if (row < n) twice |= (atomicOr(&seen[row >> 5], 1u << (row & 31)) >> (row & 31)) & 1;
    }
    if (twice) atomicOr(&out[0], 2ull);
}

// (the kinds are counted by k_dbscan_labels, from the final kind of every row)
__global__ __launch_bounds__(256) void k_dbscan_core(const uint64_t *__restrict__ src64, const uint32_t *__restrict__ src32, uint64_t src_base,
                                                     const uint64_t *__restrict__ lims, uint32_t nq, uint64_t id_offset, uint64_t min_samples,
                                                     uint8_t *__restrict__ kind) {
    const uint64_t stride = uint64_t(gridDim.x) * 256;
    for (uint64_t q = uint64_t(blockIdx.x) * 256 + threadIdx.x; q < nq; q += stride)
        kind[dbscan_row_of(src64, src32, src_base, id_offset, (uint32_t)q)] = lims[q + 1] - lims[q] >= min_samples ? DBSCAN_CORE : DBSCAN_NOISE;
}

// A wave per list.  more_chunks: the queries ascend by row and later chunks follow, so the kinds are final up to hi = the last query's row
// and every listed row above it is left to its own list; otherwise every listed row is processed.  counters[4] += the entries j != i.
__global__ __launch_bounds__(256) void k_dbscan_link(const uint64_t *__restrict__ src64, const uint32_t *__restrict__ src32, uint64_t src_base,
                                                     const uint64_t *__restrict__ lims, const uint64_t *__restrict__ ids,
                                                     const float *__restrict__ dists, uint32_t nq, uint64_t id_offset, bool more_chunks,
                                                     const uint8_t *__restrict__ kind, uint32_t *parent, unsigned long long *border,
                                                     unsigned long long *counters) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t n_waves = gridDim.x * 4;
    const uint32_t hi = more_chunks ? dbscan_row_of(src64, src32, src_base, id_offset, nq - 1) : ~uint32_t(0);
    uint64_t w_pairs = 0;  // (wave-uniform)
    for (uint64_t q = blockIdx.x * 4 + (threadIdx.x >> 6); q < nq; q += n_waves) {  // (wave-uniform)
        const uint64_t beg = lims[q], end = lims[q + 1];
        if (beg == end) continue;
        const uint32_t i = dbscan_row_of(src64, src32, src_base, id_offset, (uint32_t)q);
        const bool core_i = kind[i] == DBSCAN_CORE;
        bool self_seen = false, taken = false;  // (wave-uniform)
        for (uint64_t p0 = beg; p0 < end; p0 += 64) {
            const uint64_t p = p0 + lane;
            const bool valid = p < end;
            uint32_t j = 0;
            float d = 0.0f;
            if (valid) {
                j = (uint32_t)(ids[p] - id_offset);
                d = dists[p];
            }
            const bool self = valid && j == i;
            self_seen |= __ballot(self) != 0;
            w_pairs += (uint64_t)__popcll(__ballot(valid && !self));
            const bool live = valid && !self && j <= hi;
            const bool core_j = live && kind[j] == DBSCAN_CORE;
            if (core_i) {
                if (__ballot(core_j)) {  // (wave-uniform)
                    uint32_t ri = 0;
                    if (lane == 0) ri = comp_find(parent, i);
                    ri = (uint32_t)__shfl((int)ri, 0);
                    if (core_j) {
                        const uint32_t rj = comp_find(parent, j);
                        if (rj != ri) comp_link(parent, ri, rj);
                    }
                }
                if (live && !core_j) atomicMin(&border[j], (unsigned long long)pair_key(d, i));
            } else {
                const uint64_t cand = taken ? 0 : __ballot(core_j);
                if (cand) {  // (wave-uniform)
                    taken = true;
                    if (lane == (uint32_t)__ffsll((unsigned long long)cand) - 1) atomicMin(&border[i], (unsigned long long)pair_key(d, j));
                }
                if (taken && self_seen) {  // the rest of the list cannot change border[i], and none of it is the row itself
                    w_pairs += p0 + 64 < end ? end - (p0 + 64) : 0;
                    break;
                }
            }
        }
    }
    if (lane == 0 && w_pairs) atomicAdd(&counters[4], (unsigned long long)w_pairs);
}

// label / kind_out [n]; counters[0] += clusters, [1] += core rows, [2] += border rows, [3] += noise rows, from the final kinds, one add per
// wave each
__global__ __launch_bounds__(256) void k_dbscan_labels(uint32_t *parent, const uint8_t *__restrict__ kind, const uint64_t *__restrict__ border,
                                                       uint64_t n, uint64_t id_offset, uint64_t *__restrict__ label,
                                                       uint8_t *__restrict__ kind_out, unsigned long long *counters) {
    const uint64_t stride = uint64_t(gridDim.x) * 256;
    const uint32_t lane = threadIdx.x & 63;
    uint64_t w_clusters = 0, w_core = 0, w_border = 0, w_noise = 0;  // (wave-uniform)
    for (uint64_t i0 = uint64_t(blockIdx.x) * 256 + (threadIdx.x & ~63u); i0 < n; i0 += stride) {  // (wave-uniform)
        const uint64_t i = i0 + lane;
        uint8_t k = DBSCAN_OUTSIDE;
        bool root = false;
        if (i < n) {
            k = kind[i];
            uint64_t lab = DBSCAN_ROW_NONE;
            if (k == DBSCAN_CORE) {
                const uint32_t r = comp_find_ro(parent, (uint32_t)i);
                root = r == (uint32_t)i;
                lab = uint64_t(r) + id_offset;
            } else if (k == DBSCAN_NOISE) {
                const uint64_t b = border[i];
                if (b != PAIR_NONE) {
                    k = DBSCAN_BORDER;
                    lab = uint64_t(comp_find_ro(parent, (uint32_t)b)) + id_offset;  // (the key's low half: the core row)
                } else
                    lab = DBSCAN_ROW_NOISE;
            }
            label[i] = lab;
            kind_out[i] = k;
        }
        w_clusters += (uint64_t)__popcll(__ballot(root));
        w_core += (uint64_t)__popcll(__ballot(k == DBSCAN_CORE));
        w_border += (uint64_t)__popcll(__ballot(k == DBSCAN_BORDER));
        w_noise += (uint64_t)__popcll(__ballot(k == DBSCAN_NOISE));
    }
    if (lane == 0) {
        if (w_clusters) atomicAdd(&counters[0], (unsigned long long)w_clusters);
        if (w_core) atomicAdd(&counters[1], (unsigned long long)w_core);
        if (w_border) atomicAdd(&counters[2], (unsigned long long)w_border);
        if (w_noise) atomicAdd(&counters[3], (unsigned long long)w_noise);
    }
}

static unsigned dbscan_grid(uint64_t items, int num_cu, unsigned per_cu) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((items + 255) / 256, uint64_t(std::max(num_cu, 1)) * per_cu));
}
void launch_dbscan_init(const uint64_t *bits, uint64_t n, uint32_t *parent, uint64_t *border, uint8_t *kind, uint64_t *counters, int num_cu,
                        hipStream_t s) {
    launch_comp_init(parent, nullptr, n, num_cu, s);
    hipLaunchKernelGGL(k_dbscan_init, dim3(dbscan_grid(n, num_cu, 8)), dim3(256), 0, s, bits, n, border, kind,
                       reinterpret_cast<unsigned long long *>(counters));
}
void launch_dbscan_sources(const uint64_t *src, uint64_t nq, uint64_t n, uint64_t id_offset, uint32_t *seen, uint64_t *out, int num_cu, hipStream_t s) {
    hipLaunchKernelGGL(k_dbscan_sources, dim3(dbscan_grid(nq, num_cu, 8)), dim3(256), 0, s, src, nq, n, id_offset, seen,
                       reinterpret_cast<unsigned long long *>(out));
}
void launch_dbscan_chunk(const uint64_t *src64, const uint32_t *src32, uint64_t src_base, const uint64_t *lims, const uint64_t *ids,
                         const float *dists, uint64_t nq, uint64_t id_offset, uint64_t min_samples, bool more_chunks, uint8_t *kind, uint32_t *parent,
                         uint64_t *border, uint64_t *counters, int num_cu, hipStream_t s) {
    if (nq == 0) return;
    hipLaunchKernelGGL(k_dbscan_core, dim3(dbscan_grid(nq, num_cu, 8)), dim3(256), 0, s, src64, src32, src_base, lims, (uint32_t)nq, id_offset,
                       min_samples, kind);
    // four lists per workgroup, up to 16 workgroups per CU: a list is long by construction, so a wave has work
    hipLaunchKernelGGL(k_dbscan_link, dim3(dbscan_grid(nq * 64, num_cu, 16)), dim3(256), 0, s, src64, src32, src_base, lims, ids, dists, (uint32_t)nq,
                       id_offset, more_chunks, kind, parent, reinterpret_cast<unsigned long long *>(border),
                       reinterpret_cast<unsigned long long *>(counters));
}
void launch_dbscan_labels(uint32_t *parent, const uint8_t *kind, const uint64_t *border, uint64_t n, uint64_t id_offset, uint64_t *label,
                          uint8_t *kind_out, uint64_t *counters, int num_cu, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_dbscan_labels, dim3(dbscan_grid(n, num_cu, 8)), dim3(256), 0, s, parent, kind, border, n, id_offset, label, kind_out,
                       reinterpret_cast<unsigned long long *>(counters));
}

}  // namespace vdb
