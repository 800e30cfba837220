// k_components.hip -- connected components over CSR edge lists (Index::flat_dup_groups_device, Index::link_pairs_device; dup_plan.hpp;
// docs/DESIGN_flat.md 4.1ab): a union-find over `parent`, one u32 per row of the table (an index has fewer than 2^32 rows).
//   init     parent[i] = i.
//   hook     a lane per pair of one chunk's CSR result: the pair's query by binary search over the limits, u = that query's source row,
//            v = the listed id.  For u != v: both roots by find with path halving, then atomicCAS(&parent[hi], hi, lo) with hi the higher
//            and lo the lower root; when the CAS loses, on from the value it read.  Only a root is ever hooked, and only under a lower
//            row: parent[x] <= x always, no cycle can form, and a row that has stopped being a root never becomes one again.  Nothing
//            waits for another thread.  When every pair has been processed both ends of every pair share a root, so a component has
//            ONE root, and it is the component's lowest row (whose parent can only be itself).  The answer is a function of the edge
//            set alone, whatever the order of waves, chunks and launches.
//   flatten  after the last chunk: r = find(i) (read only), parent[i] = r, group[i] = r + id_offset (DUP_ROW_NONE outside the mask),
//            size[r] += 1 by integer atomicAdd.
//   count    the roots of size >= 2 and the rows under them, one integer add per wave.
// Every access to `parent` that another workgroup may race with is an agent-scope relaxed atomic load, store or CAS; a stale value
// read by find is an older ancestor, which is still an ancestor.  No float atomics anywhere.
#include <algorithm>

#include "kernels.hpp"

namespace vdb {

#define COMP_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ uint32_t comp_load(uint32_t *p) { return __hip_atomic_load(p, COMP_RLX); }

// the root of x, halving the path on the way: every other row of it is pointed at its grandparent
__device__ __forceinline__ uint32_t comp_find(uint32_t *parent, uint32_t x) {
    for (;;) {
        const uint32_t p = comp_load(parent + x);
        if (p == x) return x;
        const uint32_t g = comp_load(parent + p);
        if (g == p) return p;
        __hip_atomic_store(parent + x, g, COMP_RLX);  // (x is no root and never will be: no CAS of a hook can succeed on it)
        x = g;
    }
}
__device__ __forceinline__ uint32_t comp_find_ro(uint32_t *parent, uint32_t x) {
    for (;;) {
        const uint32_t p = comp_load(parent + x);
        if (p == x) return x;
        x = p;
    }
}
__device__ __forceinline__ void comp_link(uint32_t *parent, uint32_t u, uint32_t v) {
    for (;;) {
        u = comp_find(parent, u);
        v = comp_find(parent, v);
        if (u == v) return;
        const uint32_t hi = u > v ? u : v, lo = u > v ? v : u;
        uint32_t seen = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, COMP_RLX)) return;
        u = seen;  // hi was hooked by somebody else in the meantime: on from where it points now
        v = lo;
    }
}

__global__ __launch_bounds__(256) void k_comp_init(uint32_t *__restrict__ parent, uint32_t *__restrict__ size, uint64_t n) {
    const uint64_t stride = uint64_t(gridDim.x) * 256;
    for (uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += stride) {
        parent[i] = (uint32_t)i;
        size[i] = 0;
    }
}

// the largest q < nq with lims[q] <= p (lims ascending, lims[0] <= p < lims[nq])
__device__ __forceinline__ uint32_t comp_query_of(const uint64_t *__restrict__ lims, uint32_t nq, uint64_t p) {
    uint32_t lo = 0, hi = nq;  // answer in [lo, hi)
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (lims[mid] <= p)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// Pairs [0, total) of a CSR list over nq queries; query q's source row: src64[q] - id_offset, else src32[q], else src_base + q.
// counters[2] += the pairs with u != v, counters[3] += the lists of exactly `limit` entries (limit > 0), one add per wave each.
__global__ __launch_bounds__(256) void k_comp_hook(const uint64_t *__restrict__ src64, const uint32_t *__restrict__ src32, uint64_t src_base,
                                                   const uint64_t *__restrict__ lims, const uint64_t *__restrict__ ids, uint32_t nq, uint64_t total,
                                                   uint64_t id_offset, uint64_t limit, uint32_t *parent, unsigned long long *counters) {
    const uint64_t stride = uint64_t(gridDim.x) * 256;
    const uint32_t lane = threadIdx.x & 63;
    uint64_t w_pairs = 0, w_trunc = 0;  // (wave-uniform)
    for (uint64_t p0 = uint64_t(blockIdx.x) * 256 + (threadIdx.x & ~63u); p0 < total; p0 += stride) {  // (wave-uniform)
        const uint64_t p = p0 + lane;
        bool edge = false, cut = false;
        uint32_t u = 0, v = 0;
        if (p < total) {
            const uint32_t q = comp_query_of(lims, nq, p);
            const uint64_t a = lims[q];
            u = src64 ? (uint32_t)(src64[q] - id_offset) : src32 ? src32[q] : (uint32_t)(src_base + q);
            v = (uint32_t)(ids[p] - id_offset);
            edge = u != v;
            cut = limit != 0 && p == a && lims[q + 1] - a == limit;
        }
        w_pairs += (uint64_t)__popcll(__ballot(edge));
        w_trunc += (uint64_t)__popcll(__ballot(cut));
        if (edge) comp_link(parent, u, v);
    }
    if (lane == 0) {
        if (w_pairs) atomicAdd(&counters[2], (unsigned long long)w_pairs);
        if (w_trunc) atomicAdd(&counters[3], (unsigned long long)w_trunc);
    }
}

// bits: the allowed rows (nullptr: every row); size zeroed by k_comp_init
__global__ __launch_bounds__(256) void k_comp_flatten(uint32_t *parent, const uint64_t *__restrict__ bits, uint64_t n, uint64_t id_offset,
                                                      uint64_t *__restrict__ group, uint32_t *size) {
    const uint64_t stride = uint64_t(gridDim.x) * 256;
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t i0 = uint64_t(blockIdx.x) * 256 + (threadIdx.x & ~63u); i0 < n; i0 += stride) {  // (wave-uniform)
        const uint64_t i = i0 + lane;
        bool allowed = false;
        uint32_t r = 0;
        if (i < n) {
            allowed = bits ? ((bits[i >> 6] >> (i & 63)) & 1) != 0 : true;
            r = comp_find_ro(parent, (uint32_t)i);
            __hip_atomic_store(parent + i, r, COMP_RLX);
            group[i] = allowed ? uint64_t(r) + id_offset : DUP_ROW_NONE;
        }
        // a wave whose rows mostly share a root (a large group) adds once for them: the lowest allowed lane's root first
        const uint64_t act = __ballot(allowed);
        if (act) {  // (wave-uniform)
            const uint32_t lead = (uint32_t)__ffsll((unsigned long long)act) - 1;
            const uint32_t r0 = (uint32_t)__shfl((int)r, (int)lead);
            const uint64_t same = __ballot(allowed && r == r0);
            if (lane == lead)
                atomicAdd(&size[r0], (uint32_t)__popcll(same));
            else if (allowed && r != r0)
                atomicAdd(&size[r], 1u);
        }
    }
}

// counters[0] += the roots with size >= 2, counters[1] += their sizes; after k_comp_flatten
__global__ __launch_bounds__(256) void k_comp_count(const uint32_t *__restrict__ parent, const uint32_t *__restrict__ size, uint64_t n,
                                                    unsigned long long *counters) {
    const uint64_t stride = uint64_t(gridDim.x) * 256;
    const uint32_t lane = threadIdx.x & 63;
    uint64_t w_groups = 0;  // (wave-uniform)
    unsigned long long rows = 0;
    for (uint64_t i0 = uint64_t(blockIdx.x) * 256 + (threadIdx.x & ~63u); i0 < n; i0 += stride) {  // (wave-uniform)
        const uint64_t i = i0 + lane;
        const bool big = i < n && parent[i] == (uint32_t)i && size[i] >= 2;
        w_groups += (uint64_t)__popcll(__ballot(big));
        if (big) rows += size[i];
    }
    for (int off = 32; off > 0; off >>= 1) rows += __shfl_xor(rows, off);
    if (lane == 0) {
        if (w_groups) atomicAdd(&counters[0], (unsigned long long)w_groups);
        if (rows) atomicAdd(&counters[1], rows);
    }
}

// The check of a caller-supplied CSR list (Index::link_pairs_device): out[0] |= 1 when lims[0] != 0, the limits descend somewhere, or a
// source id or a listed id is no row of the index; out[1] = lims[nq], the pairs.  out zeroed by the caller.
__global__ __launch_bounds__(256) void k_pairs_check(const uint64_t *__restrict__ src, const uint64_t *__restrict__ lims, const uint64_t *__restrict__ ids,
                                                     uint64_t nq, uint64_t n, uint64_t id_offset, unsigned long long *out) {
    const uint64_t total = lims[nq], top = total > nq ? total : nq;
    const uint64_t stride = uint64_t(gridDim.x) * 256;
    bool bad = false;
    for (uint64_t j = uint64_t(blockIdx.x) * 256 + threadIdx.x; j < top; j += stride) {
        if (j < nq) bad |= src[j] - id_offset >= n || lims[j] > lims[j + 1] || (j == 0 && lims[0] != 0);
        if (j < total) bad |= ids[j] - id_offset >= n;
    }
    if (bad) atomicOr(&out[0], 1ull);
    if (blockIdx.x == 0 && threadIdx.x == 0) out[1] = total;
}

static unsigned comp_grid(uint64_t items, int num_cu) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((items + 255) / 256, uint64_t(std::max(num_cu, 1)) * 8));
}
void launch_comp_init(uint32_t *parent, uint32_t *size, uint64_t n, int num_cu, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_comp_init, dim3(comp_grid(n, num_cu)), dim3(256), 0, s, parent, size, n);
}
void launch_comp_hook(const uint64_t *src64, const uint32_t *src32, uint64_t src_base, const uint64_t *lims, const uint64_t *ids, uint64_t nq,
                      uint64_t total, uint64_t id_offset, uint64_t limit, uint32_t *parent, uint64_t *counters, int num_cu, hipStream_t s) {
    if (nq == 0 || total == 0) return;
    hipLaunchKernelGGL(k_comp_hook, dim3(comp_grid(total, num_cu)), dim3(256), 0, s, src64, src32, src_base, lims, ids, (uint32_t)nq, total, id_offset,
                       limit, parent, reinterpret_cast<unsigned long long *>(counters));
}
void launch_comp_flatten(uint32_t *parent, const uint64_t *bits, uint64_t n, uint64_t id_offset, uint64_t *group, uint32_t *size, uint64_t *counters,
                         int num_cu, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_comp_flatten, dim3(comp_grid(n, num_cu)), dim3(256), 0, s, parent, bits, n, id_offset, group, size);
    hipLaunchKernelGGL(k_comp_count, dim3(comp_grid(n, num_cu)), dim3(256), 0, s, parent, size, n, reinterpret_cast<unsigned long long *>(counters));
}
void launch_pairs_check(const uint64_t *src, const uint64_t *lims, const uint64_t *ids, uint64_t nq, uint64_t n, uint64_t id_offset, uint64_t *out,
                        int num_cu, hipStream_t s) {
    hipLaunchKernelGGL(k_pairs_check, dim3((unsigned)std::max(num_cu, 1) * 8), dim3(256), 0, s, src, lims, ids, nq, n, id_offset,
                       reinterpret_cast<unsigned long long *>(out));
}

}  // namespace vdb
