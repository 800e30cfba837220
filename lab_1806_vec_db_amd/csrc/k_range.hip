// k_range.hip -- the kernels of the exact Flat range search (Index::flat_range_device): every row whose exact distance to the query is
// at or below the query's radius, ascending by (distance, index).
//
// 8-bit tier.  The radius IS the bound a k-NN call has to estimate: k_i8_tau_from_dk (k_redo.hip) turns r_q into the threshold tau_q of
// the 8-bit filter pass, k_range_admit keeps the query in the tier only if flat_lb_excludes(r_q, tau_q) (common.hpp) really holds --
// then every row OUTSIDE the hit list (key > tau_q) has an exact distance above r_q -- and k_range_cut, behind the exact evaluation of
// the whole hit list (launch_rerank over the counted lists), keeps the pairs with distance <= r_q and sorts them.  A query that is not
// admitted (NaN / infinite radius, a query or an index the bound cannot describe) runs the pass with tau = -inf (no hits) and, like one
// whose hit counter passed the list's capacity, is answered by the scan tier.
//
// Scan tier.  Dense exact distances of 8 queries per corpus pass (the k-NN scan's kernel), then k_range_count / k_range_offsets /
// k_range_compact: the rows at or below the radius as pair keys, in row order, ready for the row sort of k_sort.hip.
//
// Both tiers append their sorted pair keys to a pool (k_range_append); k_range_gather writes the CSR arrays of the result.
// Radius comparisons are made on the f32 distances (NaN <= r is false: a NaN distance is never inside, a NaN radius keeps nothing);
// the order is that of the 64-bit pair keys.  Row ids are 32-bit inside the keys, every offset is 64-bit.
#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"

namespace vdb {

// (RANGE_LEFT, kernels.hpp: k_range_cut's count of a query that left the 8-bit tier)
static_assert(RANGE_LEFT == 0xFFFFFFFFu, "count sentinel");

// tau[q] stays as derived from the radius only where the bound holds with it; everything else passes nothing
__global__ void k_range_admit(const float *__restrict__ radius, uint32_t nq, const float *__restrict__ qoff, const float *__restrict__ qsq,
                              float xsq_max, float xsq_min_pos, float mu_norm, uint32_t dim, int cosine, float *__restrict__ tau) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const float t = tau[q];
    // (a threshold at or above FLT_MAX would not be one: an infinite radius, an overflowed inversion)
    const bool ok = t < 3.0e38f && flat_lb_excludes(radius[q], t, qsq[q], qoff[q], cosine, xsq_max, xsq_min_pos, mu_norm, dim);
    if (!ok) tau[q] = -INFINITY;
}
void launch_range_admit(const float *radius, uint32_t nq, const float *qoff, const float *qsq, float xsq_max, float xsq_min_pos, float mu_norm,
                        uint32_t dim, int cosine, float *tau, hipStream_t s) {
    if (nq == 0) return;
    hipLaunchKernelGGL(k_range_admit, dim3((nq + 63) / 64), dim3(64), 0, s, radius, nq, qoff, qsq, xsq_max, xsq_min_pos, mu_norm, dim, cosine, tau);
}

// One workgroup per query over the exact keys of its hit list: the pairs inside the radius, compacted into LDS (wave ballot + prefix; the
// order is the sort's business), padded to a power of two, sorted by a bitonic network in LDS and written back over the row.
// o_cnt[q] = pairs kept, or RANGE_LEFT; o_hits[q] = length of the hit list (0 for a query that was not admitted).
__global__ __launch_bounds__(256) void k_range_cut(uint64_t *__restrict__ keys, uint32_t cap, const uint32_t *__restrict__ cnt,
                                                   const float *__restrict__ radius, const float *__restrict__ tau, uint32_t *__restrict__ o_cnt,
                                                   uint32_t *__restrict__ o_hits) {
    extern __shared__ __attribute__((aligned(16))) uint64_t rc_keys[];  // [cap]
    __shared__ uint32_t s_n;
    const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const uint32_t total = cnt[q];
    const bool admitted = tau[q] != -INFINITY;
    if (!admitted || total > cap) {  // block-uniform
        if (tid == 0) {
            o_cnt[q] = RANGE_LEFT;
            o_hits[q] = admitted ? total : 0u;
        }
        return;
    }
    uint64_t *row = keys + uint64_t(q) * cap;
    const float r = radius[q];
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (uint32_t base = 0; base < total; base += 256) {  // (block-uniform trip count: every wave has all lanes in the ballot)
        const uint32_t i = base + tid;
        const uint64_t key = i < total ? row[i] : PAIR_NONE;
        const bool keep = key != PAIR_NONE && f32_from_orderable(uint32_t(key >> 32)) <= r;
        const uint64_t m = __ballot(keep);
        uint32_t wbase = 0;
        if (lane == 0 && m) wbase = atomicAdd(&s_n, (uint32_t)__builtin_popcountll(m));
        wbase = __shfl(wbase, 0);
        if (keep) rc_keys[wbase + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1))] = key;
    }
    __syncthreads();
    const uint32_t kept = s_n;
    uint32_t m2 = 1;
    while (m2 < kept) m2 <<= 1;
    for (uint32_t i = kept + tid; i < m2; i += 256) rc_keys[i] = PAIR_NONE;
    __syncthreads();
    for (uint32_t k = 2; k <= m2; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = tid; t < m2 / 2; t += 256) {
                const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo + j;  // the pair of the exchange: bit j clear / set
                const uint64_t a = rc_keys[lo], b = rc_keys[hi];
                if ((a > b) == ((lo & k) == 0)) {
                    rc_keys[lo] = b;
                    rc_keys[hi] = a;
                }
            }
            __syncthreads();
        }
    for (uint32_t i = tid; i < kept; i += 256) row[i] = rc_keys[i];
    if (tid == 0) {
        o_cnt[q] = kept;
        o_hits[q] = total;
    }
}
void launch_range_cut(uint64_t *keys, uint32_t cap, const uint32_t *cnt, const float *radius, const float *tau, uint32_t nq, uint32_t *o_cnt,
                      uint32_t *o_hits, hipStream_t s) {
    if (nq == 0) return;
    VDB_REQUIRE(cap >= 1 && cap <= 16384, "range cut: list capacity");
    const size_t lds = size_t(cap) * sizeof(uint64_t);
    func_max_lds(reinterpret_cast<const void *>(k_range_cut), (int)lds);
    hipLaunchKernelGGL(k_range_cut, dim3(nq), dim3(256), lds, s, keys, cap, cnt, radius, tau, o_cnt, o_hits);
    VDB_HIP(hipGetLastError());
}

// ---- scan tier: the rows of a dense distance row that lie inside the radius ---------------------------------------------------------
constexpr uint32_t RANGE_SEG = 4096;  // rows per workgroup: 16 steps of 256
uint32_t range_scan_blocks(uint64_t n) { return (uint32_t)((n + RANGE_SEG - 1) / RANGE_SEG); }

// blk_cnt[q * nblk + b] = rows of segment b with dist <= radius[q]
__global__ __launch_bounds__(256) void k_range_count(const float *__restrict__ dist, uint64_t ld, uint64_t n, const float *__restrict__ radius,
                                                     uint32_t nblk, uint32_t *__restrict__ blk_cnt) {
    __shared__ uint32_t s_w[4];
    const uint32_t q = blockIdx.y, tid = threadIdx.x;
    const float r = radius[q];
    const float *row = dist + uint64_t(q) * ld;
    const uint64_t base = uint64_t(blockIdx.x) * RANGE_SEG;
    uint32_t c = 0;
#pragma unroll 4
    for (uint32_t st = 0; st < RANGE_SEG / 256; st++) {
        const uint64_t i = base + st * 256 + tid;
        c += (i < n && row[i] <= r) ? 1u : 0u;
    }
    for (uint32_t off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    if ((tid & 63) == 0) s_w[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) blk_cnt[uint64_t(q) * nblk + blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}
// per query: exclusive prefix of its segment counts (in place) and their total
__global__ __launch_bounds__(256) void k_range_offsets(uint32_t *__restrict__ blk_cnt, uint32_t nblk, uint32_t *__restrict__ total) {
    __shared__ uint32_t sc[256];
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    uint32_t *h = blk_cnt + uint64_t(q) * nblk;
    const uint32_t per = (nblk + 255) / 256, b0 = tid * per, b1 = b0 + per < nblk ? b0 + per : nblk;
    uint32_t sum = 0;
    for (uint32_t b = b0; b < b1; b++) sum += h[b];
    sc[tid] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < 256; off <<= 1) {  // inclusive scan of the threads' sums
        const uint32_t v = tid >= off ? sc[tid - off] : 0u;
        __syncthreads();
        sc[tid] += v;
        __syncthreads();
    }
    uint32_t run = sc[tid] - sum;
    for (uint32_t b = b0; b < b1; b++) {
        const uint32_t v = h[b];
        h[b] = run;
        run += v;
    }
    if (tid == 255) total[q] = sc[255];
}
// out[q * ldo + blk_off[q][b] + rank] = pair key (distance, row) of the rank-th row of segment b inside the radius: row order preserved
// (steps in order, waves in order, lanes in order)
__global__ __launch_bounds__(256) void k_range_compact(const float *__restrict__ dist, uint64_t ld, uint64_t n, const float *__restrict__ radius,
                                                       uint32_t nblk, const uint32_t *__restrict__ blk_off, uint64_t *__restrict__ out, uint64_t ldo) {
    __shared__ uint32_t s_w[4];
    const uint32_t q = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float r = radius[q];
    const float *row = dist + uint64_t(q) * ld;
    uint64_t *orow = out + uint64_t(q) * ldo;
    const uint64_t base = uint64_t(blockIdx.x) * RANGE_SEG;
    uint32_t run = blk_off[uint64_t(q) * nblk + blockIdx.x];
    for (uint32_t st = 0; st < RANGE_SEG / 256; st++) {
        const uint64_t i = base + st * 256 + tid;
        const float d = i < n ? row[i] : 0.0f;
        const bool keep = i < n && d <= r;
        const uint64_t m = __ballot(keep);
        if (lane == 0) s_w[wave] = (uint32_t)__builtin_popcountll(m);
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < 4; w++) {
            before += w < wave ? s_w[w] : 0u;
            all += s_w[w];
        }
        const uint64_t pos = uint64_t(run) + before + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1));
        if (keep && pos < ldo) orow[pos] = pair_key(d, uint32_t(i));
        run += all;
        __syncthreads();  // s_w is rewritten by the next step
    }
}
void launch_range_scan_select(const float *dist, uint64_t ld, uint64_t n, const float *radius, uint32_t nq, uint32_t *blk, uint32_t *total,
                              hipStream_t s) {
    if (nq == 0 || n == 0) return;
    const uint32_t nblk = range_scan_blocks(n);
    hipLaunchKernelGGL(k_range_count, dim3(nblk, nq), dim3(256), 0, s, dist, ld, n, radius, nblk, blk);
    hipLaunchKernelGGL(k_range_offsets, dim3(nq), dim3(256), 0, s, blk, nblk, total);
}
void launch_range_compact(const float *dist, uint64_t ld, uint64_t n, const float *radius, uint32_t nq, const uint32_t *blk_off, uint64_t *out,
                          uint64_t ldo, hipStream_t s) {
    if (nq == 0 || n == 0 || ldo == 0) return;
    const uint32_t nblk = range_scan_blocks(n);
    hipLaunchKernelGGL(k_range_compact, dim3(nblk, nq), dim3(256), 0, s, dist, ld, n, radius, nblk, blk_off, out, ldo);
}

// ---- result assembly ----------------------------------------------------------------------------------------------------------------------
// pool[off[q] + j] = keys[q * ld + j], j < take[q]  (off / take: device memory or device-visible pinned host memory)
__global__ __launch_bounds__(256) void k_range_append(const uint64_t *__restrict__ keys, uint64_t ld, const uint64_t *__restrict__ off,
                                                      const uint32_t *__restrict__ take, uint64_t *__restrict__ pool) {
    const uint32_t q = blockIdx.y;
    const uint64_t t = take[q], o = off[q];
    const uint64_t *row = keys + uint64_t(q) * ld;
    for (uint64_t j = uint64_t(blockIdx.x) * 256 + threadIdx.x; j < t; j += uint64_t(gridDim.x) * 256) pool[o + j] = row[j];
}
void launch_range_append(const uint64_t *keys, uint64_t ld, const uint64_t *off, const uint32_t *take, uint32_t nq, uint64_t max_take, uint64_t *pool,
                         hipStream_t s) {
    if (nq == 0 || max_take == 0) return;
    const uint64_t gx = (max_take + 1023) / 1024;
    hipLaunchKernelGGL(k_range_append, dim3((unsigned)(gx < 256 ? gx : 256), nq), dim3(256), 0, s, keys, ld, off, take, pool);
}
// CSR arrays from the pool: query q's pairs pool[off[q] ..) -> out_idx / out_dist [lims[q], lims[q + 1])
__global__ __launch_bounds__(256) void k_range_gather(const uint64_t *__restrict__ pool, const uint64_t *__restrict__ off,
                                                      const uint64_t *__restrict__ lims, uint64_t id_offset, uint64_t *__restrict__ out_idx,
                                                      float *__restrict__ out_dist) {
    const uint32_t q = blockIdx.y;
    const uint64_t l0 = lims[q], t = lims[q + 1] - l0, o = off[q];
    for (uint64_t j = uint64_t(blockIdx.x) * 256 + threadIdx.x; j < t; j += uint64_t(gridDim.x) * 256) {
        const uint64_t c = pool[o + j];
        out_idx[l0 + j] = uint64_t(uint32_t(c)) + id_offset;
        out_dist[l0 + j] = f32_from_orderable(uint32_t(c >> 32));
    }
}
void launch_range_gather(const uint64_t *pool, const uint64_t *off, const uint64_t *lims, uint64_t nq, uint64_t max_take, uint64_t id_offset,
                         uint64_t *out_idx, float *out_dist, hipStream_t s) {
    if (nq == 0 || max_take == 0) return;
    const uint64_t gx = (max_take + 1023) / 1024;
    constexpr uint64_t QY = 32768;  // grid.y
    for (uint64_t q0 = 0; q0 < nq; q0 += QY)
        hipLaunchKernelGGL(k_range_gather, dim3((unsigned)(gx < 256 ? gx : 256), (unsigned)std::min<uint64_t>(QY, nq - q0)), dim3(256), 0, s, pool,
                           off + q0, lims + q0, id_offset, out_idx, out_dist);
}

}  // namespace vdb
