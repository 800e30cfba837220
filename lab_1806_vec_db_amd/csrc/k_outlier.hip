// k_outlier.hip -- the kernels of the k-NN self-join and of the outlier scores on its graph (Index::flat_knn_graph_device,
// Index::flat_outliers_device, Index::lof_lists_device; outlier_plan.hpp states the rule; docs/DESIGN_flat.md 4.1ah).
//
// The graph of a call: nbr u32 [m][k] (LOCAL rows), nd f32 [m][k], cnt u32 [m], by POSITION among the allowed rows; kdist f32 [n] and
// lrd64 f64 [n] by ROW of the table, so that the dependent gathers kdist[nbr] / lrd64[nbr] need no row-to-position map under a mask.
//   k_knn_self_pack  a WAVE per source row over one chunk's exact sorted lists [nb][ld] of the search at k + 1 (ids u64 = row +
//                    id_offset), in tiles of 64 positions, tile t + 1's loads issued before tile t is worked on.  A ballot finds the lane
//                    that holds the row's own id, a prefix popcount closes the gap (the k_like_drop walk with one listed id); the walk
//                    stops at kk kept, which drops the last entry of a list that does not hold the row itself.  The lane that wrote slot
//                    count - 1 writes kdist[row]; zeros fill the slots behind the count.
//   k_lof_lrd        lrd of every source row.  k <= 64: G = pow2ceil(k) lanes share a row and a wave works on 64 / G rows at once, one
//                    lane per (row, neighbour), so k = 20 keeps 40 of 64 lanes busy instead of 20.  A lane gathers kdist[nbr], takes the
//                    NaN-propagating max with its own distance and widens to f64; a fixed butterfly inside the lane group (lane_xor64:
//                    partners 1, 2, .. G / 2) forms the sum in every lane of the group; the group's first lane writes lrd (f32, by
//                    position) and lrd64 (by row).  k > 64: a wave per row, every lane adds its positions lane, lane + 64, .. in that
//                    order, then the same butterfly over 64.
//   k_lof_score      the same split over lrd64[nbr]: the mean, divided by the row's own lrd64, rounded to f32 once.
// lrd of EVERY row must exist before any lof: the two stages are two launches.  No float atomics; the order of every sum is fixed by the
// list and the lane layout alone, so two calls give the same bits.  a + b and b + a are the same f64, so both partners of a butterfly
// step hold the same sum.
#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"

namespace vdb {

__global__ __launch_bounds__(256) void k_knn_self_pack(const uint64_t *__restrict__ ids, const float *__restrict__ dists,
                                                       const uint64_t *__restrict__ counts, uint32_t nb, uint64_t ld,
                                                       const uint32_t *__restrict__ src32, uint64_t base, uint64_t id_offset, uint32_t k, uint32_t kk,
                                                       uint32_t *__restrict__ nbr, uint64_t *__restrict__ out_ids, float *__restrict__ nd,
                                                       uint32_t *__restrict__ cnt32, uint64_t *__restrict__ cnt64, float *__restrict__ kdist) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t n_waves = gridDim.x * 4;
    const uint64_t lt = (1ull << lane) - 1;
    for (uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6); b < nb; b += n_waves) {  // (wave-uniform)
        const uint64_t c = counts[b] < ld ? counts[b] : ld;
        const uint64_t pos = base + b;
        const uint32_t row = src32 ? src32[b] : (uint32_t)pos;
        const uint64_t self = uint64_t(row) + id_offset;
        const uint64_t *L = ids + uint64_t(b) * ld;
        const float *D = dists + uint64_t(b) * ld;
        uint64_t id_n = 0;
        float d_n = 0.0f;
        if (lane < c) {
            id_n = L[lane];
            d_n = D[lane];
        }
        uint32_t kept = 0, my_at = ~0u;  // my_at / my_d: the last slot this lane wrote
        float my_d = 0.0f;
        for (uint64_t t0 = 0; t0 < c && kept < kk; t0 += 64) {  // (wave-uniform)
            const uint64_t id = id_n;
            const float d = d_n;
            const uint64_t nx = t0 + 64 + lane;  // the next tile's loads, before this one is worked on
            if (nx < c) {
                id_n = L[nx];
                d_n = D[nx];
            }
            const bool keep = t0 + lane < c && id != self;
            const uint64_t kb = __ballot(keep);
            const uint32_t at = kept + (uint32_t)__popcll(kb & lt);
            if (keep && at < kk) {
                const uint64_t o = pos * k + at;
                if (nbr) nbr[o] = (uint32_t)(id - id_offset);
                if (out_ids) out_ids[o] = id;
                nd[o] = d;
                my_at = at;
                my_d = d;
            }
            kept += (uint32_t)__popcll(kb);
        }
        if (kept > kk) kept = kk;
        for (uint32_t i = kept + lane; i < k; i += 64) {
            const uint64_t o = pos * k + i;
            if (nbr) nbr[o] = 0;
            if (out_ids) out_ids[o] = 0;
            nd[o] = 0.0f;
        }
        if (lane == 0) {
            if (cnt32) cnt32[pos] = kept;
            if (cnt64) cnt64[pos] = kept;
        }
        if (kdist) {
            if (kept == 0) {
                if (lane == 0) kdist[row] = __builtin_nanf("");
            } else if (my_at == kept - 1)
                kdist[row] = my_d;
        }
    }
}

// the stage-alone entry: *flag = 1 when a count passes k or a counted slot names a row at or past n (flag zeroed by the caller)
__global__ __launch_bounds__(256) void k_lof_check(const uint32_t *__restrict__ nbr, const uint32_t *__restrict__ cnt, uint64_t m, uint32_t k, uint64_t n,
                                                   uint32_t *flag) {
    // a wave per list: the count is read once, and only the counted slots are (no division per slot)
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t n_waves = uint64_t(gridDim.x) * 4;
    bool bad = false;
    for (uint64_t pos = uint64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); pos < m; pos += n_waves) {  // (wave-uniform)
        const uint32_t c = cnt[pos];
        bad |= c > k;
        for (uint32_t j = lane; j < (c < k ? c : k); j += 64) bad |= nbr[pos * k + j] >= n;
    }
    if (bad) atomicOr(flag, 1u);
}

// ... and its kdist, from the lists themselves: the distance of the last counted slot, NaN for an empty list
__global__ __launch_bounds__(256) void k_lof_kdist(const float *__restrict__ nd, const uint32_t *__restrict__ cnt, uint64_t m, uint32_t k,
                                                   float *__restrict__ kdist) {
    const uint64_t stride = uint64_t(gridDim.x) * 256;
    for (uint64_t pos = uint64_t(blockIdx.x) * 256 + threadIdx.x; pos < m; pos += stride) {
        const uint32_t c = cnt[pos];
        kdist[pos] = c ? nd[pos * k + (c - 1)] : __builtin_nanf("");
    }
}

// the sum of v over the W lanes that share lane / W, in every one of them; all 64 lanes of the wave are active
template <uint32_t W>
__device__ __forceinline__ double lane_group_sum(double v, uint32_t lane) {
#define VDB_SUM_STEP(J) \
    if constexpr (W > J) v += __longlong_as_double((long long)lane_xor64<J>((uint64_t)__double_as_longlong(v), lane));
    VDB_SUM_STEP(1) VDB_SUM_STEP(2) VDB_SUM_STEP(4) VDB_SUM_STEP(8) VDB_SUM_STEP(16) VDB_SUM_STEP(32)
#undef VDB_SUM_STEP
    return v;
}

// max(a, b), NaN when either is
__device__ __forceinline__ float max_nan(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : (a > b ? a : b); }

// The work split of both score stages.  G lanes per source row (a power of two up to 64), 64 / G rows per wave; G = 0: a wave per row,
// striding.  SCORE false: term = max(kdist[o], d), the row's lrd -> lrd64[row], out32[pos], its kdist -> out_kd[pos]; true: term =
// lrd64[o], mean / lrd64[row] -> out32[pos].
template <uint32_t G, bool SCORE>
__device__ __forceinline__ void lof_stage(const uint32_t *__restrict__ nbr, const float *__restrict__ nd, const uint32_t *__restrict__ cnt,
                                          const uint32_t *__restrict__ src32, uint64_t m, uint32_t k, const float *__restrict__ kdist, double *lrd64,
                                          float *__restrict__ out32, float *__restrict__ out_kd) {
    constexpr uint32_t W = G ? G : 64, R = 64 / W;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t sub = lane / W, j0 = lane % W;
    const uint64_t n_waves = uint64_t(gridDim.x) * 4;
    for (uint64_t p0 = (uint64_t(blockIdx.x) * 4 + (threadIdx.x >> 6)) * R; p0 < m; p0 += n_waves * R) {  // (wave-uniform)
        const uint64_t pos = p0 + sub;
        const bool live = pos < m;
        uint32_t c = live ? cnt[pos] : 0;
        c = c < k ? c : k;
        double s = 0.0;
        for (uint32_t j = j0; j < c; j += W) {  // (one trip at most when G != 0: c <= k <= G)
            const uint32_t o = nbr[pos * k + j];
            if constexpr (SCORE)
                s += lrd64[o];
            else
                s += (double)max_nan(kdist[o], nd[pos * k + j]);
        }
        s = lane_group_sum<W>(s, lane);
        if (live && j0 == 0) {
            const uint64_t row = src32 ? src32[pos] : pos;
            const double mean = s / (double)c;  // (c == 0: NaN)
            if constexpr (SCORE) {
                out32[pos] = (float)(mean / lrd64[row]);
            } else {
                const double l = 1.0 / (mean + 1e-10);
                lrd64[row] = l;
                if (out32) out32[pos] = (float)l;
                if (out_kd) out_kd[pos] = kdist[row];
            }
        }
    }
}

template <uint32_t G>
__global__ __launch_bounds__(256) void k_lof_lrd(const uint32_t *__restrict__ nbr, const float *__restrict__ nd, const uint32_t *__restrict__ cnt,
                                                 const uint32_t *__restrict__ src32, uint64_t m, uint32_t k, const float *__restrict__ kdist,
                                                 double *__restrict__ lrd64, float *__restrict__ lrd, float *__restrict__ out_kd) {
    lof_stage<G, false>(nbr, nd, cnt, src32, m, k, kdist, lrd64, lrd, out_kd);
}
template <uint32_t G>
__global__ __launch_bounds__(256) void k_lof_score(const uint32_t *__restrict__ nbr, const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ src32,
                                                   uint64_t m, uint32_t k, const double *lrd64, float *__restrict__ lof) {
    lof_stage<G, true>(nbr, nullptr, cnt, src32, m, k, nullptr, const_cast<double *>(lrd64), lof, nullptr);
}

static unsigned outlier_grid(uint64_t items, int num_cu, unsigned per_cu) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((items + 255) / 256, uint64_t(std::max(num_cu, 1)) * per_cu));
}

void launch_knn_self_pack(const uint64_t *ids, const float *dists, const uint64_t *counts, uint64_t nb, uint64_t ld, const uint32_t *src32, uint64_t base,
                          uint64_t id_offset, uint32_t k, uint32_t kk, uint32_t *nbr, uint64_t *out_ids, float *nd, uint32_t *cnt32, uint64_t *cnt64,
                          float *kdist, int num_cu, hipStream_t s) {
    if (nb == 0) return;
    hipLaunchKernelGGL(k_knn_self_pack, dim3(outlier_grid(nb * 64, num_cu, 16)), dim3(256), 0, s, ids, dists, counts, (uint32_t)nb, ld, src32, base,
                       id_offset, k, kk, nbr, out_ids, nd, cnt32, cnt64, kdist);
}

void launch_lof_check(const uint32_t *nbr, const uint32_t *cnt, uint64_t m, uint32_t k, uint64_t n, uint32_t *flag, int num_cu, hipStream_t s) {
    if (m == 0) return;
    hipLaunchKernelGGL(k_lof_check, dim3(outlier_grid(m * 64, num_cu, 16)), dim3(256), 0, s, nbr, cnt, m, k, n, flag);
}

void launch_lof_kdist(const float *nd, const uint32_t *cnt, uint64_t m, uint32_t k, float *kdist, int num_cu, hipStream_t s) {
    if (m == 0) return;
    hipLaunchKernelGGL(k_lof_kdist, dim3(outlier_grid(m, num_cu, 8)), dim3(256), 0, s, nd, cnt, m, k, kdist);
}

// both stages, in stream order: lrd of every row, then lof (nullptr: the second launch is left out)
void launch_lof_stages(const uint32_t *nbr, const float *nd, const uint32_t *cnt, const uint32_t *src32, uint64_t m, uint32_t k, const float *kdist,
                       double *lrd64, float *out_kdist, float *out_lrd, float *out_lof, int num_cu, hipStream_t s) {
    if (m == 0) return;
    const uint32_t g = outlier_group(k);
    const uint64_t waves = g ? (m + 64 / g - 1) / (64 / g) : m;
    const dim3 grid(outlier_grid(waves * 64, num_cu, 16)), block(256);
#define VDB_LOF_CASE(G)                                                                                                          \
    case G:                                                                                                                      \
        hipLaunchKernelGGL(k_lof_lrd<G>, grid, block, 0, s, nbr, nd, cnt, src32, m, k, kdist, lrd64, out_lrd, out_kdist);        \
        if (out_lof) hipLaunchKernelGGL(k_lof_score<G>, grid, block, 0, s, nbr, cnt, src32, m, k, (const double *)lrd64, out_lof); \
        break;
    switch (g) {
        VDB_LOF_CASE(0) VDB_LOF_CASE(1) VDB_LOF_CASE(2) VDB_LOF_CASE(4) VDB_LOF_CASE(8) VDB_LOF_CASE(16) VDB_LOF_CASE(32) VDB_LOF_CASE(64)
    }
#undef VDB_LOF_CASE
}

}  // namespace vdb
