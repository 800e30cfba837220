// k_filter.hip -- the kernels of the filtered Flat searches (Index::flat_knn_masked_device, the mask of Index::flat_range_device): exact
// search over the rows of an allow-list (RowMask, index.hpp).
//
// Direct path.  k_scan_gather_* are the strict-order scans of k_exact.hip over a GATHERED row set: column j of the dense output is row
// ids[j] of the ascending allow-list, so a (distance, column) pair key orders like (distance, row id) and the k-NN selections of
// k_topk.hip / k_sort.hip apply as they are; k_filter_finalize maps the column back to the row.  The fold and the epilogue are the
// reference's, bit for bit (products and sums separately rounded, ascending in the dimension; the file is compiled with
// -ffp-contract=off and the pragma below repeats that).
//
// 8-bit tier.  The filter pass of k_gemm8.hip reads {C_r, M_r} per row and keeps key = C_r + M_r (s_q I) <= tau_q; rows past n carry
// {+inf, 0}.  k_mask_rowc writes a per-mask copy of those constants in which every DISALLOWED row carries {+inf, 0} as well, and
// k_tau_clamp keeps the thresholds finite so that such a key never passes.  The pass, the exact stage behind it and its bound then run
// unchanged: the hit list holds allowed rows only and every allowed row outside it has key > tau.
//
// Range scan.  k_mask_dense_nan turns the dense distance of every disallowed row into NaN: "a NaN distance is never inside".
// With one mask per query (Index::flat_range_masked_multi_device) k_range_gather_grouped folds the gathered rows of many allow-lists in
// one launch and keeps the pairs with D <= radius itself.
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "common.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace vdb {

namespace {

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

__device__ __forceinline__ bool mask_bit(const uint64_t *__restrict__ bits, uint64_t i) { return (bits[i >> 6] >> (i & 63)) & 1ull; }

}  // namespace

// ---------------------------------------------------------------------------------------------
// gathered scan, generic variant: one thread per allowed row reading its row straight from global memory (every dim).
// blockIdx.y walks the groups of BQ queries: Q, qsq and out advance by BQ queries per group.
// ---------------------------------------------------------------------------------------------
template <int BQ, int FOLD>
__global__ __launch_bounds__(256) void k_scan_gather_simple(const float *__restrict__ X, const uint32_t *__restrict__ ids, uint64_t m, uint32_t dim,
                                                            const float *__restrict__ Q, int metric, const float *__restrict__ xsq,
                                                            const float *__restrict__ qsq, float *__restrict__ out, uint64_t ld) {
    const uint64_t j = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (j >= m) return;
    Q += uint64_t(blockIdx.y) * BQ * dim;
    qsq += uint64_t(blockIdx.y) * BQ;
    out += uint64_t(blockIdx.y) * BQ * ld;
    const uint32_t r = ids[j];
    const float *x = X + uint64_t(r) * dim;
    float acc[BQ];
#pragma unroll
    for (int b = 0; b < BQ; b++) acc[b] = 0.0f;
    if ((dim & 3) == 0) {
        const float4 *x4 = reinterpret_cast<const float4 *>(x);
        for (uint32_t c = 0; c < dim / 4; c++) {
            float4 v = x4[c];
#pragma unroll
            for (int b = 0; b < BQ; b++) {
                const float *q = Q + size_t(b) * dim + 4 * c;  // wave-uniform -> scalar loads
                acc[b] = fold1<FOLD>(acc[b], v.x, q[0]);
                acc[b] = fold1<FOLD>(acc[b], v.y, q[1]);
                acc[b] = fold1<FOLD>(acc[b], v.z, q[2]);
                acc[b] = fold1<FOLD>(acc[b], v.w, q[3]);
            }
        }
    } else {
        for (uint32_t c = 0; c < dim; c++) {
            float v = x[c];
#pragma unroll
            for (int b = 0; b < BQ; b++) acc[b] = fold1<FOLD>(acc[b], v, Q[size_t(b) * dim + c]);
        }
    }
    float xs = (metric == MET_L2_DIRECT) ? 0.0f : xsq[r];
#pragma unroll
    for (int b = 0; b < BQ; b++) {
        float qs = (metric == MET_L2_DIRECT) ? 0.0f : qsq[b];
        out[uint64_t(b) * ld + j] = epilogue(metric, acc[b], xs, qs);
    }
}

// ---------------------------------------------------------------------------------------------
// gathered scan, LDS-staged variant (dim % 4 == 0): the 256 allowed rows of a tile are streamed in 32-column chunks with fully
// used 128-B lines (8 lanes x 16 B per row segment) and transposed through LDS so that thread t folds row t in order
// (k_scan_exact_lds; row stride 36 floats keeps the ds_read_b128 of a 16-lane group conflict-free).  The tile's row ids are
// staged once.
// ---------------------------------------------------------------------------------------------
constexpr int G_TR = 256;
constexpr int G_CW = 32;
constexpr int G_LDT = G_CW + 4;

template <int BQ, int FOLD>
__global__ __launch_bounds__(256) void k_scan_gather_lds(const float *__restrict__ X, const uint32_t *__restrict__ ids, uint64_t m, uint32_t dim,
                                                         const float *__restrict__ Q, int metric, const float *__restrict__ xsq,
                                                         const float *__restrict__ qsq, float *__restrict__ out, uint64_t ld) {
    __shared__ __attribute__((aligned(16))) float tile[2][G_TR * G_LDT];
    __shared__ uint32_t s_ids[G_TR];
    const uint32_t tid = threadIdx.x;
    const uint64_t j0 = uint64_t(blockIdx.x) * G_TR;
    const uint32_t nchunk = (dim + G_CW - 1) / G_CW;
    Q += uint64_t(blockIdx.y) * BQ * dim;
    qsq += uint64_t(blockIdx.y) * BQ;
    out += uint64_t(blockIdx.y) * BQ * ld;
    {
        const uint64_t j = j0 + tid;
        s_ids[tid] = ids[j < m ? j : m - 1];  // (the tail of the last tile folds the last allowed row again; nothing of it is written)
    }
    __syncthreads();

    float4 stage[8];
    auto load_chunk = [&](uint32_t c) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
            uint32_t f = i * 256 + tid;
            uint32_t r = f >> 3, c4 = f & 7;
            uint32_t col = c * G_CW + c4 * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (col < dim) v = *reinterpret_cast<const float4 *>(X + uint64_t(s_ids[r]) * dim + col);
            stage[i] = v;
        }
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
            uint32_t f = i * 256 + tid;
            uint32_t r = f >> 3, c4 = f & 7;
            *reinterpret_cast<float4 *>(&tile[buf][r * G_LDT + c4 * 4]) = stage[i];
        }
    };

    float acc[BQ];
#pragma unroll
    for (int b = 0; b < BQ; b++) acc[b] = 0.0f;

    load_chunk(0);
    store_chunk(0);
    __syncthreads();
    for (uint32_t c = 0; c < nchunk; c++) {
        int buf = c & 1;
        if (c + 1 < nchunk) load_chunk(c + 1);
        uint32_t cols = dim - c * G_CW;
        if (cols > G_CW) cols = G_CW;
        const float *trow = &tile[buf][tid * G_LDT];
        for (uint32_t jj = 0; jj < cols; jj += 4) {
            float4 v = *reinterpret_cast<const float4 *>(trow + jj);
#pragma unroll
            for (int b = 0; b < BQ; b++) {
                const float *q = Q + size_t(b) * dim + c * G_CW + jj;  // wave-uniform
                acc[b] = fold1<FOLD>(acc[b], v.x, q[0]);
                acc[b] = fold1<FOLD>(acc[b], v.y, q[1]);
                acc[b] = fold1<FOLD>(acc[b], v.z, q[2]);
                acc[b] = fold1<FOLD>(acc[b], v.w, q[3]);
            }
        }
        if (c + 1 < nchunk) store_chunk(buf ^ 1);
        __syncthreads();
    }
    const uint64_t j = j0 + tid;
    if (j < m) {
        float xs = (metric == MET_L2_DIRECT) ? 0.0f : xsq[s_ids[tid]];
#pragma unroll
        for (int b = 0; b < BQ; b++) {
            float qs = (metric == MET_L2_DIRECT) ? 0.0f : qsq[b];
            out[uint64_t(b) * ld + j] = epilogue(metric, acc[b], xs, qs);
        }
    }
}

template <int BQ>
static void scan_gather_bq(const float *X, const uint32_t *ids, uint64_t m, uint32_t dim, const float *Q, uint32_t groups, int metric,
                           const float *xsq, const float *qsq, float *out, uint64_t ld, bool lds, hipStream_t s) {
    dim3 grid((unsigned)((m + 255) / 256), groups), block(256);
    if (metric == MET_L2_DIRECT) {
        if (lds)
            hipLaunchKernelGGL((k_scan_gather_lds<BQ, FOLD_L2>), grid, block, 0, s, X, ids, m, dim, Q, metric, xsq, qsq, out, ld);
        else
            hipLaunchKernelGGL((k_scan_gather_simple<BQ, FOLD_L2>), grid, block, 0, s, X, ids, m, dim, Q, metric, xsq, qsq, out, ld);
    } else {
        if (lds)
            hipLaunchKernelGGL((k_scan_gather_lds<BQ, FOLD_DOT>), grid, block, 0, s, X, ids, m, dim, Q, metric, xsq, qsq, out, ld);
        else
            hipLaunchKernelGGL((k_scan_gather_simple<BQ, FOLD_DOT>), grid, block, 0, s, X, ids, m, dim, Q, metric, xsq, qsq, out, ld);
    }
}

// out[q * ld + j] = D(row ids[j], query q) for nq <= 65535 * 8 queries and the m >= 1 rows of the ascending list ids (ids[j] < the rows
// X holds); the whole groups of 8 queries in one launch (blockIdx.y), the remaining 1..7 in a second one
void launch_scan_gather(const float *X, const uint32_t *ids, uint64_t m, uint32_t dim, const float *Q, uint32_t nq, int metric, const float *xsq,
                        const float *qsq, float *out, uint64_t ld, bool use_lds, hipStream_t s) {
    if (m == 0 || nq == 0) return;
    VDB_REQUIRE(metric == MET_L2_DIRECT || metric == MET_COSINE, "scan_gather: metric");
    VDB_REQUIRE(m < (1ull << 32) && ld >= m && nq / 8 <= 65535, "scan_gather: shape");
    const bool lds = use_lds && (dim & 3) == 0;
    const uint32_t full = nq / 8, rem = nq % 8;
    if (full) scan_gather_bq<8>(X, ids, m, dim, Q, full, metric, xsq, qsq, out, ld, lds, s);
    const float *Qr = Q + uint64_t(full) * 8 * dim, *qr = qsq + uint64_t(full) * 8;
    float *outr = out + uint64_t(full) * 8 * ld;
    switch (rem) {
        case 1: scan_gather_bq<1>(X, ids, m, dim, Qr, 1, metric, xsq, qr, outr, ld, lds, s); break;
        case 2: scan_gather_bq<2>(X, ids, m, dim, Qr, 1, metric, xsq, qr, outr, ld, lds, s); break;
        case 3: scan_gather_bq<3>(X, ids, m, dim, Qr, 1, metric, xsq, qr, outr, ld, lds, s); break;
        case 4: scan_gather_bq<4>(X, ids, m, dim, Qr, 1, metric, xsq, qr, outr, ld, lds, s); break;
        case 5: scan_gather_bq<5>(X, ids, m, dim, Qr, 1, metric, xsq, qr, outr, ld, lds, s); break;
        case 6: scan_gather_bq<6>(X, ids, m, dim, Qr, 1, metric, xsq, qr, outr, ld, lds, s); break;
        case 7: scan_gather_bq<7>(X, ids, m, dim, Qr, 1, metric, xsq, qr, outr, ld, lds, s); break;
        default: break;
    }
    VDB_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------
// pair keys (distance, column j) -> reference-shaped outputs with the row ids[j] (twin of k_finalize, k_exact.hip)
// ---------------------------------------------------------------------------------------------
__global__ void k_filter_finalize(const uint64_t *__restrict__ keys, uint64_t ldk, uint32_t ksel, uint32_t kstride, const uint32_t *__restrict__ ids,
                                  uint64_t m, uint64_t id_offset, uint64_t *__restrict__ out_idx, float *__restrict__ out_dist,
                                  uint64_t *__restrict__ out_count) {
    const uint32_t q = blockIdx.x;
    uint32_t cnt = 0;
    for (uint32_t j = threadIdx.x; j < ksel; j += blockDim.x) {
        const uint64_t c = keys[uint64_t(q) * ldk + j];
        const bool ok = c != PAIR_NONE && uint32_t(c) < m;
        out_idx[uint64_t(q) * kstride + j] = ok ? uint64_t(ids[uint32_t(c)]) + id_offset : 0;
        out_dist[uint64_t(q) * kstride + j] = ok ? f32_from_orderable(uint32_t(c >> 32)) : 0.0f;
        cnt += ok;
    }
    // keys are sorted with PAIR_NONE last, so the count is the number of valid entries
    __shared__ uint32_t total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    atomicAdd(&total, cnt);
    __syncthreads();
    if (threadIdx.x == 0 && out_count) out_count[q] = total;
}
void launch_filter_finalize(const uint64_t *keys, uint64_t ldk, uint32_t nq, uint32_t ksel, uint32_t kstride, const uint32_t *ids, uint64_t m,
                            uint64_t id_offset, uint64_t *out_idx, float *out_dist, uint64_t *out_count, hipStream_t s) {
    if (nq == 0) return;
    hipLaunchKernelGGL(k_filter_finalize, dim3(nq), dim3(64), 0, s, keys, ldk, ksel, kstride, ids, m, id_offset, out_idx, out_dist, out_count);
}

// ---------------------------------------------------------------------------------------------
// gathered scan over MANY allow-lists in one launch (one mask per query: Index::flat_knn_masked_multi_device, multi_plan.hpp).
// One workgroup per work item = (a mask's id list, one tile of 256 of its rows, nb <= 8 slots of that mask's bucket); thread t folds
// column tile * 256 + t for the item's nb queries with the statements of k_scan_gather_simple -- the same fold1 / epilogue, ascending in
// the dimension, so the same bits.  The item and everything reached through it (the id list's base, the slots' query rows) are indexed by
// blockIdx alone: wave-uniform, read by scalar loads.  Nothing is written but out[(slot + b) * ld + j], j < m.
// Two folds, like the simple variant: float4 fetches of the row when dim % 4 == 0, element by element otherwise.
// ---------------------------------------------------------------------------------------------
template <int BQ, int FOLD>
__device__ __forceinline__ void scan_grouped_body(const float *__restrict__ x, uint32_t r, uint64_t j, uint32_t dim, const uint32_t *__restrict__ sq,
                                                  const float *__restrict__ Q, int metric, const float *__restrict__ xsq,
                                                  const float *__restrict__ qsq, float *__restrict__ out, uint64_t ld) {
    const float *qp[BQ];
#pragma unroll
    for (int b = 0; b < BQ; b++) qp[b] = Q + uint64_t(sq[b]) * dim;  // wave-uniform
    float acc[BQ];
#pragma unroll
    for (int b = 0; b < BQ; b++) acc[b] = 0.0f;
    if ((dim & 3) == 0) {
        const float4 *x4 = reinterpret_cast<const float4 *>(x);
        for (uint32_t c = 0; c < dim / 4; c++) {
            float4 v = x4[c];
#pragma unroll
            for (int b = 0; b < BQ; b++) {
                const float *q = qp[b] + 4 * c;
                acc[b] = fold1<FOLD>(acc[b], v.x, q[0]);
                acc[b] = fold1<FOLD>(acc[b], v.y, q[1]);
                acc[b] = fold1<FOLD>(acc[b], v.z, q[2]);
                acc[b] = fold1<FOLD>(acc[b], v.w, q[3]);
            }
        }
    } else {
        for (uint32_t c = 0; c < dim; c++) {
            float v = x[c];
#pragma unroll
            for (int b = 0; b < BQ; b++) acc[b] = fold1<FOLD>(acc[b], v, qp[b][c]);
        }
    }
    float xs = (metric == MET_L2_DIRECT) ? 0.0f : xsq[r];
#pragma unroll
    for (int b = 0; b < BQ; b++) {
        float qs = (metric == MET_L2_DIRECT) ? 0.0f : qsq[sq[b]];
        out[uint64_t(b) * ld + j] = epilogue(metric, acc[b], xs, qs);
    }
}

template <int FOLD>
__global__ __launch_bounds__(256) void k_scan_gather_grouped(const float *__restrict__ X, uint32_t dim, const GroupedItem *__restrict__ items,
                                                             const uint32_t *__restrict__ slot_q, const float *__restrict__ Q, int metric,
                                                             const float *__restrict__ xsq, const float *__restrict__ qsq, float *__restrict__ out,
                                                             uint64_t ld) {
    const GroupedItem it = items[blockIdx.x];
    const uint64_t j = uint64_t(it.tile) * 256 + threadIdx.x;
    if (j >= it.m) return;
    const uint32_t r = it.ids[j];
    const float *x = X + uint64_t(r) * dim;
    const uint32_t *sq = slot_q + it.slot;
    float *o = out + uint64_t(it.slot) * ld;
    switch (it.nb) {  // wave-uniform
        case 1: scan_grouped_body<1, FOLD>(x, r, j, dim, sq, Q, metric, xsq, qsq, o, ld); break;
        case 2: scan_grouped_body<2, FOLD>(x, r, j, dim, sq, Q, metric, xsq, qsq, o, ld); break;
        case 3: scan_grouped_body<3, FOLD>(x, r, j, dim, sq, Q, metric, xsq, qsq, o, ld); break;
        case 4: scan_grouped_body<4, FOLD>(x, r, j, dim, sq, Q, metric, xsq, qsq, o, ld); break;
        case 5: scan_grouped_body<5, FOLD>(x, r, j, dim, sq, Q, metric, xsq, qsq, o, ld); break;
        case 6: scan_grouped_body<6, FOLD>(x, r, j, dim, sq, Q, metric, xsq, qsq, o, ld); break;
        case 7: scan_grouped_body<7, FOLD>(x, r, j, dim, sq, Q, metric, xsq, qsq, o, ld); break;
        case 8: scan_grouped_body<8, FOLD>(x, r, j, dim, sq, Q, metric, xsq, qsq, o, ld); break;
        default: break;
    }
}

void launch_scan_gather_grouped(const float *X, uint32_t dim, const GroupedItem *items, uint64_t nitems, const uint32_t *slot_q, const float *Q,
                                int metric, const float *xsq, const float *qsq, float *out, uint64_t ld, hipStream_t s) {
    if (nitems == 0) return;
    VDB_REQUIRE(metric == MET_L2_DIRECT || metric == MET_COSINE, "scan_gather_grouped: metric");
    VDB_REQUIRE(nitems < (1ull << 31), "scan_gather_grouped: too many work items");
    dim3 grid((unsigned)nitems), block(256);
    if (metric == MET_L2_DIRECT)
        hipLaunchKernelGGL((k_scan_gather_grouped<FOLD_L2>), grid, block, 0, s, X, dim, items, slot_q, Q, metric, xsq, qsq, out, ld);
    else
        hipLaunchKernelGGL((k_scan_gather_grouped<FOLD_DOT>), grid, block, 0, s, X, dim, items, slot_q, Q, metric, xsq, qsq, out, ld);
    VDB_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------
// gathered RANGE scan over many allow-lists in one launch (one mask per query: Index::flat_range_masked_multi_device).  The work item,
// the fold and the epilogue are those of k_scan_gather_grouped -- the same statements, so the same bits -- but the radius is known, so the
// distance is not stored: the pair (slot b, column j) is inside when d <= radius[slot_q[b]] (false for a NaN on either side), and its
// pair key (orderable(d), ROW ids[j]) is appended to the slot's row of `keys`.  The append: a wave ballot, one atomicAdd on the slot's
// counter by lane 0, every lane writing at base + its prefix in the ballot.  Every (slot, column) is evaluated once, so a slot's counter
// never passes its m <= ld.  The order of arrival is not deterministic; the keys of a slot are distinct (distinct rows) and are sorted next.
// A thread whose column is past the list folds nothing and votes "outside": every wave reaches every ballot with all its lanes.
// ---------------------------------------------------------------------------------------------
template <int BQ, int FOLD>
__device__ __forceinline__ void range_grouped_body(const float *__restrict__ x, uint32_t r, bool valid, uint32_t dim, const uint32_t *__restrict__ sq,
                                                   const float *__restrict__ Q, int metric, const float *__restrict__ xsq,
                                                   const float *__restrict__ qsq, const float *__restrict__ radius, uint64_t *__restrict__ keys,
                                                   uint64_t ld, uint32_t *__restrict__ cnt) {
    const float *qp[BQ];
#pragma unroll
    for (int b = 0; b < BQ; b++) qp[b] = Q + uint64_t(sq[b]) * dim;  // wave-uniform
    float acc[BQ];
#pragma unroll
    for (int b = 0; b < BQ; b++) acc[b] = 0.0f;
    if (valid) {
        if ((dim & 3) == 0) {
            const float4 *x4 = reinterpret_cast<const float4 *>(x);
            for (uint32_t c = 0; c < dim / 4; c++) {
                float4 v = x4[c];
#pragma unroll
                for (int b = 0; b < BQ; b++) {
                    const float *q = qp[b] + 4 * c;
                    acc[b] = fold1<FOLD>(acc[b], v.x, q[0]);
                    acc[b] = fold1<FOLD>(acc[b], v.y, q[1]);
                    acc[b] = fold1<FOLD>(acc[b], v.z, q[2]);
                    acc[b] = fold1<FOLD>(acc[b], v.w, q[3]);
                }
            }
        } else {
            for (uint32_t c = 0; c < dim; c++) {
                float v = x[c];
#pragma unroll
                for (int b = 0; b < BQ; b++) acc[b] = fold1<FOLD>(acc[b], v, qp[b][c]);
            }
        }
    }
    const float xs = (metric == MET_L2_DIRECT || !valid) ? 0.0f : xsq[r];
    const uint32_t lane = threadIdx.x & 63;
#pragma unroll
    for (int b = 0; b < BQ; b++) {
        const float qs = (metric == MET_L2_DIRECT) ? 0.0f : qsq[sq[b]];
        const float d = epilogue(metric, acc[b], xs, qs);
        const bool keep = valid && d <= radius[sq[b]];  // (the radius is wave-uniform, like the query rows)
        const uint64_t vote = __ballot(keep);
        if (vote == 0) continue;  // wave-uniform
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(cnt + b, (uint32_t)__builtin_popcountll(vote));
        base = __shfl(base, 0);
        if (keep) keys[uint64_t(b) * ld + base + (uint32_t)__builtin_popcountll(vote & ((1ull << lane) - 1))] = pair_key(d, r);
    }
}

template <int FOLD>
__global__ __launch_bounds__(256) void k_range_gather_grouped(const float *__restrict__ X, uint32_t dim, const GroupedItem *__restrict__ items,
                                                              const uint32_t *__restrict__ slot_q, const float *__restrict__ Q, int metric,
                                                              const float *__restrict__ xsq, const float *__restrict__ qsq,
                                                              const float *__restrict__ radius, uint64_t *__restrict__ keys, uint64_t ld,
                                                              uint32_t *__restrict__ cnt) {
    const GroupedItem it = items[blockIdx.x];
    const uint64_t j = uint64_t(it.tile) * 256 + threadIdx.x;
    const bool valid = j < it.m;
    const uint32_t r = valid ? it.ids[j] : 0;
    const float *x = X + uint64_t(r) * dim;
    const uint32_t *sq = slot_q + it.slot;
    uint64_t *o = keys + uint64_t(it.slot) * ld;
    uint32_t *c = cnt + it.slot;
    switch (it.nb) {  // wave-uniform
        case 1: range_grouped_body<1, FOLD>(x, r, valid, dim, sq, Q, metric, xsq, qsq, radius, o, ld, c); break;
        case 2: range_grouped_body<2, FOLD>(x, r, valid, dim, sq, Q, metric, xsq, qsq, radius, o, ld, c); break;
        case 3: range_grouped_body<3, FOLD>(x, r, valid, dim, sq, Q, metric, xsq, qsq, radius, o, ld, c); break;
        case 4: range_grouped_body<4, FOLD>(x, r, valid, dim, sq, Q, metric, xsq, qsq, radius, o, ld, c); break;
        case 5: range_grouped_body<5, FOLD>(x, r, valid, dim, sq, Q, metric, xsq, qsq, radius, o, ld, c); break;
        case 6: range_grouped_body<6, FOLD>(x, r, valid, dim, sq, Q, metric, xsq, qsq, radius, o, ld, c); break;
        case 7: range_grouped_body<7, FOLD>(x, r, valid, dim, sq, Q, metric, xsq, qsq, radius, o, ld, c); break;
        case 8: range_grouped_body<8, FOLD>(x, r, valid, dim, sq, Q, metric, xsq, qsq, radius, o, ld, c); break;
        default: break;
    }
}

void launch_range_gather_grouped(const float *X, uint32_t dim, const GroupedItem *items, uint64_t nitems, const uint32_t *slot_q, const float *Q,
                                 int metric, const float *xsq, const float *qsq, const float *radius, uint64_t *keys, uint64_t ld, uint32_t *cnt,
                                 hipStream_t s) {
    if (nitems == 0) return;
    VDB_REQUIRE(metric == MET_L2_DIRECT || metric == MET_COSINE, "range_gather_grouped: metric");
    VDB_REQUIRE(nitems < (1ull << 31), "range_gather_grouped: too many work items");
    dim3 grid((unsigned)nitems), block(256);
    if (metric == MET_L2_DIRECT)
        hipLaunchKernelGGL((k_range_gather_grouped<FOLD_L2>), grid, block, 0, s, X, dim, items, slot_q, Q, metric, xsq, qsq, radius, keys, ld, cnt);
    else
        hipLaunchKernelGGL((k_range_gather_grouped<FOLD_DOT>), grid, block, 0, s, X, dim, items, slot_q, Q, metric, xsq, qsq, radius, keys, ld, cnt);
    VDB_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------
// twin of k_filter_finalize for a chunk of slots with a list of their own each: slot s = query slot_q[s] of the call, the columns of its
// keys index slot_ids[s], slot_m[s] of them are real.  A padding column (>= slot_m[s]) carries a NaN distance and sorts behind every
// real column, so the real keys are a prefix of the sorted row and the cut is `column < slot_m[s]`.  Every one of the query's kstride
// output slots is written (zero past the count), and its count.
// ---------------------------------------------------------------------------------------------
__global__ void k_filter_finalize_grouped(const uint64_t *__restrict__ keys, uint64_t ldk, uint32_t ksel, uint32_t kstride,
                                          const uint32_t *const *__restrict__ slot_ids, const uint32_t *__restrict__ slot_m,
                                          const uint32_t *__restrict__ slot_q, uint64_t id_offset, uint64_t *__restrict__ out_idx,
                                          float *__restrict__ out_dist, uint64_t *__restrict__ out_count) {
    const uint32_t sl = blockIdx.x;
    const uint32_t q = slot_q[sl], mg = slot_m[sl];
    const uint32_t *ids = slot_ids[sl];
    uint32_t cnt = 0;
    for (uint32_t j = threadIdx.x; j < kstride; j += blockDim.x) {
        const uint64_t c = j < ksel ? keys[uint64_t(sl) * ldk + j] : PAIR_NONE;
        const bool ok = c != PAIR_NONE && uint32_t(c) < mg;
        out_idx[uint64_t(q) * kstride + j] = ok ? uint64_t(ids[uint32_t(c)]) + id_offset : 0;
        out_dist[uint64_t(q) * kstride + j] = ok ? f32_from_orderable(uint32_t(c >> 32)) : 0.0f;
        cnt += ok;
    }
    __shared__ uint32_t total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    atomicAdd(&total, cnt);
    __syncthreads();
    if (threadIdx.x == 0) out_count[q] = total;
}
void launch_filter_finalize_grouped(const uint64_t *keys, uint64_t ldk, uint32_t nslots, uint32_t ksel, uint32_t kstride, const uint32_t *const *slot_ids,
                                    const uint32_t *slot_m, const uint32_t *slot_q, uint64_t id_offset, uint64_t *out_idx, float *out_dist,
                                    uint64_t *out_count, hipStream_t s) {
    if (nslots == 0) return;
    hipLaunchKernelGGL(k_filter_finalize_grouped, dim3(nslots), dim3(64), 0, s, keys, ldk, ksel, kstride, slot_ids, slot_m, slot_q, id_offset, out_idx,
                       out_dist, out_count);
}

// ---------------------------------------------------------------------------------------------
// masked copy of the 8-bit pass's row constants: {+inf, 0} where the bit is clear, the index's own pair elsewhere (rows in
// [n, rows_pad) have no bit and are copied: they carry {+inf, 0} already)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mask_rowc(const float2 *__restrict__ rowc, const uint64_t *__restrict__ bits, uint64_t n, uint64_t rows_pad,
                                                   float2 *__restrict__ out) {
    const uint64_t r = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (r >= rows_pad) return;
    float2 v = rowc[r];
    if (r < n && !mask_bit(bits, r)) v = make_float2(INFINITY, 0.0f);
    out[r] = v;
}
void launch_mask_rowc(const float *rowc, const uint64_t *bits, uint64_t n, uint64_t rows_pad, float *out, hipStream_t s) {
    if (rows_pad == 0) return;
    hipLaunchKernelGGL(k_mask_rowc, dim3((unsigned)((rows_pad + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const float2 *>(rowc), bits, n,
                       rows_pad, reinterpret_cast<float2 *>(out));
}

// tau[q] = min(tau[q], FLT_MAX); NaN -> -inf.  The filter keeps key <= tau and a masked row's key is +inf: a threshold of +inf (a
// sample with fewer allowed rows than the selection's rank) would let every masked row through.  Clamped, such a query collects every
// allowed row with a finite key.
__global__ void k_tau_clamp(float *__restrict__ tau, uint32_t nq) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const float t = tau[q];
    tau[q] = t != t ? -INFINITY : fminf(t, FLT_MAX);
}
void launch_tau_clamp(float *tau, uint32_t nq, hipStream_t s) {
    if (nq == 0) return;
    hipLaunchKernelGGL(k_tau_clamp, dim3((nq + 255) / 256), dim3(256), 0, s, tau, nq);
}

// dist[q * ld + i] = NaN for every row i < n whose bit is clear (range scan: such a row is never inside a radius)
__global__ __launch_bounds__(256) void k_mask_dense_nan(float *__restrict__ dist, uint64_t ld, uint64_t n, const uint64_t *__restrict__ bits) {
    const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    if (!mask_bit(bits, i)) dist[uint64_t(blockIdx.y) * ld + i] = __uint_as_float(0x7fc00000u);
}
void launch_mask_dense_nan(float *dist, uint64_t ld, uint64_t n, uint32_t nq, const uint64_t *bits, hipStream_t s) {
    if (nq == 0 || n == 0) return;
    hipLaunchKernelGGL(k_mask_dense_nan, dim3((unsigned)((n + 255) / 256), nq), dim3(256), 0, s, dist, ld, n, bits);
}

}  // namespace vdb
