// k_kmeans.hip -- the kernels of one Lloyd iteration over the rows of an f32 index (flat_kmeans.hip drives them, kmeans_plan.hpp lays them
// out; docs/DESIGN_flat.md 4.1ad).
//
// THE RULE: row i belongs to the centroid with the smallest pair_key(D(centroid, row), centroid id) -- D the reference's pair distance (strict
// left fold over the dimension, products and sums separately rounded; the difference form for L2Sqr, 1 - dot / max(|a||b|, 1e-10) with
// strict-fold norms for Cosine), NaN greatest, ties to the lowest id.  Evaluating it costs rows x centroids dependent folds, so:
//
// k_kmeans_assign   the matrix pass.  A workgroup of 4 waves owns 128 rows and streams the centroid set past them, 64 centroids x 32
//                   dimensions per step.  Both operands go through LDS as split-bf16 planes in MFMA fragment order: the centroids'
//                   planes are made once per iteration (k_kmeans_prep), a step's 8 KB of them is a straight copy; the rows are split in
//                   flight, each thread converting the 2 x 8 floats whose fragment slots it owns.  A wave multiplies its 2 row blocks of
//                   16 with the 4 centroid blocks of 16: 8 accumulators, 3 MFMAs each per step (hi.hi, hi.lo, lo.hi).  The CENTROIDS are the
//                   A operand, so a lane's four accumulator words are four centroids of ONE row (lane & 15) and the argmin runs down
//                   registers: per row block a lane keeps (best score, best id, second-best score) over every centroid tile, and only
//                   after the last tile the four lanes that share a row meet, by lane_xor32<16> / <32>.  second - best > E(row)
//                   (kmeans_err_bound) settles the row; the others -- ties, NaN, close calls -- are appended to the unsure list: a wave
//                   ballot, a prefix popcount, one integer atomic per wave.
//                   128 x 64: 32 accumulator, 24 operand and 16 prefetch registers per lane leave the wave far below 128 VGPRs (two
//                   workgroups per SIMD pair hide each other's barriers), a step issues 24 MFMAs per 12 ds_read_b128, and at 1024
//                   centroids a row tile is fetched 16 times, all but the first from L2.  256 rows per workgroup would halve the operand
//                   reads per MFMA but double every per-lane state; 64 rows would leave the centroid copy unamortised.
// k_kmeans_resolve  one wave per unsure row: the row staged in LDS, lanes striding over the centroids, each pair through the strict fold,
//                   the minimum pair_key by lane_xor64.  Overwrites assign[] and best[] of the row.
// k_kmeans_best     the exact distance of every row to its centroid, only when inertia or per-row distances are wanted: a wave per 64
//                   rows shares the reads (coalesced, through LDS), a lane folds one row.
// k_kmeans_count / _scan / _order_*  rows placed by cluster, stably: member counts by integer atomics, their exclusive scan, and an LSD
//                   counting sort of the positions by the 8-bit digits of the cluster id -- per-workgroup digit histograms, a scan in
//                   (digit, workgroup) order, a stable scatter by wave ballots -- so every cluster lists its members in ascending row order.
// k_kmeans_update   one workgroup of 16 waves per (cluster, 64 columns): a lane owns a column, wave s folds segment s of the member list
//                   (kmeans_segment: a function of the member count alone) into an f64 register, the 16 partial sums meet in LDS and are
//                   added in segment order, divided by the count in f64 and rounded to f32 once.  A cluster without members keeps its
//                   centroid (kmeans_group, pq.hip, does the same).
// k_kmeans_reduce_* rows that changed cluster (an integer count) and the inertia: f64 sums in a fixed tree per 4096 positions, the
//                   partial sums added in order by one workgroup.
// No float atomics anywhere: every output is a function of (rows, centroids) alone.
#include <algorithm>
#include <cmath>

#include "common.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace vdb {

typedef __bf16 km_bf16x8 __attribute__((ext_vector_type(8)));
typedef float km_f32x4 __attribute__((ext_vector_type(4)));

// hi/lo split of 8 consecutive f32 -> two packed bf16x8 (round to nearest even twice; NaN stays NaN)
__device__ __forceinline__ void km_split8(const float (&v)[8], uint4 &hi, uint4 &lo) {
    uint32_t h[8], l[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const __bf16 hb = (__bf16)v[i];
        const __bf16 lb = (__bf16)(v[i] - (float)hb);
        h[i] = __builtin_bit_cast(unsigned short, hb);
        l[i] = __builtin_bit_cast(unsigned short, lb);
    }
    hi = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
    lo = make_uint4(l[0] | (l[1] << 16), l[2] | (l[3] << 16), l[4] | (l[5] << 16), l[6] | (l[7] << 16));
}
// columns [col, col + 8) of a row of `dim` floats, zero past its end; VEC4: dim % 4 == 0 and the row is 16-byte aligned
template <bool VEC4>
__device__ __forceinline__ void km_load8(const float *row, uint32_t dim, uint32_t col, float (&v)[8]) {
    if (VEC4) {
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 a = col < dim ? *reinterpret_cast<const float4 *>(row + col) : z;
        const float4 b = col + 4 < dim ? *reinterpret_cast<const float4 *>(row + col + 4) : z;
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = col + i < dim ? row[col + i] : 0.0f;
    }
}

// the reference's pair distance from the fold: acc = sum (a - b)^2, or the dot with both strict-fold |.|^2 (k_exact.hip's epilogue)
__device__ __forceinline__ float km_fold1(bool cosine, float acc, float x, float q) {
    if (cosine) {
        const float p = x * q;
        return acc + p;
    }
    const float df = x - q;
    const float sq = df * df;
    return acc + sq;
}
__device__ __forceinline__ float km_epilogue(bool cosine, float acc, float xsq, float csq) {
    if (!cosine) return acc;
    const float den = fmaxf(sqrtf(csq) * sqrtf(xsq), 1e-10f);
    const float r = acc / den;
    return 1.0f - r;
}
__device__ __forceinline__ uint64_t km_row_of(const uint32_t *ids, uint64_t pos) { return ids ? uint64_t(ids[pos]) : pos; }

// ---- centroid preparation ---------------------------------------------------------------------------------------------------------------
// planes[(((tile * KB + kb) * 4 + sub) * 2 + plane) * 64 + lane]: centroid tile * 64 + sub * 16 + (lane & 15), columns kb * 32 + 8 * (lane >> 4) ..
// + 8, zero for centroids >= c and columns >= dim
__global__ __launch_bounds__(256) void k_kmeans_prep(const float *__restrict__ C, uint32_t c, uint32_t dim, uint32_t KB, uint64_t total,
                                                     uint4 *__restrict__ planes) {
    const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;  // (tile, kb, sub, lane)
    if (i >= total) return;
    const uint32_t l = uint32_t(i & 63), sub = uint32_t(i >> 6) & 3;
    const uint64_t tk = i >> 8;
    const uint32_t kb = uint32_t(tk % KB), tile = uint32_t(tk / KB);
    const uint32_t cid = tile * KM_CENT_TILE + sub * 16 + (l & 15), col = kb * KM_KBLOCK + 8 * (l >> 4);
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (cid < c) km_load8<false>(C + uint64_t(cid) * dim, dim, col, v);
    uint4 hi, lo;
    km_split8(v, hi, lo);
    planes[(i >> 6) * 128 + l] = hi;
    planes[(i >> 6) * 128 + 64 + l] = lo;
}
// csq[j] = strict-fold |c_j|^2 (launch_row_sqnorm's fold), 0 for the padding up to c_pad; counters word: the largest of them as f32 bits
// (non-negative floats order as their bits; a NaN lies above every number and makes every row unsure)
__global__ __launch_bounds__(256) void k_kmeans_cnorm(const float *__restrict__ C, uint32_t c, uint32_t c_pad, uint32_t dim, float *__restrict__ csq,
                                                      uint32_t *__restrict__ cmax_bits) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= c_pad) return;
    float acc = 0.0f;
    if (j < c) {
        const float *x = C + uint64_t(j) * dim;
        for (uint32_t d = 0; d < dim; d++) acc = km_fold1(true, acc, x[d], x[d]);
        atomicMax(cmax_bits, __float_as_uint(acc));
    }
    csq[j] = acc;
}

// ---- the matrix pass ----------------------------------------------------------------------------------------------------------------------
struct KmAssignArgs {
    const float *X;       // the index's rows
    const float *xsq;     // their strict-fold |x|^2
    const uint32_t *ids;  // the allowed rows, ascending (nullptr: position = row)
    uint64_t m;           // positions
    uint32_t dim, KB, c, n_ctiles;
    const uint4 *planes;
    const float *csq;
    const uint32_t *cmax_bits;
    int cosine;
    uint32_t *assign;  // [row]
    float *best;       // [row]: the approximate distance (k_kmeans_best / k_kmeans_resolve replace it)
    uint32_t *unsure;  // positions
    unsigned long long *unsure_n;
};

struct KmBest {
    float best, second;
    uint32_t id, nan;
};
__device__ __forceinline__ void km_offer(KmBest &b, float s, uint32_t id) {
    if (s != s)
        b.nan = 1;
    else if (s < b.best) {
        b.second = b.best;
        b.best = s;
        b.id = id;
    } else if (s < b.second)
        b.second = s;
}
// the state of the lane J away folded in (the two lanes saw disjoint centroids of the same row)
template <uint32_t J>
__device__ __forceinline__ void km_meet(KmBest &b, uint32_t lane) {
    const float ob = __uint_as_float(lane_xor32<J>(__float_as_uint(b.best), lane));
    const float os = __uint_as_float(lane_xor32<J>(__float_as_uint(b.second), lane));
    const uint32_t oi = lane_xor32<J>(b.id, lane);
    b.nan |= lane_xor32<J>(b.nan, lane);
    if (ob < b.best) {
        b.second = fminf(b.best, os);
        b.best = ob;
        b.id = oi;
    } else {
        b.second = fminf(b.second, ob);
    }
}

template <bool VEC4>
__global__ __launch_bounds__(256) void k_kmeans_assign(const KmAssignArgs a) {
    __shared__ uint4 s_x[8 * 2 * 64];  // [row block][hi | lo][lane]
    __shared__ uint4 s_c[4 * 2 * 64];  // [centroid block][hi | lo][lane]
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
    const uint64_t p0 = uint64_t(blockIdx.x) * KM_ROW_TILE;

    // the two (row, 8 columns) fragment slots this thread fills per step: slot u = tid + 256 i is row block u >> 6, lane u & 63
    const float *xrow[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const uint32_t u = tid + 256 * i;
        const uint64_t pos = p0 + (u >> 6) * 16 + (u & 15);
        xrow[i] = pos < a.m ? a.X + km_row_of(a.ids, pos) * a.dim : nullptr;
    }
    const uint32_t xcol = 8 * g;  // (u & 63) >> 4 == lane >> 4 for both slots

    // this wave's rows: row block 2 wave + j, row r of it
    uint64_t my_row[2];
    float my_xsq[2];
    bool my_valid[2];
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const uint64_t pos = p0 + (2 * wave + j) * 16 + r;
        my_valid[j] = pos < a.m;
        my_row[j] = my_valid[j] ? km_row_of(a.ids, pos) : 0;
        my_xsq[j] = my_valid[j] ? a.xsq[my_row[j]] : 0.0f;
    }
    KmBest st[2];
#pragma unroll
    for (int j = 0; j < 2; j++) st[j] = {INFINITY, INFINITY, 0u, 0u};

    km_f32x4 acc[2][4];
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
        for (int t = 0; t < 4; t++) acc[j][t] = {0.f, 0.f, 0.f, 0.f};

    float xv[2][8];
    uint4 cv[2];
    auto fetch = [&](uint32_t ct, uint32_t kb) {
#pragma unroll
        for (int i = 0; i < 2; i++) {
#pragma unroll
            for (int e = 0; e < 8; e++) xv[i][e] = 0.0f;
            if (xrow[i]) km_load8<VEC4>(xrow[i], a.dim, kb * KM_KBLOCK + xcol, xv[i]);
        }
        const uint4 *src = a.planes + (uint64_t(ct) * a.KB + kb) * 512;
        cv[0] = src[tid];
        cv[1] = src[tid + 256];
    };

    fetch(0, 0);
    for (uint32_t ct = 0; ct < a.n_ctiles; ct++) {
        for (uint32_t kb = 0; kb < a.KB; kb++) {
            __syncthreads();  // every wave has read the previous step's fragments
#pragma unroll
            for (int i = 0; i < 2; i++) {
                uint4 hi, lo;
                km_split8(xv[i], hi, lo);
                const uint32_t u = tid + 256 * i;
                s_x[((u >> 6) * 2 + 0) * 64 + (u & 63)] = hi;
                s_x[((u >> 6) * 2 + 1) * 64 + (u & 63)] = lo;
            }
            s_c[tid] = cv[0];
            s_c[tid + 256] = cv[1];
            __syncthreads();
            // the next step's operands travel while this one multiplies
            if (kb + 1 < a.KB)
                fetch(ct, kb + 1);
            else if (ct + 1 < a.n_ctiles)
                fetch(ct + 1, 0);
            km_bf16x8 xh[2], xl[2];
#pragma unroll
            for (int j = 0; j < 2; j++) {
                xh[j] = __builtin_bit_cast(km_bf16x8, s_x[((2 * wave + j) * 2 + 0) * 64 + lane]);
                xl[j] = __builtin_bit_cast(km_bf16x8, s_x[((2 * wave + j) * 2 + 1) * 64 + lane]);
            }
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const km_bf16x8 ch = __builtin_bit_cast(km_bf16x8, s_c[(t * 2 + 0) * 64 + lane]);
                const km_bf16x8 cl = __builtin_bit_cast(km_bf16x8, s_c[(t * 2 + 1) * 64 + lane]);
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    acc[j][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ch, xh[j], acc[j][t], 0, 0, 0);
                    acc[j][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ch, xl[j], acc[j][t], 0, 0, 0);
                    acc[j][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cl, xh[j], acc[j][t], 0, 0, 0);
                }
            }
        }
        // the tile's epilogue: accumulator word e of block t is centroid ct * 64 + t * 16 + 4 g + e against row r
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const uint32_t id0 = ct * KM_CENT_TILE + t * 16 + 4 * g;
            const float4 cs4 = *reinterpret_cast<const float4 *>(a.csq + id0);  // (csq is padded to whole tiles)
            const float cs[4] = {cs4.x, cs4.y, cs4.z, cs4.w};
#pragma unroll
            for (int j = 0; j < 2; j++) {
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    float s;
                    if (a.cosine) {
                        s = km_epilogue(true, acc[j][t][e], my_xsq[j], cs[e]);
                    } else {
                        const float tw = 2.0f * acc[j][t][e];
                        s = cs[e] - tw;
                    }
                    if (id0 + e < a.c) km_offer(st[j], s, id0 + e);
                    acc[j][t][e] = 0.0f;
                }
            }
        }
    }

    // the four lanes of a row meet; lanes 0 .. 15 write
    const float cmax = __uint_as_float(*a.cmax_bits);
    bool unsure[2];
#pragma unroll
    for (int j = 0; j < 2; j++) {
        km_meet<16>(st[j], lane);
        km_meet<32>(st[j], lane);
        const float xs = my_xsq[j];
        const float d_best = a.cosine ? st[j].best : st[j].best + xs;
        const float E = kmeans_err_bound(a.dim, a.cosine, sqrtf(xs) * 1.01f, sqrtf(cmax) * 1.01f, fmaxf(d_best, 0.0f) * 1.01f);
        const float gap = st[j].second - st[j].best;
        const bool writer = g == 0 && my_valid[j];
        unsure[j] = writer && (st[j].nan || !(gap > E));  // (NaN anywhere: unsure)
        if (writer) {
            a.assign[my_row[j]] = st[j].id;
            a.best[my_row[j]] = d_best;
        }
    }
    const uint64_t b0 = __ballot(unsure[0]), b1 = __ballot(unsure[1]);
    const uint32_t n0 = (uint32_t)__builtin_popcountll(b0), n1 = (uint32_t)__builtin_popcountll(b1);
    if (n0 + n1) {  // wave-uniform
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(a.unsure_n, (unsigned long long)(n0 + n1));
        base = __shfl(base, 0);
        const uint64_t lt = (1ull << lane) - 1;
        if (unsure[0]) a.unsure[base + __builtin_popcountll(b0 & lt)] = uint32_t(p0 + (2 * wave + 0) * 16 + r);
        if (unsure[1]) a.unsure[base + n0 + __builtin_popcountll(b1 & lt)] = uint32_t(p0 + (2 * wave + 1) * 16 + r);
    }
}

// ---- the exact decision of the unsure rows ------------------------------------------------------------------------------------------------
// one wave per listed position (a grid-stride walk: the list's length is known on the device only)
template <bool VEC4>
__global__ __launch_bounds__(64) void k_kmeans_resolve(const float *__restrict__ X, const float *__restrict__ xsq, const uint32_t *__restrict__ ids,
                                                       uint32_t dim, const float *__restrict__ C, const float *__restrict__ csq, uint32_t c, int cosine,
                                                       const uint32_t *__restrict__ unsure, const unsigned long long *__restrict__ unsure_n,
                                                       uint32_t *__restrict__ assign, float *__restrict__ best) {
    extern __shared__ __attribute__((aligned(16))) float s_row[];
    const uint32_t lane = threadIdx.x;
    const uint64_t total = *unsure_n;
    for (uint64_t u = blockIdx.x; u < total; u += gridDim.x) {
        const uint64_t row = km_row_of(ids, unsure[u]);
        const float *x = X + row * dim;
        __syncthreads();  // the previous row has been folded
        for (uint32_t j = lane; j < dim; j += 64) s_row[j] = x[j];
        __syncthreads();
        const float xs = cosine ? xsq[row] : 0.0f;
        uint64_t key = PAIR_NONE;
        float dmin = 0.0f;
        for (uint32_t cid = lane; cid < c; cid += 64) {
            const float *cr = C + uint64_t(cid) * dim;
            float acc = 0.0f;
            if (VEC4) {
                const float4 *c4 = reinterpret_cast<const float4 *>(cr);
                const float4 *x4 = reinterpret_cast<const float4 *>(s_row);
                for (uint32_t j = 0; j < dim / 4; j++) {
                    const float4 v = c4[j], w = x4[j];
                    acc = km_fold1(cosine, acc, v.x, w.x);
                    acc = km_fold1(cosine, acc, v.y, w.y);
                    acc = km_fold1(cosine, acc, v.z, w.z);
                    acc = km_fold1(cosine, acc, v.w, w.w);
                }
            } else {
                for (uint32_t j = 0; j < dim; j++) acc = km_fold1(cosine, acc, cr[j], s_row[j]);
            }
            const float d = km_epilogue(cosine, acc, xs, cosine ? csq[cid] : 0.0f);
            const uint64_t k = pair_key(d, cid);
            if (k < key) {
                key = k;
                dmin = d;
            }
        }
        uint64_t kmin = key;
        uint64_t o;
        o = lane_xor64<32>(kmin, lane), kmin = o < kmin ? o : kmin;
        o = lane_xor64<16>(kmin, lane), kmin = o < kmin ? o : kmin;
        o = lane_xor64<8>(kmin, lane), kmin = o < kmin ? o : kmin;
        o = lane_xor64<4>(kmin, lane), kmin = o < kmin ? o : kmin;
        o = lane_xor64<2>(kmin, lane), kmin = o < kmin ? o : kmin;
        o = lane_xor64<1>(kmin, lane), kmin = o < kmin ? o : kmin;
        if (key == kmin) {  // exactly one lane: the id is part of the key (c >= 1, so a key exists)
            assign[row] = uint32_t(kmin);
            best[row] = dmin;
        }
    }
}

// ---- the exact distance of every row to its centroid --------------------------------------------------------------------------------------
// One wave per 64 positions.  A strict fold is a chain of dim dependent adds, so a wave cannot share one; what it can share is the reads:
// for every 64 columns the wave fetches the 64 rows and their centroids one after the other, 256 contiguous bytes each, into two
// [64][65] LDS tiles, and lane r then folds row r's 64 columns out of its own (conflict-free) tile row.
__global__ __launch_bounds__(64) void k_kmeans_best(const float *__restrict__ X, const float *__restrict__ xsq, const uint32_t *__restrict__ ids,
                                                    uint64_t m, uint32_t dim, const float *__restrict__ C, const float *__restrict__ csq, uint32_t c,
                                                    int cosine, const uint32_t *__restrict__ assign, float *__restrict__ best) {
    __shared__ float sx[64][65], sc[64][65];
    __shared__ uint64_t s_row[64];
    __shared__ uint32_t s_cid[64];
    const uint32_t lane = threadIdx.x;
    const uint64_t pos = uint64_t(blockIdx.x) * 64 + lane;
    const uint64_t row = pos < m ? km_row_of(ids, pos) : 0;
    const uint32_t cid = pos < m ? assign[row] : KM_LABEL_NONE;
    const bool ok = cid < c;  // (every position has been assigned: the test only keeps a stray id inside the arrays)
    s_row[lane] = row;
    s_cid[lane] = ok ? cid : KM_LABEL_NONE;
    __syncthreads();
    float acc = 0.0f;
    for (uint32_t c0 = 0; c0 < dim; c0 += 64) {
        const uint32_t col = c0 + lane;
        for (uint32_t r = 0; r < 64; r++) {
            const uint32_t rc = s_cid[r];  // wave-uniform
            if (rc == KM_LABEL_NONE) continue;
            sx[r][lane] = col < dim ? X[s_row[r] * dim + col] : 0.0f;
            sc[r][lane] = col < dim ? C[uint64_t(rc) * dim + col] : 0.0f;
        }
        __syncthreads();
        const uint32_t len = dim - c0 < 64 ? dim - c0 : 64;
        if (ok)
            for (uint32_t j = 0; j < len; j++) acc = km_fold1(cosine, acc, sc[lane][j], sx[lane][j]);
        __syncthreads();
    }
    if (ok) best[row] = km_epilogue(cosine, acc, cosine ? xsq[row] : 0.0f, cosine ? csq[cid] : 0.0f);
}

// ---- rows by cluster ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_kmeans_count(const uint32_t *__restrict__ assign, const uint32_t *__restrict__ ids, uint64_t m,
                                                      uint32_t c, uint32_t *__restrict__ count) {
    const uint64_t p = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (p >= m) return;
    const uint32_t cid = assign[km_row_of(ids, p)];
    if (cid < c) atomicAdd(&count[cid], 1u);  // (every position has been assigned: the test only keeps a stray id inside the array)
}
// offsets[0 .. c] = the exclusive scan of count[0 .. c), sizes[j] = count[j]; one workgroup of 1024 threads, a run of clusters per thread
__global__ __launch_bounds__(1024) void k_kmeans_scan(const uint32_t *__restrict__ count, uint32_t c, uint32_t *__restrict__ offsets,
                                                      uint64_t *__restrict__ sizes) {
    __shared__ uint32_t sc[1024];
    const uint32_t tid = threadIdx.x, per = (c + 1023) / 1024;
    const uint32_t a = tid * per < c ? tid * per : c, b = a + per < c ? a + per : c;
    uint32_t sum = 0;
    for (uint32_t j = a; j < b; j++) sum += count[j];
    sc[tid] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) {
        const uint32_t v = tid >= off ? sc[tid - off] : 0u;
        __syncthreads();
        sc[tid] += v;
        __syncthreads();
    }
    uint32_t run = sc[tid] - sum;
    for (uint32_t j = a; j < b; j++) {
        offsets[j] = run;
        sizes[j] = count[j];
        run += count[j];
    }
    if (tid == 1023) offsets[c] = sc[1023];
}
// One pass of the counting sort over the 8-bit digit `shift` of the cluster id.  FIRST: item i is position i; else item i is in[i].
template <bool FIRST>
__device__ __forceinline__ uint32_t km_item(const uint32_t *in, uint64_t i) { return FIRST ? uint32_t(i) : in[i]; }
// hist[digit * nblk + blk] = items of workgroup blk with that digit
template <bool FIRST>
__global__ __launch_bounds__(256) void k_kmeans_order_hist(const uint32_t *__restrict__ in, const uint32_t *__restrict__ assign,
                                                           const uint32_t *__restrict__ ids, uint64_t m, uint32_t nblk, uint32_t shift,
                                                           uint32_t *__restrict__ hist) {
    __shared__ uint32_t hs[256];
    const uint32_t blk = blockIdx.x, tid = threadIdx.x;
    hs[tid] = 0;
    __syncthreads();
    const uint64_t base = uint64_t(blk) * KM_ORDER_CHUNK;
    for (uint32_t i = tid; i < KM_ORDER_CHUNK; i += 256)
        if (base + i < m) atomicAdd(&hs[(assign[km_row_of(ids, km_item<FIRST>(in, base + i))] >> shift) & 255u], 1u);
    __syncthreads();
    hist[uint64_t(tid) * nblk + blk] = hs[tid];
}
// the exclusive prefix of the histogram in (digit, workgroup) order: the first output slot of every (digit, workgroup)
__global__ __launch_bounds__(256) void k_kmeans_order_scan(uint32_t *__restrict__ hist, uint32_t nblk) {
    __shared__ uint32_t sc[256];
    const uint32_t tid = threadIdx.x;
    uint32_t *h = hist + uint64_t(tid) * nblk;
    uint32_t sum = 0;
    for (uint32_t b = 0; b < nblk; b++) sum += h[b];
    sc[tid] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < 256; off <<= 1) {
        const uint32_t v = tid >= off ? sc[tid - off] : 0u;
        __syncthreads();
        sc[tid] += v;
        __syncthreads();
    }
    uint32_t run = sc[tid] - sum;
    for (uint32_t b = 0; b < nblk; b++) {
        const uint32_t v = h[b];
        h[b] = run;
        run += v;
    }
}
// the stable scatter: a wave owns 1024 contiguous items and places them 64 at a time, in order -- an item's slot is the first slot of its
// (digit, workgroup) + the items of that digit in earlier waves, in earlier steps of this wave and in lower lanes of this step
template <bool FIRST>
__global__ __launch_bounds__(256) void k_kmeans_order_scatter(const uint32_t *__restrict__ in, const uint32_t *__restrict__ assign,
                                                              const uint32_t *__restrict__ ids, uint64_t m, uint32_t nblk, uint32_t shift,
                                                              const uint32_t *__restrict__ hist, uint32_t *__restrict__ out) {
    __shared__ uint32_t wh[4][256];
    const uint32_t blk = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (uint32_t i = tid; i < 4 * 256; i += 256) (&wh[0][0])[i] = 0;
    __syncthreads();
    const uint64_t wbase = uint64_t(blk) * KM_ORDER_CHUNK + uint64_t(wave) * 1024;
    uint32_t item[16], digit[16];
#pragma unroll
    for (int st = 0; st < 16; st++) {
        const uint64_t i = wbase + st * 64 + lane;
        item[st] = 0, digit[st] = 0;
        if (i < m) {
            item[st] = km_item<FIRST>(in, i);
            digit[st] = (assign[km_row_of(ids, item[st])] >> shift) & 255u;
            atomicAdd(&wh[wave][digit[st]], 1u);
        }
    }
    __syncthreads();
    {  // counts -> running bases
        uint32_t run = hist[uint64_t(tid) * nblk + blk];
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const uint32_t cnt = wh[w][tid];
            wh[w][tid] = run;
            run += cnt;
        }
    }
    __syncthreads();
    const uint64_t lt = (1ull << lane) - 1;
#pragma unroll
    for (int st = 0; st < 16; st++) {
        const bool valid = wbase + st * 64 + lane < m;
        const uint32_t d = digit[st];
        uint64_t same = __ballot(valid);  // the lanes of this step with the same digit
#pragma unroll
        for (int bit = 0; bit < 8; bit++) {
            const bool one = (d >> bit) & 1u;
            const uint64_t bm = __ballot(one);
            same &= one ? bm : ~bm;
        }
        const uint32_t rank = (uint32_t)__builtin_popcountll(same & lt), cnt = (uint32_t)__builtin_popcountll(same);
        uint32_t slot = 0;
        if (valid) slot = wh[wave][d] + rank;
        __builtin_amdgcn_wave_barrier();
        if (valid && rank + 1 == cnt) wh[wave][d] += cnt;  // one lane per digit moves the base on
        __builtin_amdgcn_wave_barrier();
        if (valid) out[slot] = item[st];
    }
}

// ---- the centroid update ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_kmeans_update(const float *__restrict__ X, const uint32_t *__restrict__ ids, uint32_t dim,
                                                        const uint32_t *__restrict__ offsets, const uint32_t *__restrict__ members,
                                                        float *__restrict__ C) {
    __shared__ double part[KM_SEGMENTS][64];
    const uint32_t cid = blockIdx.x, lane = threadIdx.x & 63, seg = threadIdx.x >> 6;
    const uint32_t col = blockIdx.y * 64 + lane;
    const uint32_t first = offsets[cid], count = offsets[cid + 1] - first;
    if (count == 0) return;  // (workgroup-uniform) a cluster without members keeps its centroid
    uint32_t s0, len;
    kmeans_segment(count, seg, s0, len);
    const uint32_t *mem = members + first + s0;
    const bool live = col < dim;
    double acc = 0.0;
    uint32_t i = 0;
    for (; i + 4 <= len; i += 4) {  // the sum is a chain, the loads are not
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; q++) v[q] = live ? X[km_row_of(ids, mem[i + q]) * dim + col] : 0.0f;
#pragma unroll
        for (int q = 0; q < 4; q++) acc += double(v[q]);
    }
    for (; i < len; i++) acc += live ? double(X[km_row_of(ids, mem[i]) * dim + col]) : 0.0;
    part[seg][lane] = acc;
    __syncthreads();
    if (seg == 0 && live) {
        double total = 0.0;
#pragma unroll
        for (uint32_t s = 0; s < KM_SEGMENTS; s++) total += part[s][lane];
        C[uint64_t(cid) * dim + col] = float(total / double(count));
    }
}

// ---- changed rows and inertia -------------------------------------------------------------------------------------------------------------
// a fixed tree: thread t of workgroup b adds positions b * 4096 + t, + 256, .. in that order, then the 256 sums halve in LDS
__device__ __forceinline__ double km_block_sum(double v, double *s) {
    const uint32_t tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (uint32_t w = 128; w > 0; w >>= 1) {
        if (tid < w) s[tid] += s[tid + w];
        __syncthreads();
    }
    return s[0];
}
__global__ __launch_bounds__(256) void k_kmeans_reduce_part(const uint32_t *__restrict__ assign, const uint32_t *__restrict__ prev,
                                                            const float *__restrict__ best, const uint32_t *__restrict__ ids, uint64_t m,
                                                            double *__restrict__ partial, unsigned long long *__restrict__ changed) {
    __shared__ double s[256];
    const uint64_t base = uint64_t(blockIdx.x) * KM_REDUCE_CHUNK;
    double v = 0.0;
    uint32_t ch = 0;
    for (uint32_t i = threadIdx.x; i < KM_REDUCE_CHUNK; i += 256) {
        if (base + i >= m) break;
        const uint64_t row = km_row_of(ids, base + i);
        v += double(best[row]);
        ch += assign[row] != prev[row];
    }
    const double total = km_block_sum(v, s);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
    const uint32_t wave_ch = (uint32_t)__builtin_popcountll(__ballot(ch & 1)) + 2 * (uint32_t)__builtin_popcountll(__ballot(ch & 2)) +
                             4 * (uint32_t)__builtin_popcountll(__ballot(ch & 4)) + 8 * (uint32_t)__builtin_popcountll(__ballot(ch & 8)) +
                             16 * (uint32_t)__builtin_popcountll(__ballot(ch & 16));
    if ((threadIdx.x & 63) == 0 && wave_ch) atomicAdd(changed, (unsigned long long)wave_ch);
}
__global__ __launch_bounds__(256) void k_kmeans_reduce_final(const double *__restrict__ partial, uint32_t nblk, double *__restrict__ inertia) {
    __shared__ double s[256];
    double v = 0.0;
    for (uint32_t i = threadIdx.x; i < nblk; i += 256) v += partial[i];
    const double total = km_block_sum(v, s);
    if (threadIdx.x == 0) *inertia = total;
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------------
void launch_kmeans_prep(const float *C, uint32_t c, uint32_t dim, uint4 *planes, float *csq, uint32_t *cmax_bits, hipStream_t s) {
    const uint32_t KB = (dim + KM_KBLOCK - 1) / KM_KBLOCK, tiles = (c + KM_CENT_TILE - 1) / KM_CENT_TILE;
    const uint64_t total = uint64_t(tiles) * KB * 256;
    hipLaunchKernelGGL(k_kmeans_prep, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, C, c, dim, KB, total, planes);
    hipLaunchKernelGGL(k_kmeans_cnorm, dim3((tiles * KM_CENT_TILE + 255) / 256), dim3(256), 0, s, C, c, tiles * KM_CENT_TILE, dim, csq, cmax_bits);
}
void launch_kmeans_assign(const float *X, const float *xsq, const uint32_t *ids, uint64_t m, uint32_t dim, uint32_t c, const uint4 *planes,
                          const float *csq, const uint32_t *cmax_bits, bool cosine, uint32_t *assign, float *best, uint32_t *unsure,
                          uint64_t *unsure_n, hipStream_t s) {
    if (m == 0) return;
    KmAssignArgs a;
    a.X = X, a.xsq = xsq, a.ids = ids, a.m = m, a.dim = dim, a.KB = (dim + KM_KBLOCK - 1) / KM_KBLOCK, a.c = c;
    a.n_ctiles = (c + KM_CENT_TILE - 1) / KM_CENT_TILE;
    a.planes = planes, a.csq = csq, a.cmax_bits = cmax_bits, a.cosine = cosine ? 1 : 0;
    a.assign = assign, a.best = best, a.unsure = unsure, a.unsure_n = reinterpret_cast<unsigned long long *>(unsure_n);
    const dim3 grid((unsigned)((m + KM_ROW_TILE - 1) / KM_ROW_TILE));
    if (dim % 4 == 0)
        hipLaunchKernelGGL(k_kmeans_assign<true>, grid, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(k_kmeans_assign<false>, grid, dim3(256), 0, s, a);
}
void launch_kmeans_resolve(const float *X, const float *xsq, const uint32_t *ids, uint64_t m, uint32_t dim, const float *C, const float *csq,
                           uint32_t c, bool cosine, const uint32_t *unsure, const uint64_t *unsure_n, uint32_t *assign, float *best, int num_cu,
                           hipStream_t s) {
    if (m == 0) return;
    const unsigned grid = (unsigned)std::min<uint64_t>(m, uint64_t(num_cu) * 16);
    const size_t lds = size_t(dim + 3) / 4 * 4 * sizeof(float);
    const unsigned long long *un = reinterpret_cast<const unsigned long long *>(unsure_n);
    if (dim % 4 == 0)
        hipLaunchKernelGGL(k_kmeans_resolve<true>, dim3(grid), dim3(64), lds, s, X, xsq, ids, dim, C, csq, c, cosine ? 1 : 0, unsure, un, assign, best);
    else
        hipLaunchKernelGGL(k_kmeans_resolve<false>, dim3(grid), dim3(64), lds, s, X, xsq, ids, dim, C, csq, c, cosine ? 1 : 0, unsure, un, assign, best);
}
void launch_kmeans_best(const float *X, const float *xsq, const uint32_t *ids, uint64_t m, uint32_t dim, const float *C, const float *csq,
                        uint32_t c, bool cosine, const uint32_t *assign, float *best, hipStream_t s) {
    if (m == 0) return;
    hipLaunchKernelGGL(k_kmeans_best, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, s, X, xsq, ids, m, dim, C, csq, c, cosine ? 1 : 0, assign, best);
}
void launch_kmeans_order(const uint32_t *assign, const uint32_t *ids, uint64_t m, uint32_t c, uint32_t *count, uint32_t *offsets, uint64_t *sizes,
                         uint32_t *hist, uint32_t *tmp, uint32_t *members, hipStream_t s) {
    if (m == 0) return;
    hipLaunchKernelGGL(k_kmeans_count, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, assign, ids, m, c, count);
    hipLaunchKernelGGL(k_kmeans_scan, dim3(1), dim3(1024), 0, s, count, c, offsets, sizes);
    const uint32_t nblk = (uint32_t)((m + KM_ORDER_CHUNK - 1) / KM_ORDER_CHUNK);
    const bool two = c > 256;
    uint32_t *out0 = two ? tmp : members;
    hipLaunchKernelGGL(k_kmeans_order_hist<true>, dim3(nblk), dim3(256), 0, s, (const uint32_t *)nullptr, assign, ids, m, nblk, 0u, hist);
    hipLaunchKernelGGL(k_kmeans_order_scan, dim3(1), dim3(256), 0, s, hist, nblk);
    hipLaunchKernelGGL(k_kmeans_order_scatter<true>, dim3(nblk), dim3(256), 0, s, (const uint32_t *)nullptr, assign, ids, m, nblk, 0u, hist, out0);
    if (two) {
        hipLaunchKernelGGL(k_kmeans_order_hist<false>, dim3(nblk), dim3(256), 0, s, tmp, assign, ids, m, nblk, 8u, hist);
        hipLaunchKernelGGL(k_kmeans_order_scan, dim3(1), dim3(256), 0, s, hist, nblk);
        hipLaunchKernelGGL(k_kmeans_order_scatter<false>, dim3(nblk), dim3(256), 0, s, tmp, assign, ids, m, nblk, 8u, hist, members);
    }
}
void launch_kmeans_update(const float *X, const uint32_t *ids, uint32_t dim, uint32_t c, const uint32_t *offsets, const uint32_t *members, float *C,
                          hipStream_t s) {
    hipLaunchKernelGGL(k_kmeans_update, dim3(c, (dim + 63) / 64), dim3(1024), 0, s, X, ids, dim, offsets, members, C);
}
void launch_kmeans_reduce(const uint32_t *assign, const uint32_t *prev, const float *best, const uint32_t *ids, uint64_t m, double *partial,
                          uint64_t *changed, double *inertia, hipStream_t s) {
    const uint32_t nblk = (uint32_t)((m + KM_REDUCE_CHUNK - 1) / KM_REDUCE_CHUNK);
    hipLaunchKernelGGL(k_kmeans_reduce_part, dim3(nblk), dim3(256), 0, s, assign, prev, best, ids, m, partial,
                       reinterpret_cast<unsigned long long *>(changed));
    hipLaunchKernelGGL(k_kmeans_reduce_final, dim3(1), dim3(256), 0, s, partial, nblk, inertia);
}

}  // namespace vdb
