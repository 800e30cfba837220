// k_mmr.hip -- the greedy selection of the diversified Flat k-NN (Index::flat_knn_mmr_device / Index::mmr_select_device, mmr_plan.hpp;
// docs/DESIGN_flat.md 4.1u): maximal marginal relevance over a query's candidate list.  Position 0 is selected first; every later step
// selects the unselected position p with the smallest score_p = (lambda * d_p) - ((1 - lambda) * m_p), m_p = the smallest distance from
// row p to a row selected so far, ties to the lowest position, a NaN score counting as +inf; min(k, list length) positions are selected
// and come out in selection order.
//
// The row-to-row distance D(p, s) is the reference's: the strict left fold over the dimension, products and sums separately rounded (the
// file is compiled with -ffp-contract=off and the pragma below repeats it) -- the difference form for L2Sqr, the dot form with the
// cached |x|^2 of both rows for Cosine -- so D(p, s) is what the Flat search reports for row s when row p is the query.  Both forms are
// symmetric bit for bit ((a - b)^2 == (b - a)^2, a * b == b * a, |a| * |b| == |b| * |a|), which lets the kernel fold "candidate against
// the selected row" where the definition says "row p against row s".
//
// k_mmr_select: ONE WORKGROUP PER QUERY, a lane per candidate position (64 threads for lists of up to 64 positions, otherwise 256 and a
// lane takes positions tid, tid + 256, ..).  No F x F matrix: a step evaluates only D(p, s_last) for the unselected p and folds it into
// m_p (`if (D < m_p) m_p = D`: a NaN D is ignored), (kk - 1) x F folds at most and O(F) state.  The row selected last is staged in LDS --
// every lane reads the same address, a broadcast -- and A LANE WALKS ITS OWN CANDIDATE ROW in global memory, 8 x 16 B loads in flight
// ahead of the chain of dependent adds (k_row_sqnorm's pattern).  A fold is a chain of `dim` dependent adds whatever feeds it, a
// candidate row is used once per step, and the F rows of a query (40 x 3840 B at the measured shape) stay in L2 between steps: staging
// them through LDS as k_small.hip does would add a write and a read per element and cap F, for loads the chain already hides.  A staged
// row longer than MMR_STAGE_FLOATS goes through in pieces, the partial sums parked in LDS between pieces.  d_p, m_p and the selected
// bytes live in LDS; the argmin under (score, position) is a shuffle reduction per wave and one LDS exchange between waves.  An id that
// is no row of the index is never gathered: its distances read as NaN (mmr_select_device refuses such a list before the launch).
// Outputs of query b go to row slot_q[b] (nullptr: b) of [..][k] arrays: the selected pairs, zeros behind them, and the count.
#include <algorithm>
#include <cmath>

#include "common.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace vdb {

template <bool COS>
__device__ __forceinline__ float mmr_fold1(float acc, float x, float q) {
    if (COS) {
        const float p = x * q;
        return acc + p;
    }
    const float df = x - q;
    const float sq = df * df;
    return acc + sq;
}

template <bool COS>
__device__ __forceinline__ float mmr_fold4(float acc, const float4 v, const float4 w) {
    acc = mmr_fold1<COS>(acc, v.x, w.x);
    acc = mmr_fold1<COS>(acc, v.y, w.y);
    acc = mmr_fold1<COS>(acc, v.z, w.z);
    return mmr_fold1<COS>(acc, v.w, w.w);
}

// acc folded over x[0 .. len) against the staged q[0 .. len), ascending; VEC4: len is a multiple of 4 and both are 16-byte aligned
template <bool COS, bool VEC4>
__device__ __forceinline__ float mmr_fold(float acc, const float *__restrict__ x, const float *q, uint32_t len) {
    if (VEC4) {
        const float4 *x4 = reinterpret_cast<const float4 *>(x);
        const float4 *q4 = reinterpret_cast<const float4 *>(q);
        const uint32_t nv = len / 4;
        uint32_t j = 0;
        for (; j + 8 <= nv; j += 8) {  // the fold is a strict chain, the loads are not
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) v[u] = x4[j + u];
#pragma unroll
            for (int u = 0; u < 8; u++) acc = mmr_fold4<COS>(acc, v[u], q4[j + u]);
        }
        for (; j < nv; j++) acc = mmr_fold4<COS>(acc, x4[j], q4[j]);
    } else {
        for (uint32_t j = 0; j < len; j++) acc = mmr_fold1<COS>(acc, x[j], q[j]);
    }
    return acc;
}

// (score a, position a) comes before (score b, position b): smaller score, ties (-0 == +0, +inf == +inf) to the lower position
__device__ __forceinline__ bool mmr_before(float sa, uint32_t pa, float sb, uint32_t pb) { return sa < sb || (sa == sb && pa < pb); }

template <bool COS, bool VEC4>
__global__ __launch_bounds__(MMR_THREADS) void k_mmr_select(const uint64_t *__restrict__ ids, const float *__restrict__ dists,
                                                            const uint64_t *__restrict__ counts, uint64_t ld, const float *__restrict__ X,
                                                            const float *__restrict__ xsq, uint64_t n, uint32_t dim, uint64_t id_offset, uint32_t k,
                                                            float lambda, const uint32_t *__restrict__ slot_q, uint64_t *__restrict__ out_idx,
                                                            float *__restrict__ out_dist, uint64_t *__restrict__ out_cnt) {
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    const uint32_t tid = threadIdx.x, nt = blockDim.x;
    const uint64_t b = blockIdx.x;
    // the layout of mmr_lds_bytes(ld, dim)
    const uint32_t fp = (uint32_t)((ld + 3) & ~3ull), stage = (dim + 3) & ~3u;
    const uint32_t stage_floats = stage < MMR_STAGE_FLOATS ? stage : MMR_STAGE_FLOATS;
    float *s_d = s_mem, *s_m = s_d + fp, *s_acc = s_m + fp, *s_row = s_acc + fp;
    float *s_best = s_row + stage_floats;
    uint32_t *s_bpos = reinterpret_cast<uint32_t *>(s_best + MMR_MAX_WAVES);
    uint8_t *s_sel = reinterpret_cast<uint8_t *>(s_bpos + MMR_MAX_WAVES);

    const uint32_t F = (uint32_t)(counts[b] < ld ? counts[b] : ld);
    const uint32_t kk = k < F ? k : F;
    const uint64_t *my_ids = ids + b * ld;
    const float *my_d = dists + b * ld;
    const uint64_t o = slot_q ? slot_q[b] : b;
    uint64_t *o_idx = out_idx + o * k;
    float *o_dist = out_dist + o * k;
    const float mu = 1.0f - lambda;

    for (uint32_t p = tid; p < F; p += nt) {
        s_d[p] = my_d[p];
        s_m[p] = INFINITY;
        s_sel[p] = p == 0;
    }
    for (uint32_t i = kk + tid; i < k; i += nt) {
        o_idx[i] = 0;
        o_dist[i] = 0.0f;
    }
    if (tid == 0) {
        out_cnt[o] = kk;
        if (kk) {
            o_idx[0] = my_ids[0];
            o_dist[0] = my_d[0];
        }
    }
    __syncthreads();

    uint32_t last = 0;
    for (uint32_t t = 1; t < kk; t++) {  // (workgroup-uniform, as is everything that decides a barrier below)
        // m_p <- min(m_p, D(p, last)) for every unselected p
        const uint64_t id_s = my_ids[last];
        const uint64_t row_s = id_s - id_offset;
        if (id_s >= id_offset && row_s < n) {
            const float *xs = X + row_s * dim;
            const float ss = COS ? xsq[row_s] : 0.0f;
            for (uint32_t c0 = 0; c0 < dim; c0 += stage_floats) {
                const uint32_t len = dim - c0 < stage_floats ? dim - c0 : stage_floats;
                const bool last_piece = c0 + len == dim;
                if (VEC4) {
                    for (uint32_t i = tid; i < len / 4; i += nt)
                        reinterpret_cast<float4 *>(s_row)[i] = reinterpret_cast<const float4 *>(xs + c0)[i];
                } else {
                    for (uint32_t i = tid; i < len; i += nt) s_row[i] = xs[c0 + i];
                }
                __syncthreads();
                for (uint32_t p = tid; p < F; p += nt) {
                    if (s_sel[p]) continue;
                    const uint64_t id_p = my_ids[p];
                    const uint64_t row_p = id_p - id_offset;
                    if (id_p < id_offset || row_p >= n) continue;  // no row: D reads as NaN
                    float acc = c0 ? s_acc[p] : 0.0f;
                    acc = mmr_fold<COS, VEC4>(acc, X + row_p * dim + c0, s_row, len);
                    if (!last_piece) {
                        s_acc[p] = acc;
                        continue;
                    }
                    float D = acc;
                    if (COS) {  // 1 - dot / max(|a| |b|, 1e-10), the norms from the cached strict-fold |x|^2
                        const float den = fmaxf(sqrtf(ss) * sqrtf(xsq[row_p]), 1e-10f);
                        const float r = acc / den;
                        D = 1.0f - r;
                    }
                    if (D < s_m[p]) s_m[p] = D;
                }
                __syncthreads();  // the piece is read: the next one (or the next step's row) may overwrite it
            }
        }
        // argmin of the score under (score, position); a lane only ever reads the m_p it wrote itself
        float best = INFINITY;
        uint32_t bpos = 0xFFFFFFFFu;
        for (uint32_t p = tid; p < F; p += nt) {
            if (s_sel[p]) continue;
            const float rel = lambda * s_d[p];
            const float div = mu * s_m[p];
            float sc = rel - div;
            if (!(sc == sc)) sc = INFINITY;
            if (mmr_before(sc, p, best, bpos)) {
                best = sc;
                bpos = p;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float os = __shfl_xor(best, off);
            const uint32_t op = (uint32_t)__shfl_xor((int)bpos, off);
            if (mmr_before(os, op, best, bpos)) {
                best = os;
                bpos = op;
            }
        }
        if ((tid & 63) == 0) {
            s_best[tid >> 6] = best;
            s_bpos[tid >> 6] = bpos;
        }
        __syncthreads();
        best = s_best[0];
        bpos = s_bpos[0];
        for (uint32_t w = 1; w < nt / 64; w++)
            if (mmr_before(s_best[w], s_bpos[w], best, bpos)) {
                best = s_best[w];
                bpos = s_bpos[w];
            }
        last = bpos;  // (t < kk <= F: an unselected position exists, and any position comes before the 0xFFFFFFFF of an idle lane)
        if (tid == 0) {
            s_sel[last] = 1;
            o_idx[t] = my_ids[last];
            o_dist[t] = s_d[last];
        }
        __syncthreads();  // the selected byte is out, and the per-wave pairs are read before the next step writes them
    }
}

void launch_mmr_select(const uint64_t *ids, const float *dists, const uint64_t *counts, uint64_t nq, uint64_t ld, const float *X, const float *xsq,
                       uint64_t n, uint32_t dim, bool cosine, uint64_t id_offset, uint32_t k, float lambda, const uint32_t *slot_q, uint64_t *out_idx,
                       float *out_dist, uint64_t *out_cnt, hipStream_t s) {
    if (nq == 0) return;
    VDB_REQUIRE(ld >= 1 && ld <= MMR_MAX_FETCH && nq < (1ull << 31), "mmr select: list length or query count out of range");
    const dim3 grid((unsigned)nq), block(mmr_threads(ld));
    const size_t lds = mmr_lds_bytes(ld, dim);
    const bool vec4 = (dim & 3) == 0;
#define VDB_MMR_LAUNCH(C, V)                                                                                                                 \
    hipLaunchKernelGGL((k_mmr_select<C, V>), grid, block, lds, s, ids, dists, counts, ld, X, xsq, n, dim, id_offset, k, lambda, slot_q, out_idx, \
                       out_dist, out_cnt)
    if (cosine) {
        if (vec4) VDB_MMR_LAUNCH(true, true);
        else VDB_MMR_LAUNCH(true, false);
    } else {
        if (vec4) VDB_MMR_LAUNCH(false, true);
        else VDB_MMR_LAUNCH(false, false);
    }
#undef VDB_MMR_LAUNCH
}

}  // namespace vdb
