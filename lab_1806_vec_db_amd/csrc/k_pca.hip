// k_pca.hip -- the kernels of the PCA of an f32 index's rows (flat_pca.hip drives them, pca_plan.hpp lays them out; docs/DESIGN_flat.md
// 4.1ai): the column means, the covariance matrix and the projection onto a set of components, all in f64 on the matrix pipe
// (v_mfma_f64_16x16x4_f64).
//
// THE RULE (include/vdbhip.h states it in full): mean[j] = the f64 sum of double(x[j]) over the allowed rows / m, taken in 1024 row
// segments; cov[i][j] = sum of (double(x[i]) - mean[i]) (double(x[j]) - mean[j]) / (m - center), taken in R row segments, four rows per
// matrix instruction in ascending order, the segments added in ascending order; out[r][c] = f32(sum over j ascending of
// (double(x_r[j]) - mean[j]) double(W[c][j])).  An f32 widens to f64 exactly and the pipe multiplies and adds in f64, so only the
// summation order rounds, and that order is fixed by (m, dim).  No float atomics.
//
// k_pca_colsum      a workgroup per (64-column slab, 4 mean segments): wave w folds segment 4 g + w, a lane one column, rows in
//                   ascending order, 256 coalesced bytes per row; four loads in flight, added in order.  Partials [1024][dim_pad] f64.
// k_pca_mean        a thread per column adds the 1024 partials in segment order and divides by m.
// k_pca_syrk        the hot kernel.  The dim x dim matrix is cut into 64 x 64 blocks and only those with bi <= bj are launched, times R
//                   row segments (grid.y).  A workgroup of 4 waves stages a slice of 16 rows of the block's two column panels through LDS:
//                   thread t owns column t % 64 and rows t / 64 + 4 i of both panels, reads them as f32 (coalesced, 64-bit row offsets,
//                   through the mask's id list when there is one), subtracts its column's mean and widens ONCE on the way into LDS.  A
//                   panel slice is [16 rows][80 doubles]: the fragment of an MFMA k-step is one double per lane, column lane % 16 of row
//                   lane / 16, and with 80 doubles between rows the two rows a half-wave reads lie 128 B apart modulo 256 B -- 64 distinct
//                   banks.  A and B fragments have the same shape because A = X^T: a lane's A element is X[row k][panel A column i], its B
//                   element X[row k][panel B column j].  Wave w owns rows 16 w .. 16 w + 15 of the block: one A fragment and four B
//                   fragments per k-step, four 16 x 16 accumulators = 16 f64 registers per lane.  Two LDS buffers: the global loads of
//                   slice s + 1 are issued before the 16 MFMAs of slice s and land in the other buffer after them, one barrier per slice.
//                   A diagonal block stages one panel and multiplies it with itself; it is computed whole (a wave that skipped its tiles
//                   below the diagonal cost 200 registers instead of 78), and the reduction reads its upper triangle only.  Rows past the
//                   segment's end and columns past dim are staged as +0.0, which adds nothing to an f64 sum.  The partial block goes to
//                   scratch [R][blocks][64][64].
// k_pca_cov_reduce  a thread per element of an upper block adds the R partials in ascending order, divides by m - center and writes
//                   cov[i][j] and cov[j][i] from the same register.
// k_pca_project     a workgroup per 64 vectors x 64 components, a wave per 16 vectors x 64 components; the k dimension of the MFMA is the
//                   vector dimension j, staged 16 at a time: thread t owns dimension t % 16 of vectors t / 16 + 16 i (rows centred and
//                   widened, W widened), panels [64 vectors][17 doubles] so that both the staging stores and the fragment reads
//                   (vector lane % 16, dimension lane / 16) are conflict-free.  Same double buffering; one rounding to f32; a lane
//                   group of 16 stores 16 consecutive floats of an output row.
#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace vdb {

typedef double pca_f64x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t PCA_COV_PANEL = PCA_SLICE * PCA_COV_STRIDE;    // doubles of a staged covariance panel slice
constexpr uint32_t PCA_PROJ_PANEL = PCA_BLOCK * PCA_PROJ_STRIDE;  // doubles of a staged projection panel slice

// One staged slice: 4 k-steps of v_mfma_f64_16x16x4_f64 for wave `wave`'s 16 A vectors against the four B tiles of 16.  Element
// (vector v, depth d) of a panel sits at v * SV + d * SD doubles.  Operand layout of the instruction: A[i][k] and B[k][j] in lane i + 16 k /
// j + 16 k; D[i][j] in word i / 4 of lane j + 16 (i % 4), so word r of a lane is row 4 r + lane / 16, column lane % 16.
template <uint32_t SV, uint32_t SD>
__device__ __forceinline__ void pca_mma_slice(const double *pa, const double *pb, uint32_t wave, uint32_t lane, pca_f64x4 (&acc)[4]) {
    const uint32_t v = lane & 15, k = lane >> 4;
#pragma unroll
    for (uint32_t kk = 0; kk < PCA_SLICE / 4; kk++) {
        const uint32_t d = 4 * kk + k;
        const double a = pa[(16 * wave + v) * SV + d * SD];
#pragma unroll
        for (uint32_t t = 0; t < 4; t++) {
            const double b = pb[(16 * t + v) * SV + d * SD];
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
        }
    }
}

// block `blk` of the row-major walk over the blocks with bi <= bj of a b x b grid
__device__ __forceinline__ void pca_block_of(uint32_t blk, uint32_t b, uint32_t &bi, uint32_t &bj) {
    bi = 0;
    while (blk >= b - bi) {
        blk -= b - bi;
        bi++;
    }
    bj = bi + blk;
}

__global__ __launch_bounds__(256) void k_pca_colsum(const float *__restrict__ X, const uint32_t *__restrict__ ids, uint64_t m, uint32_t dim,
                                                    uint32_t dim_pad, uint64_t per, double *__restrict__ partial) {
    const uint32_t col = blockIdx.x * PCA_BLOCK + (threadIdx.x & 63);
    const uint64_t seg = blockIdx.y * 4 + (threadIdx.x >> 6);
    const uint64_t first = min(m, seg * per), end = min(m, first + per);
    double acc = 0.0;
    if (col < dim) {
        uint64_t p = first;
        for (; p + 4 <= end; p += 4) {
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; i++) v[i] = X[uint64_t(ids ? ids[p + i] : p + i) * dim + col];
#pragma unroll
            for (int i = 0; i < 4; i++) acc += double(v[i]);
        }
        for (; p < end; p++) acc += double(X[uint64_t(ids ? ids[p] : p) * dim + col]);
    }
    partial[seg * dim_pad + col] = acc;
}

__global__ __launch_bounds__(64) void k_pca_mean(const double *__restrict__ partial, uint32_t dim_pad, uint64_t m, double *__restrict__ mean) {
    const uint32_t col = blockIdx.x * 64 + threadIdx.x;
    double acc = 0.0;
    for (uint32_t s = 0; s < PCA_MEAN_SEGMENTS; s++) acc += partial[uint64_t(s) * dim_pad + col];
    mean[col] = acc / double(m);
}

struct PcaSyrkArgs {
    const float *X;
    const uint32_t *ids;  // nullptr: position = row
    const double *mean;   // [dim_pad]
    uint64_t m, seg_rows;
    uint32_t dim, block_cols, blocks;
    double *partial;  // [R][blocks][64][64]
};

// the raw f32 of slice `pos0 ..` a thread owns: rows r0 + 4 i of column `col_a` / `col_b`; bit i of `ok`: the row lies inside the segment
__device__ __forceinline__ void pca_cov_load(const PcaSyrkArgs &a, uint64_t pos0, uint64_t end, uint32_t r0, uint32_t col_a, bool ok_a, uint32_t col_b,
                                             bool ok_b, float (&va)[4], float (&vb)[4], uint32_t &ok) {
    ok = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) {
        const uint64_t pos = pos0 + r0 + 4 * i;
        va[i] = vb[i] = 0.f;
        if (pos < end) {
            ok |= 1u << i;
            const float *row = a.X + uint64_t(a.ids ? a.ids[pos] : pos) * a.dim;
            if (ok_a) va[i] = row[col_a];
            if (ok_b) vb[i] = row[col_b];
        }
    }
}
// centred, widened, into the panels of one buffer
__device__ __forceinline__ void pca_cov_store(double *pa, double *pb, uint32_t r0, uint32_t c, bool ok_a, double mean_a, bool ok_b, bool two, double mean_b,
                                              const float (&va)[4], const float (&vb)[4], uint32_t ok) {
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) {
        const bool in = (ok >> i) & 1;
        const uint32_t at = (r0 + 4 * i) * PCA_COV_STRIDE + c;
        pa[at] = in && ok_a ? double(va[i]) - mean_a : 0.0;
        if (two) pb[at] = in && ok_b ? double(vb[i]) - mean_b : 0.0;
    }
}

__global__ __launch_bounds__(256) void k_pca_syrk(PcaSyrkArgs a) {
    __shared__ double sm[2][2][PCA_COV_PANEL];  // [buffer][panel]
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = tid & 63, r0 = tid >> 6;
    uint32_t bi, bj;
    pca_block_of(blockIdx.x, a.block_cols, bi, bj);
    const bool diag = bi == bj;
    const uint64_t first = min(a.m, blockIdx.y * a.seg_rows), end = min(a.m, first + a.seg_rows);
    const uint32_t n_slices = (uint32_t)((end - first + PCA_SLICE - 1) / PCA_SLICE);
    const uint32_t col_a = bi * PCA_BLOCK + c, col_b = bj * PCA_BLOCK + c;
    const bool ok_a = col_a < a.dim, ok_b = !diag && col_b < a.dim;
    const double mean_a = ok_a ? a.mean[col_a] : 0.0, mean_b = ok_b ? a.mean[col_b] : 0.0;
    pca_f64x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; t++) acc[t] = pca_f64x4{0.0, 0.0, 0.0, 0.0};
    float va[4], vb[4];
    uint32_t ok;
    pca_cov_load(a, first, end, r0, col_a, ok_a, col_b, ok_b, va, vb, ok);
    pca_cov_store(sm[0][0], sm[0][1], r0, c, ok_a, mean_a, ok_b, !diag, mean_b, va, vb, ok);
    __syncthreads();
    for (uint32_t s = 0; s < n_slices; s++) {
        const uint32_t cur = s & 1;
        const bool more = s + 1 < n_slices;
        if (more) pca_cov_load(a, first + uint64_t(s + 1) * PCA_SLICE, end, r0, col_a, ok_a, col_b, ok_b, va, vb, ok);
        pca_mma_slice<1, PCA_COV_STRIDE>(sm[cur][0], sm[cur][diag ? 0 : 1], wave, lane, acc);
        if (more) pca_cov_store(sm[cur ^ 1][0], sm[cur ^ 1][1], r0, c, ok_a, mean_a, ok_b, !diag, mean_b, va, vb, ok);
        __syncthreads();
    }
    double *out = a.partial + (uint64_t(blockIdx.y) * a.blocks + blockIdx.x) * (PCA_BLOCK * PCA_BLOCK);
#pragma unroll
    for (uint32_t t = 0; t < 4; t++)
#pragma unroll
        for (uint32_t r = 0; r < 4; r++) out[(16 * wave + 4 * r + (lane >> 4)) * PCA_BLOCK + 16 * t + (lane & 15)] = acc[t][r];
}

__global__ __launch_bounds__(256) void k_pca_cov_reduce(const double *__restrict__ partial, uint32_t segments, uint32_t blocks, uint32_t block_cols,
                                                        uint32_t dim, double denom, double *__restrict__ cov) {
    uint32_t bi, bj;
    pca_block_of(blockIdx.x, block_cols, bi, bj);
    const uint32_t e = blockIdx.y * 256 + threadIdx.x;
    const uint32_t gi = bi * PCA_BLOCK + e / PCA_BLOCK, gj = bj * PCA_BLOCK + e % PCA_BLOCK;
    if (gi >= dim || gj >= dim || gi > gj) return;
    double acc = 0.0;
    for (uint32_t s = 0; s < segments; s++) acc += partial[(uint64_t(s) * blocks + blockIdx.x) * (PCA_BLOCK * PCA_BLOCK) + e];
    const double v = acc / denom;
    cov[uint64_t(gi) * dim + gj] = v;
    cov[uint64_t(gj) * dim + gi] = v;
}

struct PcaProjArgs {
    const float *X;       // rows of `dim` floats
    const uint32_t *ids;  // nullptr: position = row
    const float *W;       // [n_comp][dim]
    const double *mean;   // [dim] or nullptr: zeros
    uint64_t n;           // positions
    uint32_t dim, n_comp;
    float *out;  // [n][n_comp]
};

__global__ __launch_bounds__(256) void k_pca_project(PcaProjArgs a) {
    __shared__ double sm[2][2][PCA_PROJ_PANEL];  // [buffer][rows | components]
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, d = tid & 15, v0 = tid >> 4;
    const uint64_t pos0 = uint64_t(blockIdx.x) * PCA_BLOCK;
    const uint32_t comp0 = blockIdx.y * PCA_BLOCK;
    const float *xrow[4], *wrow[4];  // nullptr: past the end, staged as zeros
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) {
        const uint64_t pos = pos0 + v0 + 16 * i;
        const uint32_t comp = comp0 + v0 + 16 * i;
        xrow[i] = pos < a.n ? a.X + uint64_t(a.ids ? a.ids[pos] : pos) * a.dim : nullptr;
        wrow[i] = comp < a.n_comp ? a.W + uint64_t(comp) * a.dim : nullptr;
    }
    const uint32_t n_slices = (a.dim + PCA_SLICE - 1) / PCA_SLICE;
    pca_f64x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; t++) acc[t] = pca_f64x4{0.0, 0.0, 0.0, 0.0};
    float vx[4], vw[4];
    double mj;
    bool in;
    auto load = [&](uint32_t s) {
        const uint32_t j = s * PCA_SLICE + d;
        in = j < a.dim;
        mj = in && a.mean ? a.mean[j] : 0.0;
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) {
            vx[i] = in && xrow[i] ? xrow[i][j] : 0.f;
            vw[i] = in && wrow[i] ? wrow[i][j] : 0.f;
        }
    };
    auto store = [&](uint32_t buf) {
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) {
            const uint32_t at = (v0 + 16 * i) * PCA_PROJ_STRIDE + d;
            sm[buf][0][at] = in && xrow[i] ? double(vx[i]) - mj : 0.0;
            sm[buf][1][at] = double(vw[i]);
        }
    };
    load(0);
    store(0);
    __syncthreads();
    for (uint32_t s = 0; s < n_slices; s++) {
        const uint32_t cur = s & 1;
        const bool more = s + 1 < n_slices;
        if (more) load(s + 1);
        pca_mma_slice<PCA_PROJ_STRIDE, 1>(sm[cur][0], sm[cur][1], wave, lane, acc);
        if (more) store(cur ^ 1);
        __syncthreads();
    }
#pragma unroll
    for (uint32_t t = 0; t < 4; t++) {
        const uint32_t comp = comp0 + 16 * t + (lane & 15);
#pragma unroll
        for (uint32_t r = 0; r < 4; r++) {
            const uint64_t pos = pos0 + 16 * wave + 4 * r + (lane >> 4);
            if (pos < a.n && comp < a.n_comp) a.out[pos * a.n_comp + comp] = float(acc[t][r]);
        }
    }
}

void launch_pca_mean(const float *X, const uint32_t *ids, uint64_t m, uint32_t dim, const PcaPlan &p, double *partial, double *mean, hipStream_t s) {
    hipLaunchKernelGGL(k_pca_colsum, dim3((unsigned)p.block_cols, PCA_MEAN_SEGMENTS / 4), dim3(256), 0, s, X, ids, m, dim, (uint32_t)p.dim_pad,
                       p.mean_rows, partial);
    hipLaunchKernelGGL(k_pca_mean, dim3((unsigned)p.block_cols), dim3(64), 0, s, partial, (uint32_t)p.dim_pad, m, mean);
}
void launch_pca_syrk(const float *X, const uint32_t *ids, uint64_t m, uint32_t dim, const PcaPlan &p, const double *mean, double *partial,
                     hipStream_t s) {
    PcaSyrkArgs a{X, ids, mean, m, p.seg_rows, dim, (uint32_t)p.block_cols, (uint32_t)p.blocks, partial};
    hipLaunchKernelGGL(k_pca_syrk, dim3((unsigned)p.blocks, (unsigned)p.segments), dim3(256), 0, s, a);
}
void launch_pca_cov_reduce(const double *partial, uint32_t dim, const PcaPlan &p, double denom, double *cov, hipStream_t s) {
    hipLaunchKernelGGL(k_pca_cov_reduce, dim3((unsigned)p.blocks, PCA_BLOCK * PCA_BLOCK / 256), dim3(256), 0, s, partial, (uint32_t)p.segments,
                       (uint32_t)p.blocks, (uint32_t)p.block_cols, dim, denom, cov);
}
void launch_pca_project(const float *X, const uint32_t *ids, uint64_t n, uint32_t dim, const float *W, uint32_t n_comp, const double *mean, float *out,
                        hipStream_t s) {
    PcaProjArgs a{X, ids, W, mean, n, dim, n_comp, out};
    const uint64_t row_blocks = (n + PCA_BLOCK - 1) / PCA_BLOCK;
    hipLaunchKernelGGL(k_pca_project, dim3((unsigned)row_blocks, (n_comp + PCA_BLOCK - 1) / PCA_BLOCK), dim3(256), 0, s, a);
}

}  // namespace vdb
