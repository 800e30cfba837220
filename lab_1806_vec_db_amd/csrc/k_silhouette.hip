// k_silhouette.hip -- the kernels of the silhouette scoring of a labelled f32 index (flat_silhouette.hip drives them, silhouette_plan.hpp
// lays them out; docs/DESIGN_flat.md 4.1aj): every pairwise distance among the scored rows in f64 on the matrix pipe
// (v_mfma_f64_16x16x4_f64), reduced on the fly to the two numbers a row's score needs.  Neither the m x m distance matrix nor an m x C
// matrix of cluster sums is ever stored.
//
// THE RULE (include/vdbhip.h states it in full): d(i, j) from the f64 Gram entry and the f64 norms; a(i) the mean of d over the other
// scored rows of i's cluster, b(i) the least mean of d over another cluster, s = (b - a) / max(a, b).  An f32 widens to f64 exactly and
// the pipe multiplies and adds in f64, so only summation rounds, and its order is fixed by the cluster sizes and dim.  No float atomics.
//
// k_sil_prepare   a wave per candidate row (the mask's, or every row): lane l squares elements l, l + 64, .. in f64 (exact products),
//                 adds them in ascending order, a fixed lane butterfly adds the 64 partial sums; a ballot says whether every element
//                 is finite.  key[p] = the row's code, or LABEL_NONE when the row is not usable; nrm[p] = |x|^2 (Cosine: |x|).
// k_sil_gather    a thread per ordered slot: the slot's row and norm (-1 for a padded slot) through the order the host made.
// k_sil_fill      NaN to every row's output; the scored rows are overwritten by k_sil_finish.
// k_sil_pairs     the hot kernel.  A workgroup of 4 waves owns a block of 64 ordered rows and walks ALL column tiles of 64 ordered rows
//                 in order.  Per tile pair it accumulates the 64 x 64 Gram block over the dimension in slices of 16: thread t owns
//                 dimension t % 16 of rows t / 16 + 16 i of both panels, reads them as f32 through the slot's row id (64-bit row
//                 offsets, 64 contiguous bytes per row and slice) and widens ONCE on the way into LDS.  A panel slice is [64 rows][18
//                 doubles]: the fragment of an MFMA k-step is one double per lane, row lane % 16 at depth lane / 16, and with 18 doubles
//                 between rows the 32 lanes of two depths read 32 distinct 8-byte bank pairs.  Wave w owns rows 16 w .. 16 w + 15 of
//                 the block: one A fragment and four B fragments per k-step, four 16 x 16 accumulators = 16 f64 registers per lane.
//                 Two LDS buffers; the walk over (tile, slice) is ONE pipeline: the global loads of the next step -- the next slice,
//                 or slice 0 of the next tile -- are issued before the 16 MFMAs of this one and land in the other buffer after them,
//                 one barrier per step; the row ids of the next tile are fetched a tile ahead.  After a tile's last slice the fused
//                 epilogue turns the block into distances with the norms, drops padded columns and the pair (i, i) by POSITION, adds a
//                 lane's four columns in ascending order and the 16 lanes of a row by a fixed butterfly, and adds the row's partial to
//                 the running sum of the tile's cluster.  On the cluster's last tile the sum becomes a's numerator (own cluster) or its
//                 mean enters the running minimum b.  Padded rows are staged as +0.0.
// k_sil_finish    a thread per ordered slot: s from a, b and the cluster size, f32 to out_s[row], f64 to the slot's place for the mean.
// k_sil_mean      one workgroup: thread t adds the s of mean segment t in ascending slot order, a fixed tree adds the 256 segments.
#include "common.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace vdb {

typedef double sil_f64x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t SIL_PANEL = SIL_TILE * SIL_STRIDE;  // doubles of a staged panel slice

template <uint32_t J>
__device__ __forceinline__ double sil_xor(double v, uint32_t lane) {
    return __longlong_as_double((long long)lane_xor64<J>((uint64_t)__double_as_longlong(v), lane));
}

__global__ __launch_bounds__(256) void k_sil_prepare(const float *__restrict__ X, const uint32_t *__restrict__ ids, const uint32_t *__restrict__ col,
                                                     uint64_t cand, uint32_t dim, int cosine, uint32_t *__restrict__ key, double *__restrict__ nrm) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t p = uint64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (p >= cand) return;  // (wave-uniform: the butterfly below runs with every lane active)
    const uint64_t row = ids ? ids[p] : p;
    const float *x = X + row * dim;
    double acc = 0.0;
    bool finite = true;
    for (uint32_t j = lane; j < dim; j += 64) {
        const float v = x[j];
        finite = finite && (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u;
        acc += double(v) * double(v);
    }
    acc += sil_xor<32>(acc, lane);
    acc += sil_xor<16>(acc, lane);
    acc += sil_xor<8>(acc, lane);
    acc += sil_xor<4>(acc, lane);
    acc += sil_xor<2>(acc, lane);
    acc += sil_xor<1>(acc, lane);
    const bool usable = __ballot(!finite) == 0 && (!cosine || acc > 0.0);
    if (lane == 0) {
        key[p] = usable ? col[row] : LABEL_NONE;
        nrm[p] = cosine ? sqrt(acc) : acc;
    }
}

__global__ __launch_bounds__(256) void k_sil_gather(const uint32_t *__restrict__ ord, const uint32_t *__restrict__ ids, const double *__restrict__ nrm,
                                                    uint64_t padded, uint32_t *__restrict__ orow, double *__restrict__ onorm) {
    const uint64_t slot = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (slot >= padded) return;
    const uint32_t p = ord[slot];
    const bool pad = p == LABEL_NONE;
    orow[slot] = pad ? LABEL_NONE : ids ? ids[p] : p;
    onorm[slot] = pad ? -1.0 : nrm[p];
}

__global__ __launch_bounds__(256) void k_sil_fill(float *__restrict__ out, uint64_t n) {
    const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) out[i] = __uint_as_float(0x7fc00000u);
}

struct SilPairArgs {
    const float *X;
    const uint32_t *orow;     // [padded] row of an ordered slot, LABEL_NONE: padding
    const double *onorm;      // [padded] |x|^2 (Cosine: |x|), -1: padding
    const uint32_t *tile_cl;  // [tiles] the cluster a tile belongs to
    const uint32_t *cl_size;  // [clusters]
    uint32_t tiles, dim, n_slices;
    double *sum_a;  // [padded] the sum of d over the other rows of the slot's own cluster
    double *min_b;  // [padded] the least mean of d over another cluster
};

enum { SIL_L2SQR = 0, SIL_ROOT = 1, SIL_COSINE = 2 };

template <int MODE>
__global__ __launch_bounds__(256) void k_sil_pairs(SilPairArgs a) {
    __shared__ double sm[2][2][SIL_PANEL];  // [buffer][row block | column tile]
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, d = tid & 15, v0 = tid >> 4;
    const uint32_t rb = blockIdx.x;
    const uint64_t slot0 = uint64_t(rb) * SIL_TILE;
    // staging: the rows this thread reads, nullptr for a padded slot (staged as zeros)
    const float *arow[4], *brow[4];
    uint32_t bnext[4];
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) {
        const uint32_t r = a.orow[slot0 + v0 + 16 * i];
        arow[i] = r == LABEL_NONE ? nullptr : a.X + uint64_t(r) * a.dim;
        bnext[i] = a.orow[v0 + 16 * i];
        brow[i] = nullptr;
    }
    // epilogue: word r of an accumulator is row 16 wave + 4 r + lane / 16 of the block, column lane % 16 of the accumulator's 16
    const uint32_t cj = lane & 15, ri = lane >> 4;
    const uint32_t own = a.tile_cl[rb];
    double nrow[4], cur[4], sa[4], mb[4];
#pragma unroll
    for (uint32_t r = 0; r < 4; r++) {
        nrow[r] = a.onorm[slot0 + 16 * wave + 4 * r + ri];
        cur[r] = sa[r] = 0.0;
        mb[r] = __longlong_as_double(0x7ff0000000000000ll);
    }
    sil_f64x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; t++) acc[t] = sil_f64x4{0.0, 0.0, 0.0, 0.0};
    float va[4], vb[4];
    auto load = [&](uint32_t ct, uint32_t s) {
        if (s == 0) {  // a new column tile: its rows were fetched a tile ago, the next tile's are fetched now
#pragma unroll
            for (uint32_t i = 0; i < 4; i++) {
                brow[i] = bnext[i] == LABEL_NONE ? nullptr : a.X + uint64_t(bnext[i]) * a.dim;
                if (ct + 1 < a.tiles) bnext[i] = a.orow[uint64_t(ct + 1) * SIL_TILE + v0 + 16 * i];
            }
        }
        const uint32_t j = s * SIL_SLICE + d;
        const bool in = j < a.dim;
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) {
            va[i] = in && arow[i] ? arow[i][j] : 0.f;
            vb[i] = in && brow[i] ? brow[i][j] : 0.f;
        }
    };
    auto store = [&](uint32_t buf) {
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) {
            const uint32_t at = (v0 + 16 * i) * SIL_STRIDE + d;
            sm[buf][0][at] = double(va[i]);
            sm[buf][1][at] = double(vb[i]);
        }
    };
    // Operand layout of v_mfma_f64_16x16x4_f64: A[i][k] and B[k][j] in lane i + 16 k / j + 16 k; D[i][j] in word i / 4 of lane j + 16 (i % 4)
    auto mma = [&](uint32_t buf) {
        const double *pa = sm[buf][0], *pb = sm[buf][1];
#pragma unroll
        for (uint32_t kk = 0; kk < SIL_SLICE / 4; kk++) {
            const uint32_t dd = 4 * kk + ri;
            const double fa = pa[(16 * wave + cj) * SIL_STRIDE + dd];
#pragma unroll
            for (uint32_t t = 0; t < 4; t++) {
                const double fb = pb[(16 * t + cj) * SIL_STRIDE + dd];
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa, fb, acc[t], 0, 0, 0);
            }
        }
    };
    auto epilogue = [&](uint32_t ct) {
        const uint64_t col0 = uint64_t(ct) * SIL_TILE;
        double ncol[4];
#pragma unroll
        for (uint32_t t = 0; t < 4; t++) ncol[t] = a.onorm[col0 + 16 * t + cj];
#pragma unroll
        for (uint32_t r = 0; r < 4; r++) {
            const uint32_t i = 16 * wave + 4 * r + ri;
            double sum = 0.0;
#pragma unroll
            for (uint32_t t = 0; t < 4; t++) {
                const double g = acc[t][r];
                double dist = MODE == SIL_COSINE ? 1.0 - g / (nrow[r] * ncol[t]) : (nrow[r] + ncol[t]) - 2.0 * g;
                dist = dist > 0.0 ? dist : 0.0;
                if (MODE == SIL_ROOT) dist = sqrt(dist);
                const bool keep = ncol[t] >= 0.0 && !(ct == rb && 16 * t + cj == i);
                sum += keep ? dist : 0.0;
            }
            sum += sil_xor<1>(sum, lane);
            sum += sil_xor<2>(sum, lane);
            sum += sil_xor<4>(sum, lane);
            sum += sil_xor<8>(sum, lane);
            cur[r] += sum;
        }
        const uint32_t c = a.tile_cl[ct];
        if (ct + 1 == a.tiles || a.tile_cl[ct + 1] != c) {  // (uniform) the cluster's last tile
            const double size = double(a.cl_size[c]);
#pragma unroll
            for (uint32_t r = 0; r < 4; r++) {
                if (c == own) {
                    sa[r] = cur[r];
                } else {
                    const double mean = cur[r] / size;
                    mb[r] = mean < mb[r] ? mean : mb[r];
                }
                cur[r] = 0.0;
            }
        }
#pragma unroll
        for (int t = 0; t < 4; t++) acc[t] = sil_f64x4{0.0, 0.0, 0.0, 0.0};
    };
    const uint64_t steps = uint64_t(a.tiles) * a.n_slices;
    load(0, 0);
    store(0);
    __syncthreads();
    uint32_t ct = 0, s = 0;
    for (uint64_t g = 0; g < steps; g++) {
        const uint32_t buf = uint32_t(g & 1);
        const bool last = s + 1 == a.n_slices, more = g + 1 < steps;
        const uint32_t ct1 = last ? ct + 1 : ct, s1 = last ? 0 : s + 1;
        if (more) load(ct1, s1);
        mma(buf);
        if (more) store(buf ^ 1);
        if (last) epilogue(ct);
        __syncthreads();
        ct = ct1;
        s = s1;
    }
    if (cj == 0) {
#pragma unroll
        for (uint32_t r = 0; r < 4; r++) {
            const uint64_t slot = slot0 + 16 * wave + 4 * r + ri;
            a.sum_a[slot] = sa[r];
            a.min_b[slot] = mb[r];
        }
    }
}

__global__ __launch_bounds__(256) void k_sil_finish(const uint32_t *__restrict__ orow, const uint32_t *__restrict__ tile_cl,
                                                    const uint32_t *__restrict__ cl_size, const double *__restrict__ sum_a,
                                                    const double *__restrict__ min_b, uint64_t padded, float *__restrict__ out_s,
                                                    double *__restrict__ s64) {
    const uint64_t slot = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (slot >= padded) return;
    const uint32_t row = orow[slot];
    double s = 0.0;
    if (row != LABEL_NONE) {
        const uint32_t size = cl_size[tile_cl[slot / SIL_TILE]];
        if (size > 1) {
            const double av = sum_a[slot] / double(size - 1), bv = min_b[slot];
            const double mx = av > bv ? av : bv;
            if (mx > 0.0) s = (bv - av) / mx;
        }
        out_s[row] = float(s);
    }
    s64[slot] = s;  // (a padded slot adds +0.0 to the mean's sum)
}

__global__ __launch_bounds__(SIL_MEAN_SEGMENTS) void k_sil_mean(const double *__restrict__ s64, uint64_t padded, uint64_t per, uint64_t m,
                                                                double *__restrict__ out_mean) {
    __shared__ double part[SIL_MEAN_SEGMENTS];
    const uint32_t t = threadIdx.x;
    const uint64_t first = min(padded, t * per), end = min(padded, first + per);
    double acc = 0.0;
    for (uint64_t i = first; i < end; i++) acc += s64[i];
    part[t] = acc;
    __syncthreads();
    for (uint32_t w = SIL_MEAN_SEGMENTS / 2; w > 0; w >>= 1) {
        if (t < w) part[t] += part[t + w];
        __syncthreads();
    }
    if (t == 0) *out_mean = part[0] / double(m);
}

void launch_sil_prepare(const float *X, const uint32_t *ids, const uint32_t *col, uint64_t cand, uint32_t dim, bool cosine, uint32_t *key, double *nrm,
                        hipStream_t s) {
    hipLaunchKernelGGL(k_sil_prepare, dim3((unsigned)((cand + 3) / 4)), dim3(256), 0, s, X, ids, col, cand, dim, cosine ? 1 : 0, key, nrm);
}
void launch_sil_gather(const uint32_t *ord, const uint32_t *ids, const double *nrm, uint64_t padded, uint32_t *orow, double *onorm, float *out_s,
                       uint64_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_sil_gather, dim3((unsigned)((padded + 255) / 256)), dim3(256), 0, s, ord, ids, nrm, padded, orow, onorm);
    hipLaunchKernelGGL(k_sil_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, out_s, n);
}
void launch_sil_pairs(const float *X, uint32_t dim, bool cosine, bool root, const SilPlan &p, const uint32_t *orow, const double *onorm,
                      const uint32_t *tile_cl, const uint32_t *cl_size, double *sum_a, double *min_b, hipStream_t s) {
    SilPairArgs a{X, orow, onorm, tile_cl, cl_size, (uint32_t)p.tiles, dim, (uint32_t)p.slices, sum_a, min_b};
    const dim3 grid((unsigned)p.tiles), block(256);
    if (cosine)
        hipLaunchKernelGGL(k_sil_pairs<SIL_COSINE>, grid, block, 0, s, a);
    else if (root)
        hipLaunchKernelGGL(k_sil_pairs<SIL_ROOT>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(k_sil_pairs<SIL_L2SQR>, grid, block, 0, s, a);
}
void launch_sil_finish(const SilPlan &p, const uint32_t *orow, const uint32_t *tile_cl, const uint32_t *cl_size, const double *sum_a,
                       const double *min_b, float *out_s, double *s64, double *out_mean, hipStream_t s) {
    hipLaunchKernelGGL(k_sil_finish, dim3((unsigned)((p.padded + 255) / 256)), dim3(256), 0, s, orow, tile_cl, cl_size, sum_a, min_b, p.padded, out_s,
                       s64);
    hipLaunchKernelGGL(k_sil_mean, dim3(1), dim3(SIL_MEAN_SEGMENTS), 0, s, s64, p.padded, p.mean_slots, p.m, out_mean);
}

}  // namespace vdb
