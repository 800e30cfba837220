// k_gemm_u8.hip -- the Flat shortlist pass of a VecSet<u8> index on the STORED bytes: 128 queries per HBM pass over the row-major
// table at 1 B/element, no mirror (docs/DESIGN_flat.md 4.1af).
//
// Operands.  v_mfma_i32_16x16x64_i8 sums over k, so any assignment of a row's bytes to the 64 k slots of a k-block is valid as long
// as the query image uses the same one.  The one used here gives lane l of a 16-row tile the 16 CONTIGUOUS bytes
//     row 16 tile + (l & 15),  columns 64 kb + 16 (l >> 4) .. + 15
// i.e. one 16-B global load per lane and k-block straight out of d_rows; the four lanes of a row cover 64 contiguous bytes, and the
// two k-blocks of a 128-B line are loaded back to back.  x' = x XOR 0x80 per byte is x - 128 as int8: one v_xor_b32 per dword between
// the load and the MFMA.  The query image holds q' = q - 128 in the same order ([group][kb][half][lane] 16 int8, zero where a
// k-block runs past dim -- the row side then needs no masking there), and stays resident in LDS for the group's pass (128 x dim
// bytes).  A wave owns units of U8_TW tiles with its U8_TW x 8 accumulator tiles in registers; nothing in the unit loop is shared
// between waves, so each runs on its own counted waits.
//
// Keys.  I = sum x'q' is exact in i32, so with the row constants {sum x'^2, sum x'} (k_u8_row_consts) and the query's
// {sum q'^2, sum q'} (k_u8_query_prep)
//     D_int   = sum x'^2 + sum q'^2 - 2 I                        = sum (x - q)^2, exactly
//     dot_int = I + 128 sum x' + 128 sum q' + 16384 dim          = sum x q, exactly
// The reference folds the widened elements in f32 (distance/mod.rs:79-95): every term is an integer below 2^16, so the fold is exact
// while the total is below 2^24 (the terms are non-negative, so no partial sum is larger) -- always for dim <= 258 -- and loses or
// gains at most 2 per step once a partial sum has passed 2^24 (sums stay below 2^26: ulp 4, dim <= 1024; the first 258 steps cannot
// get there).  With E = 0 for a total below 2^24, else 2 (dim - 258) + 2 (the + 2: the int -> f32 conversion of a value in
// [2^25, 2^26)):
//     L2Sqr   key = f32(D_int - E)  <= the reference's distance, and EQUAL to it for D_int < 2^24
//     Cosine  key = 1 - f32(dot_int + E) / max(sqrt(qsq) sqrt(xsq), 1e-10) with the STORED f32 norms: the reference's own epilogue on an
//             upper bound of its folded dot product; division and subtraction are monotone under round-to-nearest, so the key is
//             <= the reference's distance with no further term, and equal to it for dot_int < 2^24.
// Keys are certified lower bounds, never estimates.  Rows at and past n get +inf and are never appended.
#include <algorithm>

#include "common.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace vdb {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t U8_NH = 8;           // 16-query halves per group
constexpr uint32_t U8_BQ = 16 * U8_NH;  // 128 queries per pass (= gemm_group())
constexpr int U8_TW = 3;                // 16-row tiles per unit
constexpr uint32_t U8_UNIT = 16 * U8_TW;
constexpr uint32_t U8_WGBUF = 2048;     // LDS hit buffer entries per workgroup and group (what does not fit is appended directly)
constexpr uint32_t U8_NT = 512, U8_NW = 8;

bool flat_u8_supported(uint32_t dim) { return dim >= 16 && dim % 16 == 0 && dim <= 1024; }
int32_t flat_u8_fold_slack(uint32_t dim) { return dim <= 258 ? 0 : int32_t(2 * (dim - 258) + 2); }

// ---- row constants: {sum x'^2, sum x'} per row, 16 lanes per row, one 16-B load per lane and 256 columns ---------------------------
__global__ __launch_bounds__(256) void k_u8_row_consts(const uint8_t *__restrict__ X, uint64_t r0, uint64_t r1, uint32_t dim, int2 *__restrict__ out) {
    const uint64_t row = r0 + (uint64_t(blockIdx.x) * 256 + threadIdx.x) / 16;
    const uint32_t sub = threadIdx.x & 15;
    int s2 = 0, s1 = 0;
    if (row < r1)
        for (uint32_t c = sub * 16; c < dim; c += 256) {
            const uint4 v = *reinterpret_cast<const uint4 *>(X + row * dim + c);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const int x = int((w[a] >> (8 * b)) & 0xff) - 128;
                    s2 += x * x;
                    s1 += x;
                }
        }
#pragma unroll
    for (int d = 8; d > 0; d >>= 1) {
        s2 += __shfl_xor(s2, d);
        s1 += __shfl_xor(s1, d);
    }
    if (row < r1 && sub == 0) out[row] = make_int2(s2, s1);
}
void launch_u8_row_consts(const uint8_t *X, uint64_t r0, uint64_t r1, uint32_t dim, void *rowc, hipStream_t s) {
    if (r1 <= r0) return;
    hipLaunchKernelGGL(k_u8_row_consts, dim3((unsigned)((r1 - r0 + 15) / 16)), dim3(256), 0, s, X, r0, r1, dim, static_cast<int2 *>(rowc));
}

// ---- query side: the int8 image in fragment order, {sum q'^2, sum q'}, the eligible flag, the zeroed hit counter; a wave per query ----
// eligible: every element an integer in [0, 255] (NaN, fractions and anything out of range fail the test).  Padding queries
// (q >= nq) get a zero image and are not eligible.
__global__ __launch_bounds__(64) void k_u8_query_prep(const float *__restrict__ Q, uint32_t nq, uint32_t dim, uint32_t KB, uint4 *__restrict__ img,
                                                      int2 *__restrict__ qc, uint32_t *__restrict__ elig, uint32_t *__restrict__ hits) {
    const uint32_t q = blockIdx.x, grp = q / U8_BQ, half = (q % U8_BQ) / 16, r = q & 15;
    int s2 = 0, s1 = 0;
    bool ok = q < nq;
    for (uint32_t c = threadIdx.x; c < KB * 4; c += 64) {  // c: 16-column piece = (k-block c / 4, lane quarter c % 4)
        uint32_t w[4] = {0, 0, 0, 0};
        for (uint32_t j = 0; j < 16; j++) {
            const uint32_t col = c * 16 + j;
            if (col >= dim || q >= nq) continue;
            const float v = Q[uint64_t(q) * dim + col];
            const bool e = v >= 0.0f && v <= 255.0f && v == floorf(v);
            ok = ok && e;
            const int x = e ? int(v) - 128 : 0;
            s2 += x * x;
            s1 += x;
            w[j >> 2] |= uint32_t(x & 0xff) << (8 * (j & 3));
        }
        img[(uint64_t(grp * KB + c / 4) * U8_NH + half) * 64 + (c & 3) * 16 + r] = make_uint4(w[0], w[1], w[2], w[3]);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        s2 += __shfl_xor(s2, d);
        s1 += __shfl_xor(s1, d);
    }
    const bool all_ok = __ballot(!ok) == 0;
    if (threadIdx.x == 0) {
        qc[q] = make_int2(s2, s1);
        elig[q] = all_ok ? 1u : 0u;
        hits[q] = 0;
    }
}
void launch_u8_query_prep(const float *Q, uint32_t nq, uint32_t nq_pad, uint32_t dim, void *img, void *qc, uint32_t *elig, uint32_t *hits,
                          hipStream_t s) {
    if (nq_pad == 0) return;
    hipLaunchKernelGGL(k_u8_query_prep, dim3(nq_pad), dim3(64), 0, s, Q, nq, dim, (dim + 63) / 64, static_cast<uint4 *>(img), static_cast<int2 *>(qc),
                       elig, hits);
}

// tau[q] = -inf for a query that is not eligible: it collects no hits and is reported as not certified (k_u8_finish)
__global__ void k_u8_tau_close(float *__restrict__ tau, const uint32_t *__restrict__ elig, uint32_t nq_pad) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < nq_pad && !elig[q]) tau[q] = -INFINITY;
}
void launch_u8_tau_close(float *tau, const uint32_t *elig, uint32_t nq_pad, hipStream_t s) {
    if (nq_pad == 0) return;
    hipLaunchKernelGGL(k_u8_tau_close, dim3((nq_pad + 255) / 256), dim3(256), 0, s, tau, elig, nq_pad);
}

// ---- the corpus pass --------------------------------------------------------------------------------------------------------------
struct U8Args {
    const uint8_t *X;  // row-major u8 rows, 16-B aligned rows (dim % 16 == 0)
    uint64_t n;
    uint32_t dim, KB, n_units, ngroups;
    uint32_t unit_step;  // U8_SAMPLE: every unit_step-th unit is scored (n_units counts the sampled ones); else 1
    const uint4 *img;    // [group][kb][half][lane]
    const int2 *qc;      // [ngroups * 128] {sum q'^2, sum q'}
    const int2 *rowc;    // [n] {sum x'^2, sum x'}
    const float *xsq, *qsq;  // Cosine: the stored strict-fold norms (d_sq, the call's qsq)
    int32_t slack;       // E(dim)
    float *out;          // U8_SAMPLE: dense keys out[q * ld + v * 48 + row in unit] (+inf past n)
    uint64_t ld;
    const float *tau;    // [ngroups * 128]
    uint64_t *cand;      // [ngroups * 128][cap]
    uint32_t *cnt;       // [ngroups * 128]
    uint32_t cap;
};
enum { U8_FILTER = 0, U8_SAMPLE = 1 };

static size_t flat_u8_lds(uint32_t KB) {
    return size_t(KB) * U8_NH * 64 * sizeof(uint4) + U8_WGBUF * (sizeof(uint64_t) + sizeof(uint32_t)) + (5 * U8_BQ + 4) * sizeof(uint32_t);
}

template <int MODE, bool COS>
__global__ __launch_bounds__(512, 1) void k_flat_u8(U8Args a) {
    constexpr int TW = U8_TW, NH = U8_NH;
    extern __shared__ __attribute__((aligned(16))) uint4 smem_u8[];  // the group's image [KB][8][64], then the hit buffer and the per-query words
    const uint32_t KB = a.KB;
    uint64_t *hit_key = reinterpret_cast<uint64_t *>(smem_u8 + size_t(KB) * NH * 64);
    uint32_t *hit_q = reinterpret_cast<uint32_t *>(hit_key + U8_WGBUF);
    uint32_t *lcnt = hit_q + U8_WGBUF;                          // [128] hits of the query in the buffer
    uint32_t *lbase = lcnt + U8_BQ;                             // [128] their first slot in the query's candidate list
    float *tau_s = reinterpret_cast<float *>(lbase + U8_BQ);    // [128]
    int *qa_s = reinterpret_cast<int *>(tau_s + U8_BQ);         // [128] L2Sqr: sum q'^2;  Cosine: 128 sum q' + 16384 dim
    float *qn_s = reinterpret_cast<float *>(qa_s + U8_BQ);      // [128] Cosine: sqrt(qsq)
    uint32_t *hit_n = reinterpret_cast<uint32_t *>(qn_s + U8_BQ);

    const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t r = lane & 15, g4 = lane >> 4;
    const uint32_t nwaves = gridDim.x * U8_NW, gw = blockIdx.x * U8_NW + wave;
    const uint64_t n = a.n;
    const uint32_t dim = a.dim, KP = (KB + 1) / 2;

    for (uint32_t grp = 0; grp < a.ngroups; grp++) {
        __syncthreads();  // the previous group's hand-over has read the buffer and the image
        for (uint32_t i = threadIdx.x; i < KB * NH * 64; i += U8_NT) smem_u8[i] = a.img[uint64_t(grp) * KB * NH * 64 + i];
        if (threadIdx.x < U8_BQ) {
            const uint32_t gq = grp * U8_BQ + threadIdx.x;
            const int2 c = a.qc[gq];
            lcnt[threadIdx.x] = 0;
            tau_s[threadIdx.x] = MODE == U8_FILTER ? a.tau[gq] : 0.0f;
            qa_s[threadIdx.x] = COS ? 128 * c.y + 16384 * int(dim) : c.x;
            qn_s[threadIdx.x] = COS ? sqrtf(a.qsq[gq]) : 0.0f;
        }
        if (threadIdx.x == 0) hit_n[0] = 0;
        __syncthreads();

        for (uint32_t v = gw; v < a.n_units; v += nwaves) {
            const uint64_t row0 = uint64_t(v) * a.unit_step * U8_UNIT;
            // this lane's share of a k-block of tile t: 16 bytes at row (row0 + 16 t + r), column 64 kb + 16 g4; nothing is read for a
            // row at or past n or a column at or past dim (d_rows has 16 bytes of slack, not a tile's worth)
            const uint8_t *xp[TW];
            bool xok[TW];
#pragma unroll
            for (int t = 0; t < TW; t++) {
                const uint64_t row = row0 + 16 * t + r;
                xok[t] = row < n;
                xp[t] = a.X + (xok[t] ? row : 0) * dim + 16 * g4;
            }
            auto load_pair = [&](uint32_t kp, i32x4 (&x)[2][TW]) {  // the two k-blocks of a 128-B line back to back
#pragma unroll
                for (int t = 0; t < TW; t++)
#pragma unroll
                    for (int b = 0; b < 2; b++) {
                        const uint32_t col = 64 * (2 * kp + b) + 16 * g4;
                        i32x4 w = {0, 0, 0, 0};
                        if (xok[t] && col < dim) w = *reinterpret_cast<const i32x4 *>(xp[t] + 64 * (2 * kp + b));
                        x[b][t] = w ^ int(0x80808080u);  // u8 -> int8 of x - 128
                    }
            };
            i32x4 acc[TW][NH];
#pragma unroll
            for (int t = 0; t < TW; t++)
#pragma unroll
                for (int h = 0; h < NH; h++) acc[t][h] = i32x4{0, 0, 0, 0};
            i32x4 cur[2][TW], nxt[2][TW];
            load_pair(0, cur);
            for (uint32_t kp = 0; kp < KP; kp++) {
                if (kp + 1 < KP) load_pair(kp + 1, nxt);
#pragma unroll
                for (int b = 0; b < 2; b++) {
                    const uint32_t kb = 2 * kp + b;
                    if (kb < KB) {  // (uniform)
#pragma unroll
                        for (int h = 0; h < NH; h++) {
                            const uint4 qu = smem_u8[(kb * NH + h) * 64 + lane];
                            const i32x4 qv = {int(qu.x), int(qu.y), int(qu.z), int(qu.w)};
#pragma unroll
                            for (int t = 0; t < TW; t++) acc[t][h] = __builtin_amdgcn_mfma_i32_16x16x64_i8(cur[b][t], qv, acc[t][h], 0, 0, 0);
                        }
                    }
                }
#pragma unroll
                for (int b = 0; b < 2; b++)
#pragma unroll
                    for (int t = 0; t < TW; t++) cur[b][t] = nxt[b][t];
            }
            // ---- epilogue: the lane holds rows 4 g4 .. 4 g4 + 3 of every tile for query r of every half; scalar-form integer / f32 VALU ----
#pragma unroll
            for (int t = 0; t < TW; t++) {
                const uint64_t rb = row0 + 16 * t + 4 * g4;
                int ra[4];      // L2Sqr: sum x'^2;  Cosine: 128 sum x'
                float rn[4];    // Cosine: sqrt(xsq)
                bool rok[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    rok[j] = rb + j < n;
                    const int2 c = rok[j] ? a.rowc[rb + j] : make_int2(0, 0);
                    ra[j] = COS ? 128 * c.y : c.x;
                    rn[j] = COS && rok[j] ? sqrtf(a.xsq[rb + j]) : 0.0f;
                }
#pragma unroll
                for (int h = 0; h < NH; h++) {
                    const int qa = qa_s[h * 16 + r];
                    float key[4];
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        float kf;
                        // (a sum below 2^24 is folded exactly whatever dim is -- its terms are non-negative integers, so every
                        // partial sum is one too: the slack applies only from 2^24 on)
                        if (COS) {
                            const int dv = acc[t][h][j] + ra[j] + qa;
                            const float den = fmaxf(qn_s[h * 16 + r] * rn[j], 1e-10f);
                            const float q = float(dv >= (1 << 24) ? dv + a.slack : dv) / den;
                            kf = 1.0f - q;
                        } else {
                            const int dv = ra[j] + qa - 2 * acc[t][h][j];
                            kf = float(dv >= (1 << 24) ? dv - a.slack : dv);
                        }
                        key[j] = rok[j] ? kf : INFINITY;
                    }
                    if (MODE == U8_SAMPLE) {
                        *reinterpret_cast<float4 *>(a.out + (uint64_t(grp) * U8_BQ + h * 16 + r) * a.ld + uint64_t(v) * U8_UNIT + 16 * t + 4 * g4) =
                            make_float4(key[0], key[1], key[2], key[3]);
                        continue;
                    }
                    const float tau_h = tau_s[h * 16 + r];
                    const uint32_t gq = grp * U8_BQ + h * 16 + r;
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const bool pass = rok[j] && key[j] <= tau_h;
                        const uint64_t pm = __ballot(pass);
                        if (pm == 0) continue;  // (uniform)
                        // ballot + ONE integer atomic: the first lane reserves the wave's slots in the workgroup's buffer
                        uint32_t base = 0;
                        if (lane == 0) base = atomicAdd(hit_n, (uint32_t)__builtin_popcountll(pm));
                        base = __builtin_amdgcn_readfirstlane(base);
                        if (pass) {
                            const uint32_t slot = base + __builtin_amdgcn_mbcnt_hi(uint32_t(pm >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(pm), 0u));
                            const uint64_t pk = pair_key(key[j], uint32_t(rb + j));
                            if (slot < U8_WGBUF) {
                                hit_key[slot] = pk;
                                hit_q[slot] = h * 16 + r;
                            } else {  // buffer full: straight into the query's list
                                const uint32_t gs = atomicAdd(&a.cnt[gq], 1u);
                                if (gs < a.cap) a.cand[uint64_t(gq) * a.cap + gs] = pk;
                            }
                        }
                    }
                }
            }
        }
        if (MODE == U8_SAMPLE) continue;
        // ---- group end: the parked hits go to the per-query candidate lists, one global atomic per query ----
        __syncthreads();
        const uint32_t total = hit_n[0] < U8_WGBUF ? hit_n[0] : U8_WGBUF;
        uint32_t rank[U8_WGBUF / U8_NT];
#pragma unroll
        for (uint32_t j = 0; j < U8_WGBUF / U8_NT; j++) {
            const uint32_t i = threadIdx.x + j * U8_NT;
            rank[j] = i < total ? atomicAdd(&lcnt[hit_q[i]], 1u) : 0u;
        }
        __syncthreads();
        if (threadIdx.x < U8_BQ) lbase[threadIdx.x] = lcnt[threadIdx.x] ? atomicAdd(&a.cnt[grp * U8_BQ + threadIdx.x], lcnt[threadIdx.x]) : 0u;
        __syncthreads();
#pragma unroll
        for (uint32_t j = 0; j < U8_WGBUF / U8_NT; j++) {
            const uint32_t i = threadIdx.x + j * U8_NT;
            if (i < total) {
                const uint32_t q = hit_q[i], slot = lbase[q] + rank[j];
                if (slot < a.cap) a.cand[(uint64_t(grp) * U8_BQ + q) * a.cap + slot] = hit_key[i];
            }
        }
    }
}

template <int MODE>
static void flat_u8_launch(const U8Args &a, int num_cu, hipStream_t s) {
    const size_t lds = flat_u8_lds(a.KB);
    const uint32_t grid = std::max<uint32_t>(1, std::min<uint32_t>((uint32_t)num_cu, (a.n_units + U8_NW - 1) / U8_NW));
    auto go = [&](auto kern) {
        func_max_lds(reinterpret_cast<const void *>(kern), (int)lds);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(U8_NT), lds, s, a);
    };
    if (a.xsq)
        go(k_flat_u8<MODE, true>);
    else
        go(k_flat_u8<MODE, false>);
}

static U8Args flat_u8_args(const uint8_t *X, uint64_t n, uint32_t dim, const void *img, const void *qc, uint32_t ngroups, const void *rowc,
                           const float *xsq, const float *qsq, int cosine) {
    VDB_REQUIRE(flat_u8_supported(dim), "flat_u8: dim must be a multiple of 16, at most 1024");
    VDB_REQUIRE(n < (1ull << 32), "flat_u8: too many rows for one shard");
    VDB_REQUIRE(ngroups <= 65535, "flat_u8: too many query groups");
    U8Args a{};
    a.X = X;
    a.n = n;
    a.dim = dim;
    a.KB = (dim + 63) / 64;
    a.ngroups = ngroups;
    a.unit_step = 1;
    a.img = static_cast<const uint4 *>(img);
    a.qc = static_cast<const int2 *>(qc);
    a.rowc = static_cast<const int2 *>(rowc);
    a.xsq = cosine ? xsq : nullptr;
    a.qsq = cosine ? qsq : nullptr;
    a.slack = flat_u8_fold_slack(dim);
    return a;
}

void launch_flat_u8_filter(const uint8_t *X, uint64_t n, uint32_t dim, const void *img, const void *qc, uint32_t ngroups, const void *rowc,
                           const float *xsq, const float *qsq, int cosine, const float *tau, uint64_t *cand, uint32_t *cnt, uint32_t cap,
                           int num_cu, hipStream_t s) {
    if (n == 0 || ngroups == 0) return;
    U8Args a = flat_u8_args(X, n, dim, img, qc, ngroups, rowc, xsq, qsq, cosine);
    a.n_units = (uint32_t)((n + U8_UNIT - 1) / U8_UNIT);
    a.tau = tau;
    a.cand = cand;
    a.cnt = cnt;
    a.cap = cap;
    flat_u8_launch<U8_FILTER>(a, num_cu, s);
}

uint64_t flat_u8_sample_rows(uint64_t n, uint32_t unit_step) {
    const uint64_t units = (n + U8_UNIT - 1) / U8_UNIT;
    return (units + unit_step - 1) / unit_step * U8_UNIT;
}
// dense keys of every unit_step-th unit for every query of every group: out[q * ld + j], j < flat_u8_sample_rows(n, unit_step), +inf past n
void launch_flat_u8_sample(const uint8_t *X, uint64_t n, uint32_t dim, const void *img, const void *qc, uint32_t ngroups, const void *rowc,
                           const float *xsq, const float *qsq, int cosine, uint32_t unit_step, float *out, uint64_t ld, int num_cu, hipStream_t s) {
    if (n == 0 || ngroups == 0) return;
    VDB_REQUIRE(unit_step >= 1 && (ld & 3) == 0 && ld >= flat_u8_sample_rows(n, unit_step), "flat_u8: ld must cover the sample");
    U8Args a = flat_u8_args(X, n, dim, img, qc, ngroups, rowc, xsq, qsq, cosine);
    a.unit_step = unit_step;
    a.n_units = (uint32_t)(flat_u8_sample_rows(n, unit_step) / U8_UNIT);
    a.out = out;
    a.ld = ld;
    flat_u8_launch<U8_SAMPLE>(a, num_cu, s);
}

// ---- finish: certification by the lower-bound rule under the (distance, index) order, overflow check, outputs ---------------------
// ek = the ksel-th smallest EXACT pair of the shortlist, ak = the k'-th smallest KEY pair of the hit list (PAIR_NONE: the list holds
// fewer than k' hits and the shortlist is the whole list).  A row outside the shortlist has (key, row) > ak, or -- not a hit -- key >
// tau; its distance is >= its key, so its (distance, row) pair is above ak, respectively above every pair at tau.  Certified when
// ek <= that bound: nothing outside can precede the k-th answer, ties included.
__global__ __launch_bounds__(64) void k_u8_finish(const uint64_t *__restrict__ exact_sorted, uint32_t lde, const uint64_t *__restrict__ approx_sorted,
                                                  uint32_t lda, uint32_t ksel, uint32_t kstride, uint32_t kprime, const float *__restrict__ tau,
                                                  const uint32_t *__restrict__ elig, const uint32_t *__restrict__ cnt, uint32_t cap,
                                                  uint64_t id_offset, uint8_t *__restrict__ flags, uint64_t *__restrict__ out_idx,
                                                  float *__restrict__ out_dist, uint64_t *__restrict__ out_count) {
    const uint32_t q = blockIdx.x;
    if (threadIdx.x == 0) {
        const uint64_t ek = exact_sorted[uint64_t(q) * lde + (ksel - 1)];
        const uint64_t ak = approx_sorted[uint64_t(q) * lda + (kprime - 1)];
        const uint64_t bound = ak != PAIR_NONE ? ak : pair_key(tau[q], 0xFFFFFFFFu);
        const bool ok = elig[q] && cnt[q] <= cap && ek != PAIR_NONE && ek <= bound;
        flags[q] = ok ? 0 : 1;
    }
    uint32_t c = 0;
    for (uint32_t j = threadIdx.x; j < ksel; j += blockDim.x) {
        const uint64_t e = exact_sorted[uint64_t(q) * lde + j];
        const bool ok = e != PAIR_NONE;
        out_idx[uint64_t(q) * kstride + j] = ok ? uint64_t(uint32_t(e)) + id_offset : 0;
        out_dist[uint64_t(q) * kstride + j] = ok ? f32_from_orderable(uint32_t(e >> 32)) : 0.0f;
        c += ok;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
    if (threadIdx.x == 0 && out_count) out_count[q] = c;
}
void launch_u8_finish(const uint64_t *exact_sorted, uint32_t lde, const uint64_t *approx_sorted, uint32_t lda, uint32_t nq, uint32_t ksel,
                      uint32_t kstride, uint32_t kprime, const float *tau, const uint32_t *elig, const uint32_t *cnt, uint32_t cap,
                      uint64_t id_offset, uint8_t *flags, uint64_t *out_idx, float *out_dist, uint64_t *out_count, hipStream_t s) {
    if (nq == 0) return;
    hipLaunchKernelGGL(k_u8_finish, dim3(nq), dim3(64), 0, s, exact_sorted, lde, approx_sorted, lda, ksel, kstride, kprime, tau, elig, cnt, cap,
                       id_offset, flags, out_idx, out_dist, out_count);
}

}  // namespace vdb
