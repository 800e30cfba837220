// k_pq.hip -- the product-quantisation kernels for gfx950 and their launchers: lookup-table build, the asymmetric-distance
// (ADC) scans -- f32 tables (k_pq_adc), 4-bit codes on 16-bit tables (k_pq_adc16), 8-bit codes on one-byte and sliced tables
// (k_pq_adc8, k_pq_adc16x8, k_pq_adc8x16) --, the exact sums of their candidates, the reference-order re-sort, the GPU encoder and
// the shard merge.  Reference: src/distance/pq_table.rs, FlatIndex::knn_pq (src/index_algorithm/flat_index.rs:84-104),
// ResultSet::pq_resort (src/index_algorithm/candidate_pair.rs:102-108).  The host state and the search drivers are in pq.hip.
//
// Bit-exactness: an ADC distance is sum_{i<m} lut[i*k + code_i] accumulated from 0.0 in ascending
// group order (pq_table.rs:254-292).  One thread owns one code row and adds in that order, so the sums
// equal the reference's bit for bit; the LUT entries themselves are strict-order folds.
//
// Every launcher (bottom of the file) computes the dynamic LDS bytes of its kernel itself, beside the layout they mirror.
#include <algorithm>
#include <cmath>

#include "common.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace vdb {

// ---------------------------------------------------------------------------------------------------
// create_lookup (pq_table.rs:195-224): lut[q][g*kc + c] = l2(qslice, cent) | dot(qslice, cent)
// ---------------------------------------------------------------------------------------------------
__global__ void k_pq_lut(const float *__restrict__ Q, uint32_t dim, const float *__restrict__ cent,
                         const uint64_t *__restrict__ gstart, uint32_t m, uint32_t kc, int cosine,
                         float *__restrict__ lut) {
    uint32_t q = blockIdx.y;
    uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m * kc) return;
    uint32_t g = e / kc, c = e % kc;
    uint32_t s = (uint32_t)gstart[g], gd = (uint32_t)gstart[g + 1] - s;
    const float *v = Q + uint64_t(q) * dim + s;
    const float *cc = cent + uint64_t(kc) * s + uint64_t(c) * gd;
    float acc = 0.0f;
    if (cosine) {
        for (uint32_t j = 0; j < gd; j++) {
            float p = v[j] * cc[j];
            acc = acc + p;
        }
    } else {
        for (uint32_t j = 0; j < gd; j++) {
            float df = v[j] - cc[j];
            float sq = df * df;
            acc = acc + sq;
        }
    }
    lut[uint64_t(q) * m * kc + e] = acc;
}

// ---------------------------------------------------------------------------------------------------
// ADC scan (pq_table.rs:239-301 applied to every code row, flat_index.rs:98-101).
// BQ queries per pass share each code byte; their lookup tables sit in LDS (m*kc floats each;
// 20 KB for m=320, 4 bit).  16 consecutive floats of one group span 16 distinct banks, so a
// ds_read_b32 gather by code value is conflict-free whatever the codes are.
// LUT_IN_LDS = false: tables too large for LDS (8-bit codes with large m) are read through L1/L2.
// ---------------------------------------------------------------------------------------------------
// MODE 0 (dense): out[b*ld + j] for the visited rows (row blocks of blockDim.x rows, every `blk_step`-th block;
//                 j = dense position among the visited rows; +inf for rows >= n).  blk_step = 1 is the plain scan,
//                 blk_step > 1 the strided sample whose ef-th smallest value per query bounds the global one.
// MODE 1 (filter): all rows; pairs with adc <= tau[b] are parked in an LDS buffer and handed to cand[b][..] when
//                 the workgroup is done (one global atomic per query per workgroup) -- no dense N x B matrix, no
//                 separate top-ef pass over it.  ADC values are exact, so {adc <= tau} is a superset of the exact
//                 top-ef and the select that follows is the reference's (adc, idx) order.
constexpr uint32_t ADC_WGBUF = 2048;  // LDS hit buffer entries per workgroup (MODE 1)

// One code row of the Gist1M-shaped table (4-bit codes, every nibble a group, 16-B code words) against 4 lookup tables
// held entry-major / query-minor in LDS: 8 independent ds_read_b128 per code word half, then the strict-order adds
// (two packed adds per lookup serve the 4 queries).  A separate, non-inlined function: inside k_pq_adc the register
// allocator shares 128 VGPRs with every other path of that kernel and spills the loaded entries to scratch.
template <bool COS>
__device__ __noinline__ float4 adc_row_fast(const uint4 *cw, uint32_t nwords, const char *lbase, const char *cbase,
                                            float &cdp_out) {
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    f32x2_t s01 = {0.0f, 0.0f}, s23 = {0.0f, 0.0f};
    float cdp = 0.0f;
    uint4 v = cw[0];
    for (uint32_t w = 0; w < nwords; w++) {
        const uint32_t words[4] = {v.x, v.y, v.z, v.w};
        if (w + 1 < nwords) v = cw[w + 1];  // next code word while this one is looked up
#pragma unroll
        for (int wi = 0; wi < 4; wi++) {
            float4 t[8];
            float cc[8];
#pragma unroll
            for (int j = 0; j < 8; j++) {  // nibble j of the word = group 32w + 8wi + j (low nibble of a byte first)
                const uint32_t off = (w * 32 + 8 * wi + j) * 256 + (((words[wi] >> (4 * j)) & 0xf) << 4);
                t[j] = *reinterpret_cast<const float4 *>(lbase + off);
                if (COS) cc[j] = *reinterpret_cast<const float *>(cbase + (off >> 2));
            }
#pragma unroll
            for (int j = 0; j < 8; j++) {
                s01 += (f32x2_t){t[j].x, t[j].y};
                s23 += (f32x2_t){t[j].z, t[j].w};
                if (COS) cdp = cdp + cc[j];
            }
        }
    }
    cdp_out = cdp;
    return make_float4(s01.x, s01.y, s23.x, s23.y);
}

template <int BQ, int NBITS, bool LUT_IN_LDS, int MODE>
__global__ __launch_bounds__(1024) void k_pq_adc(AdcArgs a) {
    {   // sub-batch blockIdx.y: BQ consecutive queries of the launch
        const uint32_t q0 = blockIdx.y * BQ;
        a.nq = a.nq_total - q0 < (uint32_t)BQ ? a.nq_total - q0 : (uint32_t)BQ;
        a.lut += uint64_t(q0) * a.m * (1u << NBITS);
        a.qsq += q0;
        if (MODE == 0) {
            a.out += uint64_t(q0) * a.ld;
        } else {
            a.tau += q0;
            a.cand += uint64_t(q0) * a.cap;
            a.cnt += q0;
        }
    }
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr uint32_t KC = 1u << NBITS;
    const uint32_t m = a.m, enc_dim = a.enc_dim;
    const uint64_t n = a.n;
    const int cosine = a.cosine;
    const uint32_t lsz = m * KC;
    const float *lut[BQ];
    const float *ccache = a.cent_cache;
    uint32_t lds_floats = 0;
    if (LUT_IN_LDS) {
        // entry-major, query-minor: the BQ values of one (group, code) entry are adjacent, so one ds_read_b128
        // (BQ = 4) serves all queries of the pass -- half the LDS cycles of four ds_read_b32 gathers.  Distinct
        // codes of a group still land in distinct banks (16 entries x 16 B = all 64 banks).
        for (uint32_t i = threadIdx.x; i < lsz * BQ; i += blockDim.x) {
            uint32_t b = i / lsz, e = i % lsz;
            smem[e * BQ + b] = b < a.nq ? a.lut[i] : 0.0f;
        }
        if (cosine)
            for (uint32_t i = threadIdx.x; i < lsz; i += blockDim.x) smem[lsz * BQ + i] = a.cent_cache[i];
        ccache = smem + lsz * BQ;
        lds_floats = lsz * BQ + (cosine ? lsz : 0);
    } else {
#pragma unroll
        for (int b = 0; b < BQ; b++) lut[b] = a.lut + (b < (int)a.nq ? b : 0) * uint64_t(lsz);
    }
    // hit buffer behind the tables (MODE 1)
    uint64_t *hit_key = reinterpret_cast<uint64_t *>(smem + ((lds_floats + 3) & ~3u));
    uint32_t *hit_q = reinterpret_cast<uint32_t *>(hit_key + ADC_WGBUF);
    uint32_t *hit_n = hit_q + ADC_WGBUF;  // [0] entries, [1..BQ] per-query counts, [1+BQ..2BQ] bases
    if (MODE == 1 && threadIdx.x < 1 + 2 * BQ) hit_n[threadIdx.x] = 0;
    float tau[BQ];
#pragma unroll
    for (int b = 0; b < BQ; b++) tau[b] = (MODE == 1 && b < (int)a.nq) ? a.tau[b] : -INFINITY;
    __syncthreads();

    const uint64_t nblk = (n + blockDim.x - 1) / blockDim.x;
    for (uint64_t vb = blockIdx.x; vb * a.blk_step < nblk; vb += gridDim.x) {
        const uint64_t row = vb * a.blk_step * blockDim.x + threadIdx.x;
        const bool valid = row < n;
        const uint8_t *cr = a.codes + (valid ? row : n - 1) * enc_dim;
        float sum[BQ];
#pragma unroll
        for (int b = 0; b < BQ; b++) sum[b] = 0.0f;
        float cdp = 0.0f;
        auto push = [&](uint32_t i, uint32_t code) {
            if (i >= m) return;  // pq_table.rs:258-260
            uint32_t at = i * KC + code;
            if (LUT_IN_LDS) {
                if (BQ == 4) {
                    const float4 v = *reinterpret_cast<const float4 *>(smem + at * 4);
                    sum[0] = sum[0] + v.x;
                    sum[1 % BQ] = sum[1 % BQ] + v.y;
                    sum[2 % BQ] = sum[2 % BQ] + v.z;
                    sum[3 % BQ] = sum[3 % BQ] + v.w;
                } else if (BQ == 2) {
                    const float2 v = *reinterpret_cast<const float2 *>(smem + at * 2);
                    sum[0] = sum[0] + v.x;
                    sum[1 % BQ] = sum[1 % BQ] + v.y;
                } else {
                    sum[0] = sum[0] + smem[at];
                }
            } else {
#pragma unroll
                for (int b = 0; b < BQ; b++) sum[b] = sum[b] + lut[b][at];
            }
            if (cosine) cdp = cdp + ccache[at];
        };
        if (LUT_IN_LDS && BQ == 4 && NBITS == 4 && a.fast && (enc_dim & 15) == 0 && m == 2 * enc_dim) {
            // Fast path (the Gist1M table: m = 320, 4 bit, 160-B code rows): every nibble is a group, so no bound checks,
            // and the 8 lookups of a code word are issued together -- addresses first, then 8 independent
            // ds_read_b128, then the strict-order adds.  (The generic path below waits for each lookup before it
            // issues the next and branches per nibble: measured 24.6 us per query and 1M rows against an LDS-gather
            // floor of ~8 us.)
            float4 r4;
            if (cosine)
                r4 = adc_row_fast<true>(reinterpret_cast<const uint4 *>(cr), enc_dim / 16, reinterpret_cast<const char *>(smem),
                                        reinterpret_cast<const char *>(ccache), cdp);
            else
                r4 = adc_row_fast<false>(reinterpret_cast<const uint4 *>(cr), enc_dim / 16, reinterpret_cast<const char *>(smem),
                                         nullptr, cdp);
            sum[0] = r4.x;
            sum[1 % BQ] = r4.y;
            sum[2 % BQ] = r4.z;
            sum[3 % BQ] = r4.w;
        } else if ((enc_dim & 15) == 0) {  // 16 code bytes per load
            const uint4 *cw = reinterpret_cast<const uint4 *>(cr);
            for (uint32_t w = 0; w < enc_dim / 16; w++) {
                const uint4 v = cw[w];
                const uint32_t words[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int wi = 0; wi < 4; wi++) {
#pragma unroll
                    for (int byte = 0; byte < 4; byte++) {
                        uint32_t u = (words[wi] >> (8 * byte)) & 0xff;
                        uint32_t bi = w * 16 + wi * 4 + byte;
                        if (NBITS == 4) {
                            push(2 * bi, u & 0xf);  // low nibble = even group (pq_table.rs:274-280)
                            push(2 * bi + 1, u >> 4);
                        } else {
                            push(bi, u);
                        }
                    }
                }
            }
        } else if ((enc_dim & 3) == 0) {
            const uint32_t *cw = reinterpret_cast<const uint32_t *>(cr);
            for (uint32_t w = 0; w < enc_dim / 4; w++) {
                uint32_t word = cw[w];
#pragma unroll
                for (int byte = 0; byte < 4; byte++) {
                    uint32_t u = (word >> (8 * byte)) & 0xff;
                    uint32_t bi = w * 4 + byte;
                    if (NBITS == 4) {
                        push(2 * bi, u & 0xf);
                        push(2 * bi + 1, u >> 4);
                    } else {
                        push(bi, u);
                    }
                }
            }
        } else {
            for (uint32_t bi = 0; bi < enc_dim; bi++) {
                uint32_t u = cr[bi];
                if (NBITS == 4) {
                    push(2 * bi, u & 0xf);
                    push(2 * bi + 1, u >> 4);
                } else {
                    push(bi, u);
                }
            }
        }
#pragma unroll
        for (int b = 0; b < BQ; b++) {
            if (b >= (int)a.nq) break;
            float d = sum[b];
            if (cosine) {  // pq_table.rs:294-299
                float norm0 = sqrtf(cdp);
                float norm1 = sqrtf(a.qsq[b]);
                float den = fmaxf(norm0 * norm1, 1e-10f);
                float r = sum[b] / den;
                d = 1.0f - r;
            }
            if (MODE == 0) {
                a.out[uint64_t(b) * a.ld + vb * blockDim.x + threadIdx.x] = valid ? d : INFINITY;
            } else if (valid && d <= tau[b]) {
                uint32_t pos = atomicAdd(hit_n, 1u);
                if (pos < ADC_WGBUF) {
                    hit_key[pos] = pair_key(d, uint32_t(row));
                    hit_q[pos] = b;
                } else {
                    atomicAdd(&a.cnt[b], a.cap + 1);  // mark the query as overflowed (-> dense path)
                }
            }
        }
    }
    if (MODE == 1) {
        __syncthreads();
        uint32_t total = hit_n[0];
        if (total > ADC_WGBUF) total = ADC_WGBUF;
        // ranks: each thread walks its strided entries (total <= 2048)
        for (uint32_t i = threadIdx.x; i < total; i += blockDim.x) {
            uint32_t r_ = atomicAdd(&hit_n[1 + hit_q[i]], 1u);
            hit_q[i] |= r_ << 8;  // park the rank beside the query id (BQ <= 4, rank < 2048)
        }
        __syncthreads();
        if (threadIdx.x < BQ && hit_n[1 + threadIdx.x] > 0)
            hit_n[1 + BQ + threadIdx.x] = atomicAdd(&a.cnt[threadIdx.x], hit_n[1 + threadIdx.x]);
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < total; i += blockDim.x) {
            uint32_t q = hit_q[i] & 0xff, r_ = hit_q[i] >> 8;
            uint32_t slot = hit_n[1 + BQ + q] + r_;
            if (slot < a.cap) a.cand[uint64_t(q) * a.cap + slot] = hit_key[i];
        }
    }
}


// ---------------------------------------------------------------------------------------------------
// Quantised first pass of the ADC scan (4-bit codes, L2Sqr).
// The f32 scan above is bound by the LDS gather rate: one ds_read_b128 per (row, group) serves 4 queries (8 us per
// query and 1M rows at the LDS array's 256 B/clk/CU; measured 15.5).  The scan only has to find the rows whose ADC
// value is <= tau[q], so it can run on a coarser table as long as it never drops such a row:
//   lut16[q][g][c] = floor((lut[q][g][c] - mn[q][g]) / D[q]),   mn = min_c lut[q][g][.],   D[q] = sum_g range_g / 65000
// 16-bit entries, 8 queries side by side in one 16-B LDS entry -> one ds_read_b128 per (row, group) serves 8 queries,
// and because no 16-bit field can overflow (sum_g max_c lut16 <= 65000) the 8 sums are accumulated with plain 32-bit
// adds, two lookups per v_add3_u32.  For every row  M + D * S16 <= sum_g lut[g][code_g]  (real arithmetic; M = sum mn),
// and the reference's f32 left fold S of m non-negative terms satisfies S >= real * (1 - gamma_{m-1}), so
//   S <= tau   ==>   S16 <= T16 := floor((tau * (1 + 2 m 2^-24) - M (1 - 1e-12)) / D) + 2
// (the +2 and the 1e-12 cover the double-precision evaluation).  Rows with S16 <= T16 go to the candidate list of the
// query as bare row ids; k_pq_adc_exact then computes THEIR f32 ADC sums in group order with the f32 table in LDS and
// keeps those <= tau -- the same set, the same values, the same (adc, idx) order as the f32 scan produces.
// Queries whose table holds a non-finite or negative entry are flagged and take the f32 scan.
// ---------------------------------------------------------------------------------------------------
// Code rows are 160 B apart (m = 320): with one lane per row a 16-B code-word load of a wave touches 64 different
// 128-B lines, and the 1024 rows of a workgroup iteration (160 KB) do not fit the L1, so every line came from L2 up to 8
// times.  The scan therefore reads a word-major mirror of the codes: tile of 64 rows x word w x lane -> one wave load
// = 1 KB contiguous, every line fetched once.  Built once per table (the codes are immutable until the next build).
// Code rows that are not whole 16-B words (odd m, m not a multiple of 32: the DB's default m = ceil(dim / 3) gives 171 groups at
// dim 512, 342 at dim 1024) are padded with zero bytes up to the next word: the padded nibbles select entries of groups beyond
// m, whose tables are all zero in the quantised image (k_pq_quant16), so they add nothing to any sum.
__global__ __launch_bounds__(256) void k_pq_tile_codes(const uint8_t *__restrict__ codes, uint64_t n, uint32_t enc_dim, uint32_t nwords,
                                                       uint4 *__restrict__ tiled) {
    const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;  // output entry: ((tile * nwords) + w) * 64 + lane
    const uint64_t total = (n + 63) / 64 * 64 * nwords;
    if (i >= total) return;
    const uint64_t lane = i & 63, tw = i >> 6, tile = tw / nwords, w = tw - tile * nwords;
    const uint64_t row = tile * 64 + lane;
    uint32_t v[4] = {0u, 0u, 0u, 0u};
    if (row < n) {
        const uint8_t *src = codes + row * enc_dim;
        if ((enc_dim & 15u) == 0) {
            const uint4 x = reinterpret_cast<const uint4 *>(src)[w];
            v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
        } else {
            for (uint32_t b = 0; b < 16; b++) {
                const uint32_t at = uint32_t(w) * 16 + b;
                if (at < enc_dim) v[b >> 2] |= uint32_t(src[at]) << (8 * (b & 3));
            }
        }
    }
    tiled[i] = make_uint4(v[0], v[1], v[2], v[3]);
}

constexpr uint32_t ADC16_WGBUF = 2048;   // LDS hit buffer entries per workgroup

// one workgroup per query: table -> 16-bit image [q / NQ][g][c][q % NQ], offset M and step D.
// L2Sqr (NQ = 8): entries floor((lut - mn_g) / D), D = sum_g range_g / 65000: a LOWER bound of the sum.
// Cosine (NQ = 7): the ADC value is 1 - S / max(sqrt(C) |q|, 1e-10) with S = sum of dot-product entries (any sign) and
// C = sum of |centroid|^2 entries (pq_table.rs:262-299).  Slots 0..6 hold ceil((lut - mn_g) / D), D = sum range / 64000
// -- an UPPER bound of S --, slot 7 of every entry holds floor((cc - mnc_g) / DC): a lower bound of C, the same for all
// queries (written by the block of the group's first query).  A row survives when S_ub >= 0 and
// S_ub^2 >= rho^2 |q|^2 C_lb with rho = 1 - tau (less slack), see k_pq_adc16.
// m_pad = groups of the image (32 per 16-B code word); the entries of groups m .. m_pad - 1 are zero (padded code bytes).
__global__ __launch_bounds__(256) void k_pq_quant16(const float *__restrict__ lut, const float *__restrict__ cent_cache, uint32_t m, uint32_t m_pad,
                                                    uint32_t nq, int cosine, uint16_t *__restrict__ img, double *__restrict__ qM,
                                                    double *__restrict__ qD, double *__restrict__ qMC, double *__restrict__ qDC,
                                                    uint32_t *__restrict__ qflag) {
    const uint32_t q = blockIdx.x, t = threadIdx.x;
    const uint32_t NQ = cosine ? 7u : 8u;
    __shared__ double sR[256], sM[256], sA[256];
    __shared__ uint32_t sbad;
    if (t == 0) sbad = 0;
    __syncthreads();
    auto reduce3 = [&](double &a, double &b, double &c) {
        sR[t] = a;
        sM[t] = b;
        sA[t] = c;
        __syncthreads();
        for (uint32_t s = 128; s > 0; s >>= 1) {
            if (t < s) {
                sR[t] += sR[t + s];
                sM[t] += sM[t + s];
                sA[t] += sA[t + s];
            }
            __syncthreads();
        }
        a = sR[0];
        b = sM[0];
        c = sA[0];
        __syncthreads();
    };
    const float *lq = lut + uint64_t(q) * m * 16;
    double R = 0.0, M = 0.0, A = 0.0;  // sum of ranges, of minima, of the largest magnitudes (rounding slack of a mixed-sign sum)
    bool bad = false;
    for (uint32_t g = t; g < m; g += 256) {
        float mn = INFINITY, mx = -INFINITY, am = 0.0f;
#pragma unroll
        for (int c = 0; c < 16; c++) {
            const float v = lq[g * 16 + c];
            if (cosine ? !(fabsf(v) <= 3.0e38f) : (!(v >= 0.0f) || v > 3.0e38f)) bad = true;  // NaN, inf (L2Sqr: negative)
            mn = fminf(mn, v);
            mx = fmaxf(mx, v);
            am = fmaxf(am, fabsf(v));
        }
        R += double(mx) - double(mn);
        M += double(mn);
        A += double(am);
    }
    if (bad) atomicOr(&sbad, 1u);
    reduce3(R, M, A);
    const bool flag = sbad != 0 || !(R < 1.0e300) || !(fabs(M) < 1.0e300);
    const double D = (!flag && R > 0.0) ? R / (cosine ? 64000.0 : 65000.0) : 1.0;
    uint16_t *dst = img + uint64_t(q / NQ) * m_pad * 16 * 8 + (q % NQ);
    for (uint32_t i = m * 16 + t; i < m_pad * 16; i += 256) dst[i * 8] = 0;
    for (uint32_t g = t; g < m; g += 256) {
        float mn = INFINITY;
#pragma unroll
        for (int c = 0; c < 16; c++) mn = fminf(mn, lq[g * 16 + c]);
#pragma unroll
        for (int c = 0; c < 16; c++) {
            const double y = (double(lq[g * 16 + c]) - double(mn)) / D;
            double x = flag ? 0.0 : (cosine ? ceil(y) : floor(y));
            x = x < 0.0 ? 0.0 : (x > 65000.0 ? 65000.0 : x);  // (unreachable clamps: sum of the maxima <= 64000 + m)
            dst[(g * 16 + c) * 8] = (uint16_t)x;
        }
    }
    double MC = 0.0, DC = 1.0;
    if (cosine) {  // the |centroid|^2 table: the same numbers in every block; the group's first query writes slot 7
        double RC = 0.0, Z = 0.0;
        MC = 0.0;
        for (uint32_t g = t; g < m; g += 256) {
            float mn = INFINITY, mx = -INFINITY;
#pragma unroll
            for (int c = 0; c < 16; c++) {
                const float v = cent_cache[g * 16 + c];
                mn = fminf(mn, v);
                mx = fmaxf(mx, v);
            }
            RC += double(mx) - double(mn);
            MC += double(mn);
        }
        reduce3(RC, MC, Z);
        DC = RC > 0.0 && RC < 1.0e300 ? RC / 65000.0 : 1.0;
        if (q % NQ == 0) {
            uint16_t *dc = img + uint64_t(q / NQ) * m_pad * 16 * 8 + 7;
            for (uint32_t i = m * 16 + t; i < m_pad * 16; i += 256) dc[i * 8] = 0;
            for (uint32_t g = t; g < m; g += 256) {
                float mn = INFINITY;
#pragma unroll
                for (int c = 0; c < 16; c++) mn = fminf(mn, cent_cache[g * 16 + c]);
#pragma unroll
                for (int c = 0; c < 16; c++) {
                    double x = floor((double(cent_cache[g * 16 + c]) - double(mn)) / DC);
                    x = x < 0.0 ? 0.0 : (x > 65000.0 ? 65000.0 : x);
                    dc[(g * 16 + c) * 8] = (uint16_t)x;
                }
            }
        }
    }
    if (t == 0) {
        // Cosine: the f32 left fold of mixed-sign terms errs by at most gamma_m * sum |t_g| <= m 2^-23 * A: part of the upper bound
        qM[q] = cosine ? M + 2.0 * double(m) * 0x1p-24 * A : M;
        qD[q] = D;
        qMC[q] = MC;
        qDC[q] = DC;
        qflag[q] = flag ? 1u : 0u;
    }
}

// NW = 16-B code words per row (enc_dim / 16) as a compile-time constant: the row loop is fully unrolled, every
// group's table offset is an instruction immediate and the address register of a lookup is ONE v_perm_b32 (byte b of
// the packed nibble offsets, plus bit 16 for the groups beyond the 16-bit immediate range).  NW = 0: runtime count,
// one extra add per lookup.  (Shift + mask + base add per lookup made the loop VALU-bound: 154 vector instructions
// per 32 lookups against 128 LDS cycles.)
// Early exit of rows that are out (L2Sqr: the running sums only grow; once all eight are above their thresholds in every lane of
// a wave, the wave's 64 rows cannot qualify).  Exact, but on the bench corpus (1M low-rank gist-like rows, 4-bit m = 320, ef =
// 100) it LOSES: 6.04 instead of 5.45 ms per 1000 queries -- the smallest of a wave's 512 (row, query) sums crosses its
// threshold too late for the skipped lookups to pay for one check per code word.  Measurement switch (make EXTRA=-DADC16_ABANDON=1).
#ifndef ADC16_ABANDON
#define ADC16_ABANDON 0
#endif
// SAMPLE = true (L2Sqr only): the same row sums over a strided block sample, written densely -- the threshold sample of the
// scan at the scan's own rate (the f32 kernel needed 0.36 ms for 17 408 rows x 1000 queries, a quarter of this kernel's rate
// per lookup).  The threshold only steers how many rows the scan keeps (the count is CHECKED afterwards and a short list is
// redone densely), so it may come from quantised sums: tau = M + D (s* + m/2), s* = the r-th smallest sampled sum, m/2 = the
// expected loss of the m floors.
template <int NW, bool COS, bool SAMPLE = false>
__global__ __launch_bounds__(1024) void k_pq_adc16(Adc16Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem16[];
    constexpr uint32_t NQ = COS ? 7 : 8;  // query slots of an entry (Cosine: slot 7 = the |centroid|^2 table)
    const uint32_t tid = threadIdx.x;
    const uint32_t m = a.m;
    const uint32_t q0 = blockIdx.y * NQ;
    uint4 *tab = reinterpret_cast<uint4 *>(smem16);                   // [m*16] entries of 8 x u16
    int32_t *thr = reinterpret_cast<int32_t *>(tab + m * 16);         // L2Sqr: [8] T16 per slot (-1: unused / flagged); Cosine: [8][4] floats
    uint32_t *hit_row = reinterpret_cast<uint32_t *>(thr + 32);       // [ADC16_WGBUF]
    uint32_t *hit_q = hit_row + ADC16_WGBUF;                          // [ADC16_WGBUF] slot | rank << 8
    uint32_t *hit_n = hit_q + ADC16_WGBUF;                            // [0] entries, [1..8] per-slot counts, [9..16] bases
    // the lookups address the table with absolute LDS offsets from 0: the dynamic segment is the kernel's only LDS
    // object, so it starts there; if a toolchain ever places it elsewhere the queries go to the f32 scan
    if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)smem16 != 0u) {
        if (tid < NQ && q0 + tid < a.nq) atomicAdd(&a.cnt[q0 + tid], a.cap + 1);
        return;
    }
    {
        const uint4 *src = a.img + uint64_t(blockIdx.y) * m * 16;
        for (uint32_t i = tid; i < m * 16; i += 1024) tab[i] = src[i];
        if (tid < 1 + 2 * ADC16_Q) hit_n[tid] = 0;
        if (!COS && !SAMPLE && tid < NQ) {
            int32_t T = -1;
            const uint32_t q = q0 + tid;
            if (q < a.nq && a.qflag[q] == 0) {
                const double tau = double(a.tau[q]);
                const double M = a.qM[q], D = a.qD[q];
                const double x = floor((tau * (1.0 + 2.0 * double(m) * 0x1p-24) - M * (1.0 - 1e-12)) / D) + 2.0;
                // tau = +inf / NaN (fewer sampled rows than the rank, NaN rows): everything passes -> the candidate list
                // overflows and the query takes the f32 scan
                T = !(x < 70000.0) ? 70000 : (x < 0.0 ? -1 : (int32_t)x);
            }
            thr[tid] = T;
        }
        if (COS && tid < 8) {
            // per query slot: S_ub = Ms + Ds * s16 (constants rounded up), test S_ub >= 0 && S_ub^2 (1 + 1e-6) >= K * C_lb with
            // K = rho^2 |q|^2 (1 - 1e-5), rho = (1 - tau) - 1e-6 (2 - tau): d_f32 <= tau implies S_f32 / den_f32 >= rho.
            // rho <= 0 (tau >= 1: rows of the opposite half-space qualify), a tiny |q| (the 1e-10 clamp of the reference can
            // act) or a flagged table: Ms = -inf, the query takes the f32 scan (too few hits).  Slot 7: the C table's constants.
            float *f = reinterpret_cast<float *>(thr) + tid * 4;
            float Ms = -INFINITY, Ds = 0.0f, K = INFINITY, tq = -1.0f;  // (unused / unsupported slot: neither test can pass)
            const uint32_t q = q0 + tid;
            if (tid < NQ && q < a.nq && a.qflag[q] == 0) {
                const double tau = double(a.tau[q]), qs = double(a.qsq[q]);
                const double rho = (1.0 - tau) - 1e-6 * (2.0 + fabs(tau));
                if (rho > 0.0 && rho <= 2.0 && qs > 1e-30 && qs < 1e30) {
                    Ms = float(a.qM[q] + fabs(a.qM[q]) * 1e-6 + 1e-30);
                    Ds = float(a.qD[q] * (1.0 + 1e-6));
                    K = float(rho * rho * qs * (1.0 - 1e-5));
                    tq = float(4e-20 / qs);  // C below this: |centroid sum| |q| may be under the reference's 1e-10 clamp
                }
            }
            if (tid == 7 && a.nq > 0) {  // C_lb = (MC + DC * c16) (1 - 4 m 2^-24 - 1e-6): the f32 fold of C and this evaluation round
                const double g1 = 1.0 - 4.0 * double(m) * 0x1p-24 - 1e-6;
                Ms = float(fmax(a.qMC[0], 0.0) * g1);
                Ds = float(a.qDC[0] * g1);
                K = 0.0f;
                tq = 0.0f;
            }
            f[0] = Ms;
            f[1] = Ds;
            f[2] = K;
            f[3] = tq;
        }
    }
    __syncthreads();
    int32_t T[8];
    float cMs[8], cDs[8], cK[8], cT[8];
#pragma unroll
    for (int b = 0; b < 8; b++) {
        T[b] = thr[b];
        if (COS) {
            const float *f = reinterpret_cast<const float *>(thr) + b * 4;
            cMs[b] = f[0];
            cDs[b] = f[1];
            cK[b] = f[2];
            cT[b] = f[3];
        }
    }
    // (ADC16_ABANDON) Tp = T + 1 per 16-bit half, 0 for an unused slot (always "above"), 65535 when T does not fit (never abandoned);
    // checked after every code word of the second half: one v_pk_max_u16 + compare per register
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    uint32_t Tp[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int32_t t0 = T[2 * i] + 1, t1 = T[2 * i + 1] + 1;
        Tp[i] = uint32_t(t0 > 65535 ? 65535 : t0) | (uint32_t(t1 > 65535 ? 65535 : t1) << 16);
    }
    // scan: this workgroup's contiguous share of the rows; sample: sampled blocks blockIdx.x, + gridDim.x, ... (block j of the
    // sample = rows [j * blk_step * 1024, + 1024))
    const uint64_t n_sb = SAMPLE ? ((a.n + 1023) / 1024 + a.blk_step - 1) / a.blk_step : 0;
    const uint64_t r_begin = SAMPLE ? uint64_t(blockIdx.x) * a.blk_step * 1024 : uint64_t(blockIdx.x) * a.rows_per_wg;
    const uint64_t r_end = SAMPLE ? (blockIdx.x < n_sb ? (n_sb - 1) * a.blk_step * 1024 + 1 : 0)
                                  : (r_begin + a.rows_per_wg < a.n ? r_begin + a.rows_per_wg : a.n);
    const uint64_t r_inc = SAMPLE ? uint64_t(gridDim.x) * a.blk_step * 1024 : 1024;
    const uint32_t nwords = NW ? (uint32_t)NW : a.m / 32;
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(3))) uint4 lds_u4;
#endif
    for (uint64_t rb = r_begin; rb < r_end; rb += r_inc) {
        const uint64_t row = rb + tid;
        const bool valid = SAMPLE ? row < a.n : row < r_end;
        // word w of row (rb + tid): tile = row / 64 (uniform in the wave: rb is a multiple of 64), lane = row % 64; rows
        // past n inside the last tile are zero padding
        // Lanes past the workgroup's share (a share is shorter than the 1024 lanes when the table has fewer than 1024 rows per
        // CU) must not form addresses from their row number: the last workgroup's reach up to 1023 rows past the table, i.e.
        // past the mirror -- found by tools/fuzz_pq.py as a memory-access fault on a 74 205-row table whose mirror ended on
        // a page boundary (configuration #727, seed 4242; the over-read is as old as the kernel).  They re-read a valid row.
        const uint64_t lrow = valid ? row : (SAMPLE ? a.n - 1 : r_end - 1);
        const uint4 *cw = a.codes_t + (lrow >> 6) * nwords * 64 + (lrow & 63);
        uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
        // one 16-B code word = 32 groups.  Byte b of a 32-bit word: low nibble = group 8wi + 2b, high nibble the next one;
        // their byte offsets inside the group's 256-B block (code * 16) sit packed in the bytes of e4 / o4.
        // A step = the 8 groups of one 32-bit code word: byte b holds group 2b (low nibble) and 2b+1 (high nibble); their
        // byte offsets inside a group's 256-B block (code * 16) sit packed in the bytes of e4 / o4.  gbyte = byte offset
        // of the step's first group block, folded into the instructions' immediates; the table starts at LDS address 0
        // (checked at kernel entry), so a lookup's address register is the permute alone.
        auto issue = [&](uint32_t word, uint32_t gbyte, uint32_t hi /* 0 or 0x04: adds bit 16 through the permute */, uint4 *E, uint4 *O) {
            const uint32_t e4 = (word & 0x0f0f0f0fu) << 4, o4 = word & 0xf0f0f0f0u;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const uint32_t sel = 0x0c000c00u | (hi << 16) | (uint32_t)b | (hi ? 0u : 0x000c0000u);
                const uint32_t oe = __builtin_amdgcn_perm(1u, e4, sel), oo = __builtin_amdgcn_perm(1u, o4, sel);
#if defined(__HIP_DEVICE_COMPILE__)
                E[b] = *reinterpret_cast<const lds_u4 *>(oe + gbyte + (2 * b) * 256);
                O[b] = *reinterpret_cast<const lds_u4 *>(oo + gbyte + (2 * b + 1) * 256);
#else
                E[b] = O[b] = make_uint4(oe, oo, gbyte, 0);  // (host pass of the single-source compile: never runs)
#endif
            }
        };
        auto consume = [&](const uint4 *E, const uint4 *O) {
#pragma unroll
            for (int b = 0; b < 4; b++) {
                a0 = a0 + E[b].x + O[b].x;
                a1 = a1 + E[b].y + O[b].y;
                a2 = a2 + E[b].z + O[b].z;
                a3 = a3 + E[b].w + O[b].w;
            }
            // pin the four running sums here: left alone, the optimiser re-associates the unrolled row into four
            // separate 320-term chains, finishes one and parks the other three components of every table entry
            // in scratch (measured: 1.7 - 7.8 KB of spills per lane)
            asm volatile("" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3));
        };
        if (NW) {
            // software pipeline over the 4 NW steps of the row: the lookups of step i+1 are issued before the sums of
            // step i are taken, so 8 - 16 ds_read_b128 per wave are in flight while the adds run
            uint4 cv[NW ? NW : 1];
#pragma unroll
            for (int w = 0; w < NW; w++) cv[w] = cw[w * 64];
            uint4 E[2][4], O[2][4];
            issue(cv[0].x, 0u, 0u, E[0], O[0]);
            bool done = false;  // wave-uniform: every row of the wave is out (a `break` would keep the loop from unrolling)
#pragma unroll
            for (int st = 0; st < 4 * NW; st++) {
                if (done) continue;
                if (st + 1 < 4 * NW) {
                    const int w = (st + 1) >> 2, wi = (st + 1) & 3;
                    const uint32_t word = wi == 0 ? cv[w].x : (wi == 1 ? cv[w].y : (wi == 2 ? cv[w].z : cv[w].w));
                    // groups 32w .. 32w+31 at byte offset w * 8192: beyond 65535 the immediate cannot hold it -> bit 16
                    // rides in the address register (sel byte 2 = 4 picks the 0x01 of the constant operand)
                    issue(word, (w < 8 ? w : w - 8) * 8192 + wi * 2048, w < 8 ? 0u : 0x04u, E[(st + 1) & 1], O[(st + 1) & 1]);
                    __builtin_amdgcn_sched_barrier(0);  // (the scheduler otherwise sinks these reads below the adds of step st)
                }
                consume(E[st & 1], O[st & 1]);
                if (!COS && ADC16_ABANDON && (st & 3) == 3 && st + 1 < 4 * NW && st >= 2 * NW - 1) {
                    auto above = [](uint32_t acc, uint32_t tp) {
                        return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2, acc), __builtin_bit_cast(u16x2, tp))) == acc;
                    };
                    const bool out = !valid || (above(a0, Tp[0]) && above(a1, Tp[1]) && above(a2, Tp[2]) && above(a3, Tp[3]));
                    done = __ballot(!out) == 0;  // the threshold test below then sees sums that are already above
                }
            }
        } else {
            uint4 v = cw[0];
            for (uint32_t w = 0; w < nwords; w++) {
                const uint4 cur = v;
                if (w + 1 < nwords) v = cw[(w + 1) * 64];  // next code word while this one is looked up
                const uint32_t words[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
                for (int wi = 0; wi < 4; wi++) {
                    uint4 E[4], O[4];
                    issue(words[wi], w * 8192 + wi * 2048, 0u, E, O);
                    consume(E, O);
                }
            }
        }
        const int32_t s[8] = {int32_t(a0 & 0xffffu), int32_t(a0 >> 16), int32_t(a1 & 0xffffu), int32_t(a1 >> 16),
                              int32_t(a2 & 0xffffu), int32_t(a2 >> 16), int32_t(a3 & 0xffffu), int32_t(a3 >> 16)};
        if (SAMPLE) {
            const uint64_t col = rb / (uint64_t(a.blk_step) * 1024) * 1024 + tid;  // position in the sample
#pragma unroll
            for (int b = 0; b < (int)NQ; b++)
                if (q0 + b < a.nq) a.s16_out[uint64_t(q0 + b) * a.ld_s + col] = valid ? float(s[b]) : INFINITY;
            continue;
        }
        float c_lb = 0.0f;
        if (COS) c_lb = fmaxf(cMs[7] + cDs[7] * float(s[7]), 0.0f);
#pragma unroll
        for (int b = 0; b < (int)NQ; b++) {
            bool pass;
            if (COS) {
                const float sub = cMs[b] + cDs[b] * float(s[b]);
                // (second term: even the lower bound of C cannot rule out the reference's 1e-10 clamp -> the exact stage decides)
                pass = (sub >= 0.0f && sub * sub * 1.000001f >= cK[b] * c_lb) || c_lb <= cT[b];
            } else {
                pass = s[b] <= T[b];
            }
            if (valid && pass) {
                const uint32_t pos = atomicAdd(hit_n, 1u);
                if (pos < ADC16_WGBUF) {
                    hit_row[pos] = uint32_t(row);
                    hit_q[pos] = b;
                } else {
                    atomicAdd(&a.cnt[q0 + b], a.cap + 1);  // mark the query as overflowed (-> f32 scan)
                }
            }
        }
    }
    if (SAMPLE) return;
    __syncthreads();
    uint32_t total = hit_n[0];
    if (total > ADC16_WGBUF) total = ADC16_WGBUF;
    for (uint32_t i = tid; i < total; i += 1024) {
        const uint32_t r_ = atomicAdd(&hit_n[1 + hit_q[i]], 1u);
        hit_q[i] |= r_ << 8;
    }
    __syncthreads();
    if (tid < NQ && hit_n[1 + tid] > 0) hit_n[1 + ADC16_Q + tid] = atomicAdd(&a.cnt[q0 + tid], hit_n[1 + tid]);
    __syncthreads();
    for (uint32_t i = tid; i < total; i += 1024) {
        const uint32_t b = hit_q[i] & 0xffu, r_ = hit_q[i] >> 8;
        const uint32_t slot = hit_n[1 + ADC16_Q + b] + r_;
        if (slot < a.cap) a.cand[uint64_t(q0 + b) * a.cap + slot] = hit_row[i];
    }
}

// exact f32 ADC sums (strict group order, pq_table.rs:254-292) of the candidates of every query: row ids in, pair keys
// out (PAIR_NONE for sums above tau); valid[q] counts the pairs kept.  One workgroup per query, its f32 table in LDS.
template <bool COS>
__global__ __launch_bounds__(256) void k_pq_adc_exact(const uint8_t *__restrict__ codes, uint32_t enc_dim, uint32_t m,
                                                      const float *__restrict__ lut, const float *__restrict__ cent_cache,
                                                      const float *__restrict__ qsq, const float *__restrict__ tau,
                                                      uint64_t *__restrict__ cand, const uint32_t *__restrict__ cnt,
                                                      uint32_t cap, uint32_t *__restrict__ valid) {
    extern __shared__ __attribute__((aligned(16))) float slut[];  // the query's table; Cosine: the |centroid|^2 table behind it
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t total = cnt[q];
    if (total > cap) return;  // overflowed list: the query is redone by the f32 scan
    const float *lq = lut + uint64_t(q) * m * 16;
    for (uint32_t i = tid; i < m * 16; i += 256) slut[i] = lq[i];
    const float *scc = slut + m * 16;
    if (COS)
        for (uint32_t i = tid; i < m * 16; i += 256) slut[m * 16 + i] = cent_cache[i];
    __syncthreads();
    const float t = tau[q];
    uint64_t *cq = cand + uint64_t(q) * cap;
    uint32_t kept = 0;
    for (uint32_t i = tid; i < total; i += 256) {
        const uint32_t row = uint32_t(cq[i]);
        const uint4 *cw = reinterpret_cast<const uint4 *>(codes + uint64_t(row) * enc_dim);
        float sum = 0.0f, cdp = 0.0f;
        const bool words = (enc_dim & 15u) == 0 && m == 2 * enc_dim;  // whole 16-B words AND every nibble a real group
        if (!words) {  // otherwise byte by byte, same group order (an odd m leaves the last high nibble without a table:
            // tools/fuzz_pq.py, Cosine, m = 31 / 63 -- the word loop below would add whatever sits behind the query's table)
            const uint8_t *cb = codes + uint64_t(row) * enc_dim;
            for (uint32_t g = 0; g < m; g += 2) {
                const uint32_t byte = cb[g >> 1];
                const uint32_t a0 = g * 16 + (byte & 0xf), a1 = (g + 1) * 16 + (byte >> 4);
                sum = sum + slut[a0];
                if (COS) cdp = cdp + scc[a0];
                if (g + 1 < m) {
                    sum = sum + slut[a1];
                    if (COS) cdp = cdp + scc[a1];
                }
            }
        }
        // code words in batches of WB, the next batch in flight while this one is looked up: every load is executed by every lane
        // of the branch (clamped word index) -- the earlier form fetched ONE word ahead under a
        // condition, i.e. a branch per word and a full round trip to the code rows (L2 / Infinity Cache) per 16 bytes: 10 per candidate
        // at m = 320, 131 us per 1000 queries of which the 320 table lookups and adds of a candidate are ~1.5 us
        constexpr uint32_t WB = 5;
        const uint32_t nw = words ? enc_dim / 16 : 0u, lastw = nw ? nw - 1 : 0u;
        uint4 cur[WB], nxt[WB];
        if (words) {  // (uniform; rows of other shapes are not 16-B aligned and were summed above)
#pragma unroll
        for (uint32_t j = 0; j < WB; j++) cur[j] = cw[j < lastw ? j : lastw];
        for (uint32_t w0 = 0; w0 < nw; w0 += WB) {
#pragma unroll
            for (uint32_t j = 0; j < WB; j++) {
                const uint32_t wn = w0 + WB + j;
                nxt[j] = cw[wn < lastw ? wn : lastw];
            }
#pragma unroll
            for (uint32_t jw = 0; jw < WB; jw++) {
                const uint32_t w = w0 + jw;
                if (w >= nw) break;  // uniform; no load behind it
                const uint32_t wd[4] = {cur[jw].x, cur[jw].y, cur[jw].z, cur[jw].w};
#pragma unroll
                for (int wi = 0; wi < 4; wi++) {
                    float e[8], c[8];
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        const uint32_t at = (w * 32 + 8 * wi + j) * 16 + ((wd[wi] >> (4 * j)) & 0xf);
                        e[j] = slut[at];
                        if (COS) c[j] = scc[at];
                    }
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        sum = sum + e[j];
                        if (COS) cdp = cdp + c[j];
                    }
                }
            }
#pragma unroll
            for (uint32_t j = 0; j < WB; j++) cur[j] = nxt[j];
        }
        }
        if (COS) {  // pq_table.rs:294-299, the operation order of k_pq_adc
            float norm0 = sqrtf(cdp);
            float norm1 = sqrtf(qsq[q]);
            float den = fmaxf(norm0 * norm1, 1e-10f);
            float r = sum / den;
            sum = 1.0f - r;
        }
        const bool keep = sum <= t;
        cq[i] = keep ? pair_key(sum, row) : PAIR_NONE;
        kept += keep ? 1u : 0u;
    }
    if (kept) atomicAdd(&valid[q], kept);
}

// ---------------------------------------------------------------------------------------------------
// 8-bit codes (n_bits = 8, pq_table.rs:142-145: 256 centroids per group) on a quantised pass of their own (round 3).
// A query's f32 table is m x 256 entries -- 327 KB at m = 320: no form of it that serves several queries fits LDS, and the
// f32 scan reads it through L1 / L2 (0.37 ms per query per 1M rows).  One query's table at ONE BYTE per entry does fit
// (m x 256 B = 80 KB):  lut8[g][c] = min(255, floor((lut[g][c] - mn_g) / D)),  D = sum_g range_g / (128 m).
// The minimum with 255 only lowers an entry, so M + D * S8 <= sum_g lut[g][code_g] still holds (M = sum mn_g) and the
// superset threshold of the 16-bit pass carries over:  S <= tau  ==>  S8 <= T8 := floor((tau (1 + 2 m 2^-24) - M (1 - 1e-12)) / D) + 2.
// All lanes of a wave look up the SAME group at a time: its 256 one-byte entries are exactly one word per LDS bank, so a
// wave's 64 lookups never conflict.  The scan is bound by the code bytes -- m bytes per row and query, one query per pass
// -- i.e. by HBM: 320 MB per query at m = 320.  Candidates get their exact f32 sums in group order (k_pq_adc_exact8: the
// query's f32 table read through L2) and the pairs above tau are dropped, as on the 16-bit pass.  L2Sqr only.
__global__ __launch_bounds__(256) void k_pq_quant8(const float *__restrict__ lut, uint32_t m, uint32_t m_pad, uint32_t nq, uint8_t *__restrict__ img,
                                                   double *__restrict__ qM, double *__restrict__ qD, uint32_t *__restrict__ qflag) {
    const uint32_t q = blockIdx.x, t = threadIdx.x;
    __shared__ double sR[256], sM[256];
    __shared__ float smn[1024];  // group minima (m <= 1024: the table of a larger m does not fit LDS anyway)
    __shared__ uint32_t sbad;
    if (t == 0) sbad = 0;
    __syncthreads();
    const float *lq = lut + uint64_t(q) * m * 256;
    double R = 0.0, M = 0.0;
    bool bad = false;
    // a wave per group, 4 entries per lane: coalesced reads, wave-level min / max
    for (uint32_t g = t >> 6; g < m; g += 4) {
        const float4 v = reinterpret_cast<const float4 *>(lq + g * 256)[t & 63];
        const float e[4] = {v.x, v.y, v.z, v.w};
        float mn = INFINITY, mx = -INFINITY;
        bool b = false;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (!(e[j] >= 0.0f) || e[j] > 3.0e38f) b = true;  // NaN, negative, inf: the query takes the f32 scan
            mn = fminf(mn, e[j]);
            mx = fmaxf(mx, e[j]);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            mn = fminf(mn, __shfl_xor(mn, off));
            mx = fmaxf(mx, __shfl_xor(mx, off));
        }
        if (__ballot(b) != 0) bad = true;
        if ((t & 63) == 0) {
            smn[g] = mn;
            R += double(mx) - double(mn);
            M += double(mn);
        }
    }
    if (bad) atomicOr(&sbad, 1u);
    sR[t] = R;
    sM[t] = M;
    __syncthreads();
    for (uint32_t st = 128; st > 0; st >>= 1) {
        if (t < st) {
            sR[t] += sR[t + st];
            sM[t] += sM[t + st];
        }
        __syncthreads();
    }
    R = sR[0];
    M = sM[0];
    const bool flag = sbad != 0 || !(R < 1.0e300) || !(fabs(M) < 1.0e300);
    const double D = (!flag && R > 0.0) ? R / (128.0 * double(m)) : 1.0;
    uint8_t *dst = img + uint64_t(q) * m_pad * 256;
    for (uint32_t i = m * 256 + t; i < m_pad * 256; i += 256) dst[i] = 0;  // groups of the padded code bytes
    for (uint32_t i = t; i < m * 256; i += 256) {
        const float mn = smn[i >> 8];
        double x = flag ? 0.0 : floor((double(lq[i]) - double(mn)) / D);
        x = x < 0.0 ? 0.0 : (x > 255.0 ? 255.0 : x);
        dst[i] = (uint8_t)x;
    }
    if (t == 0) {
        qM[q] = M;
        qD[q] = D;
        qflag[q] = flag ? 1u : 0u;
    }
}

constexpr uint32_t ADC8_WGBUF = 4096;  // LDS hit buffer entries (one query per workgroup)

template <bool SAMPLE>
__global__ __launch_bounds__(1024) void k_pq_adc8(Adc8Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem8[];
    const uint32_t tid = threadIdx.x, q = blockIdx.y;
    const uint32_t tab_bytes = a.nwords * 16 * 256;
    uint8_t *tab = smem8;                                                  // [16 nwords][256]
    uint32_t *hit_row = reinterpret_cast<uint32_t *>(smem8 + tab_bytes);   // [ADC8_WGBUF]
    uint32_t *hit_n = hit_row + ADC8_WGBUF;                                // [0] entries, [1] threshold, [2] base of the flush
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(a.img + uint64_t(q) * tab_bytes);
        uint4 *dst = reinterpret_cast<uint4 *>(tab);
        for (uint32_t i = tid; i < tab_bytes / 16; i += 1024) dst[i] = src[i];
        if (tid == 0) {
            hit_n[0] = 0;
            int32_t T = -1;
            if (!SAMPLE && a.qflag[q] == 0) {
                const double x = floor((double(a.tau[q]) * (1.0 + 2.0 * double(a.m) * 0x1p-24) - a.qM[q] * (1.0 - 1e-12)) / a.qD[q]) + 2.0;
                // tau = +inf / NaN: everything passes -> the list overflows and the query takes the f32 scan
                T = !(x < 2.0e9) ? 2000000000 : (x < 0.0 ? -1 : (int32_t)x);
            }
            hit_n[1] = (uint32_t)T;
        }
    }
    __syncthreads();
    const int32_t T = (int32_t)hit_n[1];
    const uint64_t n_sb = SAMPLE ? ((a.n + 1023) / 1024 + a.blk_step - 1) / a.blk_step : 0;
    const uint64_t r_begin = SAMPLE ? uint64_t(blockIdx.x) * a.blk_step * 1024 : uint64_t(blockIdx.x) * a.rows_per_wg;
    const uint64_t r_end = SAMPLE ? (blockIdx.x < n_sb ? (n_sb - 1) * a.blk_step * 1024 + 1 : 0)
                                  : (r_begin + a.rows_per_wg < a.n ? r_begin + a.rows_per_wg : a.n);
    const uint64_t r_inc = SAMPLE ? uint64_t(gridDim.x) * a.blk_step * 1024 : 1024;
    const uint32_t nwords = a.nwords;
    for (uint64_t rb = r_begin; rb < r_end; rb += r_inc) {
        const uint64_t row = rb + tid;
        const bool valid = SAMPLE ? row < a.n : row < r_end;
        const uint64_t lrow = valid ? row : (SAMPLE ? a.n - 1 : r_end - 1);  // (see k_pq_adc16: idle lanes re-read a valid row)
        const uint4 *cw = a.codes_t + (lrow >> 6) * nwords * 64 + (lrow & 63);
        uint32_t s0 = 0, s1 = 0;  // two running sums: the lookups of a word are independent, the adds need not be one chain
        uint4 v = cw[0];
        for (uint32_t w = 0; w < nwords; w++) {
            const uint4 cur = v;
            if (w + 1 < nwords) v = cw[(w + 1) * 64];  // next code word while this one is looked up
            const uint8_t *tw = tab + w * 4096;       // 16 groups x 256 entries
            const uint32_t words[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
            for (int wi = 0; wi < 4; wi++) {
                const uint32_t c = words[wi];
                const uint32_t e0 = tw[(4 * wi + 0) * 256 + (c & 0xffu)], e1 = tw[(4 * wi + 1) * 256 + ((c >> 8) & 0xffu)];
                const uint32_t e2 = tw[(4 * wi + 2) * 256 + ((c >> 16) & 0xffu)], e3 = tw[(4 * wi + 3) * 256 + (c >> 24)];
                s0 += e0 + e2;
                s1 += e1 + e3;
            }
        }
        const uint32_t S8 = s0 + s1;
        if (SAMPLE) {
            const uint64_t col = rb / (uint64_t(a.blk_step) * 1024) * 1024 + tid;
            a.s8_out[uint64_t(q) * a.ld_s + col] = valid ? float(S8) : INFINITY;
            continue;
        }
        if (valid && (int32_t)S8 <= T) {
            const uint32_t pos = atomicAdd(&hit_n[0], 1u);
            if (pos < ADC8_WGBUF)
                hit_row[pos] = uint32_t(row);
            else
                atomicAdd(&a.cnt[q], a.cap + 1);  // mark the query as overflowed (-> f32 scan)
        }
    }
    if (SAMPLE) return;
    __syncthreads();
    uint32_t total = hit_n[0];
    if (total > ADC8_WGBUF) total = ADC8_WGBUF;
    if (tid == 0 && total > 0) hit_n[2] = atomicAdd(&a.cnt[q], total);
    __syncthreads();
    const uint32_t base = hit_n[2];
    for (uint32_t i = tid; i < total; i += 1024) {
        const uint32_t slot = base + i;
        if (slot < a.cap) a.cand[uint64_t(q) * a.cap + slot] = hit_row[i];
    }
}

// ---------------------------------------------------------------------------------------------------
// 8-bit codes, EIGHT queries per pass (round 4).  k_pq_adc8 above reads the whole code mirror once per QUERY (one byte table per query
// fills the LDS): 320 GB of code bytes per 1000 queries at 1M rows, m = 320 -- 44 ms.  The 4-bit scan's scheme (k_pq_adc16: 16-bit
// entries, 8 queries side by side in a 16-B LDS entry, one ds_read_b128 per (row, group) for all eight) needs 256 entries x 16 B = 4 KB
// per group here, 1.3 MB for the table of 8 queries: it does not fit.  So the table is cut into SLICES of 32 groups (128 KB, two 16-B
// code words of a row): a workgroup keeps 4 rows per thread (4096 rows), and for every slice loads the slice of the image into LDS and
// adds the slice's 32 lookups to the rows' eight packed 16-bit sums, which stay in registers across the slices.  The image of a query
// group is re-read from L2 by every workgroup (1.3 MB against the 1.3 MB of code bytes of its 4096 rows), the code mirror once per 8
// queries.  Same quantisation and the same superset proof as k_pq_adc16 (entries floor((lut - mn_g) / D), D = sum of ranges / 65000:
// M + D S16 <= the reference's f32 sum up to its gamma_m, so S <= tau implies S16 <= T16); the candidates' exact f32 sums, the
// (adc, idx) order and the re-rank are k_pq_adc_exact8's and the merge's, unchanged.  L2Sqr tables (as the one-byte scan).
// ---------------------------------------------------------------------------------------------------
constexpr uint32_t ADC16X8_WGBUF = 2048;  // LDS hit buffer entries per workgroup

// per query: the minimum of every group's 256 table entries (mn[q][g]), M = their sum, D = sum of the ranges / 65000
__global__ __launch_bounds__(256) void k_pq_quant16x8_stats(const float *__restrict__ lut, uint32_t m, uint32_t nq, float *__restrict__ mn_out,
                                                            double *__restrict__ qM, double *__restrict__ qD, uint32_t *__restrict__ qflag,
                                                            double divisor) {
    const uint32_t q = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    __shared__ double sR[4], sM[4];
    __shared__ uint32_t sbad;
    if (t == 0) sbad = 0;
    __syncthreads();
    const float *lq = lut + uint64_t(q) * m * 256;
    double R = 0.0, M = 0.0;
    bool bad = false;
    for (uint32_t g = wave; g < m; g += 4) {  // a wave per group: 4 entries per lane
        const float4 e = reinterpret_cast<const float4 *>(lq + uint64_t(g) * 256)[lane];
        const float v[4] = {e.x, e.y, e.z, e.w};
        float mn = INFINITY, mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (!(v[j] >= 0.0f) || v[j] > 3.0e38f) bad = true;  // NaN, negative, inf: the query takes the f32 scan
            mn = fminf(mn, v[j]);
            mx = fmaxf(mx, v[j]);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            mn = fminf(mn, __shfl_xor(mn, off));
            mx = fmaxf(mx, __shfl_xor(mx, off));
        }
        if (lane == 0) {
            mn_out[uint64_t(q) * m + g] = mn;
            R += double(mx) - double(mn);
            M += double(mn);
        }
    }
    if (__ballot(bad) != 0 && lane == 0) atomicOr(&sbad, 1u);
    if (lane == 0) {
        sR[wave] = R;
        sM[wave] = M;
    }
    __syncthreads();
    if (t == 0) {
        R = (sR[0] + sR[1]) + (sR[2] + sR[3]);
        M = (sM[0] + sM[1]) + (sM[2] + sM[3]);
        const bool flag = sbad != 0 || !(R < 1.0e300) || !(fabs(M) < 1.0e300);
        qM[q] = M;
        qD[q] = (!flag && R > 0.0) ? R / divisor : 1.0;  // (65000 for 16-bit entries; k_pq_adc8x16: see there)
        qflag[q] = flag ? 1u : 0u;
    }
}
// the image: img[(grp * m_pad + g) * 256 + c] = 8 x u16, slot b = floor((lut[8 grp + b][g][c] - mn) / D) (0 for g >= m, for query slots
// past nq and for flagged queries: padded code bytes select entry 0 of an all-zero group).  One thread per 16-B entry.
__global__ __launch_bounds__(256) void k_pq_quant16x8_img(const float *__restrict__ lut, const float *__restrict__ mn, const double *__restrict__ qD,
                                                          const uint32_t *__restrict__ qflag, uint32_t m, uint32_t m_pad, uint32_t nq,
                                                          uint4 *__restrict__ img) {
    const uint32_t grp = blockIdx.y, g = blockIdx.x, c = threadIdx.x;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (g < m) {
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const uint32_t q = grp * 8 + b;
            if (q < nq && qflag[q] == 0) {
                const double y = (double(lut[(uint64_t(q) * m + g) * 256 + c]) - double(mn[uint64_t(q) * m + g])) / qD[q];
                double x = floor(y);
                x = x < 0.0 ? 0.0 : (x > 65000.0 ? 65000.0 : x);  // (unreachable clamps: the sum of the maxima is <= 65000)
                w[b >> 1] |= uint32_t(x) << (16 * (b & 1));
            }
        }
    }
    img[(uint64_t(grp) * m_pad + g) * 256 + c] = make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ __launch_bounds__(1024) void k_pq_adc16x8(Adc16x8Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem168[];
    constexpr uint32_t RPT = ADC16X8_RPT, GS = ADC16X8_GS;
    uint4 *tab = reinterpret_cast<uint4 *>(smem168);                                   // [GS][256] entries of 8 x u16
    uint32_t *hit_row = reinterpret_cast<uint32_t *>(smem168 + size_t(GS) * 256 * 16);  // [WGBUF]
    uint32_t *hit_q = hit_row + ADC16X8_WGBUF;                                         // [WGBUF] slot | rank << 8
    uint32_t *hit_n = hit_q + ADC16X8_WGBUF;                                           // [0] entries, [1..8] per-slot counts, [9..16] bases
    int32_t *thr = reinterpret_cast<int32_t *>(hit_n + 20);                            // [8] T16 per slot (-1: unused / flagged)
    const uint32_t tid = threadIdx.x, q0 = blockIdx.y * 8, m = a.m, nwords = a.nwords;
    if (tid < 17) hit_n[tid] = 0;
    if (tid < 8) {
        int32_t T = -1;
        const uint32_t q = q0 + tid;
        if (q < a.nq && a.qflag[q] == 0) {
            const double x = floor((double(a.tau[q]) * (1.0 + 2.0 * double(m) * 0x1p-24) - a.qM[q] * (1.0 - 1e-12)) / a.qD[q]) + 2.0;
            // tau = +inf / NaN: everything passes -> the candidate list overflows and the query takes the f32 scan
            T = !(x < 70000.0) ? 70000 : (x < 0.0 ? -1 : (int32_t)x);
        }
        thr[tid] = T;
    }
    __syncthreads();
    int32_t T[8];
#pragma unroll
    for (int b = 0; b < 8; b++) T[b] = thr[b];
    const uint4 *img = a.img + uint64_t(blockIdx.y) * a.nslices * GS * 256;
    const uint64_t r_begin = uint64_t(blockIdx.x) * a.rows_per_wg;
    const uint64_t r_end = r_begin + a.rows_per_wg < a.n ? r_begin + a.rows_per_wg : a.n;
    for (uint64_t rb = r_begin; rb < r_end; rb += uint64_t(RPT) * 1024) {
        uint32_t acc[RPT][4];
        const uint4 *cw[RPT];
        bool valid[RPT];
#pragma unroll
        for (int j = 0; j < (int)RPT; j++) {
            acc[j][0] = acc[j][1] = acc[j][2] = acc[j][3] = 0u;
            const uint64_t row = rb + uint64_t(j) * 1024 + tid;
            valid[j] = row < r_end;
            const uint64_t lrow = valid[j] ? row : r_end - 1;  // (idle lanes re-read a valid row: see k_pq_adc16)
            cw[j] = a.codes_t + (lrow >> 6) * nwords * 64 + (lrow & 63);
        }
        for (uint32_t sl = 0; sl < a.nslices; sl++) {
            __syncthreads();  // the previous slice's readers are done
            {
                const uint4 *src = img + uint64_t(sl) * GS * 256;
#pragma unroll
                for (int i = 0; i < 8; i++) tab[i * 1024 + tid] = src[i * 1024 + tid];
            }
            // the slice's two code words of the thread's rows (zero words past the mirror's last: entry 0 of an all-zero group)
            uint4 c0[RPT], c1[RPT];
            const uint32_t w0 = 2 * sl, w1 = 2 * sl + 1;
#pragma unroll
            for (int j = 0; j < (int)RPT; j++) {
                c0[j] = w0 < nwords ? cw[j][w0 * 64] : make_uint4(0u, 0u, 0u, 0u);
                c1[j] = w1 < nwords ? cw[j][w1 * 64] : make_uint4(0u, 0u, 0u, 0u);
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < (int)RPT; j++) {
                const uint32_t words[8] = {c0[j].x, c0[j].y, c0[j].z, c0[j].w, c1[j].x, c1[j].y, c1[j].z, c1[j].w};
                uint32_t a0 = acc[j][0], a1 = acc[j][1], a2 = acc[j][2], a3 = acc[j][3];
                // software pipeline over the 8 words: the four lookups of word k + 1 are issued before the sums of word k are taken
                uint4 E[2][4];
                auto issue = [&](int k, uint4 *e) {
#pragma unroll
                    for (int b = 0; b < 4; b++) e[b] = tab[(4 * k + b) * 256 + ((words[k] >> (8 * b)) & 0xffu)];
                };
                issue(0, E[0]);
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    if (k + 1 < 8) {
                        issue(k + 1, E[(k + 1) & 1]);
                        __builtin_amdgcn_sched_barrier(0);  // (the scheduler otherwise sinks these reads below the adds of word k)
                    }
                    const uint4 *e = E[k & 1];
                    a0 = a0 + e[0].x + e[1].x;
                    a1 = a1 + e[0].y + e[1].y;
                    a2 = a2 + e[0].z + e[1].z;
                    a3 = a3 + e[0].w + e[1].w;
                    a0 = a0 + e[2].x + e[3].x;
                    a1 = a1 + e[2].y + e[3].y;
                    a2 = a2 + e[2].z + e[3].z;
                    a3 = a3 + e[2].w + e[3].w;
                    asm volatile("" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3));  // (keeps the four running sums four: see k_pq_adc16)
                }
                acc[j][0] = a0;
                acc[j][1] = a1;
                acc[j][2] = a2;
                acc[j][3] = a3;
            }
        }
#pragma unroll
        for (int j = 0; j < (int)RPT; j++) {
            const int32_t s[8] = {int32_t(acc[j][0] & 0xffffu), int32_t(acc[j][0] >> 16), int32_t(acc[j][1] & 0xffffu), int32_t(acc[j][1] >> 16),
                                  int32_t(acc[j][2] & 0xffffu), int32_t(acc[j][2] >> 16), int32_t(acc[j][3] & 0xffffu), int32_t(acc[j][3] >> 16)};
            const uint32_t row = uint32_t(rb + uint64_t(j) * 1024 + tid);
#pragma unroll
            for (int b = 0; b < 8; b++) {
                if (valid[j] && s[b] <= T[b]) {
                    const uint32_t pos = atomicAdd(hit_n, 1u);
                    if (pos < ADC16X8_WGBUF) {
                        hit_row[pos] = row;
                        hit_q[pos] = b;
                    } else {
                        atomicAdd(&a.cnt[q0 + b], a.cap + 1);  // mark the query as overflowed (-> f32 scan)
                    }
                }
            }
        }
        // hand the block's hits to the per-query candidate lists (one global atomic per query), leave an empty buffer
        __syncthreads();
        uint32_t total = hit_n[0];
        if (total > ADC16X8_WGBUF) total = ADC16X8_WGBUF;
        for (uint32_t i = tid; i < total; i += 1024) {
            const uint32_t r_ = atomicAdd(&hit_n[1 + hit_q[i]], 1u);
            hit_q[i] |= r_ << 8;
        }
        __syncthreads();
        if (tid < 8 && hit_n[1 + tid] > 0) hit_n[9 + tid] = atomicAdd(&a.cnt[q0 + tid], hit_n[1 + tid]);
        __syncthreads();
        for (uint32_t i = tid; i < total; i += 1024) {
            const uint32_t b = hit_q[i] & 0xffu, r_ = hit_q[i] >> 8;
            const uint32_t slot = hit_n[9 + b] + r_;
            if (slot < a.cap) a.cand[uint64_t(q0 + b) * a.cap + slot] = hit_row[i];
        }
        __syncthreads();
        if (tid < 17) hit_n[tid] = 0;
    }
}

// ---------------------------------------------------------------------------------------------------
// 8-bit codes, SIXTEEN queries per pass on one-byte entries (round 4, second step).  k_pq_adc16x8 is bound by the LDS: a group's 256
// entries of 16 B span 4 KB, the 16 lanes of a ds_read_b128 quarter hit random 4-bank groups (expected worst load ~4.3 against the 2 of
// a conflict-free read), 0.27 cycles per lane lookup.  The conflicts are in the data (the codes); what can change is how many queries
// one 16-B lookup serves: here an entry holds ONE BYTE for each of 16 queries,
//     e8[g][c] = min(255, floor((lut[g][c] - mn_g) / D)),   D = sum_g range_g / min(65000, 512 m)
// so the same LDS time serves twice the queries and the code mirror is read once per 16 of them.  The minimum with 255 only LOWERS an
// entry (M + D S8 <= the f32 sum still holds, as in k_pq_adc8) and it only touches entries far up a group's range -- lookups of rows
// that are far from the query in that group; D itself is the 16-bit pass's (R / 65000 from m = 127 on), so rows near the threshold
// keep the resolution they had.  The sums of a row stay below 2^16 without saturation or wrap: sum_g e8 <= sum_g range_g / D <=
// 65000.  A dword of an entry holds slots 4d, 4d+2, 4d+1, 4d+3 (bytes 0 .. 3): `x & 0x00ff00ff` is the pair of 16-bit addends of slots
// (4d, 4d+1) and one v_perm_b32 that of (4d+2, 4d+3); eight packed 16-bit pairs per row, two rows per thread (2048 rows per workgroup),
// slices of 16 groups (see the kernel).  Same superset rule, same exact stage and order.  L2Sqr tables.
// ---------------------------------------------------------------------------------------------------
constexpr uint32_t ADC8X16_WGBUF = 2048;  // LDS hit buffer entries per workgroup

// the image: img[(grp * m_pad + g) * 256 + c] = 16 bytes, slot b of dword b / 4 at byte {0, 2, 1, 3}[b % 4] (0 for g >= m, for query
// slots past nq and for flagged queries).  One thread per 16-B entry.
__global__ __launch_bounds__(256) void k_pq_quant8x16_img(const float *__restrict__ lut, const float *__restrict__ mn, const double *__restrict__ qD,
                                                          const uint32_t *__restrict__ qflag, uint32_t m, uint32_t m_pad, uint32_t nq,
                                                          uint4 *__restrict__ img) {
    const uint32_t grp = blockIdx.y, g = blockIdx.x, c = threadIdx.x;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (g < m) {
#pragma unroll
        for (int b = 0; b < 16; b++) {
            const uint32_t q = grp * 16 + b;
            if (q < nq && qflag[q] == 0) {
                const double y = (double(lut[(uint64_t(q) * m + g) * 256 + c]) - double(mn[uint64_t(q) * m + g])) / qD[q];
                double x = floor(y);
                x = x < 0.0 ? 0.0 : (x > 255.0 ? 255.0 : x);
                const int j = b & 3, pos = j == 1 ? 2 : (j == 2 ? 1 : j);
                w[b >> 2] |= uint32_t(x) << (8 * pos);
            }
        }
    }
    img[(uint64_t(grp) * m_pad + g) * 256 + c] = make_uint4(w[0], w[1], w[2], w[3]);
}

// 16-B piece per lane from global memory straight into LDS (no register destination): lane l's piece lands at lds_dst + 16 l
__device__ __forceinline__ void pq_glds16(const void *gsrc, uint32_t lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc), "s"(lds_dst)
                 : "memory");
}

// The slices are 16 groups (one code word, 64 KB) in TWO LDS blocks: while a slice is scanned the next one is on its way into the other
// block by LDS-DMA and the rows' next code words into registers -- with one 128-KB block the workgroup stood still for every load (all
// waves at the barrier: ~5 k of ~23 k cycles per slice).
// SAMPLE: the threshold sample on the same image (it was a pass of its own on one-byte tables of ONE query per workgroup, k_pq_adc8<true> +
// k_pq_quant8: 0.97 ms per 1000 queries): a workgroup scores RPT sampled blocks of 1024 rows for its 16 queries and writes the sums.
template <bool SAMPLE>
__global__ __launch_bounds__(1024) void k_pq_adc8x16(Adc16x8Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem816[];
    constexpr uint32_t RPT = ADC8X16_RPT, GS = ADC8X16_GS, BLK = GS * 256 * 16;        // 64 KB per block
    uint32_t *hit_row = reinterpret_cast<uint32_t *>(smem816 + 2 * size_t(BLK));       // [WGBUF]
    uint32_t *hit_q = hit_row + ADC8X16_WGBUF;                                         // [WGBUF] slot | rank << 8
    uint32_t *hit_n = hit_q + ADC8X16_WGBUF;                                           // [0] entries, [1..16] per-slot counts, [17..32] bases
    int32_t *thr = reinterpret_cast<int32_t *>(hit_n + 36);                            // [16] T8 per slot (-1: unused / flagged)
    const uint32_t tid = threadIdx.x, q0 = blockIdx.y * 16, m = a.m, nwords = a.nwords, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // the lookups form LDS byte addresses themselves: the table has to start at LDS address 0 (it does: the kernel has no static LDS);
    // were it ever not so, every query of the group is marked as overflowed and answered by the f32 scan
    typedef uint32_t v4u_t __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) const v4u_t *lds_u4;
    typedef __attribute__((address_space(3))) unsigned char *lds_b;
    if ((uint32_t)(uintptr_t)(lds_b)smem816 != 0u) {
        if (tid < 16 && q0 + tid < a.nq && blockIdx.x == 0) atomicAdd(&a.cnt[q0 + tid], a.cap + 1);
        return;
    }
    if (tid < 33) hit_n[tid] = 0;
    if (!SAMPLE && tid < 16) {
        int32_t T = -1;
        const uint32_t q = q0 + tid;
        if (q < a.nq && a.qflag[q] == 0) {
            const double x = floor((double(a.tau[q]) * (1.0 + 2.0 * double(m) * 0x1p-24) - a.qM[q] * (1.0 - 1e-12)) / a.qD[q]) + 2.0;
            // tau = +inf / NaN: everything passes -> the candidate list overflows and the query takes the f32 scan
            T = !(x < 70000.0) ? 70000 : (x < 0.0 ? -1 : (int32_t)x);
        }
        thr[tid] = T;
    }
    const uint4 *img = a.img + uint64_t(blockIdx.y) * a.nslices * GS * 256;
    // SAMPLE: ONE pass; thread tid's j-th row is row tid of sampled block RPT blockIdx.x + j (block b = rows [b blk_step 1024, + 1024))
    const uint64_t r_begin = SAMPLE ? 0 : uint64_t(blockIdx.x) * a.rows_per_wg;
    const uint64_t r_end = SAMPLE ? 1 : (r_begin + a.rows_per_wg < a.n ? r_begin + a.rows_per_wg : a.n);
    uint32_t four = 4u, blk1 = BLK;
    asm volatile("" : "+s"(four), "+s"(blk1));
    // slice sl -> block bk: 4 DMA instructions per wave (4096 entries of 16 B, wave w moves entries 1024 i + 64 w .. + 63)
    auto dma = [&](uint32_t sl, uint32_t bk) {
        const uint4 *src = img + uint64_t(sl) * GS * 256 + tid;
#pragma unroll
        for (int i = 0; i < 4; i++) pq_glds16(src + i * 1024, bk * BLK + (i * 1024 + wave * 64) * 16);
    };
    for (uint64_t rb = r_begin; rb < r_end; rb += uint64_t(RPT) * 1024) {
        uint32_t acc[RPT][8];
        const uint4 *cw[RPT];
        bool valid[RPT];
        uint4 cnext[RPT];
        __syncthreads();  // (thresholds / counters written; the previous block's readers are done)
        dma(0, 0);
#pragma unroll
        for (int j = 0; j < (int)RPT; j++) {
#pragma unroll
            for (int d = 0; d < 8; d++) acc[j][d] = 0u;
            const uint64_t sblk = uint64_t(blockIdx.x) * RPT + j;
            const uint64_t row = SAMPLE ? sblk * a.blk_step * 1024 + tid : rb + uint64_t(j) * 1024 + tid;
            valid[j] = SAMPLE ? (sblk < a.n_sb && row < a.n) : row < r_end;
            const uint64_t lrow = valid[j] ? row : (SAMPLE ? a.n - 1 : r_end - 1);  // (idle lanes re-read a valid row: see k_pq_adc16)
            cw[j] = a.codes_t + (lrow >> 6) * nwords * 64 + (lrow & 63);
            cnext[j] = cw[j][0];
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        auto slice = [&](uint32_t sl, auto bkc) {
            constexpr uint32_t BK = decltype(bkc)::value;
            uint32_t words[RPT][4];
#pragma unroll
            for (int j = 0; j < (int)RPT; j++) {
                words[j][0] = cnext[j].x;
                words[j][1] = cnext[j].y;
                words[j][2] = cnext[j].z;
                words[j][3] = cnext[j].w;
            }
            if (sl + 1 < a.nslices) {  // the next slice: its entries into the other block, the rows' next code word into registers
                dma(sl + 1, BK ^ 1u);
#pragma unroll
                for (int j = 0; j < (int)RPT; j++) cnext[j] = sl + 1 < nwords ? cw[j][uint64_t(sl + 1) * 64] : make_uint4(0u, 0u, 0u, 0u);
            }
            // entry address = code byte x 16 + group x 4096 (+ 64 KB in block 1): the byte comes out of its word shifted in ONE
            // instruction (SDWA source select), the group part is the immediate offset of the ds_read
            uint4 E[2][4];
            auto issue = [&](int t, uint4 *e) {
                const int j = t >> 2, k = t & 3;
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    uint32_t off;
                    if (b == 0) asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "=v"(off) : "s"(four), "v"(words[j][k]));
                    if (b == 1) asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "=v"(off) : "s"(four), "v"(words[j][k]));
                    if (b == 2) asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2" : "=v"(off) : "s"(four), "v"(words[j][k]));
                    if (b == 3) asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3" : "=v"(off) : "s"(four), "v"(words[j][k]));
                    if (BK) off += blk1;
                    const v4u_t ev = *(lds_u4)(uintptr_t)(off + (4 * k + b) * 4096);
                    e[b] = make_uint4(ev.x, ev.y, ev.z, ev.w);
                }
            };
            issue(0, E[0]);
#pragma unroll
            for (int t = 0; t < 4 * (int)RPT; t++) {
                if (t + 1 < 4 * (int)RPT) {
                    issue(t + 1, E[(t + 1) & 1]);
                    __builtin_amdgcn_sched_barrier(0);  // (the reads of step t + 1 stay above the sums of step t)
                }
                const uint4 *e = E[t & 1];
                const int j = t >> 2;
                const uint32_t x[4][4] = {{e[0].x, e[1].x, e[2].x, e[3].x}, {e[0].y, e[1].y, e[2].y, e[3].y},
                                          {e[0].z, e[1].z, e[2].z, e[3].z}, {e[0].w, e[1].w, e[2].w, e[3].w}};
#pragma unroll
                for (int d = 0; d < 4; d++) {
                    constexpr uint32_t MK = 0x00ff00ffu, SEL = 0x0c030c01u;  // bytes 0, 2 | bytes 1, 3 as 16-bit pairs
                    uint32_t A = acc[j][2 * d], B = acc[j][2 * d + 1];
                    A = A + (x[d][0] & MK) + (x[d][1] & MK);
                    A = A + (x[d][2] & MK) + (x[d][3] & MK);
                    B = B + __builtin_amdgcn_perm(0u, x[d][0], SEL) + __builtin_amdgcn_perm(0u, x[d][1], SEL);
                    B = B + __builtin_amdgcn_perm(0u, x[d][2], SEL) + __builtin_amdgcn_perm(0u, x[d][3], SEL);
                    acc[j][2 * d] = A;
                    acc[j][2 * d + 1] = B;
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the next slice has landed (DMA is not counted by the compiler)
            __syncthreads();                                    // ... for every wave, and this slice's readers are done
        };
        for (uint32_t sl = 0; sl < a.nslices; sl += 2) {
            slice(sl, std::integral_constant<uint32_t, 0>{});
            if (sl + 1 < a.nslices) slice(sl + 1, std::integral_constant<uint32_t, 1>{});
        }
        if constexpr (SAMPLE) {
#pragma unroll
            for (int j = 0; j < (int)RPT; j++) {
                const uint64_t sblk = uint64_t(blockIdx.x) * RPT + j;
                if (sblk >= a.n_sb) continue;  // uniform
#pragma unroll
                for (int b = 0; b < 16; b++) {
                    const uint32_t sb = (b & 1) ? (acc[j][b >> 1] >> 16) : (acc[j][b >> 1] & 0xffffu);
                    if (q0 + b < a.nq) a.s8_out[uint64_t(q0 + b) * a.ld_s + sblk * 1024 + tid] = valid[j] ? float(sb) : INFINITY;
                }
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < (int)RPT; j++) {
            const uint32_t row = uint32_t(rb + uint64_t(j) * 1024 + tid);
#pragma unroll
            for (int b = 0; b < 16; b++) {
                const int32_t sb = int32_t((b & 1) ? (acc[j][b >> 1] >> 16) : (acc[j][b >> 1] & 0xffffu));
                if (valid[j] && sb <= thr[b]) {
                    const uint32_t pos = atomicAdd(hit_n, 1u);
                    if (pos < ADC8X16_WGBUF) {
                        hit_row[pos] = row;
                        hit_q[pos] = b;
                    } else {
                        atomicAdd(&a.cnt[q0 + b], a.cap + 1);  // mark the query as overflowed (-> f32 scan)
                    }
                }
            }
        }
        // hand the block's hits to the per-query candidate lists (one global atomic per query), leave an empty buffer
        __syncthreads();
        uint32_t total = hit_n[0];
        if (total > ADC8X16_WGBUF) total = ADC8X16_WGBUF;
        for (uint32_t i = tid; i < total; i += 1024) {
            const uint32_t r_ = atomicAdd(&hit_n[1 + hit_q[i]], 1u);
            hit_q[i] |= r_ << 8;
        }
        __syncthreads();
        if (tid < 16 && hit_n[1 + tid] > 0) hit_n[17 + tid] = atomicAdd(&a.cnt[q0 + tid], hit_n[1 + tid]);
        __syncthreads();
        for (uint32_t i = tid; i < total; i += 1024) {
            const uint32_t b = hit_q[i] & 0xffu, r_ = hit_q[i] >> 8;
            const uint32_t slot = hit_n[17 + b] + r_;
            if (slot < a.cap) a.cand[uint64_t(q0 + b) * a.cap + slot] = hit_row[i];
        }
        __syncthreads();
        if (tid < 33) hit_n[tid] = 0;
    }
}

// exact f32 ADC sums of the candidates of an 8-bit table, strict group order (pq_table.rs:254-292).  Row ids in, pair keys out
// (PAIR_NONE above tau).  One workgroup per query, a candidate per thread: the query's f32 table (327 KB at m = 320) passes through LDS in
// slices of 32 groups, loaded with coalesced 16-B reads, and every thread adds its candidate's 32 entries of the slice to its running sum
// -- the order of the adds is the group order.  (Reading the table in place cost a 64-B sector per 4-B entry, from L2 / the Infinity
// Cache once some thirty queries' tables were in use per XCD: 1.97 ms per 1000 queries for ~1000 candidates each; code bytes one at a
// time from the row-major codes were 320 more loads per candidate.)  The code bytes come as 16-B words from the word-major mirror.
constexpr uint32_t EXACT8_GS = 32;  // groups per slice: 32 KB of LDS
constexpr uint32_t EXACT8_CPT = 4;  // candidates per thread and pass over the table
// ROWMAJOR: the 32 code bytes of a slice are two 16-B words of the row-major code row (enc_dim % 16 == 0: aligned); otherwise they come
// from the word-major mirror, whose 16-B words of one row lie 1 KB apart (a 64-B sector each: 4x the bytes)
template <bool ROWMAJOR>
__global__ __launch_bounds__(1024) void k_pq_adc_exact8(const uint8_t *__restrict__ codes, uint32_t enc_dim, const uint4 *__restrict__ codes_t, uint32_t nwords,
                                                        uint32_t m, const float *__restrict__ lut, const float *__restrict__ tau, uint64_t *__restrict__ cand,
                                                        const uint32_t *__restrict__ cnt, uint32_t cap, uint32_t *__restrict__ valid) {
    __shared__ __attribute__((aligned(16))) float tab[EXACT8_GS * 256];
    constexpr int CPT = (int)EXACT8_CPT;
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t total = cnt[q];
    if (total > cap || total == 0) return;  // overflowed list: the query is redone by the f32 scan
    const float *lq = lut + uint64_t(q) * m * 256;
    const float t = tau[q];
    uint64_t *cq = cand + uint64_t(q) * cap;
    uint32_t kept = 0;
    for (uint32_t base = 0; base < total; base += CPT * 1024) {
        uint32_t row[CPT];
        const uint4 *cw[CPT];
        float sum[CPT];
#pragma unroll
        for (int c = 0; c < CPT; c++) {
            const uint32_t i = base + c * 1024 + tid;
            row[c] = uint32_t(cq[i < total ? i : base]);
            cw[c] = ROWMAJOR ? reinterpret_cast<const uint4 *>(codes + uint64_t(row[c]) * enc_dim)
                             : codes_t + uint64_t(row[c] >> 6) * nwords * 64 + (row[c] & 63);
            sum[c] = 0.0f;
        }
        const uint32_t nlive = total - base < CPT * 1024 ? total - base : CPT * 1024;  // candidates of this pass
        for (uint32_t g0 = 0; g0 < m; g0 += EXACT8_GS) {
            const uint32_t ng = m - g0 < EXACT8_GS ? m - g0 : EXACT8_GS;
            __syncthreads();  // the previous slice's readers are done
            {
                const float4 *src = reinterpret_cast<const float4 *>(lq + uint64_t(g0) * 256);
                for (uint32_t e = tid; e < ng * 64; e += 1024) reinterpret_cast<float4 *>(tab)[e] = src[e];
            }
            const uint32_t w0 = g0 / 16;
            uint4 c0[CPT], c1[CPT];
#pragma unroll
            for (int c = 0; c < CPT; c++) {
                if (uint32_t(c) * 1024 < nlive) {  // (uniform: whole candidate ranks past the list are skipped)
                    c0[c] = cw[c][ROWMAJOR ? uint64_t(w0) : uint64_t(w0) * 64];
                    c1[c] = w0 + 1 < nwords ? cw[c][ROWMAJOR ? uint64_t(w0 + 1) : uint64_t(w0 + 1) * 64] : make_uint4(0u, 0u, 0u, 0u);
                }
            }
            __syncthreads();
#pragma unroll
            for (int c = 0; c < CPT; c++) {
                if (uint32_t(c) * 1024 >= nlive) continue;
                const uint32_t cc[8] = {c0[c].x, c0[c].y, c0[c].z, c0[c].w, c1[c].x, c1[c].y, c1[c].z, c1[c].w};
                float sm = sum[c];
                if (ng == EXACT8_GS) {
                    float e[EXACT8_GS];
#pragma unroll
                    for (int j = 0; j < (int)EXACT8_GS; j++) e[j] = tab[j * 256 + ((cc[j >> 2] >> (8 * (j & 3))) & 0xffu)];
#pragma unroll
                    for (int j = 0; j < (int)EXACT8_GS; j++) sm = sm + e[j];
                } else {
#pragma unroll
                    for (int j = 0; j < (int)EXACT8_GS; j++)
                        if ((uint32_t)j < ng) sm = sm + tab[j * 256 + ((cc[j >> 2] >> (8 * (j & 3))) & 0xffu)];
                }
                sum[c] = sm;
            }
        }
#pragma unroll
        for (int c = 0; c < CPT; c++) {
            const uint32_t i = base + c * 1024 + tid;
            const bool live = i < total, keep = live && sum[c] <= t;
            if (live) cq[i] = keep ? pair_key(sum[c], row[c]) : PAIR_NONE;
            kept += keep ? 1u : 0u;
        }
    }
    if (kept) atomicAdd(&valid[q], kept);
}

// ---------------------------------------------------------------------------------------------------
// ResultSet::pq_resort (candidate_pair.rs:102-108): replay `add` over the candidates in ADC order.
// `add` admits a pair when the set is not full, or when its DISTANCE is strictly smaller than the worst
// distance (candidate_pair.rs:61-74) -- not the lexicographic test -- so ties at the cut keep the
// earlier-in-ADC-order pair.  One wave per query keeps the set as a sorted register list.
// ---------------------------------------------------------------------------------------------------
template <int R>
__global__ __launch_bounds__(64) void k_pq_resort(const uint64_t *__restrict__ exact_keys, uint32_t ncand,
                                                  uint32_t ldc, uint32_t k, uint64_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t q = blockIdx.x;
    uint64_t v[R];
#pragma unroll
    for (int r = 0; r < R; r++) v[r] = PAIR_NONE;
    uint64_t tau = PAIR_NONE;
    // the replay is serial, the loads are not: one coalesced load fetches the next 64 keys (lane = position), the
    // offers then take them lane by lane (ncand runs into the thousands for IVF probe lists)
    for (uint32_t j0 = 0; j0 < ncand; j0 += 64) {
      const uint64_t mine = j0 + lane < ncand ? exact_keys[uint64_t(q) * ldc + j0 + lane] : PAIR_NONE;
      if (__ballot(mine != PAIR_NONE) == 0) continue;
      // only lanes whose distance beats the current worst can be admitted (tau only tightens): visit those, in offer order
      // (a serial pass over all 64 lanes cost 1.07 ms per 1000 queries x ~4000 IVF candidates)
      uint64_t todo = __ballot(mine != PAIR_NONE && uint32_t(mine >> 32) < uint32_t(tau >> 32));
      while (todo) {
        const uint32_t jj = (uint32_t)__builtin_ctzll(todo);
        todo &= todo - 1;
        uint64_t e = __shfl(mine, jj);  // wave-uniform
        if (uint32_t(e >> 32) >= uint32_t(tau >> 32)) continue;  // full and not strictly closer (tau moved since the ballot)
        bool placed = false;
#pragma unroll
        for (int r = 0; r < R; r++) {
            uint64_t cur = v[r];
            uint64_t mask = placed ? ~0ull : __ballot(cur > e);
            if (mask != 0) {
                uint32_t pos = placed ? 0u : (uint32_t)__builtin_ctzll(mask);
                uint64_t carry = __shfl(cur, 63);
                uint64_t up = __shfl_up(cur, 1);
                v[r] = lane < pos ? cur : (lane == pos ? e : up);
                e = carry;
                placed = true;
            }
        }
        uint32_t p = k - 1;
        uint64_t t = PAIR_NONE;
#pragma unroll
        for (int r = 0; r < R; r++)
            if ((p >> 6) == (uint32_t)r) t = __shfl(v[r], p & 63);
        tau = t;
      }
    }
#pragma unroll
    for (int r = 0; r < R; r++) out[uint64_t(q) * (64 * R) + r * 64 + lane] = v[r];
}

// ---------------------------------------------------------------------------------------------------
// pq_encode (pq_table.rs:66-91) + find_nearest_base (k_means.rs:40-57): per group the centroid with the
// smallest (distance, index) under the CandidatePair order; one thread per row.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool pair_less(float da, uint32_t ia, float db, uint32_t ib) {
    uint32_t oa = f32_orderable(da), ob = f32_orderable(db);
    return oa != ob ? oa < ob : ia < ib;
}

__global__ __launch_bounds__(256) void k_pq_encode(const float *__restrict__ X, uint64_t n, uint32_t dim,
                                                   const float *__restrict__ cent,
                                                   const float *__restrict__ cent_sq,
                                                   const uint64_t *__restrict__ gstart, uint32_t m, uint32_t kc,
                                                   uint32_t n_bits, int cosine, uint32_t enc_dim,
                                                   uint8_t *__restrict__ codes) {
    uint64_t row = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (row >= n) return;
    const float *x = X + row * dim;
    uint8_t *dst = codes + row * enc_dim;
    uint32_t pending = 0;
    for (uint32_t g = 0; g < m; g++) {
        uint32_t s = (uint32_t)gstart[g], gd = (uint32_t)gstart[g + 1] - s;
        const float *v = x + s;
        const float *cg = cent + uint64_t(kc) * s;
        float vnorm = 0.0f;
        if (cosine) {  // cosine_distance recomputes vec_norm(a) per pair (distance/mod.rs:60-64); same value every time
            float a = 0.0f;
            for (uint32_t j = 0; j < gd; j++) {
                float p = v[j] * v[j];
                a = a + p;
            }
            vnorm = sqrtf(a);
        }
        uint32_t best = 0;
        float bd = 0.0f;
        for (uint32_t c = 0; c < kc; c++) {
            const float *cc = cg + uint64_t(c) * gd;
            float acc = 0.0f;
            float d;
            if (cosine) {
                for (uint32_t j = 0; j < gd; j++) {
                    float p = v[j] * cc[j];
                    acc = acc + p;
                }
                float den = fmaxf(vnorm * sqrtf(cent_sq[g * kc + c]), 1e-10f);
                float r = acc / den;
                d = 1.0f - r;
            } else {
                for (uint32_t j = 0; j < gd; j++) {
                    float df = v[j] - cc[j];
                    float sq = df * df;
                    acc = acc + sq;
                }
                d = acc;
            }
            if (c == 0 || pair_less(d, c, bd, best)) {
                bd = d;
                best = c;
            }
        }
        if (n_bits == 4) {
            if ((g & 1) == 0) {
                pending = best;
                if (g == m - 1) dst[g / 2] = (uint8_t)pending;  // odd m: last byte holds one code
            } else {
                dst[g / 2] = (uint8_t)(pending | (best << 4));
            }
        } else {
            dst[g] = (uint8_t)best;
        }
    }
}

// tau[q] = M + D (s* + m/2) from the r-th smallest quantised sample sum s* (in tau[q] on entry); a flagged table (not
// quantisable) gets +inf: its list overflows and the query takes the f32 scan, as without the sample
__global__ void k_pq_tau_from16(float *__restrict__ tau, const double *__restrict__ qM, const double *__restrict__ qD,
                                const uint32_t *__restrict__ qflag, uint32_t m, uint32_t nq) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const float s = tau[q];
    tau[q] = (qflag[q] != 0 || !(s < 1.0e9f)) ? INFINITY : float(qM[q] + qD[q] * (double(s) + 0.5 * double(m)));
}

// ---------------------------------------------------------------------------------------------------
// Row-sharded PQ-Flat.  pq_resort replays the candidates in GLOBAL (ADC, id) order, so a shard cannot
// finish the re-sort alone.  Each shard exports its own ADC top-max(ef,k) as two key rows per query, both carrying
// the GLOBAL row id in the low word: the ADC key (sorted ascending) and, at the same position, the exact-distance
// key.  After one all-gather every rank merges the S sorted rows by ADC key, keeps the first max(ef,k), and replays
// ResultSet::add over the exact keys in that order -- the same operand sequence the unsharded scan produces,
// because the global ADC top-ef is contained in the union of the per-shard ADC top-ef lists.
// ---------------------------------------------------------------------------------------------------
__global__ void k_pq_export_keys(const uint64_t *__restrict__ adc, const uint64_t *__restrict__ exact, uint32_t ld,
                                 uint32_t efk_local, uint32_t efk_out, uint64_t id_offset,
                                 uint64_t *__restrict__ out_adc, uint64_t *__restrict__ out_exact) {
    const uint32_t q = blockIdx.x;
    for (uint32_t j = threadIdx.x; j < efk_out; j += blockDim.x) {
        uint64_t a = PAIR_NONE, e = PAIR_NONE;
        if (j < efk_local) {
            a = adc[uint64_t(q) * ld + j];
            e = exact[uint64_t(q) * ld + j];
            if (a != PAIR_NONE) {
                a += id_offset;  // local row < 2^32 - id_offset (checked by the launcher): no carry into the distance
                e += id_offset;
            } else {
                e = PAIR_NONE;
            }
        }
        out_adc[uint64_t(q) * efk_out + j] = a;
        out_exact[uint64_t(q) * efk_out + j] = e;
    }
}

// merge of S per-shard rows: an entry's position in the merged order is the number of entries with a smaller ADC key
// (keys are unique: global ids), found by one binary search per shard row.
__global__ __launch_bounds__(256) void k_pq_shard_merge(const uint64_t *__restrict__ adc,
                                                        const uint64_t *__restrict__ exact, uint32_t n_shards,
                                                        uint32_t nq, uint32_t efg, uint64_t *__restrict__ merged) {
    const uint32_t q = blockIdx.x;
    for (uint32_t j = threadIdx.x; j < efg; j += blockDim.x) merged[uint64_t(q) * efg + j] = PAIR_NONE;
    __syncthreads();
    const uint32_t total = n_shards * efg;
    for (uint32_t e = threadIdx.x; e < total; e += blockDim.x) {
        const uint32_t sh = e / efg, j = e - sh * efg;
        const uint64_t key = adc[(uint64_t(sh) * nq + q) * efg + j];
        if (key == PAIR_NONE) continue;
        uint32_t rank = j;  // entries of the own (sorted) row before this one
        for (uint32_t t = 0; t < n_shards && rank < efg; t++) {
            if (t == sh) continue;
            const uint64_t *row = adc + (uint64_t(t) * nq + q) * efg;
            uint32_t lo = 0, hi = efg;
            while (lo < hi) {  // first position with row[pos] >= key (PAIR_NONE pads the tail)
                uint32_t mid = (lo + hi) >> 1;
                if (row[mid] < key) lo = mid + 1;
                else hi = mid;
            }
            rank += lo;
        }
        if (rank < efg) merged[uint64_t(q) * efg + rank] = exact[(uint64_t(sh) * nq + q) * efg + j];
    }
}

// ===================================================================================================
// launchers
// ===================================================================================================
constexpr int PQ_MAX_LDS = 160 * 1024;

void launch_pq_lut(const float *Q, uint32_t dim, const float *cent, const uint64_t *gstart, uint32_t m, uint32_t kc, int cosine, uint32_t nq,
                   float *lut, hipStream_t s) {
    hipLaunchKernelGGL(k_pq_lut, dim3((m * kc + 255) / 256, nq), dim3(256), 0, s, Q, dim, cent, gstart, m, kc, cosine, lut);
}

void launch_pq_encode(const float *X, uint64_t n, uint32_t dim, const float *cent, const float *cent_cache, const uint64_t *gstart, uint32_t m,
                      uint32_t kc, uint32_t n_bits, int cosine, uint32_t enc_dim, uint8_t *codes, hipStream_t s) {
    hipLaunchKernelGGL(k_pq_encode, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, X, n, dim, cent, cent_cache, gstart, m, kc, n_bits, cosine,
                       enc_dim, codes);
}

void launch_pq_tile_codes(const uint8_t *codes, uint64_t n, uint32_t enc_dim, uint32_t nwords, uint4 *tiled, hipStream_t s) {
    const uint64_t total = (n + 63) / 64 * 64 * nwords;
    hipLaunchKernelGGL(k_pq_tile_codes, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, codes, n, enc_dim, nwords, tiled);
}

void launch_pq_resort(const uint64_t *exact_keys, uint32_t ncand, uint32_t ldc, uint32_t nq, uint32_t k, uint64_t *out, hipStream_t s) {
    uint32_t cap = topk_capacity(k);
    switch (cap / 64) {
        case 1: hipLaunchKernelGGL((k_pq_resort<1>), dim3(nq), dim3(64), 0, s, exact_keys, ncand, ldc, k, out); break;
        case 2: hipLaunchKernelGGL((k_pq_resort<2>), dim3(nq), dim3(64), 0, s, exact_keys, ncand, ldc, k, out); break;
        case 4: hipLaunchKernelGGL((k_pq_resort<4>), dim3(nq), dim3(64), 0, s, exact_keys, ncand, ldc, k, out); break;
        case 8: hipLaunchKernelGGL((k_pq_resort<8>), dim3(nq), dim3(64), 0, s, exact_keys, ncand, ldc, k, out); break;
        case 16: hipLaunchKernelGGL((k_pq_resort<16>), dim3(nq), dim3(64), 0, s, exact_keys, ncand, ldc, k, out); break;
        default: throw Error(1, "pq_resort: k must be <= 1024");
    }
}

// ---- k_pq_adc ----
AdcPlan pq_adc_plan(size_t lut_bytes, bool cosine) {
    constexpr size_t fit = 120 * 1024;
    const size_t cbytes = cosine ? lut_bytes : 0;
    AdcPlan p;
    p.BQ = lut_bytes * 4 + cbytes <= fit ? 4 : (lut_bytes * 2 + cbytes <= fit ? 2 : 1);
    p.in_lds = lut_bytes * p.BQ + cbytes <= fit;
    // LUTs in LDS: one 1024-thread workgroup per CU (16 waves keep the LDS gather pipe busy); else 8 x 256
    p.nt = p.in_lds ? 1024 : 256;
    return p;
}

template <int BQ, int NBITS, int MODE>
static void adc_launch_m(const AdcArgs &a, const AdcPlan &p, size_t lut_bytes, int num_cu, hipStream_t s) {
    const size_t tables = lut_bytes * BQ + (a.cosine ? lut_bytes : 0);
    const size_t lds = (p.in_lds ? ((tables + 15) & ~size_t(15)) : 0) + (MODE == 1 ? ADC_WGBUF * 12 + (1 + 2 * BQ) * 4 + 16 : 0);
    const uint64_t nblk = ((a.n + p.nt - 1) / p.nt + a.blk_step - 1) / a.blk_step;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(nblk, uint64_t(num_cu) * (p.in_lds ? 1 : 8));
    if (grid == 0 || a.nq_total == 0) return;
    dim3 g(grid, (a.nq_total + BQ - 1) / BQ);
    if (p.in_lds) {
        func_max_lds(reinterpret_cast<const void *>(&k_pq_adc<BQ, NBITS, true, MODE>), PQ_MAX_LDS);
        hipLaunchKernelGGL((k_pq_adc<BQ, NBITS, true, MODE>), g, dim3(p.nt), lds, s, a);
    } else {
        hipLaunchKernelGGL((k_pq_adc<BQ, NBITS, false, MODE>), g, dim3(p.nt), lds, s, a);
    }
}

template <int NBITS, int MODE>
static void adc_launch_bq(const AdcArgs &a, int num_cu, hipStream_t s) {
    const size_t lut_bytes = (size_t(a.m) << NBITS) * sizeof(float);
    const AdcPlan p = pq_adc_plan(lut_bytes, a.cosine != 0);
    if (p.BQ == 4) adc_launch_m<4, NBITS, MODE>(a, p, lut_bytes, num_cu, s);
    else if (p.BQ == 2) adc_launch_m<2, NBITS, MODE>(a, p, lut_bytes, num_cu, s);
    else adc_launch_m<1, NBITS, MODE>(a, p, lut_bytes, num_cu, s);
}

void launch_pq_adc(const AdcArgs &a, uint32_t n_bits, int mode, int num_cu, hipStream_t s) {
    if (n_bits == 4) {
        if (mode == 1) adc_launch_bq<4, 1>(a, num_cu, s);
        else adc_launch_bq<4, 0>(a, num_cu, s);
    } else {
        if (mode == 1) adc_launch_bq<8, 1>(a, num_cu, s);
        else adc_launch_bq<8, 0>(a, num_cu, s);
    }
}

// ---- k_pq_quant16 / k_pq_adc16 / k_pq_adc_exact / k_pq_tau_from16 ----
// the image of a query group (32 * nwords groups x 16 entries x 16 B), 128 B of per-query constants, the hit buffer and its counters
size_t pq_adc16_lds_bytes(uint32_t nwords) { return size_t(32 * nwords) * 256 + 128 + ADC16_WGBUF * 8 + (1 + 2 * ADC16_Q) * 4; }

void launch_pq_quant16(const float *lut, const float *cent_cache, uint32_t m, uint32_t m_pad, uint32_t nq, int cosine, uint16_t *img, double *qM,
                       double *qD, double *qMC, double *qDC, uint32_t *qflag, hipStream_t s) {
    hipLaunchKernelGGL(k_pq_quant16, dim3(nq), dim3(256), 0, s, lut, cent_cache, m, m_pad, nq, cosine, img, qM, qD, qMC, qDC, qflag);
}

template <int NW>
static void adc16_launch_nw(const Adc16Args &a, bool cosine, bool sample, dim3 grid, size_t lds, hipStream_t s) {
    void (*const kern)(Adc16Args) = sample ? k_pq_adc16<NW, false, true> : (cosine ? k_pq_adc16<NW, true> : k_pq_adc16<NW, false>);
    func_max_lds(reinterpret_cast<const void *>(kern), PQ_MAX_LDS);
    hipLaunchKernelGGL(kern, grid, dim3(1024), lds, s, a);
}

void launch_pq_adc16(const Adc16Args &a, bool cosine, bool sample, uint32_t nwords, int num_cu, hipStream_t s) {
    const uint32_t ngrp = (a.nq + (cosine ? 7 : 8) - 1) / (cosine ? 7 : 8);
    dim3 grid(1, ngrp);
    if (sample) {
        const uint64_t nblk = (a.n + 1023) / 1024, n_sb = (nblk + a.blk_step - 1) / a.blk_step;
        // one table image per workgroup: as few workgroups per query group as still fill the chip
        grid.x = (uint32_t)std::min<uint64_t>(n_sb, std::max<uint64_t>(1, (uint64_t(num_cu) + ngrp - 1) / ngrp));
    } else {
        grid.x = (uint32_t)((a.n + a.rows_per_wg - 1) / a.rows_per_wg);
    }
    const size_t lds = pq_adc16_lds_bytes(nwords);
    switch (nwords) {  // 32 * nwords groups: 128 / 171 -> 192 (dim 512 / 3) / 256 / 320 (Gist1M, dim / 3) / 342 -> 352 (dim 1024 / 3) / 512
        case 4: adc16_launch_nw<4>(a, cosine, sample, grid, lds, s); break;
        case 6: adc16_launch_nw<6>(a, cosine, sample, grid, lds, s); break;
        case 11: adc16_launch_nw<11>(a, cosine, sample, grid, lds, s); break;
        case 8: adc16_launch_nw<8>(a, cosine, sample, grid, lds, s); break;
        case 10: adc16_launch_nw<10>(a, cosine, sample, grid, lds, s); break;
        case 16: adc16_launch_nw<16>(a, cosine, sample, grid, lds, s); break;
        default: adc16_launch_nw<0>(a, cosine, sample, grid, lds, s); break;
    }
}

void launch_pq_adc_exact(bool cosine, const uint8_t *codes, uint32_t enc_dim, uint32_t m, const float *lut, const float *cent_cache, const float *qsq,
                         const float *tau, uint64_t *cand, const uint32_t *cnt, uint32_t cap, uint32_t *valid, uint32_t nq, hipStream_t s) {
    const size_t table = size_t(m) * 16 * sizeof(float);  // the query's f32 table; Cosine: the |centroid|^2 table behind it
    if (cosine)
        hipLaunchKernelGGL(k_pq_adc_exact<true>, dim3(nq), dim3(256), 2 * table, s, codes, enc_dim, m, lut, cent_cache, qsq, tau, cand, cnt, cap, valid);
    else
        hipLaunchKernelGGL(k_pq_adc_exact<false>, dim3(nq), dim3(256), table, s, codes, enc_dim, m, lut, (const float *)nullptr,
                           (const float *)nullptr, tau, cand, cnt, cap, valid);
}

void launch_pq_tau_from16(float *tau, const double *qM, const double *qD, const uint32_t *qflag, uint32_t m, uint32_t nq, hipStream_t s) {
    hipLaunchKernelGGL(k_pq_tau_from16, dim3((nq + 255) / 256), dim3(256), 0, s, tau, qM, qD, qflag, m, nq);
}

// ---- k_pq_quant8 / k_pq_adc8 ----
// the query's one-byte table (16 * nwords groups x 256 entries), the hit buffer and its counters
size_t pq_adc8_lds_bytes(uint32_t nwords) { return size_t(16 * nwords) * 256 + ADC8_WGBUF * 4 + 16; }

void launch_pq_quant8(const float *lut, uint32_t m, uint32_t m_pad, uint32_t nq, uint8_t *img, double *qM, double *qD, uint32_t *qflag, hipStream_t s) {
    hipLaunchKernelGGL(k_pq_quant8, dim3(nq), dim3(256), 0, s, lut, m, m_pad, nq, img, qM, qD, qflag);
}

void launch_pq_adc8(const Adc8Args &a, bool sample, int num_cu, hipStream_t s) {
    const size_t lds = pq_adc8_lds_bytes(a.nwords);
    if (sample) {
        const uint64_t nblk = (a.n + 1023) / 1024, n_sb = (nblk + a.blk_step - 1) / a.blk_step;
        // every workgroup loads its query's 80-KB table: few workgroups per query, enough of them to fill the chip
        const uint32_t gx = (uint32_t)std::min<uint64_t>(n_sb, std::max<uint64_t>(1, (2ull * num_cu + a.nq - 1) / a.nq));
        func_max_lds(reinterpret_cast<const void *>(&k_pq_adc8<true>), PQ_MAX_LDS);
        hipLaunchKernelGGL(k_pq_adc8<true>, dim3(gx, a.nq), dim3(1024), lds, s, a);
    } else {
        func_max_lds(reinterpret_cast<const void *>(&k_pq_adc8<false>), PQ_MAX_LDS);
        hipLaunchKernelGGL(k_pq_adc8<false>, dim3((uint32_t)((a.n + a.rows_per_wg - 1) / a.rows_per_wg), a.nq), dim3(1024), lds, s, a);
    }
}

// ---- the sliced images: k_pq_quant16x8_stats / _img, k_pq_quant8x16_img, k_pq_adc16x8, k_pq_adc8x16, k_pq_adc_exact8 ----
// one slice of 16-B entries, the hit buffer, its counters and the thresholds of the 8 queries
size_t pq_adc16x8_lds_bytes() { return size_t(ADC16X8_GS) * 256 * 16 + size_t(ADC16X8_WGBUF) * 8 + (20 + 8) * 4 + 16; }
// two blocks of one slice each, the hit buffer, its counters and the thresholds of the 16 queries
size_t pq_adc8x16_lds_bytes() { return 2 * size_t(ADC8X16_GS) * 256 * 16 + size_t(ADC8X16_WGBUF) * 8 + (36 + 16) * 4 + 16; }

void launch_pq_quant_sliced(bool sixteen, const float *lut, uint32_t m, uint32_t m_pad, uint32_t nq, double divisor, float *mn, double *qM, double *qD,
                            uint32_t *qflag, uint4 *img, hipStream_t s) {
    hipLaunchKernelGGL(k_pq_quant16x8_stats, dim3(nq), dim3(256), 0, s, lut, m, nq, mn, qM, qD, qflag, divisor);
    if (sixteen)
        hipLaunchKernelGGL(k_pq_quant8x16_img, dim3(m_pad, (nq + 15) / 16), dim3(256), 0, s, lut, mn, qD, qflag, m, m_pad, nq, img);
    else
        hipLaunchKernelGGL(k_pq_quant16x8_img, dim3(m_pad, (nq + 7) / 8), dim3(256), 0, s, lut, mn, qD, qflag, m, m_pad, nq, img);
}

void launch_pq_adc16x8(const Adc16x8Args &a, hipStream_t s) {
    func_max_lds(reinterpret_cast<const void *>(&k_pq_adc16x8), PQ_MAX_LDS);
    hipLaunchKernelGGL(k_pq_adc16x8, dim3((unsigned)((a.n + a.rows_per_wg - 1) / a.rows_per_wg), (a.nq + 7) / 8), dim3(1024), pq_adc16x8_lds_bytes(), s, a);
}

void launch_pq_adc8x16(const Adc16x8Args &a, bool sample, hipStream_t s) {
    const uint32_t ngrp = (a.nq + 15) / 16;
    if (sample) {
        func_max_lds(reinterpret_cast<const void *>(&k_pq_adc8x16<true>), PQ_MAX_LDS);
        hipLaunchKernelGGL(k_pq_adc8x16<true>, dim3((unsigned)((a.n_sb + ADC8X16_RPT - 1) / ADC8X16_RPT), ngrp), dim3(1024), pq_adc8x16_lds_bytes(), s, a);
    } else {
        func_max_lds(reinterpret_cast<const void *>(&k_pq_adc8x16<false>), PQ_MAX_LDS);
        hipLaunchKernelGGL(k_pq_adc8x16<false>, dim3((unsigned)((a.n + a.rows_per_wg - 1) / a.rows_per_wg), ngrp), dim3(1024), pq_adc8x16_lds_bytes(), s, a);
    }
}

void launch_pq_adc_exact8(const uint8_t *codes, uint32_t enc_dim, const uint4 *codes_t, uint32_t nwords, uint32_t m, const float *lut,
                          const float *tau, uint64_t *cand, const uint32_t *cnt, uint32_t cap, uint32_t *valid, uint32_t nq, hipStream_t s) {
    // (static LDS: one slice of the f32 table)
    void (*const kern)(const uint8_t *, uint32_t, const uint4 *, uint32_t, uint32_t, const float *, const float *, uint64_t *, const uint32_t *, uint32_t,
                       uint32_t *) = enc_dim % 16 == 0 ? k_pq_adc_exact8<true> : k_pq_adc_exact8<false>;
    hipLaunchKernelGGL(kern, dim3(nq), dim3(1024), 0, s, codes, enc_dim, codes_t, nwords, m, lut, tau, cand, cnt, cap, valid);
}

// ---- the shard kernels ----
void launch_pq_export_keys(const uint64_t *adc, const uint64_t *exact, uint32_t ld, uint32_t efk_local, uint32_t efk_out, uint64_t id_offset,
                           uint64_t *out_adc, uint64_t *out_exact, uint32_t nq, hipStream_t s) {
    hipLaunchKernelGGL(k_pq_export_keys, dim3(nq), dim3(256), 0, s, adc, exact, ld, efk_local, efk_out, id_offset, out_adc, out_exact);
}

void launch_pq_shard_merge(const uint64_t *adc, const uint64_t *exact, uint32_t n_shards, uint32_t nq, uint32_t efg, uint64_t *merged, hipStream_t s) {
    hipLaunchKernelGGL(k_pq_shard_merge, dim3(nq), dim3(256), 0, s, adc, exact, n_shards, nq, efg, merged);
}

}  // namespace vdb
