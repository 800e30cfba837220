// kmeans_plan.hpp -- the host part of the k-means clustering of an index's rows (Index::flat_kmeans_device / Index::kmeans_assign_device,
// flat_kmeans.hip, k_kmeans.hip; docs/DESIGN_flat.md 4.1ad): the argument check, the tile and scratch layout of one Lloyd iteration, the
// segment rule of the centroid update and THE error bound E that decides which rows the matrix pass may settle.  No HIP and no other
// header of the library; the bound is also compiled for the device (k_kmeans.hip evaluates it per row).
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>

#if defined(__HIPCC__)
#define KM_HD __host__ __device__
#else
#define KM_HD
#endif

namespace vdb {

constexpr uint32_t KM_ROW_TILE = 128;        // rows a workgroup of k_kmeans_assign owns (4 waves x 2 MFMA column blocks of 16 rows)
constexpr uint32_t KM_CENT_TILE = 64;        // centroids streamed past the row tile per step (4 MFMA row blocks of 16)
constexpr uint32_t KM_KBLOCK = 32;           // dimensions per MFMA (v_mfma_f32_16x16x32_bf16): dims are zero-padded to it in LDS
constexpr uint64_t KM_MAX_CLUSTERS = 65535;  // cluster ids are sorted as two 8-bit digits
constexpr uint64_t KM_MAX_DIM = 8192;        // the resolve kernel stages one row in LDS
constexpr uint32_t KM_SEGMENTS = 16;         // waves of an update workgroup: a cluster's members are folded in 16 segments
constexpr uint32_t KM_LABEL_NONE = 0xFFFFFFFFu;  // assign[] of a row outside the mask (= VDB_LABEL_NONE)
constexpr uint32_t KM_ORDER_CHUNK = 4096;    // positions per workgroup of the counting sort's passes
constexpr uint32_t KM_REDUCE_CHUNK = 4096;   // positions per workgroup of the inertia reduction
constexpr uint64_t KM_SEED_PER_CLUSTER = 64; // seeding looks at min(m, 64 c) rows
constexpr uint64_t KM_COUNTERS = 4;          // unsure rows | rows that changed cluster | inertia (f64 bits) | max centroid |c|^2 (f32 bits)

struct KmeansPlan {
    uint64_t row_tiles = 0;      // workgroups of the matrix pass: ceil(m / 128)
    uint64_t cent_tiles = 0;     // centroid tiles each streams: ceil(c / 64)
    uint64_t k_blocks = 0;       // MFMA k-blocks per product: ceil(dim / 32)
    uint64_t plane_bytes = 0;    // split-bf16 centroid planes in fragment order: cent_tiles x k_blocks x 8 KB
    uint64_t order_blocks = 0;   // workgroups of a counting-sort pass: ceil(m / 4096)
    uint64_t order_passes = 0;   // 8-bit digits of a cluster id: 1 up to 256 clusters, else 2
    uint64_t scratch_bytes = 0;  // device bytes of one call besides its outputs
};

// Everything vdb_flat_kmeans / vdb_kmeans_assign_device refuse that is no property of the index's state: "" when accepted
inline std::string kmeans_check_args(uint64_t n_rows, uint64_t dim, bool elem_u8, bool masked, uint64_t m, uint64_t c) {
    if (elem_u8) return "kmeans: needs f32 rows (a u8 index is not clustered)";
    if (dim < 1 || dim > KM_MAX_DIM) return "kmeans: dim must be in 1 .. 8192";
    if (n_rows >= (1ull << 32)) return "kmeans: an index of 2^32 rows or more";
    if (masked ? m > n_rows : m != n_rows) return "kmeans: " + std::to_string(m) + " allowed rows, the index holds " + std::to_string(n_rows);
    if (c == 0) return "kmeans: no clusters asked for (c = 0)";
    if (c > KM_MAX_CLUSTERS) return "kmeans: more than 65535 clusters";
    return "";
}
// what the Lloyd loop refuses on top (the assignment step alone accepts more centroids than rows)
inline std::string kmeans_check_fit(uint64_t m, uint64_t c) {
    if (c > m) return "kmeans: " + std::to_string(c) + " clusters for " + std::to_string(m) + " rows";
    return "";
}

// the plan of CHECKED arguments
inline KmeansPlan kmeans_plan(uint64_t n_rows, uint64_t dim, uint64_t m, uint64_t c) {
    KmeansPlan p;
    p.row_tiles = (m + KM_ROW_TILE - 1) / KM_ROW_TILE;
    p.cent_tiles = (c + KM_CENT_TILE - 1) / KM_CENT_TILE;
    p.k_blocks = (dim + KM_KBLOCK - 1) / KM_KBLOCK;
    p.plane_bytes = p.cent_tiles * p.k_blocks * (KM_CENT_TILE * KM_KBLOCK * 4);
    p.order_blocks = (m + KM_ORDER_CHUNK - 1) / KM_ORDER_CHUNK;
    p.order_passes = c <= 256 ? 1 : 2;
    const uint64_t m1 = std::max<uint64_t>(m, 1);
    p.scratch_bytes = p.plane_bytes + p.cent_tiles * KM_CENT_TILE * sizeof(float)  // planes, |c|^2
                      + c * dim * sizeof(float)                                     // the centroids of the iteration
                      + m1 * sizeof(uint32_t)                                       // the unsure list
                      + std::max<uint64_t>(n_rows, 1) * sizeof(uint32_t)            // the previous assignment
                      + (2 * c + 1) * sizeof(uint32_t)                              // member counts and offsets
                      + 2 * m1 * sizeof(uint32_t)                                   // the two position lists of the sort
                      + 256 * std::max<uint64_t>(p.order_blocks, 1) * sizeof(uint32_t)  // digit histograms
                      + std::max<uint64_t>((m + KM_REDUCE_CHUNK - 1) / KM_REDUCE_CHUNK, 1) * sizeof(double) + KM_COUNTERS * sizeof(uint64_t);
    return p;
}

// segment s (0 .. 15) of a cluster of `count` members covers members [first, first + len) of its ascending list: a function of the count alone
inline KM_HD void kmeans_segment(uint32_t count, uint32_t s, uint32_t &first, uint32_t &len) {
    const uint32_t per = count / KM_SEGMENTS + (count % KM_SEGMENTS != 0);
    first = s * per < count ? s * per : count;
    len = count - first < per ? count - first : per;
}

// ---- E: a row is settled by the matrix pass when (second best score) - (best score) > E -------------------------------------------
// u = 2^-24.  kappa bounds |a - <x, c>| / (|x| |c|) of the split-bf16 product a: the three dropped terms of (xh + xl + ex)(ch + cl + ec),
// each factor's residue below 2^-16 of it (round to nearest twice), together below 2^-14; and the f32 accumulation of 3 x dim_pad
// products, counted at 2^-23 per add because the matrix pipe's adder is not specified to round to nearest.
inline KM_HD float kmeans_kappa(uint32_t dim) {
    const float dim_pad = float((dim + KM_KBLOCK - 1) / KM_KBLOCK * KM_KBLOCK);
    return 1.01f * (6.1035156e-5f + 3.0f * dim_pad * 1.1920929e-7f);
}
// L2Sqr.  score(c) = |c|^2_f - 2 a(c) (the row's own |x|^2 is common to all centroids); xn >= |x|, cn >= every |c|, d_best >= the best
// centroid's score + |x|^2, clamped at 0.  Es bounds |score - (|c|^2 - 2 <x, c>)|: the strict fold of |c|^2 (dim u |c|^2), the product
// (2 kappa |x||c|), the epilogue's rounding (u (|c|^2 + 2 |x||c|)).  The strict f32 fold D_f of the direct form is within g = (dim + 2) u of
// the true distance D, relatively; D_f(c) > D_f(b) follows from D(c) - D(b) > 2 g D(b) / (1 - g).  With D(c) - D(b) >= gap - 2 Es and
// D(b) <= d_best + Es: E = 2 Es + 2.1 g (d_best + Es), and 1 % on top for the roundings of this expression itself.
// Cosine.  score(c) = 1 - a(c) / max(|x|_f |c|_f, 1e-10) with the very norms the exact form divides by, so score and exact distance
// differ by the two numerators alone: |a - dot_f| <= (kappa + dim u) |x||c|, |x||c| <= 1.01 x the denominator, 4 u for each form's
// quotient and difference: E = 2 x 1.02 (kappa + (dim + 8) u), whatever the row.
inline KM_HD float kmeans_err_bound(uint32_t dim, int cosine, float xn, float cn, float d_best) {
    const float u = 5.9604645e-8f, kappa = kmeans_kappa(dim);
    if (cosine) return 2.0f * 1.02f * (kappa + float(dim + 8) * u);
    const float g = float(dim + 2) * u * 1.01f;
    const float es = g * cn * cn + (2.0f * kappa + 3.0f * u) * xn * cn;
    return 1.01f * (2.0f * es + 2.1f * g * (d_best + es));
}

}  // namespace vdb
