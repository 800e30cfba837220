// pca_plan.hpp -- the host part of the PCA of an index's rows (Index::flat_covariance_device / flat_project_device, project_vectors_device;
// flat_pca.hip, k_pca.hip; docs/DESIGN_flat.md 4.1ai): the argument checks and the layout of one call -- the 64 x 64 blocks on or above the
// diagonal, the row segments of the covariance and of the mean, the staged slice, the scratch.  Every bound here is a function of
// (m, dim) alone, never of the device, so the summation order -- and with it every output bit -- is a property of the table.  No HIP and
// no other header of the library.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>

namespace vdb {

constexpr uint32_t PCA_BLOCK = 64;              // columns (covariance) or rows / components (projection) of a workgroup's panel
constexpr uint32_t PCA_SLICE = 16;              // rows (covariance) or dimensions (projection) staged per step: 4 MFMA k-steps of 4
constexpr uint32_t PCA_COV_STRIDE = 80;         // doubles between two staged rows of a covariance panel [16][64 + 16]: rows r, r + 1 are 128 B apart mod 256
constexpr uint32_t PCA_PROJ_STRIDE = 17;        // doubles between two staged vectors of a projection panel [64][16 + 1]
constexpr uint64_t PCA_MAX_DIM = 2048;          // the dim x dim f64 matrix goes to a host eigen-solver: 32 MB at the limit
constexpr uint64_t PCA_MAX_COMP = 1024;         // components of one projection
constexpr uint32_t PCA_MEAN_SEGMENTS = 1024;    // the column sums are taken in this many row segments, whatever m
constexpr uint64_t PCA_GRID_TARGET = 1024;      // the covariance launches about this many workgroups: the chip four times over
constexpr uint64_t PCA_MIN_SEG_SLICES = 4;      // a covariance segment is at least 64 rows (the only segment may be shorter)

struct PcaPlan {
    uint64_t dim_pad = 0;        // dim rounded up to whole blocks of 64
    uint64_t block_cols = 0;     // b = dim_pad / 64
    uint64_t blocks = 0;         // b (b + 1) / 2: the blocks with bi <= bj
    uint64_t slices = 0;         // ceil(m / 16)
    uint64_t seg_rows = 0;       // rows per covariance segment, a multiple of 16
    uint64_t segments = 0;       // R = ceil(m / seg_rows)
    uint64_t mean_rows = 0;      // rows per mean segment: ceil(m / 1024)
    uint64_t scratch_bytes = 0;  // partial blocks [R][blocks][64][64] f64 + mean partials [1024][dim_pad] f64 + the mean [dim_pad] f64
};

// Everything vdb_flat_covariance refuses that is no property of the index's state: "" when accepted
inline std::string pca_check_cov(uint64_t n_rows, uint64_t dim, bool elem_u8, bool masked, uint64_t m, bool center) {
    if (elem_u8) return "pca: needs f32 rows (a u8 index is not analysed)";
    if (dim < 1 || dim > PCA_MAX_DIM) return "pca: dim must be in 1 .. 2048";
    if (n_rows >= (1ull << 32)) return "pca: an index of 2^32 rows or more";
    if (masked ? m > n_rows : m != n_rows) return "pca: " + std::to_string(m) + " allowed rows, the index holds " + std::to_string(n_rows);
    if (m < (center ? 2u : 1u)) return "pca: a covariance needs at least " + std::to_string(center ? 2 : 1) + " rows, got " + std::to_string(m);
    return "";
}
// the same for a projection of `dim`-dimensional vectors onto W [n_comp][w_dim]
inline std::string pca_check_project(uint64_t dim, bool elem_u8, uint64_t n_comp, uint64_t w_dim) {
    if (elem_u8) return "pca: needs f32 rows (a u8 index is not projected)";
    if (dim < 1 || dim > PCA_MAX_DIM) return "pca: dim must be in 1 .. 2048";
    if (n_comp == 0) return "pca: no components asked for (n_comp = 0)";
    if (n_comp > PCA_MAX_COMP) return "pca: more than 1024 components";
    if (n_comp > dim) return "pca: " + std::to_string(n_comp) + " components of " + std::to_string(dim) + " dimensions";
    if (w_dim != dim) return "pca: component dimension mismatch: vectors have dim " + std::to_string(dim) + ", got " + std::to_string(w_dim);
    return "";
}

// the plan of CHECKED arguments (m >= 1)
inline PcaPlan pca_plan(uint64_t m, uint64_t dim) {
    PcaPlan p;
    p.block_cols = (dim + PCA_BLOCK - 1) / PCA_BLOCK;
    p.dim_pad = p.block_cols * PCA_BLOCK;
    p.blocks = p.block_cols * (p.block_cols + 1) / 2;
    p.slices = (m + PCA_SLICE - 1) / PCA_SLICE;
    const uint64_t want = (PCA_GRID_TARGET + p.blocks - 1) / p.blocks;  // segments that would fill the grid
    const uint64_t per = std::max<uint64_t>((p.slices + want - 1) / want, PCA_MIN_SEG_SLICES);
    p.seg_rows = per * PCA_SLICE;
    p.segments = (p.slices + per - 1) / per;
    p.mean_rows = (m + PCA_MEAN_SEGMENTS - 1) / PCA_MEAN_SEGMENTS;
    p.scratch_bytes = (p.segments * p.blocks * PCA_BLOCK * PCA_BLOCK + (PCA_MEAN_SEGMENTS + 1) * p.dim_pad) * sizeof(double);
    return p;
}

// covariance segment s < R covers the positions [first, first + len) of the ascending allowed rows
inline void pca_segment(const PcaPlan &p, uint64_t m, uint64_t s, uint64_t &first, uint64_t &len) {
    first = std::min(m, s * p.seg_rows);
    len = std::min(m - first, p.seg_rows);
}

}  // namespace vdb
