// silhouette_plan.hpp -- the host part of the silhouette scoring of a labelled table (Index::flat_silhouette_device; flat_silhouette.hip,
// k_silhouette.hip; docs/DESIGN_flat.md 4.1aj): the argument checks, which return the refusal text, and the layout of one call -- the
// scored rows in ascending (code, row) order, every cluster's span padded to whole tiles of 64 so that a tile holds one cluster only, the
// row blocks (one per tile), the slices of the dimension, the segments of the mean, the scratch.  Every bound here is a function of the
// cluster sizes and dim alone, never of the device, so the summation order -- and with it every output bit -- is a property of the table.
// No HIP and no other header of the library.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace vdb {

constexpr uint32_t SIL_TILE = 64;            // ordered rows of a column tile AND of a workgroup's row block
constexpr uint32_t SIL_SLICE = 16;           // dimensions staged per step: 4 MFMA k-steps of 4
constexpr uint32_t SIL_STRIDE = 18;          // doubles between two staged rows of a panel [64][16 + 2]: 16 rows x 2 depths hit 32 distinct bank pairs
constexpr uint64_t SIL_MAX_DIM = 2048;       // as for the PCA: the staged slices of one tile pair stay a short loop
constexpr uint32_t SIL_MEAN_SEGMENTS = 256;  // the mean of s(i) is taken in this many runs of ordered slots, whatever m
constexpr uint32_t SIL_LABEL_COLUMNS = 16;   // = LABEL_COLUMNS (kernels.hpp asserts it)
constexpr uint32_t SIL_LABEL_NONE = 0xFFFFFFFFu;  // = LABEL_NONE; also the row id of a padded slot
constexpr uint32_t SIL_EUCLIDEAN = 1;        // = VDB_SIL_EUCLIDEAN

struct SilPlan {
    uint64_t m = 0;              // scored rows
    uint64_t clusters = 0;       // C
    uint64_t padded = 0;         // ordered slots: the sum over the clusters of their size rounded up to whole tiles
    uint64_t tiles = 0;          // padded / 64: column tiles = row blocks = workgroups of the pair kernel
    uint64_t slices = 0;         // ceil(dim / 16): staged steps per tile pair
    uint64_t segments = 1;       // the column walk is not split: a workgroup walks every tile
    uint64_t mean_slots = 0;     // ordered slots per mean segment: ceil(padded / 256)
    uint64_t scratch_bytes = 0;  // everything the call holds on the device besides its outputs
    std::vector<uint64_t> first_tile;  // [C + 1]: cluster c owns tiles [first_tile[c], first_tile[c + 1])
};

// Everything vdb_flat_silhouette refuses by its arguments before a row is read: "" when accepted.  col_live: the column was written.
inline std::string sil_check_args(uint64_t n_rows, uint64_t dim, bool elem_u8, bool cosine, uint32_t flags, uint64_t col, bool col_live, bool masked,
                                  uint64_t m_allowed) {
    if (elem_u8) return "silhouette: needs f32 rows (a u8 index is not scored)";
    if (dim < 1 || dim > SIL_MAX_DIM) return "silhouette: dim must be in 1 .. 2048";
    if (n_rows >= (1ull << 32)) return "silhouette: an index of 2^32 rows or more";
    if (flags & ~SIL_EUCLIDEAN) return "silhouette: unknown flags " + std::to_string(flags & ~SIL_EUCLIDEAN);
    if (cosine && (flags & SIL_EUCLIDEAN)) return "silhouette: VDB_SIL_EUCLIDEAN on a Cosine table (the flag takes the root of an L2Sqr distance)";
    if (col >= SIL_LABEL_COLUMNS) return "silhouette: label column " + std::to_string(col) + ", the columns are 0 .. 15";
    if (!col_live) return "silhouette: label column " + std::to_string(col) + " was never written";
    if (masked ? m_allowed > n_rows : m_allowed != n_rows)
        return "silhouette: " + std::to_string(m_allowed) + " allowed rows, the index holds " + std::to_string(n_rows);
    return "";
}
// scikit-learn's condition on the scored rows: 2 <= C <= m - 1
inline std::string sil_check_clusters(uint64_t m, uint64_t clusters) {
    if (clusters < 2 || clusters + 1 > m)
        return "silhouette: " + std::to_string(clusters) + " clusters among " + std::to_string(m) + " scored rows, need 2 .. rows - 1";
    return "";
}

// the layout over the cluster sizes in ascending code order (every size >= 1); candidates: the rows the mask allows (all rows without one)
inline SilPlan sil_plan(const uint64_t *sizes, uint64_t clusters, uint64_t dim, uint64_t candidates) {
    SilPlan p;
    p.clusters = clusters;
    p.first_tile.assign(clusters + 1, 0);
    for (uint64_t c = 0; c < clusters; c++) {
        p.m += sizes[c];
        p.first_tile[c + 1] = p.first_tile[c] + (sizes[c] + SIL_TILE - 1) / SIL_TILE;
    }
    p.tiles = p.first_tile[clusters];
    p.padded = p.tiles * SIL_TILE;
    p.slices = (dim + SIL_SLICE - 1) / SIL_SLICE;
    p.mean_slots = (p.padded + SIL_MEAN_SEGMENTS - 1) / SIL_MEAN_SEGMENTS;
    // code u32 + norm f64 per candidate; candidate u32 + row u32 + norm f64 + own-cluster sum f64 + least other mean f64 + s f64 per slot;
    // cluster u32 per tile; size u32 per cluster
    p.scratch_bytes = candidates * (sizeof(uint32_t) + sizeof(double)) + p.padded * (2 * sizeof(uint32_t) + 4 * sizeof(double)) +
                      p.tiles * sizeof(uint32_t) + clusters * sizeof(uint32_t);
    return p;
}

}  // namespace vdb
