// ctx.hpp -- pieces shared by api.hip and ctx.hip: the handle type behind vdb_index, error plumbing, the shard merge.
#pragma once
#include <string>

#include "../../include/vdbhip.h"
#include "index.hpp"

struct vdb_index {
    vdb::Index ix;
    vdb_index(int dev, uint64_t dim, int dist, bool u8 = false) : ix(dev, dim, dist, u8) {}
};

// the result object of the range calls (api.hip: vdb_flat_range, vdb_range_merge_device; ctx.hip: vdb_sharded_flat_range)
struct vdb_range {
    vdb::RangeResult r;
};

// a row allow-list of one index (api.hip: vdb_mask_create; the filtered searches)
struct vdb_mask {
    vdb::RowMask m;
};

namespace vdb {
void set_last_error(const std::string &m);
void require_gpu();  // throws VDB_ERR_NOGPU when no HIP device is usable
// merge of S per-shard result lists on the index's GPU (arrays S x [nq][k], byte strides between shards); returns
// synchronised.  k <= 1024.
void merge_topk_dev(Index &ix, const void *d_dists, const void *d_ids, const void *d_counts, uint64_t stride_d,
                    uint64_t stride_i, uint64_t stride_c, uint64_t n_shards, uint64_t nq, uint64_t k, void *d_out_idx,
                    void *d_out_dist, void *d_out_count, void *stream);
// k_range_merge.hip: merge of S range results.  lims [n_shards][lims_ld] on the host (lims_ld >= nq + 1).
// validate: every lims row starts at 0, never decreases and ends at or below pair_cap -- what keeps the merge inside its buffers
void range_merge_validate(const uint64_t *lims, uint64_t lims_ld, uint64_t n_shards, uint64_t nq, uint64_t pair_cap);
// out_lims [nq + 1]: prefix of min(limit, sum over the shards of the query's count)  (limit 0: no limit)
void range_merge_lims(const uint64_t *lims, uint64_t lims_ld, uint64_t n_shards, uint64_t nq, uint64_t limit, uint64_t *out_lims);
// host merge: lims [n_shards][nq + 1], pairs of shard s at s * pair_stride, out_lims from range_merge_lims
void range_merge_host(const uint64_t *lims, const uint64_t *ids, const float *dists, uint64_t n_shards, uint64_t nq, uint64_t pair_stride,
                      const uint64_t *out_lims, uint64_t *out_idx, float *out_dist);
// device merge on ws.stream (the inputs must be complete): h_lims = the validated host copy of d_lims; ids / distances of shard s start
// stride_i / stride_d BYTES after shard 0's.  Fills `out` on the index's device; returns synchronised.  Throws when the result passes
// Index::range_max_results or cannot be allocated.
void range_merge_dev(Index &ix, Workspace &ws, const uint64_t *h_lims, uint64_t lims_ld, const void *d_lims, const void *d_ids, uint64_t stride_i,
                     const void *d_dists, uint64_t stride_d, uint64_t n_shards, uint64_t nq, uint64_t limit, RangeResult &out);
}  // namespace vdb

#define VDB_API_BEGIN try {
#define VDB_API_END                                   \
    return VDB_OK;                                    \
    }                                                 \
    catch (const vdb::Error &e) {                     \
        vdb::set_last_error(e.what());                \
        return e.code;                                \
    }                                                 \
    catch (const std::exception &e) {                 \
        vdb::set_last_error(e.what());                \
        return VDB_ERR_INVALID;                       \
    }                                                 \
    catch (...) {                                     \
        vdb::set_last_error("unknown error");         \
        return VDB_ERR_INVALID;                       \
    }
