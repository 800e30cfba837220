// flat_pca.hip -- PCA of an index's own rows (docs/DESIGN_flat.md 4.1ai): Index::flat_covariance_device, the column means and the covariance
// matrix of the allowed rows in f64, and Index::flat_project_device, the rows projected onto a set of components.  The rule is stated once
// in include/vdbhip.h; pca_plan.hpp checks the arguments and lays out blocks, segments and scratch, k_pca.hip holds the kernels.  A call
// is one chain of launches on the workspace's stream and no read-back: the eigen-decomposition of the dim x dim matrix is the caller's
// (VecDB.fit_pca runs it on the host; its cost does not depend on the row count).
#include <string>

#include "index.hpp"

namespace vdb {

void Index::flat_covariance_device(Workspace &ws, bool center, const RowMask *mask, double *d_mean, double *d_cov, uint64_t *out_m) {
    hipStream_t s = ws.stream;
    if (mask) check_mask(*mask);
    const uint64_t m = mask ? mask->m : n;
    const std::string bad = pca_check_cov(n, dim, elem_u8, mask != nullptr, m, center);
    VDB_REQUIRE(bad.empty(), bad);
    const PcaPlan p = pca_plan(m, dim);
    const uint32_t *ids = mask ? mask->d_ids.as<uint32_t>() : nullptr;
    const float *X = d_rows.as<float>();
    DevBuf partial, mean_parts, mean;  // pca_plan's scratch_bytes
    partial.reserve(p.segments * p.blocks * PCA_BLOCK * PCA_BLOCK * sizeof(double));
    mean.reserve(p.dim_pad * sizeof(double));
    const double bytes = double(m) * dim * sizeof(float);
    prof_begin(ws, "pca_mean", center ? bytes : 0.0);
    if (center) {
        mean_parts.reserve(PCA_MEAN_SEGMENTS * p.dim_pad * sizeof(double));
        launch_pca_mean(X, ids, m, (uint32_t)dim, p, mean_parts.as<double>(), mean.as<double>(), s);
    } else {
        VDB_HIP(hipMemsetAsync(mean.p, 0, p.dim_pad * sizeof(double), s));
    }
    prof_end(ws);
    prof_begin(ws, "pca_cov", bytes * double(p.block_cols + 1) / 2.0);  // a row segment is read once per block column pair it feeds
    launch_pca_syrk(X, ids, m, (uint32_t)dim, p, mean.as<double>(), partial.as<double>(), s);
    prof_end(ws);
    prof_begin(ws, "pca_cov_reduce", double(p.segments) * p.blocks * PCA_BLOCK * PCA_BLOCK * sizeof(double));
    launch_pca_cov_reduce(partial.as<double>(), (uint32_t)dim, p, double(m - (center ? 1 : 0)), d_cov, s);
    prof_end(ws);
    VDB_HIP(hipMemcpyAsync(d_mean, mean.p, dim * sizeof(double), hipMemcpyDeviceToDevice, s));
    VDB_SYNC(s);
    *out_m = m;
    pca_cov_calls += 1;
    pca_cov_rows += m;
}

void Index::flat_project_device(Workspace &ws, const RowMask *mask, const float *d_W, uint64_t n_comp, const double *d_mean, float *d_out) {
    hipStream_t s = ws.stream;
    if (mask) check_mask(*mask);
    const uint64_t m = mask ? mask->m : n;
    const std::string bad = pca_check_project(dim, elem_u8, n_comp, dim);
    VDB_REQUIRE(bad.empty(), bad);
    VDB_REQUIRE(n < (1ull << 32), "pca: an index of 2^32 rows or more");
    if (m) {
        prof_begin(ws, "pca_project", double(m) * dim * sizeof(float));
        launch_pca_project(d_rows.as<float>(), mask ? mask->d_ids.as<uint32_t>() : nullptr, m, (uint32_t)dim, d_W, (uint32_t)n_comp, d_mean, d_out, s);
        prof_end(ws);
    }
    VDB_SYNC(s);
    pca_project_calls += 1;
    pca_project_rows += m;
}

}  // namespace vdb
