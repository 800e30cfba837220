// k_update.hip -- in-place row update (Index::update_rows): m new rows and their norms scattered into the table in one launch.
#include <algorithm>

#include "kernels.hpp"

namespace vdb {

// Row j of `src` (m contiguous rows of row_bytes bytes) -> row ids[j] of `rows`, sq_new[j] -> sq[ids[j]].  The ids are distinct (the
// update plan checked them, update_plan.hpp) and src is a buffer of its own: no write meets another write or a read, so one launch
// needs no order.  One wave per row at a time, grid-stride over the rows; V = the widest access the row size allows (rows start at
// multiples of row_bytes from 256-B aligned bases).  Offsets in 64 bits: row x bytes passes 2^32.
template <class V>
__global__ __launch_bounds__(256) void k_rows_scatter(char *__restrict__ rows, uint64_t row_bytes, float *__restrict__ sq,
                                                      const uint32_t *__restrict__ ids, const char *__restrict__ src,
                                                      const float *__restrict__ sq_new, uint64_t m) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t waves = uint64_t(gridDim.x) * 4, per_row = row_bytes / sizeof(V);
    for (uint64_t j = uint64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); j < m; j += waves) {
        const uint64_t dst = ids[j];
        const V *from = reinterpret_cast<const V *>(src + j * row_bytes);
        V *to = reinterpret_cast<V *>(rows + dst * row_bytes);
        for (uint64_t e = lane; e < per_row; e += 64) to[e] = from[e];
        if (lane == 0) sq[dst] = sq_new[j];
    }
}

void launch_rows_scatter(void *rows, uint64_t row_bytes, float *sq, const uint32_t *ids, const void *src, const float *sq_new, uint64_t m,
                         int num_cu, hipStream_t s) {
    if (m == 0) return;
    const unsigned grid = (unsigned)std::min<uint64_t>((m + 3) / 4, uint64_t(num_cu) * 8);
    char *r = static_cast<char *>(rows);
    const char *f = static_cast<const char *>(src);
    // (src may be a caller's device pointer: the 16-B form only if it is aligned for it)
    if (row_bytes % 16 == 0 && reinterpret_cast<uintptr_t>(src) % 16 == 0)
        hipLaunchKernelGGL(k_rows_scatter<uint4>, dim3(grid), dim3(256), 0, s, r, row_bytes, sq, ids, f, sq_new, m);
    else if (row_bytes % 4 == 0)
        hipLaunchKernelGGL(k_rows_scatter<uint32_t>, dim3(grid), dim3(256), 0, s, r, row_bytes, sq, ids, f, sq_new, m);
    else
        hipLaunchKernelGGL(k_rows_scatter<uint8_t>, dim3(grid), dim3(256), 0, s, r, row_bytes, sq, ids, f, sq_new, m);
}

}  // namespace vdb
