// k_remove.hip -- bulk row removal (Index::remove_rows): the moves of a removal plan (remove_plan.hpp) applied to the rows and their
// cached norms in one launch.
#include <algorithm>

#include "kernels.hpp"

namespace vdb {

// moves[2 j] = dst, moves[2 j + 1] = src: row src -> row dst of `rows` (row_bytes bytes each) and sq[src] -> sq[dst].  Every src lies
// at or above every dst + 1 (the old tail / the holes below it): no move reads what another writes, so one launch needs no order
// and no second buffer.  One wave per move at a time, grid-stride over the moves; V = the widest access the row size allows
// (rows start at multiples of row_bytes from a 256-B aligned base).  Offsets in 64 bits: row x bytes passes 2^32.
template <class V>
__global__ __launch_bounds__(256) void k_rows_move(char *__restrict__ rows, uint64_t row_bytes, float *__restrict__ sq,
                                                   const uint32_t *__restrict__ moves, uint64_t n_moves) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t waves = uint64_t(gridDim.x) * 4, per_row = row_bytes / sizeof(V);
    for (uint64_t j = uint64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); j < n_moves; j += waves) {
        const uint64_t dst = moves[2 * j], src = moves[2 * j + 1];
        const V *from = reinterpret_cast<const V *>(rows + src * row_bytes);
        V *to = reinterpret_cast<V *>(rows + dst * row_bytes);
        for (uint64_t e = lane; e < per_row; e += 64) to[e] = from[e];
        if (lane == 0) sq[dst] = sq[src];
    }
}

void launch_rows_move(void *rows, uint64_t row_bytes, float *sq, const uint32_t *moves, uint64_t n_moves, int num_cu, hipStream_t s) {
    if (n_moves == 0) return;
    const unsigned grid = (unsigned)std::min<uint64_t>((n_moves + 3) / 4, uint64_t(num_cu) * 8);
    char *r = static_cast<char *>(rows);
    if (row_bytes % 16 == 0)
        hipLaunchKernelGGL(k_rows_move<uint4>, dim3(grid), dim3(256), 0, s, r, row_bytes, sq, moves, n_moves);
    else if (row_bytes % 4 == 0)
        hipLaunchKernelGGL(k_rows_move<uint32_t>, dim3(grid), dim3(256), 0, s, r, row_bytes, sq, moves, n_moves);
    else
        hipLaunchKernelGGL(k_rows_move<uint8_t>, dim3(grid), dim3(256), 0, s, r, row_bytes, sq, moves, n_moves);
}

}  // namespace vdb
