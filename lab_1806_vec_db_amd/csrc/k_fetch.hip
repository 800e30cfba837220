// k_fetch.hip -- bulk row fetch (Index::get_rows*): the rows of an id list gathered into m contiguous output rows, the mirror image of
// k_update.hip's scatter.  Copies only: no LDS, plain loads and stores.
#include <algorithm>

#include "kernels.hpp"

namespace vdb {

// Row ids[j] - id_offset of `rows` (row_bytes bytes each) -> row j of dst (m contiguous rows).  The list only names what is READ: any
// order, repeats allowed, and no output row is written twice, so one launch needs no order.  One wave per output row at a time,
// grid-stride over the rows; V = the widest access the row size and the destination allow (source rows start at multiples of row_bytes
// from a 256-B aligned base, the launcher looks at dst).  Offsets in 64 bits: row x bytes passes 2^32.  The ids were checked by the
// caller (fetch_plan_check on the host, k_fetch_check on the device).
template <class V, class Id>
__global__ __launch_bounds__(256) void k_rows_gather(const char *__restrict__ rows, uint64_t row_bytes, const Id *__restrict__ ids,
                                                     uint64_t id_offset, char *__restrict__ dst, uint64_t m) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t waves = uint64_t(gridDim.x) * 4, per_row = row_bytes / sizeof(V);
    for (uint64_t j = uint64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); j < m; j += waves) {
        const uint64_t src = uint64_t(ids[j]) - id_offset;
        const V *from = reinterpret_cast<const V *>(rows + src * row_bytes);
        V *to = reinterpret_cast<V *>(dst + j * row_bytes);
        for (uint64_t e = lane; e < per_row; e += 64) to[e] = from[e];
    }
}

// The same over u8 rows with f32 output, (float)byte (exact).  The first 4 * nvec elements of a row go four at a time -- one 4-byte
// load, one 16-byte store per lane -- and the rest one by one.  nvec is dim / 4 when dim % 4 == 0 and dst is 16-byte aligned (then every
// source row is 4-byte and every output row 16-byte aligned, and there is no rest), else 0 and the scalar loop takes the whole row.
template <class Id>
__global__ __launch_bounds__(256) void k_rows_gather_widen(const uint8_t *__restrict__ rows, uint64_t dim, uint64_t nvec,
                                                           const Id *__restrict__ ids, uint64_t id_offset, float *__restrict__ dst,
                                                           uint64_t m) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t waves = uint64_t(gridDim.x) * 4;
    for (uint64_t j = uint64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); j < m; j += waves) {
        const uint64_t src = uint64_t(ids[j]) - id_offset;
        const uint8_t *from = rows + src * dim;
        float *to = dst + j * dim;
        for (uint64_t e = lane; e < nvec; e += 64) {
            const uint32_t w = reinterpret_cast<const uint32_t *>(from)[e];
            reinterpret_cast<float4 *>(to)[e] =
                make_float4(float(w & 0xFFu), float((w >> 8) & 0xFFu), float((w >> 16) & 0xFFu), float(w >> 24));
        }
        for (uint64_t e = nvec * 4 + lane; e < dim; e += 64) to[e] = float(from[e]);
    }
}

// flag |= some ids[j] - id_offset is not in [0, n), before anything is gathered
__global__ __launch_bounds__(256) void k_fetch_check(const uint64_t *__restrict__ ids, uint64_t m, uint64_t n, uint64_t id_offset,
                                                     uint32_t *__restrict__ flag) {
    bool bad = false;
    for (uint64_t p = uint64_t(blockIdx.x) * 256 + threadIdx.x; p < m; p += uint64_t(gridDim.x) * 256) {
        const uint64_t id = ids[p];
        bad |= id < id_offset || id - id_offset >= n;
    }
    if (bad) *flag = 1;  // (every writer stores the same value)
}

// the same for the counted part ids[b][0 .. min(counts[b], ld)) of every list b of an [..][ld] block (blockIdx.y = b): what the list forms of the
// Flat re-rankers check before anything is walked (flat_rerank.hip)
__global__ __launch_bounds__(256) void k_list_check(const uint64_t *__restrict__ ids, const uint64_t *__restrict__ counts, uint64_t ld,
                                                    uint64_t n, uint64_t id_offset, uint32_t *__restrict__ flag) {
    const uint64_t b = blockIdx.y;
    const uint64_t cnt = counts[b] < ld ? counts[b] : ld;
    bool bad = false;
    for (uint64_t p = uint64_t(blockIdx.x) * 256 + threadIdx.x; p < cnt; p += uint64_t(gridDim.x) * 256) {
        const uint64_t id = ids[b * ld + p];
        bad |= id < id_offset || id - id_offset >= n;
    }
    if (bad) *flag = 1;  // (every writer stores the same value)
}

static unsigned fetch_grid(uint64_t m, int num_cu) { return (unsigned)std::min<uint64_t>((m + 3) / 4, uint64_t(std::max(num_cu, 1)) * 8); }

template <class Id>
static void rows_gather_any(const char *rows, uint64_t row_bytes, const Id *ids, uint64_t id_offset, char *dst, uint64_t m, int num_cu,
                            hipStream_t s) {
    const unsigned grid = fetch_grid(m, num_cu);
    // (dst may be a caller's device pointer: the 16-B form only if it is aligned for it)
    if (row_bytes % 16 == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0 && reinterpret_cast<uintptr_t>(rows) % 16 == 0)
        hipLaunchKernelGGL((k_rows_gather<uint4, Id>), dim3(grid), dim3(256), 0, s, rows, row_bytes, ids, id_offset, dst, m);
    else if (row_bytes % 4 == 0 && reinterpret_cast<uintptr_t>(dst) % 4 == 0)
        hipLaunchKernelGGL((k_rows_gather<uint32_t, Id>), dim3(grid), dim3(256), 0, s, rows, row_bytes, ids, id_offset, dst, m);
    else
        hipLaunchKernelGGL((k_rows_gather<uint8_t, Id>), dim3(grid), dim3(256), 0, s, rows, row_bytes, ids, id_offset, dst, m);
}

void launch_rows_gather(const void *rows, uint64_t row_bytes, const void *ids, bool ids_u64, uint64_t id_offset, void *dst, uint64_t m,
                        int num_cu, hipStream_t s) {
    if (m == 0 || row_bytes == 0) return;
    const char *r = static_cast<const char *>(rows);
    char *d = static_cast<char *>(dst);
    if (ids_u64)
        rows_gather_any(r, row_bytes, static_cast<const uint64_t *>(ids), id_offset, d, m, num_cu, s);
    else
        rows_gather_any(r, row_bytes, static_cast<const uint32_t *>(ids), id_offset, d, m, num_cu, s);
}

void launch_rows_gather_widen(const uint8_t *rows, uint64_t dim, const void *ids, bool ids_u64, uint64_t id_offset, float *dst, uint64_t m,
                              int num_cu, hipStream_t s) {
    if (m == 0 || dim == 0) return;
    const unsigned grid = fetch_grid(m, num_cu);
    const bool vec = dim % 4 == 0 && reinterpret_cast<uintptr_t>(dst) % 16 == 0 && reinterpret_cast<uintptr_t>(rows) % 4 == 0;
    const uint64_t nvec = vec ? dim / 4 : 0;
    if (ids_u64)
        hipLaunchKernelGGL(k_rows_gather_widen<uint64_t>, dim3(grid), dim3(256), 0, s, rows, dim, nvec, static_cast<const uint64_t *>(ids),
                           id_offset, dst, m);
    else
        hipLaunchKernelGGL(k_rows_gather_widen<uint32_t>, dim3(grid), dim3(256), 0, s, rows, dim, nvec, static_cast<const uint32_t *>(ids),
                           id_offset, dst, m);
}

void launch_fetch_check(const uint64_t *ids, uint64_t m, uint64_t n, uint64_t id_offset, uint32_t *flag, int num_cu, hipStream_t s) {
    if (m == 0) return;
    const unsigned grid = (unsigned)std::min<uint64_t>((m + 255) / 256, uint64_t(std::max(num_cu, 1)) * 8);
    hipLaunchKernelGGL(k_fetch_check, dim3(grid), dim3(256), 0, s, ids, m, n, id_offset, flag);
}

void launch_list_check(const uint64_t *ids, const uint64_t *counts, uint64_t nq, uint64_t ld, uint64_t n, uint64_t id_offset, uint32_t *flag,
                       hipStream_t s) {
    if (nq == 0 || ld == 0) return;
    const unsigned gx = (unsigned)std::min<uint64_t>((ld + 255) / 256, 64);
    for (uint64_t q0 = 0; q0 < nq; q0 += 32768) {  // (grid.y)
        const uint64_t nb = std::min<uint64_t>(32768, nq - q0);
        hipLaunchKernelGGL(k_list_check, dim3(gx, (unsigned)nb), dim3(256), 0, s, ids + q0 * ld, counts + q0, ld, n, id_offset, flag);
    }
}

}  // namespace vdb
