// comp_uf.hpp -- the device side of the union-find over `parent`, one u32 per row of the table, that k_components.hip (near-duplicate
// groups) and k_dbscan.hip (density clusters) share.  Only a root is ever hooked, and only under a LOWER row: parent[x] <= x always, no
// cycle can form, a row that has stopped being a root never becomes one again, and when every pair has been linked a component has ONE
// root, its lowest row.  Every access another workgroup may race with is an agent-scope relaxed atomic load, store or CAS; a stale value
// read by find is an older ancestor, which is still an ancestor.  Nothing waits for another thread.  Device code only.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace vdb {

#define COMP_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ uint32_t comp_load(uint32_t *p) { return __hip_atomic_load(p, COMP_RLX); }

// the root of x, halving the path on the way: every other row of it is pointed at its grandparent
__device__ __forceinline__ uint32_t comp_find(uint32_t *parent, uint32_t x) {
    for (;;) {
        const uint32_t p = comp_load(parent + x);
        if (p == x) return x;
        const uint32_t g = comp_load(parent + p);
        if (g == p) return p;
        __hip_atomic_store(parent + x, g, COMP_RLX);  // (x is no root and never will be: no CAS of a hook can succeed on it)
        x = g;
    }
}
__device__ __forceinline__ uint32_t comp_find_ro(uint32_t *parent, uint32_t x) {
    for (;;) {
        const uint32_t p = comp_load(parent + x);
        if (p == x) return x;
        x = p;
    }
}
__device__ __forceinline__ void comp_link(uint32_t *parent, uint32_t u, uint32_t v) {
    for (;;) {
        u = comp_find(parent, u);
        v = comp_find(parent, v);
        if (u == v) return;
        const uint32_t hi = u > v ? u : v, lo = u > v ? v : u;
        uint32_t seen = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, COMP_RLX)) return;
        u = seen;  // hi was hooked by somebody else in the meantime: on from where it points now
        v = lo;
    }
}

}  // namespace vdb
#endif
