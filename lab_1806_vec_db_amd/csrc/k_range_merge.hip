// k_range_merge.hip -- merge of S range results (CSR lists of (distance, id) pairs, one set per row shard) into one, per query ascending by
// the pair order (f32_orderable(distance), then id) and cut after `limit` pairs: what a row-sharded range search does behind its exchange
// (ctx.hip: vdb_sharded_flat_range; shard.py: allgather_merge_range).
//
// Merge by rank.  The S lists of a query are sorted and the ids of different shards are disjoint, so the place of the pair at position j
// of list s in the merged list is  j + sum over t != s of |{pairs of list t that precede it}|:  S - 1 binary searches per pair, no atomics,
// no sequential merge loop, the same output whatever the schedule.  "Precede" is decided by (distance, id, shard): pairs that compare equal
// across lists (which the contract excludes) still get distinct places, and for ANY pair contents a rank is below the query's input total,
// so with the offsets the host derived from the same `lims` every write stays inside the query's output segment.
// Ids are full 64-bit values (id_offset + row may pass 2^32): nothing here packs a pair into one 64-bit key.
//
// One lane per input pair.  A query whose lists hold at most RM_TILE pairs together is one workgroup: the lists are staged in LDS (12 B per
// pair) and searched there.  A longer query is cut into slices of RM_TILE input pairs, one workgroup each, that search the lists in global
// memory (they are read S - 1 times log2(length) times, from L2 after the first touch).  Workgroups are laid out by a prefix of the queries'
// slice counts, so a few long lists among many short ones cost no idle workgroups.
#include <algorithm>
#include <vector>

#include "ctx.hpp"

namespace vdb {

namespace {

constexpr uint32_t RM_TILE = 4096;   // input pairs per workgroup; also what the LDS stage holds (48 KB)
constexpr uint32_t RM_MAX_S = 256;   // lists per query on the device (their bounds live in LDS)
constexpr uint32_t RM_THREADS = 256;

// pair a precedes pair b; `a_first` breaks a full tie (a's list comes before b's)
__host__ __device__ inline bool rm_precedes(uint32_t ao, uint64_t ai, uint32_t bo, uint64_t bi, bool a_first) {
    if (ao != bo) return ao < bo;
    if (ai != bi) return ai < bi;
    return a_first;
}

// number of pairs of the sorted list [0, len) that precede (o, id); get(i) -> (orderable distance, id) of its i-th pair
template <class Get>
__device__ inline uint64_t rm_count_before(uint64_t len, uint32_t o, uint64_t id, bool list_first, Get get) {
    uint64_t lo = 0, hi = len;  // pairs [0, lo) precede, pairs [hi, len) do not
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        uint32_t mo;
        uint64_t mi;
        get(mid, mo, mi);
        if (rm_precedes(mo, mi, o, id, list_first))
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// lims [S][lims_ld] (u64, list s of query q = pairs [lims[s][q], lims[s][q + 1]) of shard s); ids / dists of shard s start stride_i / stride_d
// BYTES after those of shard 0; out_lims [nq + 1]: output offsets, out_lims[q + 1] - out_lims[q] = min(limit, input total of q);
// tile_start [nq + 1]: first workgroup of every query
__global__ __launch_bounds__(RM_THREADS) void k_range_merge(const uint64_t *__restrict__ lims, uint64_t lims_ld, const char *__restrict__ ids,
                                                            uint64_t stride_i, const char *__restrict__ dists, uint64_t stride_d, uint32_t S,
                                                            uint32_t nq, const uint64_t *__restrict__ out_lims,
                                                            const uint64_t *__restrict__ tile_start, uint64_t *__restrict__ out_idx,
                                                            float *__restrict__ out_dist) {
    __shared__ uint64_t s_pref[RM_MAX_S + 1];  // position of every list in the query's concatenated input
    __shared__ uint64_t s_base[RM_MAX_S];      // lims[s][q]
    __shared__ float s_d[RM_TILE];
    __shared__ uint64_t s_id[RM_TILE];
    const uint32_t tid = threadIdx.x;
    const uint64_t b = blockIdx.x;
    uint32_t q = 0;
    {  // the query this workgroup belongs to: tile_start[q] <= b < tile_start[q + 1]
        uint32_t lo = 0, hi = nq;
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (tile_start[mid] <= b)
                lo = mid;
            else
                hi = mid;
        }
        q = lo;
    }
    const uint64_t tile = b - tile_start[q];
    for (uint32_t s = tid; s < S; s += RM_THREADS) {
        const uint64_t l0 = lims[uint64_t(s) * lims_ld + q], l1 = lims[uint64_t(s) * lims_ld + q + 1];
        s_base[s] = l0;
        s_pref[s + 1] = l1 - l0;
    }
    __syncthreads();
    if (tid == 0) {
        uint64_t run = 0;
        s_pref[0] = 0;
        for (uint32_t s = 0; s < S; s++) {
            run += s_pref[s + 1];
            s_pref[s + 1] = run;
        }
    }
    __syncthreads();
    const uint64_t total = s_pref[S], o0 = out_lims[q], keep = out_lims[q + 1] - o0;
    // list and position of input pair e: s_pref[s] <= e < s_pref[s + 1]
    auto locate = [&](uint64_t e, uint32_t &s, uint64_t &j) {
        uint32_t lo = 0, hi = S;
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (s_pref[mid] <= e)
                lo = mid;
            else
                hi = mid;
        }
        s = lo;
        j = e - s_pref[lo];
    };
    auto g_id = [&](uint32_t s, uint64_t j) { return reinterpret_cast<const uint64_t *>(ids + uint64_t(s) * stride_i)[s_base[s] + j]; };
    auto g_d = [&](uint32_t s, uint64_t j) { return reinterpret_cast<const float *>(dists + uint64_t(s) * stride_d)[s_base[s] + j]; };
    if (total <= RM_TILE) {  // (then this is the query's only workgroup)
        for (uint32_t e = tid; e < (uint32_t)total; e += RM_THREADS) {
            uint32_t s;
            uint64_t j;
            locate(e, s, j);
            s_id[e] = g_id(s, j);
            s_d[e] = g_d(s, j);
        }
        __syncthreads();
        for (uint32_t e = tid; e < (uint32_t)total; e += RM_THREADS) {
            uint32_t s;
            uint64_t j;
            locate(e, s, j);
            if (j >= keep) continue;  // (its rank is at least j)
            const float d = s_d[e];
            const uint64_t id = s_id[e];
            const uint32_t o = f32_orderable(d);
            uint64_t rank = j;
            for (uint32_t t = 0; t < S; t++) {
                if (t == s) continue;
                const uint32_t p0 = (uint32_t)s_pref[t];
                rank += rm_count_before(s_pref[t + 1] - p0, o, id, t < s, [&](uint64_t i, uint32_t &mo, uint64_t &mi) {
                    mo = f32_orderable(s_d[p0 + (uint32_t)i]);
                    mi = s_id[p0 + (uint32_t)i];
                });
            }
            if (rank < keep) {
                out_idx[o0 + rank] = id;
                out_dist[o0 + rank] = d;
            }
        }
        return;
    }
    const uint64_t e0 = tile * RM_TILE, e1 = e0 + RM_TILE < total ? e0 + RM_TILE : total;
    for (uint64_t e = e0 + tid; e < e1; e += RM_THREADS) {
        uint32_t s;
        uint64_t j;
        locate(e, s, j);
        if (j >= keep) continue;
        const float d = g_d(s, j);
        const uint64_t id = g_id(s, j);
        const uint32_t o = f32_orderable(d);
        uint64_t rank = j;
        for (uint32_t t = 0; t < S; t++) {
            if (t == s) continue;
            rank += rm_count_before(s_pref[t + 1] - s_pref[t], o, id, t < s, [&](uint64_t i, uint32_t &mo, uint64_t &mi) {
                mo = f32_orderable(g_d(t, i));
                mi = g_id(t, i);
            });
        }
        if (rank < keep) {
            out_idx[o0 + rank] = id;
            out_dist[o0 + rank] = d;
        }
    }
}

}  // namespace

void range_merge_validate(const uint64_t *lims, uint64_t lims_ld, uint64_t n_shards, uint64_t nq, uint64_t pair_cap) {
    for (uint64_t s = 0; s < n_shards; s++) {
        const uint64_t *l = lims + s * lims_ld;
        VDB_REQUIRE(l[0] == 0, "range merge: lims of shard " + std::to_string(s) + " do not start at 0");
        for (uint64_t q = 0; q < nq; q++)
            VDB_REQUIRE(l[q] <= l[q + 1], "range merge: lims of shard " + std::to_string(s) + " decrease at query " + std::to_string(q));
        VDB_REQUIRE(l[nq] <= pair_cap, "range merge: shard " + std::to_string(s) + " declares " + std::to_string(l[nq]) + " pairs, its block holds " +
                                           std::to_string(pair_cap));
    }
}

void range_merge_lims(const uint64_t *lims, uint64_t lims_ld, uint64_t n_shards, uint64_t nq, uint64_t limit, uint64_t *out_lims) {
    uint64_t run = 0;
    for (uint64_t q = 0; q < nq; q++) {
        out_lims[q] = run;
        uint64_t t = 0;
        for (uint64_t s = 0; s < n_shards; s++) t += lims[s * lims_ld + q + 1] - lims[s * lims_ld + q];
        run += limit && limit < t ? limit : t;
    }
    out_lims[nq] = run;
}

void range_merge_host(const uint64_t *lims, const uint64_t *ids, const float *dists, uint64_t n_shards, uint64_t nq, uint64_t pair_stride,
                      const uint64_t *out_lims, uint64_t *out_idx, float *out_dist) {
    std::vector<uint64_t> head(n_shards), end(n_shards);
    for (uint64_t q = 0; q < nq; q++) {
        for (uint64_t s = 0; s < n_shards; s++) {
            head[s] = s * pair_stride + lims[s * (nq + 1) + q];
            end[s] = s * pair_stride + lims[s * (nq + 1) + q + 1];
        }
        for (uint64_t o = out_lims[q]; o < out_lims[q + 1]; o++) {
            uint64_t best = n_shards;
            uint32_t bo = 0;
            for (uint64_t s = 0; s < n_shards; s++) {  // (the lowest shard wins a full tie: the strict comparison keeps the earlier one)
                if (head[s] == end[s]) continue;
                const uint32_t so = f32_orderable(dists[head[s]]);
                if (best == n_shards || rm_precedes(so, ids[head[s]], bo, ids[head[best]], false)) {
                    best = s;
                    bo = so;
                }
            }
            out_idx[o] = ids[head[best]];
            out_dist[o] = dists[head[best]];
            head[best]++;
        }
    }
}

void range_merge_dev(Index &ix, Workspace &ws, const uint64_t *h_lims, uint64_t lims_ld, const void *d_lims, const void *d_ids, uint64_t stride_i,
                     const void *d_dists, uint64_t stride_d, uint64_t n_shards, uint64_t nq, uint64_t limit, RangeResult &out) {
    hipStream_t s = ws.stream;
    VDB_REQUIRE(n_shards >= 1 && n_shards <= RM_MAX_S, "range merge on the device: 1.." + std::to_string(RM_MAX_S) + " shards");
    VDB_REQUIRE(nq < (1ull << 32), "too many queries for one call");
    VDB_REQUIRE((stride_i & 7) == 0 && (stride_d & 3) == 0, "misaligned shard blocks");
    out.device = ix.device;
    out.nq = nq;
    out.lims.assign(nq + 1, 0);
    if (nq == 0) return;
    range_merge_lims(h_lims, lims_ld, n_shards, nq, limit, out.lims.data());
    const uint64_t total = out.lims[nq], cap_pairs = ix.range_max_results ? ix.range_max_results : ~0ull;
    if (total > cap_pairs)
        throw Error(1, "range merge: " + std::to_string(total) + " results, more than " + std::to_string(cap_pairs) +
                           " in one call (flat_range_max_results); use a limit, smaller radii or fewer queries per call");
    if (total == 0) return;
    VDB_REQUIRE(d_lims && d_ids && d_dists, "null argument");
    std::vector<uint64_t> meta(2 * (nq + 1));  // [out_lims | tile_start]
    std::copy(out.lims.begin(), out.lims.end(), meta.begin());
    uint64_t tiles = 0;
    for (uint64_t q = 0; q < nq; q++) {
        meta[nq + 1 + q] = tiles;
        uint64_t t = 0;
        for (uint64_t sh = 0; sh < n_shards; sh++) t += h_lims[sh * lims_ld + q + 1] - h_lims[sh * lims_ld + q];
        tiles += (t + RM_TILE - 1) / RM_TILE;
    }
    meta[2 * nq + 1] = tiles;
    VDB_REQUIRE(tiles < (1ull << 31), "range merge: too many pairs for one call");
    out.idx.reserve(total * sizeof(uint64_t));
    out.dist.reserve(total * sizeof(float));
    DevBuf d_meta;
    d_meta.reserve(meta.size() * sizeof(uint64_t));
    VDB_HIP(hipMemcpyAsync(d_meta.p, meta.data(), meta.size() * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    uint64_t in_pairs = 0;
    for (uint64_t sh = 0; sh < n_shards; sh++) in_pairs += h_lims[sh * lims_ld + nq];
    ix.prof_begin(ws, "range_merge", double(in_pairs + total) * 12.0);
    hipLaunchKernelGGL(k_range_merge, dim3((unsigned)tiles), dim3(RM_THREADS), 0, s, static_cast<const uint64_t *>(d_lims), lims_ld,
                       static_cast<const char *>(d_ids), stride_i, static_cast<const char *>(d_dists), stride_d, (uint32_t)n_shards, (uint32_t)nq,
                       d_meta.as<uint64_t>(), d_meta.as<uint64_t>() + nq + 1, out.idx.as<uint64_t>(), out.dist.as<float>());
    ix.prof_end(ws);
    VDB_SYNC(s);  // (`meta` and d_meta go out of scope)
}

}  // namespace vdb
