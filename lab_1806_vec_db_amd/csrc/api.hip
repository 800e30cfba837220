// api.hip -- extern "C" boundary of libvdbhip.so (declarations + reference citations: include/vdbhip.h).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "ctx.hpp"
#include "fetch_plan.hpp"
#include "pq_hnsw.hpp"
#include "remove_plan.hpp"
#include "update_plan.hpp"

using namespace vdb;

static thread_local std::string g_last_error;
void vdb::set_last_error(const std::string &m) { g_last_error = m; }
void vdb::require_gpu() {
    int cnt = 0;
    hipError_t e = hipGetDeviceCount(&cnt);
    if (e != hipSuccess || cnt <= 0)
        throw Error(VDB_ERR_NOGPU, std::string("no usable HIP device (libvdbhip has no CPU fallback): ") +
                                       hipGetErrorString(e));
}

// the device merges carry an id in the low word of a pair key: the ids of the lists must be below 2^32.  The lists themselves are
// not inspected; the shard handed in stands for them (every rank merges with its own), as in flat_knn_pq_shard_device
static void require_merge_ids_fit(const Index &ix) {
    VDB_REQUIRE(ix.id_offset <= (1ull << 32) && ix.n <= (1ull << 32) - ix.id_offset, "shard merge: global row ids must fit 32 bits");
}

// device-resident variants: inputs/outputs on the index's GPU, ids < 2^32; synchronous on return
void vdb::merge_topk_dev(Index &ix, const void *d_dists, const void *d_ids, const void *d_counts, uint64_t stride_d,
                           uint64_t stride_i, uint64_t stride_c, uint64_t n_shards, uint64_t nq, uint64_t k,
                           void *d_out_idx, void *d_out_dist, void *d_out_count, void *stream) {
    VDB_REQUIRE(d_dists && d_ids && d_counts && d_out_idx && d_out_dist && d_out_count, "null argument");
    VDB_REQUIRE(k >= 1 && k <= 1024, "k must be in 1..1024");
    VDB_REQUIRE(n_shards >= 1, "shard merge: at least one shard is needed");
    VDB_REQUIRE(nq <= 65535 && n_shards <= 65535, "too many queries or shards for one call");
    require_merge_ids_fit(ix);
    ix.use_device();
    WsLease ws(ix);
    VDB_SYNC(static_cast<hipStream_t>(stream));
    if (k <= 64) {  // one launch, no scratch lists
        launch_merge_shards64(static_cast<const float *>(d_dists), static_cast<const uint64_t *>(d_ids),
                              static_cast<const uint64_t *>(d_counts), stride_d, stride_i, stride_c, (uint32_t)n_shards,
                              (uint32_t)nq, (uint32_t)k, static_cast<uint64_t *>(d_out_idx), static_cast<float *>(d_out_dist),
                              static_cast<uint64_t *>(d_out_count), ws->stream);
        VDB_SYNC(ws->stream);
        return;
    }
    uint32_t cap = topk_capacity((uint32_t)k);
    ws->lists.reserve(nq * n_shards * cap * sizeof(uint64_t));
    ws->keys_c.reserve(nq * cap * sizeof(uint64_t));
    launch_pack_pairs(static_cast<const float *>(d_dists), static_cast<const uint64_t *>(d_ids),
                      static_cast<const uint64_t *>(d_counts), stride_d, stride_i, stride_c, (uint32_t)n_shards,
                      (uint32_t)nq, (uint32_t)k, cap, ws->lists.as<uint64_t>(), ws->stream);
    launch_topk_merge(ws->lists.as<uint64_t>(), (uint32_t)n_shards, cap, (uint32_t)nq, (uint32_t)k,
                      ws->keys_c.as<uint64_t>(), ws->stream);
    launch_finalize(ws->keys_c.as<uint64_t>(), cap, (uint32_t)nq, (uint32_t)k, (uint32_t)k, 0,
                    static_cast<uint64_t *>(d_out_idx), static_cast<float *>(d_out_dist),
                    static_cast<uint64_t *>(d_out_count), ws->stream);
    VDB_SYNC(ws->stream);
}

// ---- the front ends the search entry points below share (templates: in front of the extern "C" block) ------------------------------
static void check_query_args(const Index &ix, const void *queries, uint64_t nq, uint64_t dim, const void *out_idx,
                             const void *out_dist) {
    VDB_REQUIRE(dim == ix.dim, "query dimension mismatch: index dim " + std::to_string(ix.dim) + ", got " +
                                   std::to_string(dim));
    VDB_REQUIRE(nq == 0 || (queries && out_idx && out_dist), "null argument");
}

// the failure path of every search front end: nothing of a failed call is still running when its buffers go
template <class Body>
static void run_synced(Index &ix, Workspace &ws, Body &&body) {
    try {
        body();
    } catch (...) {
        (void)hipStreamSynchronize(ws.stream);
        ix.prof_collect(ws);
        throw;
    }
    ix.prof_collect(ws);
}

// The outputs of nb queries of a host call: ONE device block [ids | distances | counts] in ws.out_idx, and its way back to the host --
// through the workspace's pinned block (one async copy, then memcpy) when `staged`, else three copies into the caller's pageable arrays.
struct OutBlock {
    static constexpr size_t STAGE_MAX = size_t(8) << 20;  // a call whose pinned block would pass this goes unstaged
    uint64_t nb, k;
    size_t off_d, off_c, bytes;
    char *d;
    OutBlock(Workspace &ws, uint64_t nb_, uint64_t k_) : nb(nb_), k(k_) {
        const uint64_t kk = std::max<uint64_t>(k, 1);
        off_d = nb * kk * sizeof(uint64_t);
        off_c = (off_d + nb * kk * sizeof(float) + 7) & ~size_t(7);
        bytes = off_c + nb * sizeof(uint64_t);
        ws.out_idx.reserve(bytes);
        d = ws.out_idx.as<char>();
    }
    uint64_t *idx() const { return reinterpret_cast<uint64_t *>(d); }
    float *dist() const { return reinterpret_cast<float *>(d + off_d); }
    uint64_t *cnt() const { return reinterpret_cast<uint64_t *>(d + off_c); }
    // -> out_idx / out_dist [q0 ..][k], out_count [q0 ..] (nullptr: not wanted); staged: the block goes to pin_off of the pinned block, whose
    // pointer is fetched here, after the search (which may have used the block for its own flags and has synchronised after reading
    // them: the block is free again).  Returns synchronised.
    void download(Workspace &ws, bool staged, size_t pin_off, uint64_t q0, uint64_t *out_idx, float *out_dist, uint64_t *out_count) const {
        hipStream_t s = ws.stream;
        const size_t cb = nb * sizeof(uint64_t);
        if (staged) {
            char *h = static_cast<char *>(ws.pinned(pin_off + bytes)) + pin_off;
            VDB_HIP(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, s));
            VDB_SYNC(s);
            if (k) {
                std::memcpy(out_idx + q0 * k, h, nb * k * sizeof(uint64_t));
                std::memcpy(out_dist + q0 * k, h + off_d, nb * k * sizeof(float));
            }
            if (out_count) std::memcpy(out_count + q0, h + off_c, cb);
        } else {
            if (k) {
                VDB_HIP(hipMemcpyAsync(out_idx + q0 * k, d, nb * k * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
                VDB_HIP(hipMemcpyAsync(out_dist + q0 * k, d + off_d, nb * k * sizeof(float), hipMemcpyDeviceToHost, s));
            }
            std::vector<uint64_t> cnt(nb);
            VDB_HIP(hipMemcpyAsync(cnt.data(), d + off_c, cb, hipMemcpyDeviceToHost, s));
            VDB_SYNC(s);
            if (out_count) std::memcpy(out_count + q0, cnt.data(), cb);
        }
    }
};

// The k-NN front ends take the search as fn(ws, d_q, q0, nb, d_idx, d_dist, d_cnt): nb queries at d_q, which are the call's queries
// q0 .. q0 + nb (what a per-query argument such as mask_of is advanced by), answered into the three device outputs (`auto... o` in the
// lambdas below); k, ef and whatever else the search needs are the callable's own captures.
// host-pointer front end shared by all searches: stage queries, run, copy results back
template <class Fn>
static void host_search(Index &ix, const float *queries, uint64_t nq, uint64_t k, uint64_t *out_idx, float *out_dist, uint64_t *out_count, Fn &&fn) {
    if (nq == 0) return;
    ix.use_device();
    WsLease ws(ix);
    hipStream_t s = ws->stream;
    constexpr uint64_t CHUNK = 16384;
    run_synced(ix, *ws, [&] {
        for (uint64_t q0 = 0; q0 < nq; q0 += CHUNK) {
            uint64_t nb = std::min<uint64_t>(CHUNK, nq - q0);
            // ONE device block for the three outputs (OutBlock) and ONE pinned host block [queries | that block]:
            // a call moves two async copies through page-locked memory instead of four pageable ones (each of which the runtime
            // stages and waits for on its own) -- what a db.search()-shaped call of one query pays for besides its kernels
            const size_t qb = nb * ix.dim * sizeof(float), q_pad = (qb + 15) & ~size_t(15);
            ws->q.reserve(qb);
            const OutBlock out(*ws, nb, k);
            const bool staged = q_pad + out.bytes <= OutBlock::STAGE_MAX;
            if (staged) {
                char *h = static_cast<char *>(ws->pinned(q_pad + out.bytes));
                std::memcpy(h, queries + q0 * ix.dim, qb);
                VDB_HIP(hipMemcpyAsync(ws->q.p, h, qb, hipMemcpyHostToDevice, s));
            } else {
                VDB_HIP(hipMemcpyAsync(ws->q.p, queries + q0 * ix.dim, qb, hipMemcpyHostToDevice, s));
            }
            fn(*ws, ws->q.as<float>(), q0, nb, out.idx(), out.dist(), out.cnt());
            out.download(*ws, staged, q_pad, q0, out_idx, out_dist, out_count);
        }
    });
}

// what every device-pointer k-NN call requires of its arguments
static void check_device_args(const Index &ix, const void *d_queries, uint64_t nq, uint64_t dim, const void *d_out_idx, const void *d_out_dist,
                              const void *d_out_count) {
    check_query_args(ix, d_queries, nq, dim, d_out_idx, d_out_dist);
    VDB_REQUIRE(nq == 0 || d_out_count, "null out_count");
    VDB_REQUIRE(nq <= 32768, "at most 32768 queries per device call");
}

// device-pointer front end shared by all searches (queries and outputs already on the index's GPU); fn always gets q0 = 0.  (An entry
// point with checks of its own behind these calls check_device_args itself first: the order of the refusals is part of the contract.)
template <class Fn>
static void device_search(Index &ix, const void *d_queries, uint64_t nq, uint64_t dim, void *d_out_idx, void *d_out_dist, void *d_out_count,
                          void *stream, Fn &&fn) {
    check_device_args(ix, d_queries, nq, dim, d_out_idx, d_out_dist, d_out_count);
    if (nq == 0) return;
    ix.use_device();
    WsLease ws(ix);
    // order after whatever produced the queries on the caller's stream
    VDB_SYNC(static_cast<hipStream_t>(stream));
    run_synced(ix, *ws, [&] {
        fn(*ws, static_cast<const float *>(d_queries), uint64_t(0), nq, static_cast<uint64_t *>(d_out_idx), static_cast<float *>(d_out_dist),
           static_cast<uint64_t *>(d_out_count));
        VDB_SYNC(ws->stream);
    });
}

// The front end of the list forms (vdb_group_cap_device, vdb_mmr_select_device, vdb_drop_listed_device, vdb_fuse_lists_device): caller-supplied
// lists d_ids / d_dists [..][ld] with d_counts, outputs [nq][k] and d_out_count, all on the index's GPU.  An entry point keeps its own
// checks in front of these, in its order: the order of the refusals is part of the contract.
static void list_form_check(const void *d_ids, const void *d_dists, const void *d_counts, uint64_t nq, uint64_t ld, uint64_t k, const void *d_out_idx,
                            const void *d_out_dist, const void *d_out_count) {
    VDB_REQUIRE(nq == 0 || (d_counts && d_out_count && (ld == 0 || (d_ids && d_dists)) && (k == 0 || (d_out_idx && d_out_dist))), "null argument");
}
// body(Workspace &) behind whatever produced the lists on the caller's stream; nothing to do without queries
template <class Body>
static void list_form_run(Index &ix, void *stream, uint64_t nq, Body &&body) {
    if (nq == 0) return;
    ix.use_device();
    WsLease ws(ix);
    VDB_SYNC(static_cast<hipStream_t>(stream));
    run_synced(ix, *ws, [&] { body(*ws); });
}
template <class Body>
static void list_form_call(Index &ix, void *stream, const void *d_ids, const void *d_dists, const void *d_counts, uint64_t nq, uint64_t ld, uint64_t k,
                           const void *d_out_idx, const void *d_out_dist, const void *d_out_count, Body &&body) {
    list_form_check(d_ids, d_dists, d_counts, nq, ld, k, d_out_idx, d_out_dist, d_out_count);
    list_form_run(ix, stream, nq, body);
}

// exact Flat range search
static void range_check(const Index &ix, const void *queries, uint64_t nq, uint64_t dim, const void *radius, vdb_range **out) {
    VDB_REQUIRE(out, "null out");
    *out = nullptr;
    VDB_REQUIRE(dim == ix.dim, "query dimension mismatch: index dim " + std::to_string(ix.dim) + ", got " + std::to_string(dim));
    VDB_REQUIRE(nq == 0 || (queries && radius), "null argument");
    VDB_REQUIRE(nq < (1ull << 32), "too many queries for one call");
}

// the host forms' upload: [queries | radii] in ws.q -> the device pointers to the two (null without queries)
struct RangeArgs {
    const float *q = nullptr, *r = nullptr;
};
static RangeArgs stage_range_args(const Index &ix, Workspace &ws, const float *queries, const float *radius, uint64_t nq) {
    if (nq == 0) return {};
    const size_t qb = nq * ix.dim * sizeof(float), qb_pad = (qb + 255) & ~size_t(255);
    ws.q.reserve(qb_pad + nq * sizeof(float));
    VDB_HIP(hipMemcpyAsync(ws.q.p, queries, qb, hipMemcpyHostToDevice, ws.stream));
    VDB_HIP(hipMemcpyAsync(ws.q.as<char>() + qb_pad, radius, nq * sizeof(float), hipMemcpyHostToDevice, ws.stream));
    return {ws.q.as<float>(), reinterpret_cast<const float *>(ws.q.as<char>() + qb_pad)};
}

// runs body(RangeResult &) into a new vdb_range and hands that out when the body has succeeded
template <class Body>
static void range_call(Index &ix, Workspace &ws, vdb_range **out, Body &&body) {
    std::unique_ptr<vdb_range> res(new vdb_range);
    run_synced(ix, ws, [&] { body(res->r); });
    *out = res.release();
}

// "Make n masks or none", the body of the four entry points that fill out[0 .. n): every out[g] is null first; then refuse() may throw
// what the entry point checks before a mask object exists; then n fresh masks go to body(rm), and only when it returns are they
// released into `out` -- a throw destroys every one of them (and with the last of a chunk its slabs).
template <class Refuse, class Body>
static void make_masks(uint64_t n, vdb_mask **out, Refuse refuse, Body body) {
    for (uint64_t g = 0; g < n; g++) out[g] = nullptr;
    refuse();
    std::vector<std::unique_ptr<vdb_mask>> made(n);
    std::vector<RowMask *> rm(n);
    for (uint64_t g = 0; g < n; g++) {
        made[g].reset(new vdb_mask);
        rm[g] = &made[g]->m;
    }
    body(rm.data());
    for (uint64_t g = 0; g < n; g++) out[g] = made[g].release();
}

extern "C" {

const char *vdb_last_error(void) { return g_last_error.c_str(); }
int vdb_version(void) { return 100; }

int vdb_device_count(int *out) {
    VDB_API_BEGIN
    VDB_REQUIRE(out, "null out");
    int cnt = 0;
    hipError_t e = hipGetDeviceCount(&cnt);
    *out = (e == hipSuccess) ? cnt : 0;
    VDB_API_END
}

int vdb_index_create(int device_id, uint64_t dim, int dist, vdb_index **out) {
    VDB_API_BEGIN
    VDB_REQUIRE(out, "null out");
    VDB_REQUIRE(dim > 0 && dim < (1u << 24), "dim must be in 1..2^24");
    VDB_REQUIRE(dist == VDB_L2SQR || dist == VDB_COSINE, "dist must be 0 (L2Sqr) or 1 (Cosine)");
    require_gpu();
    *out = new vdb_index(device_id, dim, dist);
    VDB_API_END
}
// VecSet<u8> (scalar.rs:117-119): rows stored at one byte per element; Flat search only
int vdb_index_create_u8(int device_id, uint64_t dim, int dist, vdb_index **out) {
    VDB_API_BEGIN
    VDB_REQUIRE(out, "null out");
    VDB_REQUIRE(dim > 0 && dim < (1u << 24), "dim must be in 1..2^24");
    VDB_REQUIRE(dist == VDB_L2SQR || dist == VDB_COSINE, "dist must be 0 (L2Sqr) or 1 (Cosine)");
    require_gpu();
    *out = new vdb_index(device_id, dim, dist, true);
    VDB_API_END
}
int vdb_index_destroy(vdb_index *idx) {
    VDB_API_BEGIN
    if (idx) {
        idx->ix.use_device();
        delete idx;
    }
    VDB_API_END
}
int vdb_index_len(const vdb_index *idx, uint64_t *out) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx && out, "null argument");
    *out = idx->ix.n;
    VDB_API_END
}
int vdb_index_dim(const vdb_index *idx, uint64_t *out) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx && out, "null argument");
    *out = idx->ix.dim;
    VDB_API_END
}
int vdb_index_dist(const vdb_index *idx, int *out) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx && out, "null argument");
    *out = idx->ix.dist;
    VDB_API_END
}
int vdb_index_row(const vdb_index *idx, uint64_t i, float *out) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx && out, "null argument");
    const Index &ix = idx->ix;
    VDB_REQUIRE(i < ix.n, "row index out of bounds");
    ix.use_device();
    if (ix.elem_u8) {  // widened with `as f32` (exact)
        std::vector<uint8_t> b(ix.dim);
        VDB_HIP(hipMemcpy(b.data(), ix.d_rows.as<uint8_t>() + i * ix.dim, ix.dim, hipMemcpyDeviceToHost));
        for (uint64_t j = 0; j < ix.dim; j++) out[j] = (float)b[j];
        return VDB_OK;
    }
    VDB_HIP(hipMemcpy(out, ix.d_rows.as<float>() + i * ix.dim, ix.dim * sizeof(float), hipMemcpyDeviceToHost));
    VDB_API_END
}
int vdb_index_row_u8(const vdb_index *idx, uint64_t i, uint8_t *out) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx && out, "null argument");
    const Index &ix = idx->ix;
    VDB_REQUIRE(ix.elem_u8, "not a VecSet<u8> index");
    VDB_REQUIRE(i < ix.n, "row index out of bounds");
    ix.use_device();
    VDB_HIP(hipMemcpy(out, ix.d_rows.as<uint8_t>() + i * ix.dim, ix.dim, hipMemcpyDeviceToHost));
    VDB_API_END
}
int vdb_index_is_u8(const vdb_index *idx, int *out) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx && out, "null argument");
    *out = idx->ix.elem_u8 ? 1 : 0;
    VDB_API_END
}

static void add_common(Index &ix, const float *rows, uint64_t n, uint64_t *first_id, bool on_device) {
    VDB_REQUIRE(rows || n == 0, "null rows");
    VDB_REQUIRE(!ix.elem_u8, "this index stores VecSet<u8> rows: add them with vdb_index_add_u8");
    if (ix.ivf.present && n) ivf_clear(ix);  // IVFIndex has no add (built from_vec_set only): the clusters go stale
    // MetadataVecTable::add / batch_add clear the PQ table before they touch the index (metadata_vec_table.rs:65,77):
    // the codes cover the old rows only, a later knn_pq must fail with "needs a PQ table", not scan past d_codes
    if (ix.pq.present && n) pq_clear(ix);
    if (first_id) *first_id = ix.n;
    if (ix.hnsw.present) {
        // DynamicIndex::add on the HNSW arm (dynamic_index.rs:47-52): HNSWIndex::add per row
        std::vector<float> tmp;
        const float *h = rows;
        if (on_device) {
            tmp.resize(n * ix.dim);
            ix.use_device();
            VDB_HIP(hipMemcpy(tmp.data(), rows, n * ix.dim * sizeof(float), hipMemcpyDeviceToHost));
            h = tmp.data();
        }
        hnsw_insert_rows(ix, h, n);
        return;
    }
    ix.add_rows(rows, n, on_device);
}
int vdb_index_add(vdb_index *idx, const float *rows, uint64_t n, uint64_t *first_id) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    add_common(idx->ix, rows, n, first_id, false);
    VDB_API_END
}
int vdb_index_add_device(vdb_index *idx, const void *d_rows, uint64_t n, uint64_t *first_id) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    add_common(idx->ix, static_cast<const float *>(d_rows), n, first_id, true);
    VDB_API_END
}
// the row edits of a Flat table are refused while a structure built over the rows is attached; `call` is the edit the message names
static void require_flat_only(const Index &ix, const char *call) {
    VDB_REQUIRE(!ix.hnsw.present, std::string(call) + " needs a Flat index (clear the HNSW graph first)");
    VDB_REQUIRE(!ix.pq.present, std::string(call) + " invalidates the PQ table: clear it first");
    VDB_REQUIRE(!ix.ivf.present, std::string(call) + " invalidates the IVF clusters: clear them first");
}
int vdb_index_swap_remove(vdb_index *idx, uint64_t i) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    require_flat_only(idx->ix, "swap_remove");
    idx->ix.swap_remove(i);
    VDB_API_END
}
// the plan's outputs: the count, and the moves when the caller asked for them (out_dst / out_src go together)
static void remove_plan_out(const std::vector<uint64_t> &dst, const std::vector<uint64_t> &src, uint64_t *out_dst, uint64_t *out_src,
                            uint64_t *out_moves) {
    if (out_dst && !dst.empty()) {
        std::memcpy(out_dst, dst.data(), dst.size() * sizeof(uint64_t));
        std::memcpy(out_src, src.data(), src.size() * sizeof(uint64_t));
    }
    if (out_moves) *out_moves = dst.size();
}
int vdb_remove_plan(uint64_t n, const uint64_t *rows, uint64_t m, uint64_t *out_dst, uint64_t *out_src, uint64_t *out_moves) {
    VDB_API_BEGIN
    VDB_REQUIRE((out_dst == nullptr) == (out_src == nullptr), "out_dst and out_src go together (both NULL: the count only)");
    const char *why = remove_plan_check(n, rows, m);
    VDB_REQUIRE(!why, why);
    if (!out_dst) {
        if (out_moves) *out_moves = remove_plan_count(n, rows, m);
        return VDB_OK;
    }
    std::vector<uint64_t> dst, src;
    remove_plan(n, rows, m, dst, src);
    remove_plan_out(dst, src, out_dst, out_src, out_moves);
    VDB_API_END
}
int vdb_index_remove_rows(vdb_index *idx, const uint64_t *rows, uint64_t m, uint64_t *out_dst, uint64_t *out_src, uint64_t *out_moves) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    VDB_REQUIRE((out_dst == nullptr) == (out_src == nullptr), "out_dst and out_src go together (both NULL: no plan returned)");
    require_flat_only(idx->ix, "swap_remove");  // (the bulk form of swap_remove: its refusals carry that name)
    std::vector<uint64_t> dst, src;
    idx->ix.remove_rows(rows, m, dst, src);
    remove_plan_out(dst, src, out_dst, out_src, out_moves);
    VDB_API_END
}
int vdb_update_plan(uint64_t n, const uint64_t *rows, uint64_t m, uint32_t *out_tiles, uint64_t *out_n_tiles) {
    VDB_API_BEGIN
    VDB_REQUIRE(n < (1ull << 32), "update_plan: a shard holds at most 2^32-1 rows");
    const char *why = update_plan_check(n, rows, m);
    VDB_REQUIRE(!why, why);
    std::vector<uint32_t> tiles;
    update_plan(n, rows, m, tiles);
    if (out_tiles && !tiles.empty()) std::memcpy(out_tiles, tiles.data(), tiles.size() * sizeof(uint32_t));
    if (out_n_tiles) *out_n_tiles = tiles.size();
    VDB_API_END
}
static void update_common(vdb_index *idx, const uint64_t *rows, uint64_t m, const void *vecs, bool on_device) {
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    require_flat_only(ix, "update_rows");
    VDB_REQUIRE(!ix.elem_u8, "update_rows needs f32 rows: a VecSet<u8> index is not updated in place");
    VDB_REQUIRE(vecs || m == 0, "update_rows: null vectors");
    VDB_REQUIRE(!on_device || reinterpret_cast<uintptr_t>(vecs) % 16 == 0, "update_rows: device vectors must be 16-byte aligned");
    ix.update_rows(rows, m, vecs, on_device);
}
int vdb_index_update_rows(vdb_index *idx, const uint64_t *rows, uint64_t m, const float *vecs) {
    VDB_API_BEGIN
    update_common(idx, rows, m, vecs, false);
    VDB_API_END
}
int vdb_index_update_rows_device(vdb_index *idx, const uint64_t *rows, uint64_t m, const void *d_vecs) {
    VDB_API_BEGIN
    update_common(idx, rows, m, d_vecs, true);
    VDB_API_END
}
int vdb_fetch_plan(uint64_t n, const uint64_t *rows, uint64_t m, uint64_t out_row_bytes, uint64_t chunk_bytes, int *out_route,
                   uint64_t *out_chunk_rows, uint64_t *out_n_chunks) {
    VDB_API_BEGIN
    VDB_REQUIRE(out_row_bytes >= 1 && chunk_bytes >= 1, "fetch_plan: out_row_bytes and chunk_bytes must be at least 1");
    const char *why = fetch_plan_check(n, rows, m, out_row_bytes);
    VDB_REQUIRE(!why, why);
    const FetchPlan p = fetch_plan(rows, m, out_row_bytes, chunk_bytes);
    if (out_route) *out_route = p.route;
    if (out_chunk_rows) *out_chunk_rows = p.chunk_rows;
    if (out_n_chunks) *out_n_chunks = p.n_chunks;
    VDB_API_END
}
int vdb_index_set_id_offset(vdb_index *idx, uint64_t offset) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    idx->ix.id_offset = offset;
    VDB_API_END
}

int vdb_calc_dist(int device_id, const float *a, const float *b, uint64_t n, int dist, float *out) {
    VDB_API_BEGIN
    VDB_REQUIRE(a && b && out, "null argument");
    VDB_REQUIRE(n > 0 && n < (1u << 24), "bad length");
    VDB_REQUIRE(dist == VDB_L2SQR || dist == VDB_COSINE, "dist must be 0 or 1");
    require_gpu();
    VDB_HIP(hipSetDevice(device_id));
    DevBuf buf;
    buf.reserve((2 * n + 4) * sizeof(float));
    float *d = buf.as<float>();
    VDB_HIP(hipMemcpy(d, a, n * sizeof(float), hipMemcpyHostToDevice));       // "row"
    VDB_HIP(hipMemcpy(d + n, b, n * sizeof(float), hipMemcpyHostToDevice));   // "query"
    float *sq = d + 2 * n;  // [0]=|a|^2 [1]=|b|^2 [2]=out
    launch_row_sqnorm(d, 1, (uint32_t)n, sq, nullptr);
    launch_row_sqnorm(d + n, 1, (uint32_t)n, sq + 1, nullptr);
    launch_scan_exact(d, 1, (uint32_t)n, d + n, 1, dist == VDB_L2SQR ? MET_L2_DIRECT : MET_COSINE, sq, sq + 1, sq + 2,
                      4, false, nullptr);
    VDB_HIP(hipMemcpy(out, sq + 2, sizeof(float), hipMemcpyDeviceToHost));
    VDB_API_END
}

// ---- u8 scalar (distance/mod.rs:79-95) -----------------------------------------------------------------
// DistanceScalar for u8 converts every element with `as f32` (exact for 0..255) and then runs the f32 folds, so a
// VecSet<u8> index behaves exactly like the f32 index of the converted rows: the u8 entry points convert and forward.
static std::vector<float> widen_u8(const uint8_t *p, uint64_t count) {
    std::vector<float> out(count);
    for (uint64_t i = 0; i < count; i++) out[i] = (float)p[i];
    return out;
}
int vdb_calc_dist_u8(int device_id, const uint8_t *a, const uint8_t *b, uint64_t n, int dist, float *out) {
    VDB_API_BEGIN
    VDB_REQUIRE(a && b && out, "null argument");
    VDB_REQUIRE(n > 0 && n < (1u << 24), "bad length");
    std::vector<float> fa = widen_u8(a, n), fb = widen_u8(b, n);
    int rc = vdb_calc_dist(device_id, fa.data(), fb.data(), n, dist, out);
    if (rc != VDB_OK) return rc;
    VDB_API_END
}
int vdb_index_add_u8(vdb_index *idx, const uint8_t *rows, uint64_t n, uint64_t *first_id) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    VDB_REQUIRE(rows || n == 0, "null rows");
    if (idx->ix.elem_u8) {  // native: one byte per element in HBM
        if (first_id) *first_id = idx->ix.n;
        idx->ix.add_rows(rows, n, false);
        return VDB_OK;
    }
    std::vector<float> f = widen_u8(rows, n * idx->ix.dim);
    add_common(idx->ix, f.data(), n, first_id, false);
    VDB_API_END
}

// ---- Flat ----------------------------------------------------------------------------------------
int vdb_flat_knn(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, uint64_t k, uint64_t *out_idx,
                 float *out_dist, uint64_t *out_count) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    check_query_args(idx->ix, queries, nq, dim, out_idx, out_dist);
    Index &ix = idx->ix;
    if (nq > 0 && k > 0 && ix.flat_small_applies(nq, k)) {
        // The db.search() shape (pyo3/mod.rs:199-214): a few queries, a small table.  One launch, and no copy engine on either
        // side of it: the queries go through ONE block of pinned host memory (read by the kernel over PCIe when only a
        // handful of workgroups want them, else one async copy), the kernel writes ids / distances / counts straight back
        // into that block, and the stream synchronisation that ends the call is the only wait.
        ix.use_device();
        WsLease ws(ix);
        const size_t qb = nq * dim * sizeof(float), ib = nq * k * sizeof(uint64_t), db = nq * k * sizeof(float);
        const size_t off_i = (qb + 15) & ~size_t(15), off_d = off_i + ib, off_c = (off_d + db + 7) & ~size_t(7);
        char *h = static_cast<char *>(ws->pinned(off_c + nq * sizeof(uint64_t)));
        std::memcpy(h, queries, qb);
        const float *q = reinterpret_cast<const float *>(h);
        const uint64_t n_wg = (ix.n + flat_small_rows_per_wg(ix.n, ix.num_cu) - 1) / flat_small_rows_per_wg(ix.n, ix.num_cu);
        if (n_wg * nq > 64) {  // many readers: stage the queries in HBM once
            ws->q.reserve(qb);
            VDB_HIP(hipMemcpyAsync(ws->q.p, h, qb, hipMemcpyHostToDevice, ws->stream));
            q = ws->q.as<float>();
        }
        ix.flat_small_device(*ws, q, nq, k, reinterpret_cast<uint64_t *>(h + off_i), reinterpret_cast<float *>(h + off_d),
                             reinterpret_cast<uint64_t *>(h + off_c));
        VDB_SYNC(ws->stream);
        ix.prof_collect(*ws);
        std::memcpy(out_idx, h + off_i, ib);
        std::memcpy(out_dist, h + off_d, db);
        if (out_count) std::memcpy(out_count, h + off_c, nq * sizeof(uint64_t));
        return VDB_OK;
    }
    host_search(ix, queries, nq, k, out_idx, out_dist, out_count,
                [&](Workspace &w, const float *q, uint64_t, uint64_t nb, auto... o) { ix.flat_knn_device(w, q, nb, k, o...); });
    VDB_API_END
}

int vdb_flat_knn_u8(vdb_index *idx, const uint8_t *queries, uint64_t nq, uint64_t dim, uint64_t k, uint64_t *out_idx,
                    float *out_dist, uint64_t *out_count) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    VDB_REQUIRE(nq == 0 || queries, "null argument");
    std::vector<float> f = widen_u8(queries, nq * dim);
    Index &ix = idx->ix;
    check_query_args(ix, f.data(), nq, dim, out_idx, out_dist);
    host_search(ix, f.data(), nq, k, out_idx, out_dist, out_count,
                [&](Workspace &w, const float *q, uint64_t, uint64_t nb, auto... o) { ix.flat_knn_device(w, q, nb, k, o...); });
    VDB_API_END
}

int vdb_flat_knn_device(vdb_index *idx, const void *d_queries, uint64_t nq, uint64_t dim, uint64_t k,
                        void *d_out_idx, void *d_out_dist, void *d_out_count, void *stream) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    device_search(ix, d_queries, nq, dim, d_out_idx, d_out_dist, d_out_count, stream,
                  [&](Workspace &w, const float *q, uint64_t, uint64_t nb, auto... o) { ix.flat_knn_device(w, q, nb, k, o...); });
    VDB_API_END
}

// ---- a Flat call in two halves: software pipelining of independent query batches ----------------------------------------------
// vdb_flat_knn_device returns when the batch is answered: the host reads the certification flags (one byte per query) to
// decide whether anything must be redone.  Between that read and the first kernel of the next call the GPU idles, and the
// per-query stages at both ends of a call (query preparation, threshold sample and selection in front of the corpus pass;
// the exact stage behind it) cannot overlap each other.  begin() enqueues the whole pipeline on a workspace stream -- ordered
// behind the caller's stream through an event, not a host wait -- and returns; end() waits, reads the flags, redoes what was
// not certified.  Two batches in flight (begin(i+1) before end(i)) keep the corpus passes back to back and let the exact
// stage of batch i run beside the front stages of batch i+1.  Results are the synchronous call's, bit for bit.
struct vdb_pending {
    vdb_index *idx = nullptr;
    std::unique_ptr<Workspace> ws;
    FlatPending p;
};

int vdb_flat_knn_device_begin(vdb_index *idx, const void *d_queries, uint64_t nq, uint64_t dim, uint64_t k, void *d_out_idx,
                              void *d_out_dist, void *d_out_count, void *stream, vdb_pending **out) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx && out, "null argument");
    Index &ix = idx->ix;
    check_device_args(ix, d_queries, nq, dim, d_out_idx, d_out_dist, d_out_count);
    ix.use_device();
    std::unique_ptr<vdb_pending> pd(new vdb_pending);
    pd->idx = idx;
    pd->ws = ix.acquire_ws();
    try {
        Workspace &ws = *pd->ws;
        if (!ws.order_ev) VDB_HIP(hipEventCreateWithFlags(&ws.order_ev, hipEventDisableTiming));
        VDB_HIP(hipEventRecord(ws.order_ev, static_cast<hipStream_t>(stream)));  // whatever produced the queries / last read the outputs
        VDB_HIP(hipStreamWaitEvent(ws.stream, ws.order_ev, 0));
        ix.flat_knn_enqueue(ws, static_cast<const float *>(d_queries), nq, k, static_cast<uint64_t *>(d_out_idx),
                            static_cast<float *>(d_out_dist), static_cast<uint64_t *>(d_out_count), true, 0, pd->p);
    } catch (...) {
        (void)hipStreamSynchronize(pd->ws->stream);
        ix.release_ws(std::move(pd->ws));
        throw;
    }
    *out = pd.release();
    VDB_API_END
}

// completes the call begun with `pending` and releases it (also on error); the outputs are valid when this returns
int vdb_flat_knn_device_end(vdb_pending *pending) {
    VDB_API_BEGIN
    VDB_REQUIRE(pending, "null pending call");
    std::unique_ptr<vdb_pending> pd(pending);
    Index &ix = pd->idx->ix;
    ix.use_device();
    try {
        ix.flat_knn_finish(*pd->ws, pd->p);
        VDB_SYNC(pd->ws->stream);
        ix.prof_collect(*pd->ws);
    } catch (...) {
        (void)hipStreamSynchronize(pd->ws->stream);
        ix.release_ws(std::move(pd->ws));
        throw;
    }
    ix.release_ws(std::move(pd->ws));
    VDB_API_END
}

// ---- exact Flat range search -------------------------------------------------------------------------------------------------------
int vdb_flat_range(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, const float *radius, uint64_t limit, vdb_range **out) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    range_check(ix, queries, nq, dim, radius, out);
    ix.use_device();
    WsLease ws(ix);
    const RangeArgs a = stage_range_args(ix, *ws, queries, radius, nq);
    range_call(ix, *ws, out, [&](RangeResult &r) { ix.flat_range_device(*ws, a.q, nq, a.r, limit, r); });
    VDB_API_END
}

int vdb_flat_range_device(vdb_index *idx, const void *d_queries, uint64_t nq, uint64_t dim, const void *d_radius, uint64_t limit, void *stream,
                          vdb_range **out) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    range_check(ix, d_queries, nq, dim, d_radius, out);
    ix.use_device();
    WsLease ws(ix);
    VDB_SYNC(static_cast<hipStream_t>(stream));  // order after whatever produced the queries on the caller's stream
    range_call(ix, *ws, out, [&](RangeResult &r) {
        ix.flat_range_device(*ws, static_cast<const float *>(d_queries), nq, static_cast<const float *>(d_radius), limit, r);
    });
    VDB_API_END
}

int vdb_range_lims(const vdb_range *r, uint64_t *out_lims) {
    VDB_API_BEGIN
    VDB_REQUIRE(r && out_lims, "null argument");
    std::memcpy(out_lims, r->r.lims.data(), r->r.lims.size() * sizeof(uint64_t));
    VDB_API_END
}

int vdb_range_copy(const vdb_range *r, uint64_t *out_idx, float *out_dist) {
    VDB_API_BEGIN
    VDB_REQUIRE(r, "null argument");
    const uint64_t total = r->r.lims.empty() ? 0 : r->r.lims.back();
    if (total == 0) return VDB_OK;
    VDB_REQUIRE(out_idx && out_dist, "null argument");
    VDB_HIP(hipSetDevice(r->r.device));
    VDB_HIP(hipMemcpy(out_idx, r->r.idx.p, total * sizeof(uint64_t), hipMemcpyDeviceToHost));
    VDB_HIP(hipMemcpy(out_dist, r->r.dist.p, total * sizeof(float), hipMemcpyDeviceToHost));
    VDB_API_END
}

int vdb_range_destroy(vdb_range *r) {
    VDB_API_BEGIN
    if (r) {
        if (r->r.idx.base || r->r.dist.base) (void)hipSetDevice(r->r.device);
        delete r;
    }
    VDB_API_END
}

// ---- exact filtered Flat search over a row mask -----------------------------------------------------------------------------------------
int vdb_mask_create(vdb_index *idx, const uint64_t *bits, uint64_t n_rows, vdb_mask **out) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx && out, "null argument");
    *out = nullptr;
    Index &ix = idx->ix;
    VDB_REQUIRE(n_rows == ix.n, "mask: " + std::to_string(n_rows) + " rows, the index holds " + std::to_string(ix.n));
    VDB_REQUIRE(n_rows == 0 || bits, "null argument");
    ix.use_device();
    std::unique_ptr<vdb_mask> mk(new vdb_mask);
    RowMask &m = mk->m;
    m.owner = &ix;
    m.device = ix.device;
    m.gen = ix.write_gen.load();
    m.n_rows = n_rows;
    const uint64_t nw = (n_rows + 63) / 64;
    std::vector<uint64_t> w(bits, bits + nw);
    if (n_rows & 63) w[nw - 1] &= (1ull << (n_rows & 63)) - 1;  // bits at and past n_rows are ignored
    uint64_t cnt = 0;
    for (uint64_t x : w) cnt += (uint64_t)__builtin_popcountll(x);
    std::vector<uint32_t> ids;
    ids.reserve(cnt);
    for (uint64_t i = 0; i < nw; i++)
        for (uint64_t x = w[i]; x; x &= x - 1) ids.push_back((uint32_t)(i * 64 + (uint64_t)__builtin_ctzll(x)));
    m.m = cnt;
    try {
        m.d_bits.reserve(std::max<uint64_t>(nw, 1) * sizeof(uint64_t));
        m.d_ids.reserve(std::max<uint64_t>(cnt, 1) * sizeof(uint32_t));
        if (nw) VDB_HIP(hipMemcpy(m.d_bits.p, w.data(), nw * sizeof(uint64_t), hipMemcpyHostToDevice));
        if (cnt) VDB_HIP(hipMemcpy(m.d_ids.p, ids.data(), cnt * sizeof(uint32_t), hipMemcpyHostToDevice));
    } catch (...) {
        m.d_bits.release();
        m.d_ids.release();
        throw;
    }
    *out = mk.release();
    VDB_API_END
}

// ---- label columns; masks built from them on the device (Index::masks_where, k_labels.hip) ------------------------------------------------
static_assert(LABEL_COLUMNS == VDB_LABEL_COLUMNS && LABEL_NONE == VDB_LABEL_NONE && MASK_MAX_TERMS == VDB_MASK_MAX_TERMS, "vdbhip.h and kernels.hpp agree");
int vdb_index_labels_set(vdb_index *idx, uint32_t column, uint64_t first_row, const uint32_t *codes, uint64_t count) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    idx->ix.labels_set(column, first_row, codes, count);
    VDB_API_END
}
int vdb_index_labels_get(const vdb_index *idx, uint32_t column, uint64_t first_row, uint64_t count, uint32_t *out) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    idx->ix.labels_get(column, first_row, count, out);
    VDB_API_END
}
// ---- scattered label writes (Index::labels_scatter*, labels_set_mask) -------------------------------------------------------------------
int vdb_labels_scatter_plan(uint64_t n, const uint64_t *rows, uint64_t m, const uint32_t *columns, uint64_t n_cols, uint32_t *out_ids32) {
    VDB_API_BEGIN
    VDB_REQUIRE(n <= (1ull << 32), "labels_scatter_plan: a shard holds at most 2^32 rows");
    const char *why = labels_scatter_check(n, rows, m, columns, n_cols);
    VDB_REQUIRE(!why, why);
    if (out_ids32) labels_scatter_ids(rows, m, out_ids32);
    VDB_API_END
}
int vdb_index_labels_scatter(vdb_index *idx, const uint64_t *rows, uint64_t m, const uint32_t *columns, uint64_t n_cols, const uint32_t *codes) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    idx->ix.labels_scatter(rows, m, columns, n_cols, codes);
    VDB_API_END
}
int vdb_index_labels_scatter_device(vdb_index *idx, const void *d_ids, uint64_t m, const uint32_t *columns, uint64_t n_cols, const void *d_codes) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    idx->ix.labels_scatter_device(static_cast<const uint64_t *>(d_ids), m, columns, n_cols, static_cast<const uint32_t *>(d_codes));
    VDB_API_END
}
int vdb_index_labels_set_mask(vdb_index *idx, const vdb_mask *mask, const uint32_t *columns, const uint32_t *codes, uint64_t n_cols) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    VDB_REQUIRE(mask, "null mask");
    idx->ix.check_mask(mask->m);
    idx->ix.labels_set_mask(mask->m, columns, codes, n_cols);
    VDB_API_END
}
int vdb_mask_create_where_many(vdb_index *idx, const uint64_t *term_lims, const uint32_t *columns, const uint32_t *codes, uint64_t n_masks,
                               vdb_mask **out) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    VDB_REQUIRE(n_masks == 0 || out, "null argument");
    make_masks(n_masks, out, [] {}, [&](RowMask *const *rm) { idx->ix.masks_where(term_lims, columns, codes, n_masks, rm); });
    VDB_API_END
}
int vdb_mask_create_where(vdb_index *idx, const uint32_t *columns, const uint32_t *codes, uint64_t n_terms, vdb_mask **out) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx && out, "null argument");
    *out = nullptr;
    VDB_REQUIRE(n_terms <= MASK_MAX_TERMS, "mask terms: " + std::to_string(n_terms) + " terms, at most " + std::to_string(MASK_MAX_TERMS) +
                                               " are supported");
    const uint64_t lims[2] = {0, n_terms};
    return vdb_mask_create_where_many(idx, lims, columns, codes, 1, out);
    VDB_API_END
}
// set / range terms (Index::masks_where_sets, mask_sets.hpp)
static_assert(TERM_NEGATE == VDB_TERM_NEGATE && TERM_NONE == VDB_TERM_NONE && MASK_MAX_SET_BITS == VDB_MASK_MAX_SET_BITS, "vdbhip.h and mask_sets.hpp agree");
int vdb_mask_create_where_sets_many(vdb_index *idx, const uint64_t *term_lims, const uint32_t *columns, const uint32_t *lo, const uint32_t *hi,
                                    const uint32_t *flags, const uint64_t *set_lims, const uint64_t *set_words, uint64_t n_masks, vdb_mask **out) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    VDB_REQUIRE(n_masks == 0 || out, "null argument");
    make_masks(
        n_masks, out, [&] { VDB_REQUIRE(n_masks < (1ull << 28), "too many masks for one call"); },
        [&](RowMask *const *rm) { idx->ix.masks_where_sets(term_lims, columns, lo, hi, flags, set_lims, set_words, n_masks, rm); });
    VDB_API_END
}
int vdb_mask_create_where_sets(vdb_index *idx, const uint32_t *columns, const uint32_t *lo, const uint32_t *hi, const uint32_t *flags,
                               const uint64_t *set_lims, const uint64_t *set_words, uint64_t n_terms, vdb_mask **out) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx && out, "null argument");
    *out = nullptr;
    VDB_REQUIRE(n_terms <= MASK_MAX_TERMS, "mask terms: " + std::to_string(n_terms) + " terms, at most " + std::to_string(MASK_MAX_TERMS) +
                                               " are supported");
    const uint64_t lims[2] = {0, n_terms};
    return vdb_mask_create_where_sets_many(idx, lims, columns, lo, hi, flags, set_lims, set_words, 1, out);
    VDB_API_END
}
// an OR of conjunctions of set / range terms (Index::masks_where_any, mask_any.hpp); AND / OR / NOT of masks (Index::mask_combine)
static_assert(MASK_MAX_CLAUSES == VDB_MASK_MAX_CLAUSES && MASK_OP_AND == VDB_MASK_OP_AND && MASK_OP_OR == VDB_MASK_OP_OR, "vdbhip.h, mask_any.hpp and kernels.hpp agree");
int vdb_mask_create_where_any_many(vdb_index *idx, const uint64_t *mask_lims, const uint64_t *clause_lims, const uint32_t *columns,
                                   const uint32_t *lo, const uint32_t *hi, const uint32_t *flags, const uint64_t *set_lims,
                                   const uint64_t *set_words, uint64_t n_masks, vdb_mask **out) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    VDB_REQUIRE(n_masks == 0 || out, "null argument");
    make_masks(
        n_masks, out, [&] { VDB_REQUIRE(n_masks < (1ull << 28), "too many masks for one call"); },
        [&](RowMask *const *rm) { idx->ix.masks_where_any(mask_lims, clause_lims, columns, lo, hi, flags, set_lims, set_words, n_masks, rm); });
    VDB_API_END
}
int vdb_mask_create_where_any(vdb_index *idx, const uint64_t *clause_lims, uint64_t n_clauses, const uint32_t *columns, const uint32_t *lo,
                              const uint32_t *hi, const uint32_t *flags, const uint64_t *set_lims, const uint64_t *set_words, vdb_mask **out) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx && out, "null argument");
    *out = nullptr;
    const uint64_t lims[2] = {0, n_clauses};
    return vdb_mask_create_where_any_many(idx, lims, clause_lims, columns, lo, hi, flags, set_lims, set_words, 1, out);
    VDB_API_END
}
int vdb_mask_combine(vdb_index *idx, int op, const vdb_mask *const *in, const uint8_t *invert, uint64_t n_in, vdb_mask **out) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx && out, "null argument");
    *out = nullptr;
    VDB_REQUIRE(n_in >= 1 && n_in <= MASK_COMBINE_MAX, "mask combine: " + std::to_string(n_in) + " inputs, 1 .. " + std::to_string(MASK_COMBINE_MAX) + " are supported");
    VDB_REQUIRE(in, "null argument");
    const RowMask *rm[MASK_COMBINE_MAX];
    for (uint64_t i = 0; i < n_in; i++) {
        VDB_REQUIRE(in[i], "null mask");
        rm[i] = &in[i]->m;
    }
    std::unique_ptr<vdb_mask> mk(new vdb_mask);
    idx->ix.mask_combine(op, rm, invert, n_in, mk->m);
    *out = mk.release();
    VDB_API_END
}
// one column grouped by code in a single read of it (Index::masks_partition / Index::label_counts, mask_partition.hpp)
int vdb_mask_create_partition(vdb_index *idx, uint32_t column, const uint32_t *codes, uint64_t n_codes, vdb_mask **out) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    VDB_REQUIRE(n_codes < (1ull << 28), "too many codes for one call");  // (before `out` is written: it has room for n_codes handles)
    VDB_REQUIRE(n_codes == 0 || out, "null argument");
    make_masks(
        n_codes, out,
        [&] {  // (before a mask object is made)
            const std::string bad = mask_partition_check(column, codes, n_codes);
            VDB_REQUIRE(bad.empty(), bad);
        },
        [&](RowMask *const *rm) { idx->ix.masks_partition(column, codes, n_codes, rm); });
    VDB_API_END
}
int vdb_index_label_counts(vdb_index *idx, uint32_t column, const vdb_mask *mask, const uint32_t *codes, uint64_t n_codes, uint64_t *out_counts) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    idx->ix.label_counts(column, mask ? &mask->m : nullptr, codes, n_codes, out_counts);
    VDB_API_END
}
// the key lookup over one column (Index::label_lookup, lookup_plan.hpp)
int vdb_label_lookup_plan(uint32_t column, const uint32_t *codes, uint64_t n_codes, uint64_t table_bytes, int *out_route, uint32_t *out_base,
                          uint64_t *out_span, uint64_t *out_chunks) {
    VDB_API_BEGIN
    const std::string bad = label_lookup_check(column, codes, n_codes);
    VDB_REQUIRE(bad.empty(), bad);
    const LookupPlan p = label_lookup_plan(codes, n_codes, table_bytes);
    if (out_route) *out_route = p.route;
    if (out_base) *out_base = p.base;
    if (out_span) *out_span = p.span;
    if (out_chunks) *out_chunks = p.chunks;
    VDB_API_END
}
int vdb_index_label_lookup(vdb_index *idx, uint32_t column, const uint32_t *codes, uint64_t n_codes, uint64_t *out_first, uint64_t *out_counts) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    idx->ix.label_lookup(column, codes, n_codes, out_first, out_counts);
    VDB_API_END
}
// near-duplicate grouping: the range self-join and the components of its pairs (Index::flat_dup_groups_device, dup_plan.hpp, flat_dups.hip)
int vdb_dup_plan(uint64_t n_rows, uint64_t dim, int elem_u8, int masked, uint64_t m_allowed, float radius, uint64_t limit, uint64_t chunk,
                 uint64_t *out_chunks, uint64_t *out_last, int *out_gather, uint64_t *out_scratch_bytes) {
    VDB_API_BEGIN
    (void)limit;  // (the range call has no cap on it)
    const std::string bad = dup_check_args(n_rows, m_allowed, masked != 0, radius, chunk);
    VDB_REQUIRE(bad.empty(), bad);
    const DupPlan p = dup_plan(n_rows, dim, elem_u8 != 0, masked != 0, m_allowed, chunk);
    if (out_chunks) *out_chunks = p.n_chunks;
    if (out_last) *out_last = p.last_len;
    if (out_gather) *out_gather = p.gather ? 1 : 0;
    if (out_scratch_bytes) *out_scratch_bytes = p.scratch_bytes;
    VDB_API_END
}
// what both forms refuse before a workspace is taken -> the mask as a RowMask (nullptr: all rows)
static const RowMask *dup_groups_check(const Index &ix, float radius, const vdb_mask *mask, const void *out_group, const void *out_stats) {
    VDB_REQUIRE(out_stats && (ix.n == 0 || out_group), "dup groups: null argument");
    if (mask) ix.check_mask(mask->m);
    const std::string bad = dup_check_args(ix.n, mask ? mask->m.m : ix.n, mask != nullptr, radius, ix.dup_chunk);
    VDB_REQUIRE(bad.empty(), bad);
    return mask ? &mask->m : nullptr;
}
int vdb_flat_dup_groups(vdb_index *idx, float radius, uint64_t limit, const vdb_mask *mask, uint64_t *out_group, uint64_t *out_stats) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    const RowMask *rm = dup_groups_check(ix, radius, mask, out_group, out_stats);
    ix.use_device();
    WsLease ws(ix);
    DevBuf d_group;
    d_group.reserve(std::max<uint64_t>(ix.n, 1) * sizeof(uint64_t));
    uint64_t stats[DUP_STATS];
    run_synced(ix, *ws, [&] {
        ix.flat_dup_groups_device(*ws, radius, limit, rm, d_group.as<uint64_t>(), stats);
        if (ix.n) VDB_HIP(hipMemcpyAsync(out_group, d_group.p, ix.n * sizeof(uint64_t), hipMemcpyDeviceToHost, ws->stream));
        VDB_SYNC(ws->stream);
    });
    std::memcpy(out_stats, stats, sizeof(stats));
    VDB_API_END
}
int vdb_flat_dup_groups_device(vdb_index *idx, float radius, uint64_t limit, const vdb_mask *mask, void *d_out_group, uint64_t *out_stats, void *stream) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    const RowMask *rm = dup_groups_check(ix, radius, mask, d_out_group, out_stats);
    VDB_REQUIRE(reinterpret_cast<uintptr_t>(d_out_group) % 8 == 0, "dup groups: d_out_group must be 8-byte aligned");
    ix.use_device();
    WsLease ws(ix);
    VDB_SYNC(static_cast<hipStream_t>(stream));  // order after whatever last used the output on the caller's stream
    uint64_t stats[DUP_STATS];
    run_synced(ix, *ws, [&] { ix.flat_dup_groups_device(*ws, radius, limit, rm, static_cast<uint64_t *>(d_out_group), stats); });
    std::memcpy(out_stats, stats, sizeof(stats));
    VDB_API_END
}
int vdb_link_pairs_device(vdb_index *idx, const void *d_src, const void *d_lims, const void *d_ids, uint64_t nq, void *d_group, uint64_t *out_stats,
                          void *stream) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    VDB_REQUIRE(out_stats && (ix.n == 0 || d_group) && (nq == 0 || (d_src && d_lims && d_ids)), "link pairs: null argument");
    VDB_REQUIRE(nq < (1ull << 32), "link pairs: too many lists for one call");
    VDB_REQUIRE(reinterpret_cast<uintptr_t>(d_src) % 8 == 0 && reinterpret_cast<uintptr_t>(d_lims) % 8 == 0 && reinterpret_cast<uintptr_t>(d_ids) % 8 == 0 &&
                    reinterpret_cast<uintptr_t>(d_group) % 8 == 0,
                "link pairs: the device arrays must be 8-byte aligned");
    ix.use_device();
    WsLease ws(ix);
    VDB_SYNC(static_cast<hipStream_t>(stream));  // order after whatever produced the lists on the caller's stream
    uint64_t stats[DUP_STATS];
    run_synced(ix, *ws, [&] {
        ix.link_pairs_device(*ws, static_cast<const uint64_t *>(d_src), static_cast<const uint64_t *>(d_lims), static_cast<const uint64_t *>(d_ids), nq,
                             static_cast<uint64_t *>(d_group), stats);
    });
    std::memcpy(out_stats, stats, sizeof(stats));
    VDB_API_END
}
int vdb_mask_rows(const vdb_mask *m, uint64_t *out_bits, uint32_t *out_ids) {
    VDB_API_BEGIN
    VDB_REQUIRE(m, "null mask");
    const RowMask &rm = m->m;
    VDB_HIP(hipSetDevice(rm.device));
    const uint64_t nw = (rm.n_rows + 63) / 64;
    if (out_bits && nw) VDB_HIP(hipMemcpy(out_bits, rm.d_bits.p, nw * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (out_ids && rm.m) VDB_HIP(hipMemcpy(out_ids, rm.d_ids.p, rm.m * sizeof(uint32_t), hipMemcpyDeviceToHost));
    VDB_API_END
}

int vdb_mask_count(const vdb_mask *m, uint64_t *out) {
    VDB_API_BEGIN
    VDB_REQUIRE(m && out, "null argument");
    *out = m->m.m;
    VDB_API_END
}

int vdb_mask_destroy(vdb_mask *m) {
    VDB_API_BEGIN
    if (m) {
        (void)hipSetDevice(m->m.device);
        delete m;
    }
    VDB_API_END
}

static void filtered_check(const Index &ix, const vdb_mask *mask) {
    VDB_REQUIRE(mask, "null mask");
    require_f32_rows(ix);
    ix.check_mask(mask->m);
}

int vdb_flat_knn_filtered(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, uint64_t k, const vdb_mask *mask, uint64_t *out_idx,
                          float *out_dist, uint64_t *out_count) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    check_query_args(ix, queries, nq, dim, out_idx, out_dist);
    filtered_check(ix, mask);
    host_search(ix, queries, nq, k, out_idx, out_dist, out_count,
                [&](Workspace &w, const float *q, uint64_t, uint64_t nb, auto... o) { ix.flat_knn_masked_device(w, q, nb, k, mask->m, o...); });
    VDB_API_END
}

int vdb_flat_knn_filtered_device(vdb_index *idx, const void *d_queries, uint64_t nq, uint64_t dim, uint64_t k, const vdb_mask *mask, void *d_out_idx,
                                 void *d_out_dist, void *d_out_count, void *stream) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    check_device_args(ix, d_queries, nq, dim, d_out_idx, d_out_dist, d_out_count);
    filtered_check(ix, mask);
    device_search(ix, d_queries, nq, dim, d_out_idx, d_out_dist, d_out_count, stream,
                  [&](Workspace &w, const float *q, uint64_t, uint64_t nb, auto... o) { ix.flat_knn_masked_device(w, q, nb, k, mask->m, o...); });
    VDB_API_END
}

// one mask per query: everything that can be refused is refused here, before anything is computed or written; -> the masks as RowMask pointers
static std::vector<const RowMask *> filtered_multi_check(const Index &ix, uint64_t nq, const vdb_mask *const *masks, uint64_t n_masks,
                                                         const uint32_t *mask_of, bool knn = true) {
    if (knn) require_f32_rows(ix);
    VDB_REQUIRE(n_masks == 0 || masks, "null masks");
    VDB_REQUIRE(nq == 0 || mask_of, "null mask_of");
    VDB_REQUIRE(n_masks < (1ull << 32), "too many masks");
    std::vector<const RowMask *> rm(n_masks);
    for (uint64_t g = 0; g < n_masks; g++) {
        VDB_REQUIRE(masks[g], "null mask");
        ix.check_mask(masks[g]->m);
        rm[g] = &masks[g]->m;
    }
    for (uint64_t q = 0; q < nq; q++)
        VDB_REQUIRE(mask_of[q] < n_masks, "mask_of[" + std::to_string(q) + "] = " + std::to_string(mask_of[q]) + ": the call has " +
                                              std::to_string(n_masks) + " masks");
    return rm;
}

// the masks of an entry point that takes them optionally (grouped, diversified, by example, fused): none -> unfiltered, no RowMask pointers
static std::vector<const RowMask *> optional_masks_check(const Index &ix, uint64_t rows, const vdb_mask *const *masks, uint64_t n_masks,
                                                         const uint32_t *mask_of) {
    require_f32_rows(ix);
    if (n_masks == 0) return {};
    return filtered_multi_check(ix, rows, masks, n_masks, mask_of);
}

// (the checks and the call counter stay in front of the shared front end: they hold for a call without queries too)
int vdb_flat_knn_filtered_multi(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, uint64_t k, const vdb_mask *const *masks,
                                uint64_t n_masks, const uint32_t *mask_of, uint64_t *out_idx, float *out_dist, uint64_t *out_count) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    check_query_args(ix, queries, nq, dim, out_idx, out_dist);
    const std::vector<const RowMask *> rm = filtered_multi_check(ix, nq, masks, n_masks, mask_of);
    ix.filtered_multi_calls++;
    host_search(ix, queries, nq, k, out_idx, out_dist, out_count, [&](Workspace &w, const float *q, uint64_t q0, uint64_t nb, auto... o) {
        ix.flat_knn_masked_multi_device(w, q, nb, k, rm.data(), n_masks, mask_of + q0, o...);
    });
    VDB_API_END
}

int vdb_flat_knn_filtered_multi_device(vdb_index *idx, const void *d_queries, uint64_t nq, uint64_t dim, uint64_t k, const vdb_mask *const *masks,
                                       uint64_t n_masks, const uint32_t *mask_of, void *d_out_idx, void *d_out_dist, void *d_out_count, void *stream) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    check_device_args(ix, d_queries, nq, dim, d_out_idx, d_out_dist, d_out_count);
    const std::vector<const RowMask *> rm = filtered_multi_check(ix, nq, masks, n_masks, mask_of);
    ix.filtered_multi_calls++;
    device_search(ix, d_queries, nq, dim, d_out_idx, d_out_dist, d_out_count, stream, [&](Workspace &w, const float *q, uint64_t q0, uint64_t nb, auto... o) {
        ix.flat_knn_masked_multi_device(w, q, nb, k, rm.data(), n_masks, mask_of + q0, o...);
    });
    VDB_API_END
}

// ---- grouped k-NN: at most group_size hits per value of one label column (Index::flat_knn_grouped_device, k_group.hip) ------------------
// everything that can be refused is refused here, before anything is computed or written; -> the masks as RowMask pointers (none: unfiltered)
static std::vector<const RowMask *> grouped_check(const Index &ix, uint64_t nq, uint32_t column, uint64_t group_size, const vdb_mask *const *masks,
                                                  uint64_t n_masks, const uint32_t *mask_of) {
    VDB_REQUIRE(group_size >= 1, "grouped k-NN: group_size must be at least 1");
    VDB_REQUIRE(column < LABEL_COLUMNS, "grouped k-NN: column " + std::to_string(column) + ", an index has " + std::to_string(LABEL_COLUMNS));
    return optional_masks_check(ix, nq, masks, n_masks, mask_of);
}

int vdb_flat_knn_grouped(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, uint64_t k, uint32_t column, uint64_t group_size,
                         const vdb_mask *const *masks, uint64_t n_masks, const uint32_t *mask_of, uint64_t *out_idx, float *out_dist,
                         uint64_t *out_count) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    check_query_args(ix, queries, nq, dim, out_idx, out_dist);
    const std::vector<const RowMask *> rm = grouped_check(ix, nq, column, group_size, masks, n_masks, mask_of);
    ix.grouped_calls++;
    host_search(ix, queries, nq, k, out_idx, out_dist, out_count, [&](Workspace &w, const float *q, uint64_t q0, uint64_t nb, auto... o) {
        ix.flat_knn_grouped_device(w, q, nb, k, column, group_size, rm.data(), n_masks, n_masks ? mask_of + q0 : nullptr, o...);
    });
    VDB_API_END
}

int vdb_flat_knn_grouped_device(vdb_index *idx, const void *d_queries, uint64_t nq, uint64_t dim, uint64_t k, uint32_t column, uint64_t group_size,
                                const vdb_mask *const *masks, uint64_t n_masks, const uint32_t *mask_of, void *d_out_idx, void *d_out_dist,
                                void *d_out_count, void *stream) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    check_device_args(ix, d_queries, nq, dim, d_out_idx, d_out_dist, d_out_count);
    const std::vector<const RowMask *> rm = grouped_check(ix, nq, column, group_size, masks, n_masks, mask_of);
    ix.grouped_calls++;
    device_search(ix, d_queries, nq, dim, d_out_idx, d_out_dist, d_out_count, stream, [&](Workspace &w, const float *q, uint64_t q0, uint64_t nb, auto... o) {
        ix.flat_knn_grouped_device(w, q, nb, k, column, group_size, rm.data(), n_masks, n_masks ? mask_of + q0 : nullptr, o...);
    });
    VDB_API_END
}

int vdb_group_cap_device(vdb_index *idx, const void *d_ids, const void *d_dists, const void *d_counts, uint64_t nq, uint64_t ld, uint64_t k,
                         uint32_t column, uint64_t group_size, void *d_out_idx, void *d_out_dist, void *d_out_count, void *stream) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    VDB_REQUIRE(group_size >= 1, "grouped k-NN: group_size must be at least 1");
    VDB_REQUIRE(column < LABEL_COLUMNS, "grouped k-NN: column " + std::to_string(column) + ", an index has " + std::to_string(LABEL_COLUMNS));
    list_form_call(ix, stream, d_ids, d_dists, d_counts, nq, ld, k, d_out_idx, d_out_dist, d_out_count, [&](Workspace &ws) {
        ix.group_cap_device(ws, static_cast<const uint64_t *>(d_ids), static_cast<const float *>(d_dists), static_cast<const uint64_t *>(d_counts), nq, ld, k,
                            column, group_size, static_cast<uint64_t *>(d_out_idx), static_cast<float *>(d_out_dist), static_cast<uint64_t *>(d_out_count));
    });
    VDB_API_END
}

// ---- diversified k-NN: maximal marginal relevance over the fetch_k nearest allowed rows (Index::flat_knn_mmr_device, k_mmr.hip) ---------
// everything that can be refused is refused here, before anything is computed or written; -> the masks as RowMask pointers (none: unfiltered)
static std::vector<const RowMask *> mmr_check(const Index &ix, uint64_t nq, uint64_t k, uint64_t fetch_k, float lambda, const vdb_mask *const *masks,
                                              uint64_t n_masks, const uint32_t *mask_of) {
    const char *bad = mmr_check_args(k, fetch_k, lambda);
    VDB_REQUIRE(bad == nullptr, bad);
    return optional_masks_check(ix, nq, masks, n_masks, mask_of);
}

int vdb_flat_knn_mmr(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, uint64_t k, uint64_t fetch_k, float lambda,
                     const vdb_mask *const *masks, uint64_t n_masks, const uint32_t *mask_of, uint64_t *out_idx, float *out_dist,
                     uint64_t *out_count) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    check_query_args(ix, queries, nq, dim, out_idx, out_dist);
    const std::vector<const RowMask *> rm = mmr_check(ix, nq, k, fetch_k, lambda, masks, n_masks, mask_of);
    ix.mmr_calls++;
    host_search(ix, queries, nq, k, out_idx, out_dist, out_count, [&](Workspace &w, const float *q, uint64_t q0, uint64_t nb, auto... o) {
        ix.flat_knn_mmr_device(w, q, nb, k, fetch_k, lambda, rm.data(), n_masks, n_masks ? mask_of + q0 : nullptr, o...);
    });
    VDB_API_END
}

int vdb_flat_knn_mmr_device(vdb_index *idx, const void *d_queries, uint64_t nq, uint64_t dim, uint64_t k, uint64_t fetch_k, float lambda,
                            const vdb_mask *const *masks, uint64_t n_masks, const uint32_t *mask_of, void *d_out_idx, void *d_out_dist,
                            void *d_out_count, void *stream) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    check_device_args(ix, d_queries, nq, dim, d_out_idx, d_out_dist, d_out_count);
    const std::vector<const RowMask *> rm = mmr_check(ix, nq, k, fetch_k, lambda, masks, n_masks, mask_of);
    ix.mmr_calls++;
    device_search(ix, d_queries, nq, dim, d_out_idx, d_out_dist, d_out_count, stream, [&](Workspace &w, const float *q, uint64_t q0, uint64_t nb, auto... o) {
        ix.flat_knn_mmr_device(w, q, nb, k, fetch_k, lambda, rm.data(), n_masks, n_masks ? mask_of + q0 : nullptr, o...);
    });
    VDB_API_END
}

int vdb_mmr_select_device(vdb_index *idx, const void *d_ids, const void *d_dists, const void *d_counts, uint64_t nq, uint64_t ld, uint64_t k, float lambda,
                          void *d_out_idx, void *d_out_dist, void *d_out_count, void *stream) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    const char *bad = mmr_check_args(k, ld, lambda);
    VDB_REQUIRE(bad == nullptr, bad);
    require_f32_rows(ix);
    list_form_call(ix, stream, d_ids, d_dists, d_counts, nq, ld, k, d_out_idx, d_out_dist, d_out_count, [&](Workspace &ws) {
        ix.mmr_select_device(ws, static_cast<const uint64_t *>(d_ids), static_cast<const float *>(d_dists), static_cast<const uint64_t *>(d_counts), nq, ld, k,
                             lambda, static_cast<uint64_t *>(d_out_idx), static_cast<float *>(d_out_dist), static_cast<uint64_t *>(d_out_count));
    });
    VDB_API_END
}

// ---- search by example rows (Index::flat_knn_like_device / like_queries_device / drop_listed_device, k_like.hip, like_plan.hpp) ----------
// what every form refuses before anything is uploaded: a u8 index, limits the plan refuses, a NULL list with entries
static void like_check_lists(const Index &ix, const uint64_t *pos_lims, const void *pos, const uint64_t *neg_lims, const void *neg, uint64_t nq) {
    require_f32_rows(ix);
    const char *bad = like_check_lims(pos_lims, neg_lims, nq);
    VDB_REQUIRE(bad == nullptr, bad);
    VDB_REQUIRE(pos_lims[nq] == 0 || pos, "like: null positives");
    VDB_REQUIRE(!neg_lims || neg_lims[nq] == 0 || neg, "like: null negatives");
}

// the host forms: every row below len, then [pos_lims | neg_lims | positives u32 | negatives u32] into ws.grp_table with one copy out of
// `blob`, which the caller keeps until the stream has been waited for
static Index::LikeLists like_upload_rows(const Index &ix, Workspace &ws, std::vector<char> &blob, const uint64_t *pos_lims, const uint64_t *pos_rows,
                                         const uint64_t *neg_lims, const uint64_t *neg_rows, uint64_t nq) {
    const uint64_t np = pos_lims[nq], nn = neg_lims ? neg_lims[nq] : 0;
    const size_t lb = (nq + 1) * sizeof(uint64_t), off_nl = lb, off_p = neg_lims ? 2 * lb : lb, off_n = off_p + np * sizeof(uint32_t);
    blob.resize(off_n + nn * sizeof(uint32_t));
    std::memcpy(blob.data(), pos_lims, lb);
    if (neg_lims) std::memcpy(blob.data() + off_nl, neg_lims, lb);
    uint32_t *hp = reinterpret_cast<uint32_t *>(blob.data() + off_p), *hn = reinterpret_cast<uint32_t *>(blob.data() + off_n);
    for (uint64_t j = 0; j < np; j++) hp[j] = (uint32_t)pos_rows[j];
    for (uint64_t j = 0; j < nn; j++) hn[j] = (uint32_t)neg_rows[j];
    ws.grp_table.reserve(blob.size());
    VDB_HIP(hipMemcpyAsync(ws.grp_table.p, blob.data(), blob.size(), hipMemcpyHostToDevice, ws.stream));
    char *d = ws.grp_table.as<char>();
    Index::LikeLists ll;
    ll.pos_lims = reinterpret_cast<const uint64_t *>(d);
    ll.neg_lims = neg_lims ? reinterpret_cast<const uint64_t *>(d + off_nl) : nullptr;
    ll.pos_ids = d + off_p;
    ll.neg_ids = d + off_n;
    ll.global_ids = false;
    ll.e_max = like_e_max(pos_lims, neg_lims, nq);
    ll.n_examples = np + nn;
    return ll;
}
static void like_check_rows(const Index &ix, const uint64_t *lims, const uint64_t *rows, uint64_t nq) {
    for (uint64_t j = 0; lims && j < lims[nq]; j++)
        VDB_REQUIRE(rows[j] < ix.n, "like: row " + std::to_string(rows[j]) + " is no row of this index (len " + std::to_string(ix.n) + ")");
}

// the device forms: [pos_lims | neg_lims] into ws.grp_table, the ids where the caller has them; every id checked with one flag read-back
// (which waits for the stream: the caller's arrays are free again)
static Index::LikeLists like_upload_lims(Index &ix, Workspace &ws, const uint64_t *pos_lims, const void *d_pos_ids, const uint64_t *neg_lims,
                                         const void *d_neg_ids, uint64_t nq) {
    const size_t lb = (nq + 1) * sizeof(uint64_t);
    ws.grp_table.reserve(2 * lb);
    char *d = ws.grp_table.as<char>();
    VDB_HIP(hipMemcpyAsync(d, pos_lims, lb, hipMemcpyHostToDevice, ws.stream));
    if (neg_lims) VDB_HIP(hipMemcpyAsync(d + lb, neg_lims, lb, hipMemcpyHostToDevice, ws.stream));
    Index::LikeLists ll;
    ll.pos_lims = reinterpret_cast<const uint64_t *>(d);
    ll.neg_lims = neg_lims ? reinterpret_cast<const uint64_t *>(d + lb) : nullptr;
    ll.pos_ids = d_pos_ids;
    ll.neg_ids = d_neg_ids;
    ll.global_ids = true;
    ll.e_max = like_e_max(pos_lims, neg_lims, nq);
    ll.n_examples = pos_lims[nq] + (neg_lims ? neg_lims[nq] : 0);
    ix.like_check_ids_device(ws, static_cast<const uint64_t *>(d_pos_ids), pos_lims[nq], static_cast<const uint64_t *>(d_neg_ids),
                             neg_lims ? neg_lims[nq] : 0);
    VDB_SYNC(ws.stream);  // (a call whose lists are all empty has not waited yet)
    return ll;
}
static void like_check_device_ids(const void *d_pos_ids, const void *d_neg_ids) {
    VDB_REQUIRE(reinterpret_cast<uintptr_t>(d_pos_ids) % 8 == 0 && reinterpret_cast<uintptr_t>(d_neg_ids) % 8 == 0, "like: id lists must be 8-byte aligned");
}

int vdb_like_queries(vdb_index *idx, const uint64_t *pos_lims, const uint64_t *pos_rows, const uint64_t *neg_lims, const uint64_t *neg_rows, uint64_t nq,
                     float *out_queries) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    like_check_lists(ix, pos_lims, pos_rows, neg_lims, neg_rows, nq);
    like_check_rows(ix, pos_lims, pos_rows, nq);
    like_check_rows(ix, neg_lims, neg_rows, nq);
    if (nq == 0) return VDB_OK;
    VDB_REQUIRE(out_queries, "null argument");
    ix.use_device();
    WsLease ws(ix);
    hipStream_t s = ws->stream;
    std::vector<char> blob;
    constexpr uint64_t CHUNK = 16384;
    run_synced(ix, *ws, [&] {
        const Index::LikeLists ll = like_upload_rows(ix, *ws, blob, pos_lims, pos_rows, neg_lims, neg_rows, nq);
        ws->q.reserve(std::min(nq, CHUNK) * ix.dim * sizeof(float));
        for (uint64_t q0 = 0; q0 < nq; q0 += CHUNK) {
            const uint64_t nb = std::min<uint64_t>(CHUNK, nq - q0);
            ix.like_queries_device(*ws, ll, q0, nb, ws->q.as<float>());
            VDB_HIP(hipMemcpyAsync(out_queries + q0 * ix.dim, ws->q.p, nb * ix.dim * sizeof(float), hipMemcpyDeviceToHost, s));
            VDB_SYNC(s);
        }
        ix.like_example_rows += ll.n_examples;
    });
    VDB_API_END
}

int vdb_like_queries_device(vdb_index *idx, const uint64_t *pos_lims, const void *d_pos_ids, const uint64_t *neg_lims, const void *d_neg_ids, uint64_t nq,
                            void *d_out_queries, void *stream) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    like_check_lists(ix, pos_lims, d_pos_ids, neg_lims, d_neg_ids, nq);
    like_check_device_ids(d_pos_ids, d_neg_ids);
    if (nq == 0) return VDB_OK;
    VDB_REQUIRE(d_out_queries, "null argument");
    VDB_REQUIRE(reinterpret_cast<uintptr_t>(d_out_queries) % 4 == 0, "like: d_out_queries must be 4-byte aligned");
    ix.use_device();
    WsLease ws(ix);
    VDB_SYNC(static_cast<hipStream_t>(stream));  // order after whatever produced the ids on the caller's stream
    run_synced(ix, *ws, [&] {
        const Index::LikeLists ll = like_upload_lims(ix, *ws, pos_lims, d_pos_ids, neg_lims, d_neg_ids, nq);
        ix.like_queries_device(*ws, ll, 0, nq, static_cast<float *>(d_out_queries));
        VDB_SYNC(ws->stream);
        ix.like_example_rows += ll.n_examples;
    });
    VDB_API_END
}

int vdb_flat_knn_like(vdb_index *idx, const uint64_t *pos_lims, const uint64_t *pos_rows, const uint64_t *neg_lims, const uint64_t *neg_rows, uint64_t nq,
                      uint64_t k, int exclude, const vdb_mask *const *masks, uint64_t n_masks, const uint32_t *mask_of, uint64_t *out_idx,
                      float *out_dist, uint64_t *out_count) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    like_check_lists(ix, pos_lims, pos_rows, neg_lims, neg_rows, nq);
    like_check_rows(ix, pos_lims, pos_rows, nq);
    like_check_rows(ix, neg_lims, neg_rows, nq);
    VDB_REQUIRE(nq == 0 || k == 0 || (out_idx && out_dist), "null argument");
    VDB_REQUIRE(k < (1ull << 31), "flat knn: k too large");
    const std::vector<const RowMask *> rm = optional_masks_check(ix, nq, masks, n_masks, mask_of);
    ix.like_calls++;
    if (nq == 0) return VDB_OK;
    ix.use_device();
    WsLease ws(ix);
    std::vector<char> blob;
    constexpr uint64_t CHUNK = 16384;
    run_synced(ix, *ws, [&] {
        const Index::LikeLists ll = like_upload_rows(ix, *ws, blob, pos_lims, pos_rows, neg_lims, neg_rows, nq);
        ix.like_example_rows += ll.n_examples;
        for (uint64_t q0 = 0; q0 < nq; q0 += CHUNK) {
            const uint64_t nb = std::min<uint64_t>(CHUNK, nq - q0);
            const OutBlock out(*ws, nb, k);
            ix.flat_knn_like_device(*ws, ll, q0, nb, k, exclude != 0, rm.data(), n_masks, n_masks ? mask_of + q0 : nullptr, out.idx(), out.dist(), out.cnt());
            out.download(*ws, out.bytes <= OutBlock::STAGE_MAX, 0, q0, out_idx, out_dist, out_count);
        }
    });
    VDB_API_END
}

int vdb_flat_knn_like_device(vdb_index *idx, const uint64_t *pos_lims, const void *d_pos_ids, const uint64_t *neg_lims, const void *d_neg_ids, uint64_t nq,
                             uint64_t k, int exclude, const vdb_mask *const *masks, uint64_t n_masks, const uint32_t *mask_of, void *d_out_idx,
                             void *d_out_dist, void *d_out_count, void *stream) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    like_check_lists(ix, pos_lims, d_pos_ids, neg_lims, d_neg_ids, nq);
    like_check_device_ids(d_pos_ids, d_neg_ids);
    VDB_REQUIRE(nq == 0 || (d_out_count && (k == 0 || (d_out_idx && d_out_dist))), "null argument");
    VDB_REQUIRE(nq <= 32768, "at most 32768 queries per device call");
    VDB_REQUIRE(k < (1ull << 31), "flat knn: k too large");
    const std::vector<const RowMask *> rm = optional_masks_check(ix, nq, masks, n_masks, mask_of);
    if (nq == 0) {
        ix.like_calls++;
        return VDB_OK;
    }
    ix.use_device();
    WsLease ws(ix);
    VDB_SYNC(static_cast<hipStream_t>(stream));  // order after whatever produced the ids on the caller's stream
    run_synced(ix, *ws, [&] {
        const Index::LikeLists ll = like_upload_lims(ix, *ws, pos_lims, d_pos_ids, neg_lims, d_neg_ids, nq);  // (throws on a bad id)
        ix.like_calls++;
        ix.like_example_rows += ll.n_examples;
        ix.flat_knn_like_device(*ws, ll, 0, nq, k, exclude != 0, rm.data(), n_masks, mask_of, static_cast<uint64_t *>(d_out_idx),
                                static_cast<float *>(d_out_dist), static_cast<uint64_t *>(d_out_count));
    });
    VDB_API_END
}

int vdb_drop_listed_device(vdb_index *idx, const void *d_ids, const void *d_dists, const void *d_counts, uint64_t nq, uint64_t ld, uint64_t k,
                           const uint64_t *drop_lims, const void *d_drop_ids, void *d_out_idx, void *d_out_dist, void *d_out_count, void *stream) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    require_f32_rows(ix);
    const char *bad = like_check_drop_lims(drop_lims, nq);
    VDB_REQUIRE(bad == nullptr, bad);
    VDB_REQUIRE(drop_lims[nq] == 0 || d_drop_ids, "drop listed: null drop list");
    VDB_REQUIRE(reinterpret_cast<uintptr_t>(d_drop_ids) % 8 == 0, "drop listed: d_drop_ids must be 8-byte aligned");
    list_form_check(d_ids, d_dists, d_counts, nq, ld, k, d_out_idx, d_out_dist, d_out_count);
    VDB_REQUIRE(ld < (1ull << 31) && k < (1ull << 31), "drop listed: list length or k too large");  // (refused behind a null argument: no list_form_call)
    list_form_run(ix, stream, nq, [&](Workspace &ws) {
        const size_t lb = (nq + 1) * sizeof(uint64_t);
        ws.grp_table.reserve(lb);
        VDB_HIP(hipMemcpyAsync(ws.grp_table.p, drop_lims, lb, hipMemcpyHostToDevice, ws.stream));
        ix.drop_listed_device(ws, static_cast<const uint64_t *>(d_ids), static_cast<const float *>(d_dists), static_cast<const uint64_t *>(d_counts), nq,
                              ld, k, ws.grp_table.as<uint64_t>(), static_cast<const uint64_t *>(d_drop_ids), drop_lims[nq],
                              static_cast<uint64_t *>(d_out_idx), static_cast<float *>(d_out_dist), static_cast<uint64_t *>(d_out_count));
    });
    VDB_API_END
}

// ---- fused multi-query search: several lists per question joined on the device (Index::flat_knn_fused_device, k_fuse.hip, fuse_plan.hpp) --
// everything that can be refused is refused here, before anything is computed or written; -> the masks as RowMask pointers (none: unfiltered)
static std::vector<const RowMask *> fused_check(const Index &ix, int mode, const uint64_t *lims, uint64_t nq, uint64_t k, uint64_t fetch_k,
                                                const float *weights, float rrf_c, const vdb_mask *const *masks, uint64_t n_masks,
                                                const uint32_t *mask_of) {
    const char *bad = fuse_bad_text(fuse_check_args(mode, lims, nq, k, fetch_k, weights, rrf_c));
    VDB_REQUIRE(bad == nullptr, bad);
    return optional_masks_check(ix, lims[nq], masks, n_masks, mask_of);
}

int vdb_fuse_plan(int mode, const uint64_t *lims, uint64_t nq, uint64_t k, uint64_t fetch_k, const float *weights, float rrf_c, uint64_t budget,
                  int *out_code, uint64_t *out_s_max, uint32_t *out_table_lg, int *out_in_lds, uint64_t *out_scratch_bytes, uint64_t *out_sub_chunk) {
    VDB_API_BEGIN
    VDB_REQUIRE(out_code, "fuse_plan: null out_code");
    *out_code = fuse_check_args(mode, lims, nq, k, fetch_k, weights, rrf_c);
    if (*out_code != FUSE_OK) return VDB_OK;
    const uint64_t s_max = fuse_s_max(lims, nq);
    const uint32_t lg = fuse_table_lg(s_max, fetch_k);
    if (out_s_max) *out_s_max = s_max;
    if (out_table_lg) *out_table_lg = lg;
    if (out_in_lds) *out_in_lds = fuse_in_lds(lg) ? 1 : 0;
    if (out_scratch_bytes) *out_scratch_bytes = fuse_scratch_bytes(1, lg);
    if (out_sub_chunk) *out_sub_chunk = fuse_sub_chunk(nq, s_max, fetch_k, true, budget ? budget : LIST_BUDGET);
    VDB_API_END
}

int vdb_flat_knn_fused(vdb_index *idx, const float *queries, const uint64_t *lims, uint64_t nq, uint64_t dim, uint64_t k, uint64_t fetch_k, int mode,
                       const float *weights, float rrf_c, const vdb_mask *const *masks, uint64_t n_masks, const uint32_t *mask_of, uint64_t *out_idx,
                       float *out_dist, uint64_t *out_count) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    check_query_args(ix, queries, nq, dim, out_idx, out_dist);
    const std::vector<const RowMask *> rm = fused_check(ix, mode, lims, nq, k, fetch_k, weights, rrf_c, masks, n_masks, mask_of);
    ix.fused_calls++;
    if (nq == 0) return VDB_OK;
    ix.use_device();
    WsLease ws(ix);
    hipStream_t s = ws->stream;
    run_synced(ix, *ws, [&] {
        for (uint64_t q0 = 0; q0 < nq;) {  // chunks of whole fused queries with at most FUSE_MAX_SUBQ sub-queries (a fused query has at most 32)
            uint64_t q1 = q0 + 1;
            while (q1 < nq && lims[q1 + 1] - lims[q0] <= FUSE_MAX_SUBQ) q1++;
            const uint64_t nb = q1 - q0, j0 = lims[q0], nj = lims[q1] - j0;
            ws->q.reserve(nj * ix.dim * sizeof(float));
            const OutBlock out(*ws, nb, k);
            VDB_HIP(hipMemcpyAsync(ws->q.p, queries + j0 * ix.dim, nj * ix.dim * sizeof(float), hipMemcpyHostToDevice, s));
            ix.flat_knn_fused_device(*ws, ws->q.as<float>(), lims + q0, nb, k, fetch_k, mode, weights ? weights + j0 : nullptr, rrf_c, rm.data(), n_masks,
                                     n_masks ? mask_of + j0 : nullptr, out.idx(), out.dist(), out.cnt());
            out.download(*ws, out.bytes <= OutBlock::STAGE_MAX, 0, q0, out_idx, out_dist, out_count);
            q0 = q1;
        }
    });
    VDB_API_END
}

int vdb_flat_knn_fused_device(vdb_index *idx, const void *d_queries, const uint64_t *lims, uint64_t nq, uint64_t dim, uint64_t k, uint64_t fetch_k,
                              int mode, const float *weights, float rrf_c, const vdb_mask *const *masks, uint64_t n_masks, const uint32_t *mask_of,
                              void *d_out_idx, void *d_out_dist, void *d_out_count, void *stream) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    check_query_args(ix, d_queries, nq, dim, d_out_idx, d_out_dist);
    VDB_REQUIRE(nq == 0 || d_out_count, "null out_count");
    const std::vector<const RowMask *> rm = fused_check(ix, mode, lims, nq, k, fetch_k, weights, rrf_c, masks, n_masks, mask_of);
    VDB_REQUIRE(lims[nq] <= 32768, "at most 32768 sub-queries per device call");
    ix.fused_calls++;
    if (nq == 0) return VDB_OK;
    ix.use_device();
    WsLease ws(ix);
    VDB_SYNC(static_cast<hipStream_t>(stream));  // order after whatever produced the queries on the caller's stream
    run_synced(ix, *ws, [&] {
        ix.flat_knn_fused_device(*ws, static_cast<const float *>(d_queries), lims, nq, k, fetch_k, mode, weights, rrf_c, rm.data(), n_masks, mask_of,
                                 static_cast<uint64_t *>(d_out_idx), static_cast<float *>(d_out_dist), static_cast<uint64_t *>(d_out_count));
    });
    VDB_API_END
}

int vdb_fuse_lists_device(vdb_index *idx, const void *d_ids, const void *d_dists, const void *d_counts, const uint64_t *lims, uint64_t nq, uint64_t ld,
                          uint64_t k, int mode, const float *weights, float rrf_c, void *d_out_idx, void *d_out_dist, void *d_out_count, void *stream) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    const char *bad = fuse_bad_text(fuse_check_args(mode, lims, nq, k, ld, weights, rrf_c, true));
    VDB_REQUIRE(bad == nullptr, bad);
    require_f32_rows(ix);
    VDB_REQUIRE(k < (1ull << 31), "fuse lists: k too large");
    list_form_call(ix, stream, d_ids, d_dists, d_counts, nq, ld, k, d_out_idx, d_out_dist, d_out_count, [&](Workspace &ws) {
        ix.fuse_lists_device(ws, static_cast<const uint64_t *>(d_ids), static_cast<const float *>(d_dists), static_cast<const uint64_t *>(d_counts), lims, nq,
                             ld, k, mode, weights, rrf_c, static_cast<uint64_t *>(d_out_idx), static_cast<float *>(d_out_dist),
                             static_cast<uint64_t *>(d_out_count));
    });
    VDB_API_END
}

// ---- document-level fused search: the lists joined by the value of a label column (Index::flat_knn_fused_groups_device, k_fuse_groups.hip) --
// everything that can be refused is refused here, before anything is computed or written; -> the masks as RowMask pointers (none: unfiltered)
static std::vector<const RowMask *> fused_groups_check(const Index &ix, int mode, const uint64_t *lims, uint64_t nq, uint64_t k, uint64_t fetch_k,
                                                       const float *weights, float rrf_c, uint32_t column, const vdb_mask *const *masks,
                                                       uint64_t n_masks, const uint32_t *mask_of) {
    const char *bad = fuse_groups_bad_text(fuse_groups_check_args(mode, lims, nq, k, fetch_k, weights, rrf_c, column));
    VDB_REQUIRE(bad == nullptr, bad);
    return optional_masks_check(ix, lims[nq], masks, n_masks, mask_of);
}

int vdb_fuse_groups_plan(int mode, const uint64_t *lims, uint64_t nq, uint64_t k, uint64_t fetch_k, const float *weights, float rrf_c, uint32_t column,
                         uint64_t budget, int *out_code, uint64_t *out_s_max, uint32_t *out_table_lg, int *out_in_lds, uint64_t *out_scratch_bytes,
                         uint64_t *out_sub_chunk) {
    VDB_API_BEGIN
    VDB_REQUIRE(out_code, "fuse_groups_plan: null out_code");
    *out_code = fuse_groups_check_args(mode, lims, nq, k, fetch_k, weights, rrf_c, column);
    if (*out_code != FUSE_OK) return VDB_OK;
    const uint64_t s_max = fuse_s_max(lims, nq);
    const uint32_t lg = fuse_table_lg(s_max, fetch_k);
    if (out_s_max) *out_s_max = s_max;
    if (out_table_lg) *out_table_lg = lg;
    if (out_in_lds) *out_in_lds = fuse_groups_in_lds(lg) ? 1 : 0;
    if (out_scratch_bytes) *out_scratch_bytes = fuse_groups_scratch_bytes(1, lg);
    if (out_sub_chunk) *out_sub_chunk = fuse_groups_sub_chunk(nq, s_max, fetch_k, true, budget ? budget : LIST_BUDGET);
    VDB_API_END
}

int vdb_flat_knn_fused_groups(vdb_index *idx, const float *queries, const uint64_t *lims, uint64_t nq, uint64_t dim, uint64_t k, uint64_t fetch_k,
                              int mode, const float *weights, float rrf_c, uint32_t column, const vdb_mask *const *masks, uint64_t n_masks,
                              const uint32_t *mask_of, uint64_t *out_idx, float *out_dist, uint64_t *out_count, uint8_t *out_exact) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    check_query_args(ix, queries, nq, dim, out_idx, out_dist);
    const std::vector<const RowMask *> rm = fused_groups_check(ix, mode, lims, nq, k, fetch_k, weights, rrf_c, column, masks, n_masks, mask_of);
    ix.fused_groups_calls++;
    if (nq == 0) return VDB_OK;
    ix.use_device();
    WsLease ws(ix);
    hipStream_t s = ws->stream;
    run_synced(ix, *ws, [&] {
        for (uint64_t q0 = 0; q0 < nq;) {  // chunks of whole fused queries with at most FUSE_MAX_SUBQ sub-queries (a fused query has at most 32)
            uint64_t q1 = q0 + 1;
            while (q1 < nq && lims[q1 + 1] - lims[q0] <= FUSE_MAX_SUBQ) q1++;
            const uint64_t nb = q1 - q0, j0 = lims[q0], nj = lims[q1] - j0;
            ws->q.reserve(nj * ix.dim * sizeof(float));
            const OutBlock out(*ws, nb, k);
            uint8_t *d_exact = nullptr;
            if (out_exact) {  // (grp_q: no buffer of the list calls or of the fusion)
                ws->grp_q.reserve(nb);
                d_exact = ws->grp_q.as<uint8_t>();
            }
            VDB_HIP(hipMemcpyAsync(ws->q.p, queries + j0 * ix.dim, nj * ix.dim * sizeof(float), hipMemcpyHostToDevice, s));
            ix.flat_knn_fused_groups_device(*ws, ws->q.as<float>(), lims + q0, nb, k, fetch_k, mode, weights ? weights + j0 : nullptr, rrf_c, column,
                                            rm.data(), n_masks, n_masks ? mask_of + j0 : nullptr, out.idx(), out.dist(), out.cnt(), d_exact);
            if (out_exact) VDB_HIP(hipMemcpyAsync(out_exact + q0, d_exact, nb, hipMemcpyDeviceToHost, s));
            out.download(*ws, out.bytes <= OutBlock::STAGE_MAX, 0, q0, out_idx, out_dist, out_count);
            q0 = q1;
        }
    });
    VDB_API_END
}

int vdb_flat_knn_fused_groups_device(vdb_index *idx, const void *d_queries, const uint64_t *lims, uint64_t nq, uint64_t dim, uint64_t k,
                                     uint64_t fetch_k, int mode, const float *weights, float rrf_c, uint32_t column, const vdb_mask *const *masks,
                                     uint64_t n_masks, const uint32_t *mask_of, void *d_out_idx, void *d_out_dist, void *d_out_count,
                                     void *d_out_exact, void *stream) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    check_query_args(ix, d_queries, nq, dim, d_out_idx, d_out_dist);
    VDB_REQUIRE(nq == 0 || d_out_count, "null out_count");
    const std::vector<const RowMask *> rm = fused_groups_check(ix, mode, lims, nq, k, fetch_k, weights, rrf_c, column, masks, n_masks, mask_of);
    VDB_REQUIRE(lims[nq] <= 32768, "at most 32768 sub-queries per device call");
    ix.fused_groups_calls++;
    if (nq == 0) return VDB_OK;
    ix.use_device();
    WsLease ws(ix);
    VDB_SYNC(static_cast<hipStream_t>(stream));  // order after whatever produced the queries on the caller's stream
    run_synced(ix, *ws, [&] {
        ix.flat_knn_fused_groups_device(*ws, static_cast<const float *>(d_queries), lims, nq, k, fetch_k, mode, weights, rrf_c, column, rm.data(), n_masks,
                                        mask_of, static_cast<uint64_t *>(d_out_idx), static_cast<float *>(d_out_dist),
                                        static_cast<uint64_t *>(d_out_count), static_cast<uint8_t *>(d_out_exact));
    });
    VDB_API_END
}

int vdb_fuse_groups_device(vdb_index *idx, const void *d_ids, const void *d_dists, const void *d_counts, const uint64_t *lims, uint64_t nq, uint64_t ld,
                           uint64_t k, int mode, const float *weights, float rrf_c, uint32_t column, uint64_t trunc_len, void *d_out_idx,
                           void *d_out_dist, void *d_out_count, void *d_out_exact, void *stream) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    const char *bad = fuse_groups_bad_text(fuse_groups_check_args(mode, lims, nq, k, ld, weights, rrf_c, column, true));
    VDB_REQUIRE(bad == nullptr, bad);
    VDB_REQUIRE(trunc_len >= 1, "fuse groups: trunc_len must be at least 1");
    require_f32_rows(ix);
    VDB_REQUIRE(k < (1ull << 31), "fuse groups: k too large");
    list_form_call(ix, stream, d_ids, d_dists, d_counts, nq, ld, k, d_out_idx, d_out_dist, d_out_count, [&](Workspace &ws) {
        ix.fuse_groups_device(ws, static_cast<const uint64_t *>(d_ids), static_cast<const float *>(d_dists), static_cast<const uint64_t *>(d_counts), lims,
                              nq, ld, k, mode, weights, rrf_c, column, trunc_len, static_cast<uint64_t *>(d_out_idx), static_cast<float *>(d_out_dist),
                              static_cast<uint64_t *>(d_out_count), static_cast<uint8_t *>(d_out_exact));
    });
    VDB_API_END
}

// ---- bulk row fetch (Index::get_rows*) ----------------------------------------------------------------------------------------------
int vdb_index_get_rows(vdb_index *idx, const uint64_t *rows, uint64_t m, float *out) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    idx->ix.get_rows(rows, m, out, true);
    VDB_API_END
}
int vdb_index_get_rows_u8(vdb_index *idx, const uint64_t *rows, uint64_t m, uint8_t *out) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    idx->ix.get_rows(rows, m, out, false);
    VDB_API_END
}
int vdb_index_get_rows_mask(vdb_index *idx, const vdb_mask *mask, float *out) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    VDB_REQUIRE(mask, "null mask");
    idx->ix.check_mask(mask->m);
    idx->ix.get_rows_mask(mask->m, out);
    VDB_API_END
}
int vdb_index_get_rows_device(vdb_index *idx, const void *d_ids, uint64_t m, void *d_out, void *stream) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    VDB_REQUIRE(m <= ~uint64_t(0) / (ix.dim * sizeof(float)), "get_rows: the result does not fit the address space");
    if (m == 0) return VDB_OK;
    VDB_REQUIRE(d_ids && d_out, "get_rows: null argument");
    VDB_REQUIRE(reinterpret_cast<uintptr_t>(d_ids) % 8 == 0 && reinterpret_cast<uintptr_t>(d_out) % 4 == 0,
                "get_rows: d_ids must be 8-byte and d_out 4-byte aligned");
    ix.use_device();
    WsLease ws(ix);
    hipStream_t s = static_cast<hipStream_t>(stream);
    try {
        ix.get_rows_device(*ws, static_cast<const uint64_t *>(d_ids), m, d_out, s);
    } catch (...) {
        (void)hipStreamSynchronize(s);
        throw;
    }
    VDB_API_END
}

int vdb_flat_range_filtered(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, const float *radius, uint64_t limit, const vdb_mask *mask,
                            vdb_range **out) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    range_check(ix, queries, nq, dim, radius, out);
    VDB_REQUIRE(mask, "null mask");
    ix.check_mask(mask->m);
    ix.use_device();
    WsLease ws(ix);
    const RangeArgs a = stage_range_args(ix, *ws, queries, radius, nq);
    range_call(ix, *ws, out, [&](RangeResult &r) { ix.flat_range_device(*ws, a.q, nq, a.r, limit, r, &mask->m); });
    VDB_API_END
}

// one mask per query (Index::flat_range_masked_multi_device); the call counter moves when the call has succeeded
int vdb_flat_range_filtered_multi(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, const float *radius, uint64_t limit,
                                  const vdb_mask *const *masks, uint64_t n_masks, const uint32_t *mask_of, vdb_range **out) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    range_check(ix, queries, nq, dim, radius, out);
    const std::vector<const RowMask *> rm = filtered_multi_check(ix, nq, masks, n_masks, mask_of, false);
    ix.use_device();
    WsLease ws(ix);
    const RangeArgs a = stage_range_args(ix, *ws, queries, radius, nq);
    range_call(ix, *ws, out, [&](RangeResult &r) { ix.flat_range_masked_multi_device(*ws, a.q, nq, a.r, limit, rm.data(), rm.size(), mask_of, r); });
    ix.range_multi_calls++;
    VDB_API_END
}

int vdb_flat_range_filtered_multi_device(vdb_index *idx, const void *d_queries, uint64_t nq, uint64_t dim, const void *d_radius, uint64_t limit,
                                         const vdb_mask *const *masks, uint64_t n_masks, const uint32_t *mask_of, void *stream, vdb_range **out) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    range_check(ix, d_queries, nq, dim, d_radius, out);
    VDB_REQUIRE(nq <= 32768, "at most 32768 queries per device call");
    const std::vector<const RowMask *> rm = filtered_multi_check(ix, nq, masks, n_masks, mask_of, false);
    ix.use_device();
    WsLease ws(ix);
    VDB_SYNC(static_cast<hipStream_t>(stream));  // order after whatever produced the queries on the caller's stream
    range_call(ix, *ws, out, [&](RangeResult &r) {
        ix.flat_range_masked_multi_device(*ws, static_cast<const float *>(d_queries), nq, static_cast<const float *>(d_radius), limit, rm.data(), rm.size(),
                                          mask_of, r);
    });
    ix.range_multi_calls++;
    VDB_API_END
}

int vdb_flat_shortlist_keys(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, int tier, float *out_keys,
                            float *out_qsq, float *out_qerr, float *out_dx4) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx && queries && out_keys, "null argument");
    Index &ix = idx->ix;
    VDB_REQUIRE(dim == ix.dim, "query dimension mismatch");
    VDB_REQUIRE(tier >= 0 && tier <= 2, "tier must be 0 (fp16 operands), 1 (split-bf16 operands) or 2 (8-bit operands, lower-bound keys)");
    ix.use_device();
    WsLease ws(ix);
    ws->q.reserve(nq * ix.dim * sizeof(float));
    VDB_HIP(hipMemcpyAsync(ws->q.p, queries, nq * ix.dim * sizeof(float), hipMemcpyHostToDevice, ws->stream));
    ix.flat_debug_keys(*ws, ws->q.as<float>(), nq, tier, out_keys, out_qsq, out_qerr, out_dx4);
    VDB_API_END
}

int vdb_flat_set_mode(vdb_index *idx, int mode) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    VDB_REQUIRE(mode >= 0 && mode <= 2, "mode must be 0, 1 or 2");
    idx->ix.flat_mode = mode;
    VDB_API_END
}
int vdb_set_param(vdb_index *idx, const char *name, int64_t value) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx && name, "null argument");
    std::string n(name);
    if (n == "mfma_variant")
        mfma_set_variant((int)value);
    else if (n == "flat_share")
        mfma_set_share((int)value);
    else if (n == "flat_gemm")  // 0 auto (more than 64 queries), 1 off, 2 forced
        idx->ix.flat_gemm_mode = (int)value;
    else if (n == "hnsw_dma")
        hnsw_set_dma((int)value);
    else if (n == "hnsw_half")
        hnsw_set_half((int)value);
    else if (n == "ivf_half")
        ivf_set_half((int)value);
    else if (n == "ivf_q8")
        ivf_set_q8((int)value);
    else if (n == "hnsw_build_gpu")
        hnsw_set_build_gpu((int)value);
    else if (n == "hnsw_pool_cap")
        hnsw_set_pool_cap((int)value);
    else if (n == "pq_adc_fast")
        pq_set_adc_fast((int)value);
    else if (n == "pq_sample16")
        pq_set_adc16_sample((int)value);
    else if (n == "pq_adc16")
        pq_set_adc16((int)value);
    else if (n == "pq_adc8_sliced")  // 8-bit codes: 0 = 16 queries per pass on sliced one-byte tables (k_pq_adc8x16), 1 = one query per pass (k_pq_adc8), 2 = 8 per pass on sliced 16-bit tables
        pq_set_adc8_sliced((int)value);
    else if (n == "flat_sample_thin")
        mfma_set_sample_thin((int)value);
    else if (n == "flat_gemm_tw")
        gemm_set_tw((int)value);
    else if (n == "flat_gemm_nt")
        gemm_set_nt((int)value);
    else if (n == "flat_gemm_zigzag")
        gemm_set_zigzag((int)value);
    else if (n == "flat_gemm_block_rows") {
        VDB_REQUIRE(value >= 0, "flat_gemm_block_rows must be >= 0");
        gemm_set_block_rows((uint64_t)value);
    }
    else if (n == "flat_gemm_stagger")
        gemm_set_stagger((int)value);
    else if (n == "flat_gemm_debug")
        idx->ix.flat_gemm_debug = (int)value;
    else if (n == "flat_tail")  // exact stage of the Flat pipeline: 0 fused launch when the shortlist fits 64 rows, 1 separate kernels
        idx->ix.flat_tail_mode = (int)value;
    else if (n == "flat_tail_lb_nw")  // exact stage of the 8-bit pass: waves per query (0 auto, 8 / 4 / 2 / 1)
        flat_tail_lb_set_nw((int)value);
    else if (n == "flat_tail_lb_walk")  // exact stage of the 8-bit pass: 0 windowed walk (default), 1 a selection in every round
        flat_tail_lb_set_walk((int)value);
    else if (n == "flat_small")  // one-launch search of small tables (k_small.hip): 0 auto, 1 off, 2 whenever the shape allows
        idx->ix.flat_small_mode = (int)value;
    else if (n == "flat_small_max_rows")
        idx->ix.flat_small_max_rows = (uint64_t)value;
    else if (n == "flat_half")  // fp16 first pass of large query batches: 0 auto, 1 off, 2 on regardless of the redo rate
        idx->ix.flat_half_mode = (int)value;
    else if (n == "flat_i8")  // 8-bit first pass (L2Sqr): 0 auto, 1 off, 2 on regardless of the redo rate
        idx->ix.flat_i8_mode = (int)value;
    else if (n == "flat_i8_rows") {  // rows its exact stage may walk per query before giving up (multiple of 64)
        VDB_REQUIRE(value >= 64 && value <= 8192 && value % 64 == 0, "flat_i8_rows must be a multiple of 64 in [64, 8192]");
        idx->ix.flat_i8_kprime = (uint32_t)value;
    }
    else if (n == "flat_range_max_results") {  // ceiling on the pairs one range call may return (0: what the device can hold)
        VDB_REQUIRE(value >= 0, "flat_range_max_results must be >= 0");
        idx->ix.range_max_results = (uint64_t)value;
    }
    else if (n == "flat_filtered_direct_max") {  // filtered k-NN: allow-lists of up to this many rows take the gathered strict-order scan
        VDB_REQUIRE(value >= 0, "flat_filtered_direct_max must be >= 0");
        idx->ix.flat_filtered_direct_max = (uint64_t)value;
    }
    else if (n == "flat_grouped_oversample") {  // grouped k-NN: round 0 fetches min(m, k x this) rows per query
        VDB_REQUIRE(value >= 1, "flat_grouped_oversample must be >= 1");
        idx->ix.flat_grouped_oversample = (uint64_t)value;
    }
    else if (n == "fetch_chunk_bytes") {  // bulk row fetch: staging bytes per chunk of the gathered route (a chunk holds at least one row)
        VDB_REQUIRE(value >= 1, "fetch_chunk_bytes must be >= 1");
        idx->ix.fetch_chunk_bytes = (uint64_t)value;
    }
    else if (n == "labels_scatter_max_blocks") {  // scattered label writes: grid cap of their kernels (0: 8 blocks per CU); a small cap makes the grid-stride loop wrap at a small list (tests)
        VDB_REQUIRE(value >= 0 && value <= 0x7FFFFFFF, "labels_scatter_max_blocks must be in 0 .. 2^31-1");
        idx->ix.labels_scatter_max_blocks = (uint32_t)value;
    }
    else if (n == "label_lookup_table_bytes") {  // key lookup: scratch cap of the direct route's slot table (4 B per code of the list's span); 0: sorted route only
        VDB_REQUIRE(value >= 0 && (uint64_t)value <= LOOKUP_TABLE_BYTES_MAX, "label_lookup_table_bytes must be in 0 .. 2^32");
        idx->ix.label_lookup_table_bytes = (uint64_t)value;
    }
    else if (n == "label_lookup_max_blocks") {  // key lookup: grid cap of its kernels (0: 8 blocks per CU); a small cap makes the grid-stride loop wrap on a small table (tests)
        VDB_REQUIRE(value >= 0 && value <= 0x7FFFFFFF, "label_lookup_max_blocks must be in 0 .. 2^31-1");
        idx->ix.label_lookup_max_blocks = (uint32_t)value;
    }
    else if (n == "flat_dup_chunk") {  // near-duplicate grouping: queries (rows of the table) per range call of the self-join
        VDB_REQUIRE(value >= 1 && (uint64_t)value <= DUP_CHUNK_MAX, "flat_dup_chunk must be in 1 .. 2^20");
        idx->ix.dup_chunk = (uint64_t)value;
    }
    else if (n == "debug_alloc_fail_over")  // (testing aid, process-wide) device allocations of at least this many bytes fail; 0 = off
        devbuf_fail_over() = (size_t)value;
    else if (n == "flat_i8_unit_min")  // threshold sample of the 8-bit pass: one value per sampled unit when the units are many (0 auto, 1 off, 2 on from 2 x rank units: tests)
        idx->ix.flat_i8_unit_min = (int)value;
    else if (n == "flat_i8_full")  // second 8-bit attempt of a handful of queries: all candidates at once (0 on, 1 off: rounds of 63 rows)
        idx->ix.flat_i8_full = (int)value;
    else if (n == "flat_i8_refine") {  // hit keys of the 8-bit pass tightened from the fp16 row image before the walk: 0 auto, 1 off, 2 always
        idx->ix.flat_i8_refine = (int)value;
        idx->ix.i8_refine_on = 0;
        idx->ix.i8_refine_calls = 0;
    }
    else if (n == "flat_i8_second")  // second 8-bit attempt with thresholds from the first walk's k-th distances: 0 on, 1 off
        idx->ix.flat_i8_second = (int)value;
    else if (n == "flat_i8_stats") {  // (measurement) collect per-query rounds / hits of the 8-bit pass's exact stage; setting it resets them
        idx->ix.flat_i8_stats = (int)value;
        for (auto &h : idx->ix.i8_rounds_hist) h = 0;
        idx->ix.i8_hits_sum = 0;
        idx->ix.i8_hits_max = 0;
        idx->ix.i8_stat_queries = 0;
    }
    else if (n == "flat_i8_hits") {  // expected hits per query its threshold sample aims at
        VDB_REQUIRE(value >= 256 && value <= 4096, "flat_i8_hits must be in [256, 4096]");
        idx->ix.flat_i8_hits = (uint32_t)value;
    }
    else if (n == "flat_gemm8_sample_res")  // threshold sample of the 8-bit pass: 0 = the filter's kernel form, 1 = chunked staging (no whole-image load first)
        gemm8_set_sample_res((int)value);
    else if (n == "flat_gemm8_nt")
        gemm8_set_nt((int)value);
    else if (n == "flat_gemm8_kc")
        gemm8_set_kc((int)value);
    else if (n == "flat_gemm8_burst")
        gemm8_set_burst((int)value);
    else if (n == "flat_gemm8_res")
        gemm8_set_res((int)value);
    else if (n == "flat_gemm8_coop")
        gemm8_set_coop((int)value);
    else if (n == "flat_gemm8_grid")  // measurement: workgroups of the cooperative filter (a multiple of 32 that the sets divide per XCD; 0 = one per CU)
        gemm8_set_grid((int)value);
    else if (n == "flat_gemm8_epi")  // unit epilogue of its kernel: 0 = scalar key arithmetic + stage carried over units, 1 = the earlier form (A/B, tests)
        gemm8_set_epi((int)value);
    else if (n == "flat_gemm_coop")
        gemm_set_coop((int)value);
    else if (n == "flat_half_kmul") {  // its shortlist: max(64, kmul * k) rows per query
        VDB_REQUIRE(value >= 1 && value <= 64, "flat_half_kmul must be in [1, 64]");
        idx->ix.flat_half_kmul = (uint32_t)value;
    }
    else
        throw Error(VDB_ERR_INVALID, "unknown parameter " + n);
    VDB_API_END
}
int vdb_index_prepare(vdb_index *idx, int all_tiers) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    require_gpu();
    idx->ix.prepare_flat(all_tiers != 0);
    VDB_API_END
}
int vdb_flat_fallback_count(const vdb_index *idx, uint64_t *out) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx && out, "null argument");
    *out = idx->ix.fallback_count.load();
    VDB_API_END
}

int vdb_get_stat(const vdb_index *idx, const char *name, uint64_t *out) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx && name && out, "null argument");
    std::string n(name);
    if (n == "flat_fallback")
        *out = idx->ix.fallback_count.load();
    else if (n == "flat_half_queries")
        *out = idx->ix.half_queries.load();
    else if (n == "flat_half_redo")
        *out = idx->ix.half_redo.load();
    else if (n == "flat_half_valid")
        *out = idx->ix.half_m.valid ? 1 : 0;
    else if (n == "flat_gemm_coop_sets")  // the same of the fp16 / split-bf16 filter kernel
        *out = gemm_last_coop();
    else if (n == "flat_gemm8_coop_sets")  // workgroups per cooperative set of the most recent 8-bit filter launch of the process (0: none)
        *out = gemm8_last_coop();
    else if (n == "flat_i8_queries")
        *out = idx->ix.i8_queries.load();
    else if (n == "flat_i8_redo")
        *out = idx->ix.i8_redo.load();
    else if (n == "flat_i8_valid")
        *out = idx->ix.i8_m.valid ? 1 : 0;
    else if (n == "flat_range_queries")  // range calls: queries | answered by the 8-bit tier | by the strict-order scan | hits of the tier's | pairs returned
        *out = idx->ix.range_queries.load();
    else if (n == "flat_range_i8_queries")
        *out = idx->ix.range_i8_queries.load();
    else if (n == "flat_range_scan_queries")
        *out = idx->ix.range_scan_queries.load();
    else if (n == "flat_range_hits")
        *out = idx->ix.range_hits.load();
    else if (n == "flat_range_hits_max")  // (longest hit list of a query the tier answered)
        *out = idx->ix.range_hits_max.load();
    else if (n == "flat_range_results")
        *out = idx->ix.range_results.load();
    else if (n == "flat_filtered_queries")  // filtered k-NN: queries | answered by the direct path | through the 8-bit tier | of those, handed on to the direct path
        *out = idx->ix.filtered_queries.load();
    else if (n == "flat_filtered_direct_queries")
        *out = idx->ix.filtered_direct_queries.load();
    else if (n == "flat_filtered_i8_queries")
        *out = idx->ix.filtered_i8_queries.load();
    else if (n == "flat_filtered_fallback_queries")
        *out = idx->ix.filtered_fallback_queries.load();
    else if (n == "flat_filtered_multi_calls")  // calls with a mask per query | queries their grouped launch answered
        *out = idx->ix.filtered_multi_calls.load();
    else if (n == "flat_filtered_grouped_queries")
        *out = idx->ix.filtered_grouped_queries.load();
    else if (n == "flat_range_multi_calls")  // range calls with a mask per query | queries their grouped launch answered
        *out = idx->ix.range_multi_calls.load();
    else if (n == "flat_range_grouped_queries")
        *out = idx->ix.range_grouped_queries.load();
    else if (n.rfind("flat_i8_rounds_", 0) == 0 && n.size() == 16 && n[15] >= '0' && n[15] <= '8')  // queries whose exact stage walked N rounds (8: 8 or more)
        *out = idx->ix.i8_rounds_hist[n[15] - '0'].load();
    else if (n == "mirror_alloc_failures")  // mirrors of this index whose allocation failed (the tier was left to the next one)
        *out = idx->ix.mirror_alloc_failures.load();
    else if (n == "flat_i8_second_queries")  // queries that took the second 8-bit attempt / that it passed on to the fp16 tier
        *out = idx->ix.i8_second_queries.load();
    else if (n == "flat_i8_second_redo")
        *out = idx->ix.i8_second_redo.load();
    else if (n == "flat_i8_hits_sum")
        *out = idx->ix.i8_hits_sum.load();
    else if (n == "flat_i8_hits_max")
        *out = idx->ix.i8_hits_max.load();
    else if (n == "flat_i8_stat_queries")
        *out = idx->ix.i8_stat_queries.load();
    else if (n == "flat_i8_rows_walked")
        *out = idx->ix.i8_rows_walked.load();
    else if (n == "flat_bf16_mirror")
        *out = idx->ix.tiled_built ? 1 : 0;
    else if (n == "hnsw_heap_walk_queries")
        *out = idx->ix.hnsw.heap_walk_queries.load();
    else if (n == "hnsw_half_dropped")
        *out = idx->ix.hnsw.last_half_dropped.load();
    else if (n == "ivf_last_offers")
        *out = idx->ix.ivf.last_offers.load();
    else if (n == "ivf_last_rows_fetched_q8")
        *out = idx->ix.ivf.last_rows_fetched_q8.load();
    else if (n == "ivf_last_kept_q8")
        *out = idx->ix.ivf.last_kept_q8.load();
    else if (n == "ivf_last_kept")
        *out = idx->ix.ivf.last_kept.load();
    else if (n == "pq_adc16_queries")
        *out = idx->ix.pq.adc16_queries.load();
    else if (n == "pq_adc16_redo")
        *out = idx->ix.pq.adc16_redo.load();
    else if (n == "flat_i8_refine_queries")
        *out = idx->ix.i8_refine_queries.load();
    else if (n == "flat_i8_refine_on")
        *out = (uint64_t)idx->ix.i8_refine_on.load();
    else if (n == "pq_q8_overflow")
        *out = idx->ix.pq.q8_overflow.load();
    else if (n == "pq_q8_short")
        *out = idx->ix.pq.q8_short.load();
    else if (n == "pq_q8_hits_sum")
        *out = idx->ix.pq.q8_hits_sum.load();
    else if (n == "pq_q8_hits_max")
        *out = idx->ix.pq.q8_hits_max.load();
    else if (n == "mask_where_masks")  // masks built on the device from the label columns (vdb_mask_create_where*)
        *out = idx->ix.mask_where_masks.load();
    else if (n == "mask_where_set_masks")  // masks built from set / range terms (vdb_mask_create_where_sets*)
        *out = idx->ix.mask_where_set_masks.load();
    else if (n == "mask_where_any_masks")  // masks built from an OR of conjunctions (vdb_mask_create_where_any*)
        *out = idx->ix.mask_where_any_masks.load();
    else if (n == "mask_combine_masks")  // masks built by vdb_mask_combine
        *out = idx->ix.mask_combine_masks.load();
    else if (n == "mask_partition_masks")  // masks built by vdb_mask_create_partition
        *out = idx->ix.mask_partition_masks.load();
    else if (n == "label_count_calls")  // vdb_index_label_counts calls
        *out = idx->ix.label_count_calls.load();
    else if (n == "label_lookup_calls")  // vdb_index_label_lookup: accepted calls | codes they named | calls on the direct route | reads of the column
        *out = idx->ix.label_lookup_calls.load();
    else if (n == "label_lookup_codes")
        *out = idx->ix.label_lookup_codes.load();
    else if (n == "label_lookup_direct")
        *out = idx->ix.label_lookup_direct.load();
    else if (n == "label_lookup_passes")
        *out = idx->ix.label_lookup_passes.load();
    else if (n == "flat_dup_calls")  // vdb_flat_dup_groups / _device: calls that succeeded | range calls (chunks) under them | non-self pairs they saw
        *out = idx->ix.dup_calls.load();
    else if (n == "flat_dup_chunks")
        *out = idx->ix.dup_chunks.load();
    else if (n == "flat_dup_pairs")
        *out = idx->ix.dup_pairs.load();
    else if (n == "flat_grouped_calls")  // grouped k-NN: calls | queries | rounds run, summed over calls | queries whose last list was their whole allowed set
        *out = idx->ix.grouped_calls.load();
    else if (n == "flat_grouped_queries")
        *out = idx->ix.grouped_queries.load();
    else if (n == "flat_grouped_rounds")
        *out = idx->ix.grouped_rounds.load();
    else if (n == "flat_grouped_exhausted_queries")
        *out = idx->ix.grouped_exhausted.load();
    else if (n == "flat_mmr_calls")  // diversified k-NN: calls | queries
        *out = idx->ix.mmr_calls.load();
    else if (n == "flat_mmr_queries")
        *out = idx->ix.mmr_queries.load();
    else if (n == "flat_like_calls")  // search by example rows: calls | queries (the two search forms) | list entries the builder walked
        *out = idx->ix.like_calls.load();
    else if (n == "flat_like_queries")
        *out = idx->ix.like_queries.load();
    else if (n == "like_example_rows")
        *out = idx->ix.like_example_rows.load();
    else if (n == "flat_fused_calls")  // fused multi-query search: calls | fused queries | sub-queries (the two search forms)
        *out = idx->ix.fused_calls.load();
    else if (n == "flat_fused_queries")
        *out = idx->ix.fused_queries.load();
    else if (n == "flat_fused_lists")
        *out = idx->ix.fused_lists.load();
    else if (n == "flat_fused_groups_calls")  // document-level fused search: calls | fused queries | sub-queries (the two search forms)
        *out = idx->ix.fused_groups_calls.load();
    else if (n == "flat_fused_groups_queries")
        *out = idx->ix.fused_groups_queries.load();
    else if (n == "flat_fused_groups_lists")
        *out = idx->ix.fused_groups_lists.load();
    else if (n == "update_calls")  // vdb_index_update_rows* calls that changed rows | rows they rewrote
        *out = idx->ix.update_calls.load();
    else if (n == "update_rows")
        *out = idx->ix.updated_rows.load();
    else if (n == "fetch_calls")  // vdb_index_get_rows* calls that fetched rows | rows returned | gather launches | calls answered by a plain copy
        *out = idx->ix.fetch_calls.load();
    else if (n == "fetch_rows")
        *out = idx->ix.fetch_rows.load();
    else if (n == "fetch_chunks")
        *out = idx->ix.fetch_chunks.load();
    else if (n == "fetch_direct")
        *out = idx->ix.fetch_direct.load();
    else if (n == "labels_scatter_calls")  // vdb_index_labels_scatter / _device / _set_mask calls that wrote rows | rows they wrote | list entries per launch before the grid-stride loop wraps
        *out = idx->ix.labels_scatter_calls.load();
    else if (n == "labels_scatter_rows")
        *out = idx->ix.labels_scatter_rows.load();
    else if (n == "labels_scatter_span")
        *out = labels_scatter_span(idx->ix.num_cu, idx->ix.labels_scatter_max_blocks);
    else if (n == "label_columns")  // allocated label columns (4 B per row each)
        *out = idx->ix.label_columns();
    else if (n == "hbm_bytes_per_row")
        *out = idx->ix.hbm_bytes_per_row();
    else
        throw Error(VDB_ERR_INVALID, "unknown statistic " + n);
    VDB_API_END
}

// ---- PQ -------------------------------------------------------------------------------------------
int vdb_pq_attach(vdb_index *idx, uint64_t n_bits, uint64_t m, const float *centroids, const uint8_t *codes) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx && centroids, "null argument");
    pq_attach(idx->ix, n_bits, m, centroids, codes);
    VDB_API_END
}
int vdb_pq_build(vdb_index *idx, uint64_t n_bits, uint64_t m, uint64_t train_n, uint64_t max_iter, float tol,
                 uint64_t seed) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    pq_build(idx->ix, n_bits, m, train_n, max_iter, tol, seed);
    VDB_API_END
}
int vdb_pq_clear(vdb_index *idx) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    pq_clear(idx->ix);
    VDB_API_END
}
int vdb_pq_has(const vdb_index *idx, int *out) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx && out, "null argument");
    *out = idx->ix.pq.present ? 1 : 0;
    VDB_API_END
}
int vdb_pq_info(const vdb_index *idx, uint64_t *n_bits, uint64_t *m, uint64_t *enc_dim) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    VDB_REQUIRE(idx->ix.pq.present, "no PQ table");
    if (n_bits) *n_bits = idx->ix.pq.n_bits;
    if (m) *m = idx->ix.pq.m;
    if (enc_dim) *enc_dim = idx->ix.pq.enc_dim;
    VDB_API_END
}
int vdb_pq_export(const vdb_index *idx, float *centroids, uint8_t *codes) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    const Index &ix = idx->ix;
    VDB_REQUIRE(ix.pq.present, "no PQ table");
    if (centroids) std::memcpy(centroids, ix.pq.h_centroids.data(), ix.pq.h_centroids.size() * sizeof(float));
    if (codes && ix.n) {
        ix.use_device();
        VDB_HIP(hipMemcpy(codes, ix.pq.d_codes.p, ix.n * ix.pq.enc_dim, hipMemcpyDeviceToHost));
    }
    VDB_API_END
}

int vdb_flat_knn_pq(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, uint64_t k, uint64_t ef,
                    uint64_t *out_idx, float *out_dist, uint64_t *out_count) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    check_query_args(ix, queries, nq, dim, out_idx, out_dist);
    VDB_REQUIRE(ix.pq.present, "knn_pq needs a PQ table (vdb_pq_build / vdb_pq_attach)");
    host_search(ix, queries, nq, k, out_idx, out_dist, out_count,
                [&](Workspace &w, const float *q, uint64_t, uint64_t nb, auto... o) { flat_knn_pq_device(ix, w, q, nb, k, ef, o...); });
    VDB_API_END
}

int vdb_flat_knn_pq_device(vdb_index *idx, const void *d_queries, uint64_t nq, uint64_t dim, uint64_t k, uint64_t ef,
                           void *d_out_idx, void *d_out_dist, void *d_out_count, void *stream) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    VDB_REQUIRE(ix.pq.present, "knn_pq needs a PQ table (vdb_pq_build / vdb_pq_attach)");
    device_search(ix, d_queries, nq, dim, d_out_idx, d_out_dist, d_out_count, stream,
                  [&](Workspace &w, const float *q, uint64_t, uint64_t nb, auto... o) { flat_knn_pq_device(ix, w, q, nb, k, ef, o...); });
    VDB_API_END
}

// PQTable::create_lookup (pq_table.rs:195-224) / the ADC adapter over every row (pq_table.rs:239-301)
static const float *stage_queries(Index &ix, Workspace &ws, const float *queries, uint64_t nq) {
    ws.q.reserve(std::max<uint64_t>(nq, 1) * ix.dim * sizeof(float));
    VDB_HIP(hipMemcpyAsync(ws.q.p, queries, nq * ix.dim * sizeof(float), hipMemcpyHostToDevice, ws.stream));
    return ws.q.as<float>();
}
int vdb_pq_create_lookup(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, float *out_lut, float *out_qcache) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    VDB_REQUIRE(dim == ix.dim, "query dimension mismatch");  // assert_eq!(query.len(), self.dim) pq_table.rs:196
    VDB_REQUIRE(nq == 0 || queries, "null argument");
    VDB_REQUIRE(ix.pq.present, "create_lookup needs a PQ table (vdb_pq_build / vdb_pq_attach)");
    VDB_REQUIRE(nq <= 65535, "at most 65535 queries per call");
    if (nq == 0) return VDB_OK;
    ix.use_device();
    WsLease ws(ix);
    pq_export_lookup(ix, *ws, stage_queries(ix, *ws, queries, nq), nq, out_lut, out_qcache);
    VDB_API_END
}
int vdb_pq_adc_all(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, float *out) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    VDB_REQUIRE(dim == ix.dim, "query dimension mismatch");
    VDB_REQUIRE(nq == 0 || (queries && out), "null argument");
    VDB_REQUIRE(ix.pq.present, "ADC needs a PQ table (vdb_pq_build / vdb_pq_attach)");
    VDB_REQUIRE(nq <= 65535, "at most 65535 queries per call");
    if (nq == 0) return VDB_OK;
    ix.use_device();
    WsLease ws(ix);
    pq_export_adc_all(ix, *ws, stage_queries(ix, *ws, queries, nq), nq, out);
    VDB_API_END
}

// ---- row-sharded knn_pq ------------------------------------------------------------------
int vdb_flat_knn_pq_shard(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, uint64_t k, uint64_t ef,
                          uint64_t *out_adc_keys, uint64_t *out_exact_keys) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    check_query_args(ix, queries, nq, dim, out_adc_keys, out_exact_keys);
    VDB_REQUIRE(ix.pq.present, "knn_pq needs a PQ table (vdb_pq_build / vdb_pq_attach)");
    VDB_REQUIRE(nq <= 32768, "at most 32768 queries per shard call");
    if (nq == 0) return VDB_OK;
    const uint64_t efg = std::max(ef, k);
    ix.use_device();
    WsLease ws(ix);
    hipStream_t s = ws->stream;
    ws->q.reserve(nq * ix.dim * sizeof(float));
    ws->out_idx.reserve(2 * nq * std::max<uint64_t>(efg, 1) * sizeof(uint64_t));
    uint64_t *d_adc = ws->out_idx.as<uint64_t>(), *d_exact = d_adc + nq * efg;
    VDB_HIP(hipMemcpyAsync(ws->q.p, queries, nq * ix.dim * sizeof(float), hipMemcpyHostToDevice, s));
    flat_knn_pq_shard_device(ix, *ws, ws->q.as<float>(), nq, k, ef, d_adc, d_exact);
    VDB_HIP(hipMemcpyAsync(out_adc_keys, d_adc, nq * efg * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    VDB_HIP(hipMemcpyAsync(out_exact_keys, d_exact, nq * efg * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    VDB_SYNC(s);
    ix.prof_collect(*ws);
    VDB_API_END
}

int vdb_flat_knn_pq_shard_device(vdb_index *idx, const void *d_queries, uint64_t nq, uint64_t dim, uint64_t k,
                                 uint64_t ef, void *d_out_adc_keys, void *d_out_exact_keys, void *stream) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    check_query_args(ix, d_queries, nq, dim, d_out_adc_keys, d_out_exact_keys);
    VDB_REQUIRE(ix.pq.present, "knn_pq needs a PQ table (vdb_pq_build / vdb_pq_attach)");
    VDB_REQUIRE(nq <= 32768, "at most 32768 queries per shard call");
    if (nq == 0) return VDB_OK;
    ix.use_device();
    WsLease ws(ix);
    VDB_SYNC(static_cast<hipStream_t>(stream));
    flat_knn_pq_shard_device(ix, *ws, static_cast<const float *>(d_queries), nq, k, ef,
                             static_cast<uint64_t *>(d_out_adc_keys), static_cast<uint64_t *>(d_out_exact_keys));
    VDB_SYNC(ws->stream);
    ix.prof_collect(*ws);
    VDB_API_END
}

// host merge (no GPU needed): S rows per query sorted by ADC key -> global ADC top-efk -> ResultSet::add replay over
// the exact keys in that order (candidate_pair.rs:61-74,102-108)
int vdb_pq_merge_resort(const uint64_t *adc_keys, const uint64_t *exact_keys, uint64_t n_shards, uint64_t nq,
                        uint64_t efk, uint64_t k, uint64_t *out_idx, float *out_dist, uint64_t *out_count) {
    VDB_API_BEGIN
    VDB_REQUIRE(nq == 0 || (adc_keys && exact_keys && out_idx && out_dist), "null argument");
    VDB_REQUIRE(efk >= k, "pq merge: efk = max(ef, k) must be >= k");
    std::vector<std::pair<uint64_t, uint64_t>> all;
    std::vector<uint64_t> set;  // the ResultSet, ascending pair keys
    for (uint64_t q = 0; q < nq; q++) {
        all.clear();
        for (uint64_t s = 0; s < n_shards; s++)
            for (uint64_t j = 0; j < efk; j++) {
                uint64_t a = adc_keys[(s * nq + q) * efk + j];
                if (a != PAIR_NONE) all.push_back({a, exact_keys[(s * nq + q) * efk + j]});
            }
        std::sort(all.begin(), all.end());
        if (all.size() > efk) all.resize(efk);
        set.clear();
        for (auto &pr : all) {
            uint64_t e = pr.second;
            if (k == 0) break;
            if (set.size() >= k) {
                if (uint32_t(e >> 32) >= uint32_t(set.back() >> 32)) continue;  // not strictly closer than the worst
                set.pop_back();
            }
            set.insert(std::lower_bound(set.begin(), set.end(), e), e);
        }
        for (uint64_t j = 0; j < k; j++) {
            bool ok = j < set.size();
            out_idx[q * k + j] = ok ? uint64_t(uint32_t(set[j])) : 0;
            out_dist[q * k + j] = ok ? f32_from_orderable(uint32_t(set[j] >> 32)) : 0.0f;
        }
        if (out_count) out_count[q] = set.size();
    }
    VDB_API_END
}

int vdb_pq_merge_resort_device(vdb_index *idx, const void *d_adc_keys, const void *d_exact_keys, uint64_t n_shards,
                               uint64_t nq, uint64_t efk, uint64_t k, void *d_out_idx, void *d_out_dist,
                               void *d_out_count, void *stream) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx && d_adc_keys && d_exact_keys && d_out_idx && d_out_dist && d_out_count, "null argument");
    VDB_REQUIRE(nq <= 65535 && n_shards >= 1 && n_shards <= 1024, "too many queries or shards for one call");
    Index &ix = idx->ix;
    ix.use_device();
    WsLease ws(ix);
    VDB_SYNC(static_cast<hipStream_t>(stream));
    pq_merge_resort_device(ix, *ws, static_cast<const uint64_t *>(d_adc_keys),
                           static_cast<const uint64_t *>(d_exact_keys), n_shards, nq, efk, k,
                           static_cast<uint64_t *>(d_out_idx), static_cast<float *>(d_out_dist),
                           static_cast<uint64_t *>(d_out_count));
    VDB_SYNC(ws->stream);
    VDB_API_END
}

// ---- IVF (index_algorithm/ivf_index.rs) --------------------------------------------------------------
int vdb_ivf_build(vdb_index *idx, uint64_t k_clusters, uint64_t train_n, uint64_t max_iter, float tol, uint64_t seed) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    ivf_build(idx->ix, k_clusters, train_n, max_iter, tol, seed);
    VDB_API_END
}
int vdb_ivf_attach(vdb_index *idx, uint64_t k_clusters, const float *centroids, const uint64_t *assign) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    ivf_attach(idx->ix, k_clusters, centroids, assign);
    VDB_API_END
}
int vdb_ivf_clear(vdb_index *idx) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    ivf_clear(idx->ix);
    VDB_API_END
}
int vdb_ivf_info(const vdb_index *idx, int *present, uint64_t *k_clusters, uint64_t *default_n_probes) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    if (present) *present = idx->ix.ivf.present ? 1 : 0;
    if (k_clusters) *k_clusters = idx->ix.ivf.k;
    if (default_n_probes) *default_n_probes = idx->ix.ivf.default_n_probes;
    VDB_API_END
}
int vdb_ivf_export(vdb_index *idx, float *centroids, uint64_t *assign) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    ivf_export(idx->ix, centroids, assign);
    VDB_API_END
}
int vdb_ivf_knn(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, uint64_t k, uint64_t n_probes,
                uint64_t *out_idx, float *out_dist, uint64_t *out_count) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    check_query_args(ix, queries, nq, dim, out_idx, out_dist);
    VDB_REQUIRE(ix.ivf.present, "knn needs an IVF index (vdb_ivf_build / vdb_ivf_attach)");
    if (n_probes == 0) n_probes = ix.ivf.default_n_probes;
    host_search(ix, queries, nq, k, out_idx, out_dist, out_count,
                [&](Workspace &w, const float *q, uint64_t, uint64_t nb, auto... o) { ivf_knn_device(ix, w, q, nb, k, n_probes, o...); });
    VDB_API_END
}

int vdb_ivf_knn_device(vdb_index *idx, const void *d_queries, uint64_t nq, uint64_t dim, uint64_t k, uint64_t n_probes,
                       void *d_out_idx, void *d_out_dist, void *d_out_count, void *stream) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    VDB_REQUIRE(ix.ivf.present, "knn needs an IVF index (vdb_ivf_build / vdb_ivf_attach)");
    if (n_probes == 0) n_probes = ix.ivf.default_n_probes;
    device_search(ix, d_queries, nq, dim, d_out_idx, d_out_dist, d_out_count, stream,
                  [&](Workspace &w, const float *q, uint64_t, uint64_t nb, auto... o) { ivf_knn_device(ix, w, q, nb, k, n_probes, o...); });
    VDB_API_END
}

// ---- HNSW -----------------------------------------------------------------------------------------
int vdb_hnsw_build(vdb_index *idx, uint64_t M, uint64_t ef_construction, uint64_t seed, uint64_t batch,
                   int nthreads) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    hnsw_build(idx->ix, M, ef_construction, seed, batch, nthreads);
    VDB_API_END
}
int vdb_hnsw_attach(vdb_index *idx, uint64_t M, uint64_t ef_construction, const uint32_t *level0,
                    const uint64_t *len0, const uint64_t *vec_level, const uint32_t *upper,
                    const uint64_t *upper_len, int has_enter, uint64_t enter_point, uint64_t enter_level) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    hnsw_attach(idx->ix, M, ef_construction, level0, len0, vec_level, upper, upper_len, has_enter, enter_point,
                enter_level);
    VDB_API_END
}
int vdb_hnsw_clear(vdb_index *idx) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    hnsw_clear(idx->ix);
    VDB_API_END
}
int vdb_hnsw_has(const vdb_index *idx, int *out) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx && out, "null argument");
    *out = idx->ix.hnsw.present ? 1 : 0;
    VDB_API_END
}
int vdb_hnsw_info(const vdb_index *idx, uint64_t *m, uint64_t *max_m0, uint64_t *upper_total, int *has_enter,
                  uint64_t *enter_point, uint64_t *enter_level, uint64_t *default_ef) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    const HNSWState &h = idx->ix.hnsw;
    VDB_REQUIRE(h.present, "no HNSW graph");
    if (m) *m = h.m;
    if (max_m0) *max_m0 = h.max_m0;
    if (upper_total) *upper_total = h.upper_len.size();
    if (has_enter) *has_enter = h.has_enter ? 1 : 0;
    if (enter_point) *enter_point = h.enter_point;
    if (enter_level) *enter_level = h.enter_level;
    if (default_ef) *default_ef = h.default_ef;
    VDB_API_END
}
int vdb_hnsw_export(const vdb_index *idx, uint32_t *level0, uint64_t *len0, uint64_t *vec_level, uint32_t *upper,
                    uint64_t *upper_len) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    const HNSWState &h = idx->ix.hnsw;
    VDB_REQUIRE(h.present, "no HNSW graph");
    if (level0) std::memcpy(level0, h.level0.data(), h.level0.size() * sizeof(uint32_t));
    if (len0) std::memcpy(len0, h.len0.data(), h.len0.size() * sizeof(uint64_t));
    if (vec_level) std::memcpy(vec_level, h.vec_level.data(), h.vec_level.size() * sizeof(uint64_t));
    if (upper) std::memcpy(upper, h.upper.data(), h.upper.size() * sizeof(uint32_t));
    if (upper_len) std::memcpy(upper_len, h.upper_len.data(), h.upper_len.size() * sizeof(uint64_t));
    VDB_API_END
}

int vdb_hnsw_knn(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, uint64_t k, uint64_t ef,
                 uint64_t *out_idx, float *out_dist, uint64_t *out_count) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    check_query_args(ix, queries, nq, dim, out_idx, out_dist);
    VDB_REQUIRE(ix.hnsw.present, "knn_with_ef needs an HNSW graph (vdb_hnsw_build / vdb_hnsw_attach)");
    if (ef == 0) ef = ix.hnsw.default_ef;
    host_search(ix, queries, nq, k, out_idx, out_dist, out_count,
                [&](Workspace &w, const float *q, uint64_t, uint64_t nb, auto... o) { hnsw_knn_device(ix, w, q, nb, k, ef, false, o...); });
    VDB_API_END
}
int vdb_hnsw_knn_pq(vdb_index *idx, const float *queries, uint64_t nq, uint64_t dim, uint64_t k, uint64_t ef,
                    uint64_t *out_idx, float *out_dist, uint64_t *out_count) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    check_query_args(ix, queries, nq, dim, out_idx, out_dist);
    VDB_REQUIRE(ix.hnsw.present, "knn_pq needs an HNSW graph");
    VDB_REQUIRE(ix.pq.present, "knn_pq needs a PQ table");
    host_search(ix, queries, nq, k, out_idx, out_dist, out_count,
                [&](Workspace &w, const float *q, uint64_t, uint64_t nb, auto... o) { hnsw_knn_device(ix, w, q, nb, k, ef, true, o...); });
    VDB_API_END
}
int vdb_hnsw_knn_device(vdb_index *idx, const void *d_queries, uint64_t nq, uint64_t dim, uint64_t k, uint64_t ef,
                        int use_pq, void *d_out_idx, void *d_out_dist, void *d_out_count, void *stream) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    Index &ix = idx->ix;
    VDB_REQUIRE(ix.hnsw.present, "knn_with_ef needs an HNSW graph (vdb_hnsw_build / vdb_hnsw_attach)");
    VDB_REQUIRE(!use_pq || ix.pq.present, "knn_pq needs a PQ table");
    if (ef == 0) ef = ix.hnsw.default_ef;
    device_search(ix, d_queries, nq, dim, d_out_idx, d_out_dist, d_out_count, stream,
                  [&](Workspace &w, const float *q, uint64_t, uint64_t nb, auto... o) { hnsw_knn_device(ix, w, q, nb, k, ef, use_pq != 0, o...); });
    VDB_API_END
}
int vdb_hnsw_last_stats(const vdb_index *idx, uint64_t *n_dist, uint64_t *n_expanded) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    if (n_dist) *n_dist = idx->ix.hnsw.last_n_dist.load();
    if (n_expanded) *n_expanded = idx->ix.hnsw.last_n_expanded.load();
    VDB_API_END
}

// ---- shard merge ------------------------------------------------------------------------------------
int vdb_merge_topk(const float *dists, const uint64_t *ids, const uint64_t *counts, uint64_t n_shards, uint64_t nq,
                   uint64_t k, uint64_t *out_idx, float *out_dist, uint64_t *out_count) {
    VDB_API_BEGIN
    VDB_REQUIRE(dists && ids && counts && out_idx && out_dist, "null argument");
    struct P {
        uint32_t o;
        uint64_t i;
    };
    std::vector<P> all;
    for (uint64_t q = 0; q < nq; q++) {
        all.clear();
        for (uint64_t s = 0; s < n_shards; s++) {
            uint64_t c = std::min<uint64_t>(counts[s * nq + q], k);
            for (uint64_t j = 0; j < c; j++)
                all.push_back({f32_orderable(dists[(s * nq + q) * k + j]), ids[(s * nq + q) * k + j]});
        }
        std::sort(all.begin(), all.end(), [](const P &a, const P &b) { return a.o != b.o ? a.o < b.o : a.i < b.i; });
        uint64_t c = std::min<uint64_t>(all.size(), k);
        for (uint64_t j = 0; j < c; j++) {
            out_idx[q * k + j] = all[j].i;
            out_dist[q * k + j] = f32_from_orderable(all[j].o);
        }
        for (uint64_t j = c; j < k; j++) {
            out_idx[q * k + j] = 0;
            out_dist[q * k + j] = 0.0f;
        }
        if (out_count) out_count[q] = c;
    }
    VDB_API_END
}

// ---- merge of S range results (k_range_merge.hip) -----------------------------------------------------
int vdb_range_merge(const uint64_t *lims, const uint64_t *ids, const float *dists, uint64_t n_shards, uint64_t nq, uint64_t pair_stride,
                    uint64_t limit, uint64_t *out_lims, uint64_t *out_idx, float *out_dist) {
    VDB_API_BEGIN
    VDB_REQUIRE(lims && out_lims && n_shards >= 1, "null argument");
    VDB_REQUIRE(nq < (1ull << 32), "too many queries for one call");
    VDB_REQUIRE((out_idx == nullptr) == (out_dist == nullptr), "out_idx and out_dist go together (both NULL: offsets only)");
    range_merge_validate(lims, nq + 1, n_shards, nq, pair_stride);
    range_merge_lims(lims, nq + 1, n_shards, nq, limit, out_lims);
    if (out_idx && out_lims[nq]) {
        VDB_REQUIRE(ids && dists, "null argument");
        range_merge_host(lims, ids, dists, n_shards, nq, pair_stride, out_lims, out_idx, out_dist);
    }
    VDB_API_END
}

int vdb_range_merge_device(vdb_index *idx, const void *d_lims, const void *d_ids, const void *d_dists, uint64_t n_shards, uint64_t nq,
                           uint64_t pair_stride, uint64_t limit, void *stream, vdb_range **out) {
    VDB_API_BEGIN
    VDB_REQUIRE(out, "null out");
    *out = nullptr;
    VDB_REQUIRE(idx && n_shards >= 1, "null argument");
    VDB_REQUIRE(nq == 0 || d_lims, "null argument");
    VDB_REQUIRE(nq < (1ull << 32) && n_shards < (1ull << 16), "too many queries or shards for one call");
    Index &ix = idx->ix;
    ix.use_device();
    std::unique_ptr<vdb_range> res(new vdb_range);
    WsLease ws(ix);
    VDB_SYNC(static_cast<hipStream_t>(stream));  // order after whatever produced the inputs on the caller's stream (the all-gather)
    std::vector<uint64_t> h_lims(n_shards * (nq + 1), 0);
    if (nq) VDB_HIP(hipMemcpy(h_lims.data(), d_lims, h_lims.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    range_merge_validate(h_lims.data(), nq + 1, n_shards, nq, pair_stride);
    try {
        range_merge_dev(ix, *ws, h_lims.data(), nq + 1, d_lims, d_ids, pair_stride * sizeof(uint64_t), d_dists, pair_stride * sizeof(float), n_shards,
                        nq, limit, res->r);
    } catch (...) {
        (void)hipStreamSynchronize(ws->stream);
        ix.prof_collect(*ws);
        throw;
    }
    ix.prof_collect(*ws);
    *out = res.release();
    VDB_API_END
}

int vdb_merge_topk_device(vdb_index *idx, const void *d_dists, const void *d_ids, const void *d_counts,
                          uint64_t n_shards, uint64_t nq, uint64_t k, void *d_out_idx, void *d_out_dist,
                          void *d_out_count, void *stream) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    merge_topk_dev(idx->ix, d_dists, d_ids, d_counts, nq * k * sizeof(float), nq * k * sizeof(uint64_t),
                   nq * sizeof(uint64_t), n_shards, nq, k, d_out_idx, d_out_dist, d_out_count, stream);
    VDB_API_END
}
// same, reading the S per-rank blocks of ONE all-gather buffer in place: block s starts s*block_bytes after block 0 and
// holds ids at off_ids, distances at off_dists, counts at off_counts (bytes; 8-byte aligned ids / counts)
int vdb_merge_topk_gathered(vdb_index *idx, const void *d_gathered, uint64_t block_bytes, uint64_t off_ids,
                            uint64_t off_dists, uint64_t off_counts, uint64_t n_shards, uint64_t nq, uint64_t k,
                            void *d_out_idx, void *d_out_dist, void *d_out_count, void *stream) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx && d_gathered, "null argument");
    VDB_REQUIRE((off_ids & 7) == 0 && (off_counts & 7) == 0 && (off_dists & 3) == 0 && (block_bytes & 7) == 0,
                "misaligned block layout");
    const char *g = static_cast<const char *>(d_gathered);
    merge_topk_dev(idx->ix, g + off_dists, g + off_ids, g + off_counts, block_bytes, block_bytes, block_bytes, n_shards,
                   nq, k, d_out_idx, d_out_dist, d_out_count, stream);
    VDB_API_END
}

int vdb_merge_topk_gathered_async(vdb_index *idx, const void *d_gathered, uint64_t block_bytes, uint64_t off_ids,
                                  uint64_t off_dists, uint64_t off_counts, uint64_t n_shards, uint64_t nq, uint64_t k,
                                  void *d_out_idx, void *d_out_dist, void *d_out_count, void *stream) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx && d_gathered && d_out_idx && d_out_dist && d_out_count, "null argument");
    VDB_REQUIRE((off_ids & 7) == 0 && (off_counts & 7) == 0 && (off_dists & 3) == 0 && (block_bytes & 7) == 0,
                "misaligned block layout");
    VDB_REQUIRE(k >= 1 && k <= 64, "the enqueued merge serves k in 1..64 (one launch, no scratch); use vdb_merge_topk_gathered beyond");
    VDB_REQUIRE(n_shards >= 1, "shard merge: at least one shard is needed");
    VDB_REQUIRE(nq <= 65535 && n_shards <= 65535, "too many queries or shards for one call");
    require_merge_ids_fit(idx->ix);
    idx->ix.use_device();
    const char *g = static_cast<const char *>(d_gathered);
    launch_merge_shards64(reinterpret_cast<const float *>(g + off_dists), reinterpret_cast<const uint64_t *>(g + off_ids),
                          reinterpret_cast<const uint64_t *>(g + off_counts), block_bytes, block_bytes, block_bytes, (uint32_t)n_shards,
                          (uint32_t)nq, (uint32_t)k, static_cast<uint64_t *>(d_out_idx), static_cast<float *>(d_out_dist),
                          static_cast<uint64_t *>(d_out_count), static_cast<hipStream_t>(stream));
    VDB_HIP(hipGetLastError());
    VDB_API_END
}

// ---- measurement hooks --------------------------------------------------------------------------------
int vdb_stream_probe(int device_id, uint64_t bytes, int iters, double *out_gbps) {
    VDB_API_BEGIN
    VDB_REQUIRE(out_gbps, "null out");
    require_gpu();
    *out_gbps = stream_probe(device_id, bytes, iters);
    VDB_API_END
}
int vdb_stream_probe_rows(int device_id, uint64_t bytes, int iters, uint32_t row_bytes, double *out_gbps) {
    VDB_API_BEGIN
    VDB_REQUIRE(out_gbps, "null out");
    require_gpu();
    *out_gbps = stream_probe_pattern(device_id, bytes, iters, 1, row_bytes);
    VDB_API_END
}
int vdb_mfma_probe(int device_id, int waves_per_simd, int iters, double *out_tflops, double *out_clock_ghz) {
    VDB_API_BEGIN
    VDB_REQUIRE(out_tflops && out_clock_ghz, "null out");
    require_gpu();
    mfma_probe(device_id, waves_per_simd, iters, out_tflops, out_clock_ghz);
    VDB_API_END
}
int vdb_mfma_probe_i8(int device_id, int waves_per_simd, int iters, double *out_tops, double *out_clock_ghz) {
    VDB_API_BEGIN
    VDB_REQUIRE(out_tops && out_clock_ghz, "null out");
    require_gpu();
    mfma_probe(device_id, waves_per_simd, iters, out_tops, out_clock_ghz, 1);
    VDB_API_END
}
int vdb_latency_probe(int device_id, uint64_t bytes, uint32_t hops, double *out_ns_per_load) {
    VDB_API_BEGIN
    VDB_REQUIRE(out_ns_per_load, "null out");
    require_gpu();
    *out_ns_per_load = latency_probe(device_id, bytes, hops);
    VDB_API_END
}
int vdb_fold_probe(int device_id, uint32_t adds, double *out_ns_per_add) {
    VDB_API_BEGIN
    VDB_REQUIRE(out_ns_per_add, "null out");
    require_gpu();
    *out_ns_per_add = fold_probe(device_id, adds);
    VDB_API_END
}
int vdb_prof_enable(vdb_index *idx, int on) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    idx->ix.prof_on = on != 0;
    VDB_API_END
}
int vdb_prof_reset(vdb_index *idx) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx, "null index");
    std::lock_guard<std::mutex> g(idx->ix.prof_mu);
    idx->ix.prof.clear();
    VDB_API_END
}
int vdb_prof_get(vdb_index *idx, const char *kernel, double *total_ms, uint64_t *launches, double *bytes) {
    VDB_API_BEGIN
    VDB_REQUIRE(idx && kernel, "null argument");
    std::lock_guard<std::mutex> g(idx->ix.prof_mu);
    auto it = idx->ix.prof.find(kernel);
    ProfEntry e = it == idx->ix.prof.end() ? ProfEntry{} : it->second;
    if (total_ms) *total_ms = e.ms;
    if (launches) *launches = e.launches;
    if (bytes) *bytes = e.bytes;
    VDB_API_END
}

}  // extern "C"
