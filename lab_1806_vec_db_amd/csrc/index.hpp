// index.hpp -- the HBM-resident index object behind the C ABI (include/vdbhip.h).
#pragma once
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "common.hpp"
#include "kernels.hpp"

namespace vdb {

// growable device buffer (amortised doubling, like Vec<T>: vec_set.rs:113-118)
// VDB_EFENCE=1 (debugging aid, read once): every buffer is placed so that it ENDS where its allocation ends, and allocations are
// whole 2-MiB granules -- a kernel that reads or writes more than the 256-B alignment slack past a buffer then leaves the
// mapping and faults at once instead of silently touching whatever the allocator put there (how the over-read of
// k_pq_adc16's idle lanes stayed unseen for a round).  Used for soaks of the test suite, never in production.
inline bool devbuf_efence() {
    static const bool on = [] {
        const char *e = std::getenv("VDB_EFENCE");
        return e && e[0] == '1';
    }();
    return on;
}
// (testing aid) every DevBuf allocation of at least this many bytes fails as if the device were out of memory; 0 = off
inline std::atomic<size_t> &devbuf_fail_over() {
    static std::atomic<size_t> v{0};
    return v;
}
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    void *base = nullptr;  // what hipMalloc returned (== p unless VDB_EFENCE)
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (base) (void)hipFree(base);
        p = base = nullptr;
        cap = 0;
    }
    static void dev_malloc(void **out, size_t bytes) {
        const size_t lim = devbuf_fail_over().load();
        hipError_t e = (lim && bytes >= lim) ? hipErrorOutOfMemory : hipMalloc(out, bytes);
        if (e == hipErrorOutOfMemory) {
            (void)hipGetLastError();  // (not sticky, but the slot is read by the next VDB_SYNC)
            throw AllocError("device allocation of " + std::to_string(bytes) + " bytes failed: out of memory");
        }
        VDB_HIP(e);
    }
    static void alloc(size_t want, void **base_out, void **p_out) {
        if (!devbuf_efence()) {
            dev_malloc(base_out, want);
            *p_out = *base_out;
            return;
        }
        constexpr size_t G = size_t(2) << 20;
        const size_t total = (want + G - 1) / G * G;
        dev_malloc(base_out, total);
        *p_out = static_cast<char *>(*base_out) + ((total - want) & ~size_t(255));
    }
    // contents are NOT preserved
    void reserve(size_t bytes) {
        if (bytes <= cap) return;
        release();
        size_t want = bytes < 256 ? 256 : bytes;
        alloc(want, &base, &p);
        cap = want;
    }
    // contents preserved up to `keep` bytes
    void grow(size_t bytes, size_t keep, hipStream_t s) {
        if (bytes <= cap) return;
        size_t want = cap ? cap : 256;
        while (want < bytes) want *= 2;
        if (devbuf_efence()) want = bytes;  // (no slack capacity to hide an over-read in)
        void *nb = nullptr, *np = nullptr;
        alloc(want, &nb, &np);
        if (keep) {
            VDB_HIP(hipMemcpyAsync(np, p, keep, hipMemcpyDeviceToDevice, s));
            VDB_SYNC(s);
        }
        if (base) (void)hipFree(base);
        base = nb;
        p = np;
        cap = want;
    }
    // takes over src's allocation (what this buffer held is released; src is left empty)
    void take(DevBuf &src) {
        release();
        p = src.p;
        cap = src.cap;
        base = src.base;
        src.p = src.base = nullptr;
        src.cap = 0;
    }
    // becomes a view of `bytes` bytes at `at` inside somebody else's allocation: base stays null, so release() frees nothing (what this
    // buffer held is released first); the owner of that allocation must outlive the view
    void view(void *at, size_t bytes) {
        release();
        p = at;
        cap = bytes;
    }
    template <class T>
    T *as() const { return reinterpret_cast<T *>(p); }
};
// every view into a slab starts at a multiple of this: how hipMalloc aligns whole buffers
constexpr size_t DEVBUF_ALIGN = 256;
inline size_t devbuf_align_up(size_t bytes) { return (bytes + DEVBUF_ALIGN - 1) / DEVBUF_ALIGN * DEVBUF_ALIGN; }

struct ProfEntry {
    double ms = 0;
    uint64_t launches = 0;
    double bytes = 0;
};

// per-call scratch: one per concurrent reader (read-side calls are re-entrant, see vdbhip.h)
struct Workspace {
    hipStream_t stream = nullptr;
    DevBuf q, qsq, qfrag, qfrag_g, qaux, dense, lists, keys_a, keys_b, keys_c, flags, out_idx, out_dist, out_cnt, lut, misc;
    DevBuf pq_img16, pq_aux16;     // 8-bit PQ codes: the sliced 16-bit table images of a round of queries, their minima / offsets / steps (pq.hip)
    DevBuf small_part, small_cnt;  // k_flat_small: per-workgroup key lists, arrival counters (zero between launches)
    // grouped k-NN (Index::flat_knn_grouped_device): the compacted queries of a round, the candidate lists of a sub-chunk (ids, distances,
    // counts), [slot map | done bytes | flag], the walk's table beyond LDS -- buffers of their own, because the list calls use the others.
    // The diversified k-NN (Index::flat_knn_mmr_device) keeps its candidate lists and its flag in the same ones.
    DevBuf grp_q, grp_ids, grp_dist, grp_cnt, grp_aux, grp_table;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    struct Pending {
        std::string name;
        size_t ev;
        double bytes;
    };
    std::vector<Pending> pending;
    size_t ev_used = 0;
    // pinned host staging for the small per-call read-backs (flags, counters): a D2H copy into pageable memory goes
    // through the runtime's own staging buffer and costs an extra hop before the stream sync returns
    void *h_pinned = nullptr;
    size_t h_pinned_cap = 0;
    hipEvent_t order_ev = nullptr;  // orders this workspace's stream behind a caller's stream without a host wait (vdb_*_begin)
    // bulk row fetch (Index::fetch_gathered): the stream its device-to-host copies run on while `stream` gathers the next chunk, and
    // per staging buffer the events "gathered" / "copied out".  Made by the first fetch that has more than one chunk.
    hipStream_t copy_stream = nullptr;
    hipEvent_t fetch_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    void fetch_streams() {
        if (!copy_stream) VDB_HIP(hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking));
        for (auto &e : fetch_ev)
            if (!e) VDB_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    // The block stays valid until the next pinned() call of a larger size, which waits for `stream` before it frees the block: nothing
    // enqueued on the stream still uses it then.  (Mirror builds never take it: they read their results into storage of their own.)
    void *pinned(size_t bytes) {
        if (bytes > h_pinned_cap) {
            if (h_pinned) {
                VDB_HIP(hipStreamSynchronize(stream));
                (void)hipHostFree(h_pinned);
            }
            h_pinned = nullptr;
            size_t want = bytes < (64u << 10) ? (64u << 10) : bytes;
            VDB_HIP(hipHostMalloc(&h_pinned, want, hipHostMallocDefault));
            h_pinned_cap = want;
        }
        return h_pinned;
    }
    Workspace() {
#ifndef VDB_HOST_SANITIZER_BUILD  // (tests/cpp/tsan_host.cpp drives the pool and the host builders with no device present)
        VDB_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
#endif
    }
    ~Workspace() {
        if (h_pinned) (void)hipHostFree(h_pinned);
        if (order_ev) (void)hipEventDestroy(order_ev);
        for (auto &e : fetch_ev)
            if (e) (void)hipEventDestroy(e);
        if (copy_stream) (void)hipStreamDestroy(copy_stream);
        for (auto &e : ev_pool) {
            (void)hipEventDestroy(e.first);
            (void)hipEventDestroy(e.second);
        }
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// The id check of every call that takes ids from the device: the flag word d_flag zeroed on `s` (zeroed: the caller's upload has done
// that), enqueue(d_flag) -- launch_fetch_check / launch_list_check, which set it for an id that is no row --, ONE read-back through the
// workspace's pinned block and a wait for `s`; throws `message` when the flag is set, with nothing else of the call enqueued yet.
template <class Enqueue>
void ids_ok(Workspace &ws, hipStream_t s, uint32_t *d_flag, const char *message, Enqueue &&enqueue, bool zeroed = false) {
    if (!zeroed) VDB_HIP(hipMemsetAsync(d_flag, 0, sizeof(uint32_t), s));
    enqueue(d_flag);
    uint32_t *h_flag = static_cast<uint32_t *>(ws.pinned(sizeof(uint32_t)));
    VDB_HIP(hipMemcpyAsync(h_flag, d_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    VDB_SYNC(s);
    VDB_REQUIRE(*h_flag == 0, message);
}

struct PQState {
    bool present = false;
    uint64_t n_bits = 0, m = 0, kc = 0, enc_dim = 0;
    uint64_t n_coded = 0;            // rows d_codes covers; every PQ search requires n_coded == Index::n
    std::vector<uint64_t> gstart;    // m+1
    std::vector<float> h_centroids;  // kc*dim
    std::vector<float> h_cent_cache; // m*kc
    DevBuf d_centroids, d_cent_cache, d_codes, d_gstart;
    DevBuf d_codes_t;                // word-major mirror of d_codes for the quantised ADC scan (k_pq.hip: k_pq_tile_codes)
    bool codes_t_valid = false;
    std::atomic<uint64_t> adc16_queries{0};  // queries whose ADC scan ran on the quantised tables (k_pq_adc16)
    std::atomic<uint64_t> adc16_redo{0};     // of those, the ones handed to the f32 scan (list overflowed | fewer than ef sums at or below tau)
    std::atomic<uint64_t> q8_overflow{0}, q8_short{0};  // 8-bit codes: queries the quantised pass handed to the f32 scan (list overflowed | fewer than ef sums at or below tau)
    std::atomic<uint64_t> q8_hits_sum{0}, q8_hits_max{0};  // candidates of the quantised pass (sum over queries, largest list)
};

struct HNSWState {
    bool present = false;
    uint64_t m = 0, max_m0 = 0, ef_construction = 0, default_ef = 0;
    float inv_log_m = 0;
    std::vector<uint32_t> level0;
    std::vector<uint64_t> len0, vec_level, upper_off, upper_len;
    std::vector<uint32_t> upper;
    bool has_enter = false;
    uint64_t enter_point = 0, enter_level = 0;
    uint64_t rng_state = 0;
    // device mirror (uploaded lazily when dirty)
    bool dev_dirty = true;
    DevBuf d_level0, d_len0, d_upper, d_upper_len, d_upper_off;
    std::atomic<uint64_t> last_n_dist{0}, last_n_expanded{0};
    std::atomic<uint64_t> last_half_dropped{0};  // of last_n_dist: rows the certified half-precision pre-pass ruled out (last call)
    std::atomic<uint64_t> heap_walk_queries{0};  // queries answered by k_hnsw_search_big (ef > 1024 or LDS pool overflow)
};

// a Flat call between its two halves (Index::flat_knn_enqueue / flat_knn_finish)
struct FlatPending {
    bool active = false;  // the MFMA pipeline is on the stream, its certification flags are still to be read
    bool half = false;
    bool i8 = false;      // first pass on the 8-bit mirror (its uncertified queries go to the fp16 / split-bf16 tiers)
    bool i8_second = false;  // ... its second attempt: thresholds from the first walk's k-th distances (k_redo.hip)
    bool stats = false;      // the exact stage wrote one word of statistics per query behind the flags
    bool refined = false;    // the hit keys were tightened from the fp16 image before the walk
    uint32_t kprime = 0, ksel = 0;
    uint64_t nq = 0, k = 0;
    const float *d_q = nullptr;
    uint64_t *d_idx = nullptr;
    float *d_dist = nullptr;
    uint64_t *d_cnt = nullptr;
};

// the query side of one 8-bit filter pass over a chunk of queries (Index::i8_query_prep): all in the workspace's buffers
struct I8Queries {
    uint64_t ngroups = 0, nq_pad = 0;  // groups of gemm_group() queries, queries with the last group's padding
    float *d_tau = nullptr, *d_qscale = nullptr, *d_qoff = nullptr;  // [nq_pad] each; the thresholds are the caller's to fill
    uint32_t *d_hits = nullptr;                                      // [nq_pad] hit counters, zeroed
};

// a threshold sample: tau = the s_rank-th smallest of n_s dense keys per query (rows of ld_s floats)
struct TauSample {
    uint32_t s_step = 1, s_rank = 0;  // every s_step-th item (8-bit pass: unit) is sampled
    bool unit_min = false;            // 8-bit pass: one key per sampled unit, its smallest
    uint64_t n_s = 0, ld_s = 0;
    uint32_t nl_s = 0, cap_s = 0;     // the selection's lists beyond select_tau_max_n() keys: lists per query, slots per list
    void set_keys(uint64_t keys) {
        n_s = keys;
        ld_s = (keys + 63) & ~63ull;
        nl_s = topk_num_lists(keys);
        cap_s = topk_capacity(s_rank);
    }
};

// the answer of a range call (Index::flat_range_device): CSR over the queries, arrays on the index's device
struct RangeResult {
    int device = 0;
    uint64_t nq = 0;
    std::vector<uint64_t> lims;  // nq + 1 offsets, lims[0] = 0
    DevBuf idx, dist;            // lims[nq] ids (u64, local row + id_offset) / distances (f32), per query ascending by (distance, index)
};
// the sorted pair keys of a range call before the CSR arrays are gathered from them (Index::flat_range_collect / _assemble)
struct RangePool {
    DevBuf buf;
    uint64_t used = 0;                                           // pair keys in buf
    void room(uint64_t add, uint64_t cap_pairs, hipStream_t s);  // room for `add` more; throws past the ceiling of the call
};
// what a flat_range_collect added to the index's range counters
struct RangeTally {
    uint64_t i8 = 0, scan = 0, hits = 0;
};

// 16-row tiles of a fragment-ordered mirror of `rows` rows: whole 64-row items (k_flat_mfma), whole 2/3-tile units (k_flat_gemm, k_flat_gemm8)
inline uint64_t mirror_tiles(uint64_t rows) { return ((rows + 15) / 16 + 11) / 12 * 12; }

// One image of the rows derived from d_rows (the Flat tiers' tiled mirrors, the row-major fp16 / 8-bit images): built by the first call
// that wants it, kept in step with every row edit by Index's mirror upkeep (the private section at the end of Index: THE place a write path
// goes through).  An image that cannot be allocated is not an error of the search that wanted it: its buffers are released, the failure is
// counted, the tier is left to the next one, and ensure() does not try again until n changes.
struct RowMirror {
    std::mutex mu;                   // read-side calls are re-entrant: one of them builds, the others wait
    std::atomic<bool> valid{false};  // the buffers hold the image of rows [0, rows) (both read without the lock)
    std::atomic<uint64_t> rows{0};
    uint64_t failed_n = ~0ull;       // row count at which the allocation failed
    std::atomic<uint64_t> &failures;
    std::vector<DevBuf *> bufs;      // released when an allocation fails
    RowMirror(std::atomic<uint64_t> &f, std::initializer_list<DevBuf *> b) : failures(f), bufs(b) {}
    bool covers(uint64_t n) const { return valid && rows == n; }
    void set(uint64_t n) {
        rows = n;
        valid = true;
    }
    void invalidate() {  // (the buffers stay for the rebuild)
        valid = false;
        rows = 0;
    }
    bool attempt(const std::function<void()> &build);  // false: AllocError -- buffers released, image invalid, counted
    // under the lock: current() -> true; failed at this n -> false; else attempt(build), a failure latched at n
    bool ensure(uint64_t n, const std::function<bool()> &current, const std::function<void()> &build);
};

struct Index;
// A row allow-list of ONE index at ONE state of its rows (vdb_mask_create): the bit words, the ascending list of the allowed rows and, built
// by the first call that runs the 8-bit tier under it, the masked copy of the index's {C_r, M_r} row constants (k_filter.hip).  Read-side
// calls share a mask: everything but the lazily built copy is immutable after creation, and that copy is built under `mu`.
struct RowMask {
    const Index *owner = nullptr;
    int device = 0;
    uint64_t gen = 0;     // Index::write_gen when the mask was made: add_rows / swap_remove make it stale
    uint64_t n_rows = 0;  // rows of the index then
    uint64_t m = 0;       // allowed rows
    DevBuf d_bits;        // u64 [ceil(n_rows / 64)], bits at and past n_rows clear
    DevBuf d_ids;         // u32 [m], ascending
    // A mask of Index::masks_partition: d_bits / d_ids are VIEWS (base == nullptr: release() frees nothing) into two allocations that
    // the masks of one chunk of the call share; every mask holds a reference and the last one destroyed frees them.  Empty for every
    // other constructor.
    std::shared_ptr<DevBuf> slab_bits, slab_ids;
    mutable std::mutex mu;
    mutable DevBuf d_rowc;  // float2 [padded rows]: Index::d_rowc_i8 with {+inf, 0} for every disallowed row
    mutable const void *rowc_of = nullptr;  // the d_rowc_i8 allocation it was copied from (nullptr: not built)
    mutable uint64_t rowc_gen = 0;          // Index::rowc_gen then: update_rows rewrites constants inside that allocation
};
// IVFIndex (ivf_index.rs:34-47): centroids as a small Flat index of their own, clusters as CSR over row ids
struct IVFState {
    bool present = false;
    uint64_t k = 0, default_n_probes = 4;  // :108
    std::shared_ptr<Index> cent;           // k x dim centroids (find_n_nearest = Flat knn over them)
    std::vector<uint64_t> assign;          // cluster of every row
    std::vector<uint32_t> offsets;         // k+1
    std::vector<uint32_t> sizes_desc;      // cluster sizes, descending (bounds the candidates of n probes)
    DevBuf d_offsets, d_members;           // u32 [k+1], u32 [n] (ascending id inside a cluster)
    std::atomic<uint64_t> last_rows_fetched_q8{0};  // cluster-major 8-bit tier: rows read (once each); 0: query-major or tier not run
    std::atomic<uint64_t> last_kept_q8{0};  // offers the 8-bit tier passed on to the fp16 tier (0: that tier did not run)
    std::atomic<uint32_t> q8_overflows{0};
    std::atomic<uint64_t> last_offers{0}, last_kept{0};  // measurement on: offers of the last call / those its pre-pass kept
    std::atomic<uint32_t> half_overflows{0};  // calls whose half-precision pre-pass kept more offers than its lists hold (4: stop trying)
};

struct Index {
    int device = 0;
    int num_cu = 256;
    uint64_t dim = 0;
    int dist = 0;
    uint64_t n = 0;
    uint64_t id_offset = 0;
    // VecSet<T>: T = f32 (the DynamicIndex case) or u8 (scalar.rs:117-119): d_rows holds n * dim elements of elem_size()
    // bytes.  A u8 index serves Flat search (exact scan, MFMA shortlist over mirrors that hold u8 values exactly, native
    // u8 re-rank); PQ / HNSW / IVF are built over f32 tables only, as DynamicIndex instantiates them (dynamic_index.rs:11-14).
    bool elem_u8 = false;
    size_t elem_size() const { return elem_u8 ? 1 : sizeof(float); }
    // f32 view of rows [r0, r1) for the build-time kernels: base pointer B with B + r * dim = row r (the rows themselves,
    // or a widened copy of the chunk in `scratch` for a u8 index)
    const float *rows_f32_view(DevBuf &scratch, uint64_t r0, uint64_t r1, hipStream_t s) const;
    // fn(view, tile_a, tile_b, row_a, row_b) over the 16-row tiles [t_begin, t_end), rows clipped to n_rows: one call on
    // the rows themselves (f32), or one per widened chunk (u8); view + r * dim addresses row r for row_a <= r < row_b
    static constexpr uint64_t TILE_CHUNK = 12 * 64;  // tiles per widened chunk of a u8 index (whole mirror units): 12 288 rows
    size_t tile_chunk_bytes() const { return TILE_CHUNK * 16 * dim * sizeof(float); }  // what for_tile_chunks reserves in ws.dense (u8 index)
    template <class F>
    void for_tile_chunks(Workspace &ws, uint64_t t_begin, uint64_t t_end, uint64_t n_rows, F fn) const {
        if (!elem_u8) {
            fn(d_rows.as<float>(), t_begin, t_end, std::min(t_begin * 16, n_rows), n_rows);
            return;
        }
        constexpr uint64_t CH = TILE_CHUNK;
        ws.dense.reserve(tile_chunk_bytes());  // before the loop: a later, larger reserve would free a buffer in use
        for (uint64_t t = t_begin; t < t_end; t += CH) {
            const uint64_t tb = std::min(t_end, t + CH), ra = std::min(t * 16, n_rows), rb = std::min(tb * 16, n_rows);
            fn(rows_f32_view(ws.dense, ra, rb, ws.stream), t, tb, ra, rb);
        }
    }
    DevBuf d_rows, d_sq;
    std::atomic<uint64_t> mirror_alloc_failures{0};  // images of the rows (RowMirror) whose allocation failed
    // MFMA-fragment-ordered split-bf16 mirror of d_rows (k_mfma.hip; 4 B/element), only when mfma_supported(dim).  Built
    // LAZILY by the first search that needs it (the redo tier of the fp16 pass, calls without an fp16 mirror,
    // flat_half = 1): an index whose queries all certify on the fp16 pass never pays its N*d*4 bytes of HBM.
    DevBuf d_tiled;
    RowMirror tiled_m{mirror_alloc_failures, {&d_tiled}};
    const std::atomic<bool> &tiled_built = tiled_m.valid;  // d_tiled covers rows [0, n) (read without the lock: statistics, tests)
    bool ensure_tiled(Workspace &ws);  // false: the split-bf16 mirror could not be allocated (the exact scan answers)
    void prepare_flat(bool all_tiers);  // builds now what the first Flat search would build (vdb_index_prepare)
    uint64_t hbm_bytes_per_row() const;  // resident bytes per row over all per-row buffers (rows, norms, mirrors, codes, links)
    // scaled fp16 mirror for k_flat_gemm<GEMM_F16> (k_half.hip): rows stored as fp16(x * 2^(13 - half_exp)), every row
    // norm < 2^half_exp; half_dx_* = measured rounding error of the mirror (max |dx_r|, max |dx_r| / |x_r|)
    DevBuf d_tiled_h, d_half_err;
    int half_exp = 0;
    float half_dx_abs = 0.0f, half_dx_rel = 0.0f;
    int flat_half_mode = 0;        // 0 auto, 1 off, 2 on even after many uncertified queries
    uint32_t flat_half_kmul = 4;   // shortlist of the fp16 pass: max(64, kmul * k) rows per query
    std::atomic<uint64_t> half_queries{0}, half_redo{0};  // queries through the fp16 pass / redone with split-bf16
    void half_refresh(Workspace &ws, uint64_t n_old, uint64_t n_new);  // after rows [n_old, n_new) changed
    // An index the 8-bit pass serves (i8_defers_half) builds this mirror on FIRST NEED instead of at add time: a query the
    // 8-bit pass hands on, a call it does not take (k > 64), the walks' / IVF scan's row-major fp16 image (which shares its
    // scale and measured error).  half_m.rows = rows the mirror covers (valid = false with rows = n: this index has none).
    RowMirror half_m{mirror_alloc_failures, {&d_tiled_h}};
    bool i8_defers_half() const;
    bool ensure_half(Workspace &ws);  // false: this index has no fp16 mirror (dimension, extreme norms)
    float half_sx() const { return std::ldexp(1.0f, 13 - half_exp); }
    // Centred 8-bit mirror for k_flat_gemm8 (k_gemm8.hip, k_i8.hip; L2Sqr over f32 rows): 1 B/element in fragment order +
    // {C_r, M_r} per row.  Built by the first search that wants it (ensure_i8), extended after add_rows, kept in step by the
    // mirror upkeep below; mu / lambda are re-chosen (and everything rewritten) when the table has doubled since they were measured.
    DevBuf d_tiled_i8, d_rowc_i8, d_mu_i8;
    RowMirror i8_m{mirror_alloc_failures, {&d_tiled_i8, &d_rowc_i8}};
    uint64_t i8_mu_rows = 0;    // table size when mu / lambda were measured
    float i8_l1 = 0.0f, i8_l2 = 0.0f, i8_mu_norm = 0.0f;
    int flat_i8_mode = 0;       // 0 auto, 1 off, 2 on even after many uncertified queries
    // rows the exact stage of the FIRST attempt may walk per query (64 per round); the second attempt walks the whole candidate list.
    // 2048 = 32 rounds, i.e. the whole hit list of the sample plan's ~1000 hits: a query that exhausts its list is certified by the threshold
    // itself, and only what then is still open pays a second pass over the mirror.  Measured at 1M x 960 (bench.py --data ..., same box):
    // separable data never walk more than 4 rounds whatever the limit; loose clusters 1.51 ms per step at 512 / 1024 / 2048 (their
    // stragglers need the second attempt's longer lists either way); tight clusters 3.03 / 2.89 / 2.47 ms
    uint32_t flat_i8_kprime = 2048;
    int flat_i8_full = 0;           // second attempt of <= 96 queries: all candidates evaluated at once (0 on, 1 off: the walk)
    int flat_i8_refine = 0;         // hit keys tightened from the fp16 row image before the walk (k_flat_refine_half): 0 auto (on while the walks are long), 1 off, 2 always
    std::atomic<int> i8_refine_on{0};        // auto state
    std::atomic<uint32_t> i8_refine_calls{0};  // first-attempt calls since the state changed (every 32nd call of the on state runs without: the probe)
    std::atomic<uint64_t> i8_refine_queries{0};  // queries whose hit lists were refined
    int flat_i8_unit_min = 0;       // threshold sample of the 8-bit pass by unit minima when the sampled units are many: 0 auto, 1 off
    int flat_i8_second = 0;         // second 8-bit attempt with thresholds from the first walk (k_redo.hip): 0 on, 1 off
    std::atomic<uint64_t> i8_second_queries{0}, i8_second_redo{0};
    uint32_t flat_i8_hits = 1024;   // expected hits per query the threshold sample of the 8-bit pass aims at (>= 256 = 4 x the 64 guaranteed)
    std::atomic<uint64_t> i8_queries{0}, i8_redo{0};  // queries through the 8-bit pass / passed on to the next tier
    // (measurement, flat_i8_stats = 1) per-query work of the 8-bit pass's exact stage: queries by rounds walked, hits per query
    int flat_i8_stats = 0;
    std::atomic<uint64_t> i8_rounds_hist[9] = {};
    std::atomic<uint64_t> i8_hits_sum{0}, i8_hits_max{0}, i8_stat_queries{0};
    std::atomic<uint64_t> i8_rows_walked{0};          // (measurement) not maintained in production
    bool i8_applicable(uint32_t ksel) const;
    bool i8_mirror_applicable() const;  // its clauses about the mirror and the data alone (no k, no auto-off counters: the range search's)
    bool ensure_i8(Workspace &ws);  // false: the mirror could not be allocated (the next tier answers)
    void build_i8(Workspace &ws);
    // Row-major fp16 image of the rows, same scale and rounding as d_tiled_h (so half_dx_* bound its error as well): the
    // operand of the HNSW walk's certified pre-pass (hnsw.hip, hnsw_half_dots).  Built on the first walk that wants it,
    // extended when rows were added since, rebuilt when the scale changed.
    DevBuf d_rows_h;
    RowMirror rows_h_m{mirror_alloc_failures, {&d_rows_h}};
    int rows_h_exp = 0;
    bool ensure_rows_h(Workspace &ws);  // false: this index has no fp16 image (dim, element type, extreme norms)
    // 8-bit image of the rows with one scale and one measured error per row (half_rows.hpp, "8-bit tier"): the first tier of
    // the IVF scan's pre-pass; built on first use, extended after add, dropped by every other row edit (mirrors_shrunk, update_rows)
    DevBuf d_rows_q8, d_q8_scale, d_q8_err;
    RowMirror rows_q8_m{mirror_alloc_failures, {&d_rows_q8, &d_q8_scale, &d_q8_err}};
    bool ensure_rows_q8(Workspace &ws);  // false: no 8-bit image (dim, element type, allocation): the IVF scan goes on with the fp16 tier
    std::vector<float> h_sq;  // host mirror of d_sq (4 B/row), kept in step by each row edit itself (add, remove, update)
    float xsq_max = 0.0f;
    float xsq_min_pos = 3.4e38f;  // smallest positive row |x|^2 seen (cosine certification: clamp check)
    // lazily materialised host mirror of the rows (needed by the host-side builders and vdb_index_row)
    mutable std::vector<float> h_rows;
    mutable bool host_valid = true;
    mutable std::mutex host_mu;
    int flat_mode = 0;
    int flat_gemm_mode = 0;   // 0 auto (more than 64 queries per call), 1 off, 2 forced (k_gemm.hip)
    int flat_gemm_debug = 0;
    int flat_tail_mode = 0;  // 0 auto (fused exact stage when k' <= 64), 1 separate kernels
    int flat_small_mode = 0;          // one-launch search of small tables (k_small.hip): 0 auto, 1 off, 2 whenever the shape allows
    uint64_t flat_small_max_rows = 16384;  // auto: tables up to this many rows (where the MFMA shortlist takes over), calls of < 32 queries
    bool flat_small_applies(uint64_t nq, uint64_t k) const;
    // q / outputs: device memory or device-visible pinned host memory
    void flat_small_device(Workspace &ws, const float *q, uint64_t nq, uint64_t k, uint64_t *o_idx, float *o_dist, uint64_t *o_cnt);
    std::atomic<uint64_t> fallback_count{0};
    PQState pq;
    HNSWState hnsw;
    IVFState ivf;

    std::mutex ws_mu;
    std::vector<std::unique_ptr<Workspace>> ws_free;
    // end of the most recent Flat corpus pass enqueued on any of this index's streams (corpus_pass orders passes by it)
    std::mutex pass_mu;
    hipEvent_t pass_ev = nullptr;
    bool pass_ev_valid = false;
    bool prof_on = false;
    std::mutex prof_mu;
    std::map<std::string, ProfEntry> prof;

    Index(int dev, uint64_t d, int ds, bool u8 = false);
    ~Index() {
        if (pass_ev) (void)hipEventDestroy(pass_ev);
    }
    void use_device() const {
#ifndef VDB_HOST_SANITIZER_BUILD
        VDB_HIP(hipSetDevice(device));
#endif
    }
    std::unique_ptr<Workspace> acquire_ws();
    void release_ws(std::unique_ptr<Workspace> ws);
    const float *host_rows() const;  // materialise the host mirror if needed

    void add_rows(const void *rows, uint64_t count, bool on_device);  // elements of elem_size() bytes
    void swap_remove(uint64_t i);
    // The state that swap_remove on rows[m - 1], .., rows[0] (strictly ascending) would leave, in one pass: the moves of the removal
    // plan (remove_plan.hpp) on the device, the touched tiles of every live mirror rewritten once, one stream sync.  dst / src
    // receive the plan.  An invalid list or a failed allocation throws before anything is changed.
    void remove_rows(const uint64_t *rows, uint64_t m, std::vector<uint64_t> &dst, std::vector<uint64_t> &src);
    // New vectors (m x dim f32, host or device) for the distinct rows rows[0..m) in any order, in place (update_plan.hpp, k_update.hip): rows,
    // d_sq / h_sq (launch_row_sqnorm's strict fold) and the touched 16-row tiles of every live mirror rewritten once; xsq_max /
    // xsq_min_pos widened; the fp16 mirror's measured error folded in, or the mirror dropped when its scale no longer fits.  n, id_offset,
    // the label columns and write_gen stay: masks made before the call remain valid, rowc_gen makes their row-constant copies rebuild.
    // f32 rows only.  An invalid list or a failed allocation throws before anything is changed.
    void update_rows(const uint64_t *rows, uint64_t m, const void *vecs, bool on_device);
    static constexpr size_t UPDATE_STAGE_BYTES = size_t(64) << 20;  // host vectors are staged through at most this much of ws.dense at a time
    std::atomic<uint64_t> rowc_gen{0};  // bumped by update_rows: what a RowMask's d_rowc copy is checked against (with the allocation)
    std::atomic<uint64_t> update_calls{0}, updated_rows{0};  // update_rows calls that changed rows / rows they rewrote
    // Bulk row fetch (fetch_plan.hpp, k_fetch.hip; docs/DESIGN_flat.md 4.1s): out[j] = LOCAL row rows[j], m rows on the host, in any order,
    // repeats allowed.  as_f32: f32 output (a u8 index is widened, exactly); else the u8 rows as stored (u8 index only).  The list is
    // checked before anything is touched.  A run of consecutive rows that needs no conversion is ONE copy out of d_rows; everything
    // else uploads the ids once (u32) and goes through fetch_gathered.  Read-side and re-entrant: workspace from acquire_ws, no index state
    // written but the counters, h_rows neither read nor built.  Returns synchronised.
    void get_rows(const uint64_t *rows, uint64_t m, void *out, bool as_f32);
    // the mask's allowed rows, ascending, as f32: the ids are the mask's own d_ids, nothing is uploaded.  The caller ran check_mask.
    void get_rows_mask(const RowMask &mask, float *out);
    // d_ids: m u64 GLOBAL ids on the device (row + id_offset), d_out: m x dim f32 on the device, any alignment.  k_fetch_check and one
    // read-back of its flag first -- an id that is no row of the index throws with d_out untouched --, then ONE gather launch straight
    // into d_out, all on `s`.  Returns synchronised.
    void get_rows_device(Workspace &ws, const uint64_t *d_ids, uint64_t m, void *d_out, hipStream_t s);
    // The chunk loop of the host forms: d_ids (u32, local, checked) -> `out` through TWO staging buffers of the workspace (ws.dense,
    // ws.lists; chunk_rows output rows each, so at most 2 x fetch_chunk_bytes whatever m is): chunk c + 1 is gathered on ws.stream while
    // chunk c is copied to the host on ws.copy_stream.  widen: u8 rows -> f32 output.  Returns synchronised, also when it throws.
    void fetch_gathered(Workspace &ws, const uint32_t *d_ids, uint64_t m, void *out, bool widen, uint64_t chunk_rows);
    static constexpr uint64_t FETCH_CHUNK_BYTES_DEFAULT = uint64_t(128) << 20;  // the winner of the sweep of tools/bench_fetch.py
    uint64_t fetch_chunk_bytes = FETCH_CHUNK_BYTES_DEFAULT;  // "fetch_chunk_bytes": staging bytes per chunk (at least one row)
    // calls that fetched rows (m > 0, not refused) / rows they returned / gather launches / calls answered by a copy with no kernel
    std::atomic<uint64_t> fetch_calls{0}, fetch_rows{0}, fetch_chunks{0}, fetch_direct{0};

    // timing hooks
    void prof_begin(Workspace &ws, const char *name, double bytes);
    void prof_end(Workspace &ws);
    void prof_collect(Workspace &ws);  // after a stream sync

    // search entry points; d_* are device pointers, results [nq][k]
    // d_dk_hint (8-bit pass only): per query an upper bound of its k-th distance -> the pass runs with thresholds derived from it
    // instead of sampled ones and its exact stage may walk the whole candidate list (the second attempt of k_redo.hip)
    // flat_knn_device / flat_knn_finish return the queries the call's 8-bit pass handed on (0: the call did not run that pass)
    uint64_t flat_knn_device(Workspace &ws, const float *d_q, uint64_t nq, uint64_t k, uint64_t *d_idx, float *d_dist,
                         uint64_t *d_cnt, bool allow_half = true, uint32_t kprime_min = 0, bool allow_i8 = true,
                         const float *d_dk_hint = nullptr);
    void flat_knn_enqueue(Workspace &ws, const float *d_q, uint64_t nq, uint64_t k, uint64_t *d_idx, float *d_dist, uint64_t *d_cnt,
                          bool allow_half, uint32_t kprime_min, FlatPending &p, bool allow_i8 = true, const float *d_dk_hint = nullptr);
    uint64_t flat_knn_finish(Workspace &ws, FlatPending &p);
    // The pieces of an 8-bit filter pass that Flat k-NN, the range search, the filtered search and flat_debug_keys share (index.hip).  They
    // take data -- a chunk of queries, the row constants to filter by, an expected hit count -- and never which caller they serve.
    template <class F>
    void corpus_pass(Workspace &ws, const char *name, double bytes, F launch);  // launch() in this index's turn on the corpus, timed as `name`
    I8Queries i8_query_prep(Workspace &ws, const float *Q, uint64_t nb);        // reserves the query-side buffers, enqueues k_query_prep_i8
    TauSample i8_sample_plan() const;  // 64 guaranteed hits, flat_i8_hits expected
    void i8_sample(Workspace &ws, const I8Queries &qp, const float *rowc, const TauSample &sp);  // dense sample keys -> ws.dense
    void select_tau(Workspace &ws, const TauSample &sp, uint64_t nq_pad, uint64_t nq, float *d_tau);  // ws.dense -> tau; padding queries -inf
    void i8_filter(Workspace &ws, const I8Queries &qp, const float *rowc, const char *name, uint32_t hits_expected);  // -> ws.lists, qp.d_hits
    FlatTailArgs flat_tail_args(const Workspace &ws, const uint32_t *d_hits, const float *d_tau, const SplitErr &se) const;
    bool i8_side_tier(Workspace &ws);  // the range / filtered tiers' shape test (no k, no auto-off counters); builds the mirror
    void flat_sorted_device(Workspace &ws, const float *d_q, uint64_t nq, uint64_t ksel, uint64_t k, uint64_t *d_idx,
                            float *d_dist, uint64_t *d_cnt);
    void scan_rows(uint64_t nrows, uint32_t d, const float *Q, uint32_t nq, int metric, const float *xsq, const float *qsq, float *out,
                   uint64_t ld, bool use_lds, hipStream_t s) const;
    void rerank_rows(uint32_t d, const float *Q, uint32_t nq, int metric, const float *xsq, const float *qsq, const uint64_t *cand,
                     uint64_t *out, uint32_t ncand, uint32_t ldc, hipStream_t s) const;
    void flat_debug_keys(Workspace &ws, const float *d_q, uint64_t nq, int tier, float *h_keys, float *h_qsq, float *h_qerr,
                         float *h_dx /* [4]: dx_abs, dx_rel, xsq_max, xsq_min_pos */);
    void flat_exact_device(Workspace &ws, const float *d_q, const float *d_qsq, uint64_t nq, uint32_t ksel,
                           uint64_t k, uint64_t *d_idx, float *d_dist, uint64_t *d_cnt);
    // Exact range search (k_range.hip): per query every row with D <= d_radius[q] (the first `limit` of them when limit > 0), ascending by
    // (distance, index); returns synchronised.  8-bit tier for the queries its bound admits, strict-order scan for the rest.
    void flat_range_device(Workspace &ws, const float *d_q, uint64_t nq, const float *d_radius, uint64_t limit, RangeResult &out,
                           const RowMask *mask = nullptr);
    // (mask != nullptr: only the mask's allowed rows -- the filtered range search; nullptr: the unfiltered call, statement for statement)
    // Its two halves: the sorted pair keys of every query into a pool, then the CSR arrays from (pool, offsets, counts).
    void flat_range_collect(Workspace &ws, const float *d_q, uint64_t nq, const float *d_radius, uint64_t limit, const RowMask *mask, RangePool &rp,
                            uint64_t *h_off, uint64_t *h_cnt, RangeTally *tally);
    void flat_range_assemble(Workspace &ws, uint64_t nq, const RangePool &rp, const std::vector<uint64_t> &h_off, const std::vector<uint64_t> &h_cnt,
                             RangeResult &out);
    // The filtered range search with one mask per query (multi_plan.hpp): query q's slice is what flat_range_device returns for it alone
    // under masks[mask_of[q]] (mask_of: host).  On an f32 index the buckets of masks of at most flat_filtered_direct_max rows are answered by
    // one k_range_gather_grouped launch per chunk of queries; every other bucket is gathered and goes through flat_range_collect under its
    // mask.  One pool, one assemble.  The caller has checked the masks and mask_of; returns synchronised.  A call that fails leaves every
    // counter but the high-water mark range_hits_max as it found it.
    void flat_range_masked_multi_device(Workspace &ws, const float *d_q, uint64_t nq, const float *d_radius, uint64_t limit,
                                        const RowMask *const *masks, uint64_t n_masks, const uint32_t *mask_of, RangeResult &out);
    // Exact filtered k-NN (k_filter.hip): the first min(k, m) pairs of FlatIndex::knn over the mask's allowed rows; returns synchronised.
    // Direct path (gathered strict-order scan) for short allow-lists and wherever the 8-bit tier does not apply; otherwise the 8-bit
    // filter pass with the masked row constants + the exact stage, its open queries redone by the direct path.  A sibling of
    // flat_range_device: it neither reads nor writes the k-NN tiers' auto-off counters.
    void flat_knn_masked_device(Workspace &ws, const float *d_q, uint64_t nq, uint64_t k, const RowMask &mask, uint64_t *d_idx, float *d_dist,
                                uint64_t *d_cnt);
    void flat_masked_direct(Workspace &ws, const float *d_q, uint64_t nq, uint64_t k, const RowMask &mask, uint64_t *d_idx, float *d_dist,
                            uint64_t *d_cnt);  // enqueues; the caller synchronises
    // The same with one mask per query (multi_plan.hpp): query q under masks[mask_of[q]] (mask_of: host).  The buckets of masks of at most
    // flat_filtered_direct_max rows (k <= 1024) are scanned by one k_scan_gather_grouped launch per chunk of queries; every other bucket
    // goes through flat_knn_masked_device, gathered and scattered back.  The caller has checked the masks and mask_of; returns synchronised.
    void flat_knn_masked_multi_device(Workspace &ws, const float *d_q, uint64_t nq, uint64_t k, const RowMask *const *masks, uint64_t n_masks,
                                      const uint32_t *mask_of, uint64_t *d_idx, float *d_dist, uint64_t *d_cnt);
    void check_mask(const RowMask &mask) const;  // throws: a mask of another index (invalid argument), a stale mask (state)
    const float *masked_rowc(Workspace &ws, const RowMask &mask);  // after ensure_i8 succeeded; builds the copy on first use
    // Label columns (k_labels.hip, vdb_index_labels_*): LABEL_COLUMNS logical columns of one u32 per LOCAL row, the filterable attributes of
    // the rows as codes.  A column is allocated by its first write (4 B per row, grown with the rows); one never written reads as
    // LABEL_NONE for every row and takes no memory.  The allocated columns follow add_rows (new rows: LABEL_NONE), swap_remove and
    // remove_rows on either element type; writing labels does not bump write_gen (a mask is a set of rows) and touches no PQ / HNSW /
    // IVF state.
    DevBuf d_labels[LABEL_COLUMNS];
    bool label_live[LABEL_COLUMNS] = {};
    uint32_t *label_col(uint32_t c) const { return label_live[c] ? d_labels[c].as<uint32_t>() : nullptr; }  // nullptr: never written
    LabelCols label_cols() const;  // the allocated columns
    uint32_t label_columns() const { return label_cols().n; }
    void labels_set(uint32_t column, uint64_t first_row, const uint32_t *codes, uint64_t count);  // write-side
    void labels_get(uint32_t column, uint64_t first_row, uint64_t count, uint32_t *out) const;
    // Scattered label writes (labels_scatter_plan.hpp, k_labels_scatter / k_labels_set_mask; docs/DESIGN_flat.md 4.1t), write-side like
    // labels_set: label[columns[c]][row] for rows that are no contiguous run, n_cols columns in ONE launch, no host copy of a column.
    // Everything is checked before a column is allocated or written; a target column never written comes to life first, as in
    // labels_set (allocated for n rows, LABEL_NONE everywhere).  write_gen and rowc_gen stay: a mask is a set of rows.  All return
    // synchronised.
    //   labels_scatter: rows = m distinct LOCAL rows on the host, codes [n_cols][m] on the host; ids (as u32) and codes are uploaded once
    //     each through the workspace (keys_a, misc).
    //   labels_scatter_device: d_ids = m u64 GLOBAL ids on the device, d_codes u32 [n_cols][m] there; k_fetch_check and one read-back of its
    //     flag first -- an id that is no row of the index throws with nothing written.  An id named twice gets one of its codes.
    //   labels_set_mask: codes[c] to column columns[c] of every row the mask allows; the list is the mask's own d_ids, the pairs travel
    //     by value, nothing is uploaded.  The caller ran check_mask.
    void labels_scatter(const uint64_t *rows, uint64_t m, const uint32_t *columns, uint64_t n_cols, const uint32_t *codes);
    void labels_scatter_device(const uint64_t *d_ids, uint64_t m, const uint32_t *columns, uint64_t n_cols, const uint32_t *d_codes);
    void labels_set_mask(const RowMask &mask, const uint32_t *columns, const uint32_t *codes, uint64_t n_cols);
    // the target columns in the caller's order, the ones never written brought to life on `s` (allocates: call it after every check)
    LabelCols labels_targets(const uint32_t *columns, uint64_t n_cols, hipStream_t s);
    uint32_t labels_scatter_max_blocks = 0;  // "labels_scatter_max_blocks": grid cap of the two kernels, 0 = 8 blocks per CU
    std::atomic<uint64_t> labels_scatter_calls{0}, labels_scatter_rows{0};  // the three calls that wrote rows (m > 0, not refused) / rows they wrote
    // Row masks from the labels, on the device: mask g = the rows r with label[columns[t]][r] == codes[t] for every t in
    // [term_lims[g], term_lims[g + 1]).  Fills out[g] (fresh RowMask objects of the caller) exactly as vdb_mask_create fills a mask from
    // the equivalent bits; read-side; returns synchronised.  Everything is checked before anything is launched; on a throw the caller
    // discards every out[g].
    void masks_where(const uint64_t *term_lims, const uint32_t *columns, const uint32_t *codes, uint64_t n_masks, RowMask *const *out);
    std::atomic<uint64_t> mask_where_masks{0};  // masks built by masks_where
    // The same for set / range terms {columns[t], lo[t], hi[t], flags[t], bitmap words [set_lims[t], set_lims[t + 1]) of set_words}
    // (mask_sets.hpp states the match and checks the arguments; set_lims == nullptr: no term has a bitmap).  Same contract as masks_where.
    void masks_where_sets(const uint64_t *term_lims, const uint32_t *columns, const uint32_t *lo, const uint32_t *hi, const uint32_t *flags,
                          const uint64_t *set_lims, const uint64_t *set_words, uint64_t n_masks, RowMask *const *out);
    std::atomic<uint64_t> mask_where_set_masks{0};  // masks built by masks_where_sets
    // An OR of conjunctions of such terms (mask_any.hpp; k_mask_rows<MaskAny>): mask g = the rows that match EVERY term of SOME clause in
    // [mask_lims[g], mask_lims[g + 1]); clause c's terms are [clause_lims[c], clause_lims[c + 1]) of the term arrays.  A mask without
    // clauses is empty, a clause without terms allows every row.  Same contract as masks_where_sets.
    void masks_where_any(const uint64_t *mask_lims, const uint64_t *clause_lims, const uint32_t *columns, const uint32_t *lo, const uint32_t *hi,
                         const uint32_t *flags, const uint64_t *set_lims, const uint64_t *set_words, uint64_t n_masks, RowMask *const *out);
    std::atomic<uint64_t> mask_where_any_masks{0};  // masks built by masks_where_any
    // out = AND (op 0) / OR (op 1) over n_in (1 .. MASK_COMBINE_MAX) masks of this index, input i complemented within the rows first when
    // invert && invert[i] (k_mask_combine).  Every input is checked with check_mask before anything is computed; read-side; returns
    // synchronised; on a throw the caller discards `out`.
    void mask_combine(int op, const RowMask *const *in, const uint8_t *invert, uint64_t n_in, RowMask &out);
    std::atomic<uint64_t> mask_combine_masks{0};  // masks built by mask_combine
    // ONE column grouped by code in a single read of it (mask_partition.hpp, k_mask_partition): out[j] = the mask of the rows whose
    // label in `column` equals codes[j], bit-identical to masks_where's mask of that one term; the codes are distinct.  The masks of a
    // chunk share two allocations (RowMask::slab_bits / slab_ids) unless VDB_EFENCE.  Same contract as masks_where.
    void masks_partition(uint32_t column, const uint32_t *codes, uint64_t n_codes, RowMask *const *out);
    std::atomic<uint64_t> mask_partition_masks{0};  // masks built by masks_partition
    // out_counts[j] = the rows allowed by `mask` (nullptr: every row) whose label in `column` equals codes[j] (k_label_counts); the same
    // code rules; the mask is checked with check_mask before anything is computed; read-side; returns synchronised.
    void label_counts(uint32_t column, const RowMask *mask, const uint32_t *codes, uint64_t n_codes, uint64_t *out_counts);
    std::atomic<uint64_t> label_count_calls{0};  // label_counts calls
    // out_counts[j] = the rows whose label in `column` equals codes[j], out_first[j] = the lowest such LOCAL row (LOOKUP_ROW_NONE when
    // there is none), from ONE read of the column (direct route) or one per PART_MAX_CHUNK codes (sorted route): lookup_plan.hpp checks
    // and routes, k_lookup.hip computes.  The same code rules as label_counts; everything is checked before an output or a counter is
    // touched; read-side; returns synchronised.  docs/DESIGN_flat.md 4.1aa.
    void label_lookup(uint32_t column, const uint32_t *codes, uint64_t n_codes, uint64_t *out_first, uint64_t *out_counts);
    uint64_t label_lookup_table_bytes = LOOKUP_TABLE_BYTES_DEFAULT;  // "label_lookup_table_bytes": scratch cap of the direct route's table, 0 = sorted route only
    uint32_t label_lookup_max_blocks = 0;                            // "label_lookup_max_blocks": grid cap of the lookup kernels, 0 = 8 blocks per CU
    // accepted calls | codes they named | calls that took the direct route | reads of the column (kernel launches), summed
    std::atomic<uint64_t> label_lookup_calls{0}, label_lookup_codes{0}, label_lookup_direct{0}, label_lookup_passes{0};
    // The five builders, label_counts and label_lookup are in index_masks.hip, on two shared halves that are local to that file (4.1y).
    // The four Flat list re-rankers below -- grouped, diversified, by example, fused -- are in flat_rerank.hip, on one shared driver (4.1x).
    // Grouped Flat k-NN (k_group.hip, grouped_plan.hpp; docs/DESIGN_flat.md 4.1q): per query the first k rows, in FlatIndex::knn's order over
    // the allowed rows, of which at most g carry any one value of label column `column` (rows without a label are always kept).  Rounds:
    // the exact sorted list of K' rows per open query -- flat_knn_device without masks, flat_knn_masked_multi_device over the call's masks,
    // whose counters advance as for those calls -- walked by k_group_cap, ONE read-back of the done bytes, the open queries compacted and
    // sent round again with 4 K' until a list is the query's whole allowed set.  n_masks == 0: unfiltered (masks / mask_of not read).  The
    // caller has checked column, g >= 1, the masks and mask_of; returns synchronised.
    void flat_knn_grouped_device(Workspace &ws, const float *d_q, uint64_t nq, uint64_t k, uint32_t column, uint64_t g, const RowMask *const *masks,
                                 uint64_t n_masks, const uint32_t *mask_of, uint64_t *d_idx, float *d_dist, uint64_t *d_cnt);
    // k_group_cap alone over caller-supplied lists [nq][ld] (device): every id of the counted ranges is checked on the device first (one
    // flag read back; a bad one throws before an output is written).  Returns synchronised.
    void group_cap_device(Workspace &ws, const uint64_t *d_ids, const float *d_dists, const uint64_t *d_counts, uint64_t nq, uint64_t ld, uint64_t k,
                          uint32_t column, uint64_t g, uint64_t *d_idx, float *d_dist, uint64_t *d_cnt);
    uint64_t flat_grouped_oversample = GROUPED_OVERSAMPLE_DEFAULT;  // "flat_grouped_oversample": round 0 fetches min(m, k x this) rows
    std::atomic<uint64_t> grouped_calls{0}, grouped_queries{0}, grouped_rounds{0}, grouped_exhausted{0};
    // Diversified Flat k-NN (k_mmr.hip, mmr_plan.hpp; docs/DESIGN_flat.md 4.1u): per query the greedy maximal-marginal-relevance selection
    // of min(k, F) rows from the first F = min(fetch_k, m) rows of FlatIndex::knn's order over the allowed rows, in selection order.  ONE
    // round: the exact sorted list of F rows per query -- flat_knn_device without masks, flat_knn_masked_multi_device over the call's
    // masks, whose counters advance as for those calls -- then k_mmr_select, in sub-chunks of queries whose lists stay under
    // LIST_BUDGET.  n_masks == 0: unfiltered (masks / mask_of not read).  The caller has checked k, fetch_k, lambda (mmr_check_args),
    // the masks and mask_of; returns synchronised.
    void flat_knn_mmr_device(Workspace &ws, const float *d_q, uint64_t nq, uint64_t k, uint64_t fetch_k, float lambda, const RowMask *const *masks,
                             uint64_t n_masks, const uint32_t *mask_of, uint64_t *d_idx, float *d_dist, uint64_t *d_cnt);
    // k_mmr_select alone over caller-supplied lists [nq][ld] (device), walked as given: every id of the counted ranges is checked on the
    // device first (one flag read back; a bad one throws before an output is written).  Returns synchronised.
    void mmr_select_device(Workspace &ws, const uint64_t *d_ids, const float *d_dists, const uint64_t *d_counts, uint64_t nq, uint64_t ld, uint64_t k,
                           float lambda, uint64_t *d_idx, float *d_dist, uint64_t *d_cnt);
    std::atomic<uint64_t> mmr_calls{0}, mmr_queries{0};
    // Search by example rows (k_like.hip, like_plan.hpp; docs/DESIGN_flat.md 4.1v).  LikeLists: the example lists of a call on the device --
    // ids (u32 LOCAL rows, or global: u64 row + id_offset) and limits of nq + 1 entries each; neg_lims == nullptr: no negatives.  The caller
    // has checked the limits (like_check_lims) and every id.
    struct LikeLists {
        const void *pos_ids = nullptr, *neg_ids = nullptr;
        const uint64_t *pos_lims = nullptr, *neg_lims = nullptr;
        bool global_ids = false;
        uint64_t e_max = 0, n_examples = 0;  // like_e_max | every list entry of the call
    };
    // k_like_build alone: the query vectors of queries q0 .. q0 + nq of the lists into d_out [nq][dim]; enqueued on ws.stream, not synchronised
    void like_queries_device(Workspace &ws, const LikeLists &ll, uint64_t q0, uint64_t nq, float *d_out);
    // ONE round: the query vectors, the exact sorted list of K' = like_list_len(..) rows per query -- flat_knn_device without masks,
    // flat_knn_masked_multi_device over the call's masks, whose counters advance as for those calls -- then k_like_drop, in sub-chunks of
    // queries whose lists stay under LIST_BUDGET.  The queries are q0 .. q0 + nq of the lists (mask_of already advanced).  n_masks == 0:
    // unfiltered (masks / mask_of not read).  Returns synchronised.
    void flat_knn_like_device(Workspace &ws, const LikeLists &ll, uint64_t q0, uint64_t nq, uint64_t k, bool exclude, const RowMask *const *masks,
                              uint64_t n_masks, const uint32_t *mask_of, uint64_t *d_idx, float *d_dist, uint64_t *d_cnt);
    // k_like_drop alone over caller-supplied lists [nq][ld] (device), walked as given, against the global ids d_drop_ids under the DEVICE
    // limits d_drop_lims (n_drop = their last entry): every id of the counted ranges and every listed id is checked on the device first
    // (one flag read back; a bad one throws before an output is written).  Returns synchronised.
    void drop_listed_device(Workspace &ws, const uint64_t *d_ids, const float *d_dists, const uint64_t *d_counts, uint64_t nq, uint64_t ld, uint64_t k,
                            const uint64_t *d_drop_lims, const uint64_t *d_drop_ids, uint64_t n_drop, uint64_t *d_idx, float *d_dist, uint64_t *d_cnt);
    // one flag read-back: throws when one of the global ids d_a[0 .. ma) / d_b[0 .. mb) is no row of this index (an empty list is not read)
    void like_check_ids_device(Workspace &ws, const uint64_t *d_a, uint64_t ma, const uint64_t *d_b, uint64_t mb);
    std::atomic<uint64_t> like_calls{0}, like_queries{0}, like_example_rows{0};
    // Fused multi-query Flat search (k_fuse.hip, fuse_plan.hpp; docs/DESIGN_flat.md 4.1w): fused query q owns the sub-queries
    // lims[q] - lims[0] .. lims[q + 1] - lims[0] - 1 of d_q (lims: HOST, nq + 1 entries, any base); its answer is the fusion (mode FUSE_RRF /
    // FUSE_MIN) of their lists, each the first min(fetch_k, m_s) rows of FlatIndex::knn's order over the sub-query's allowed rows.  ONE round
    // per sub-chunk of fused queries (fuse_sub_chunk): the lists of all its sub-queries from ONE flat_knn_device call, or ONE
    // flat_knn_masked_multi_device call over the call's masks, whose counters advance as for those calls, then ONE k_fuse_lists launch.
    // weights (HOST, one per sub-query, nullptr: all 1.0f) and mask_of (one per sub-query) start at the call's first sub-query.
    // n_masks == 0: unfiltered (masks / mask_of not read).  The caller has checked the arguments (fuse_check_args), the masks and mask_of;
    // returns synchronised.
    void flat_knn_fused_device(Workspace &ws, const float *d_q, const uint64_t *lims, uint64_t nq, uint64_t k, uint64_t fetch_k, int mode,
                               const float *weights, float rrf_c, const RowMask *const *masks, uint64_t n_masks, const uint32_t *mask_of, uint64_t *d_idx,
                               float *d_dist, uint64_t *d_cnt);
    // k_fuse_lists alone over caller-supplied lists [lims[nq]][ld] (device), walked as given (lims: HOST, from 0): every id of the counted
    // ranges is checked on the device first (one flag read back; a bad one throws before an output is written).  Returns synchronised.
    void fuse_lists_device(Workspace &ws, const uint64_t *d_ids, const float *d_dists, const uint64_t *d_counts, const uint64_t *lims, uint64_t nq,
                           uint64_t ld, uint64_t k, int mode, const float *weights, float rrf_c, uint64_t *d_idx, float *d_dist, uint64_t *d_cnt);
    std::atomic<uint64_t> fused_calls{0}, fused_queries{0}, fused_lists{0};
    // Document-level fused Flat search (k_fuse_groups.hip, fuse_groups_plan.hpp; docs/DESIGN_flat.md 4.1z): flat_knn_fused_device with the
    // lists joined by GROUP, the value of label column `column` (a row without one: a group of its own), mode FUSE_RRF / FUSE_MIN /
    // FUSE_SUM; the same ONE list call per sub-chunk (fuse_groups_sub_chunk), then ONE k_fuse_groups launch.  d_exact (device u8 [nq],
    // nullptr: not wanted): whether the answer is the one the whole table would give.  The caller has checked the arguments
    // (fuse_groups_check_args), the masks and mask_of; returns synchronised.
    void flat_knn_fused_groups_device(Workspace &ws, const float *d_q, const uint64_t *lims, uint64_t nq, uint64_t k, uint64_t fetch_k, int mode,
                                      const float *weights, float rrf_c, uint32_t column, const RowMask *const *masks, uint64_t n_masks,
                                      const uint32_t *mask_of, uint64_t *d_idx, float *d_dist, uint64_t *d_cnt, uint8_t *d_exact);
    // k_fuse_groups alone over caller-supplied lists [lims[nq]][ld] (device), walked as given (lims: HOST, from 0); a list that counts
    // trunc_len entries or more is a truncated one.  Every id of the counted ranges is checked on the device first (one flag read back; a
    // bad one throws before an output is written).  Returns synchronised.
    void fuse_groups_device(Workspace &ws, const uint64_t *d_ids, const float *d_dists, const uint64_t *d_counts, const uint64_t *lims, uint64_t nq,
                            uint64_t ld, uint64_t k, int mode, const float *weights, float rrf_c, uint32_t column, uint64_t trunc_len, uint64_t *d_idx,
                            float *d_dist, uint64_t *d_cnt, uint8_t *d_exact);
    std::atomic<uint64_t> fused_groups_calls{0}, fused_groups_queries{0}, fused_groups_lists{0};
    // Near-duplicate grouping (flat_dups.hip, k_components.hip, dup_plan.hpp; docs/DESIGN_flat.md 4.1ab): the connected components of the
    // allowed rows (mask == nullptr: all rows) under the edges {i, j}, j != i on the list flat_range_device returns for query = row i at
    // `radius` under `limit` and the mask -- SINGLE LINKAGE at the radius.  d_group [n] u64 on the device: the lowest row of row i's
    // component + id_offset, DUP_ROW_NONE for a row outside the mask; stats [DUP_STATS] on the host: groups of >= 2 rows, rows in them,
    // non-self pairs seen, rows whose list reached `limit`.  The allowed rows are walked in chunks of dup_chunk queries: in place on an
    // unfiltered f32 index, gathered (widened) into ws.grp_q otherwise; ONE flat_range_device call per chunk, whose counters advance as for
    // that call, its result hooked and dropped.  Read-side, re-entrant; d_group, stats and the dup_* counters are written only when every
    // chunk has succeeded.  The caller has run dup_check_args; the mask is checked here.  Returns synchronised.
    void flat_dup_groups_device(Workspace &ws, float radius, uint64_t limit, const RowMask *mask, uint64_t *d_group, uint64_t *stats);
    // The component stage alone over a caller-supplied CSR edge list on the device: d_src [nq] u64 ids of the lists' source rows, d_lims
    // [nq + 1] from 0, d_ids [d_lims[nq]] u64 ids.  Limits and every id are checked on the device first (one read-back: the flag and the
    // pair count; a bad one throws before an output is written).  stats as above, truncated = 0.  Returns synchronised.
    void link_pairs_device(Workspace &ws, const uint64_t *d_src, const uint64_t *d_lims, const uint64_t *d_ids, uint64_t nq, uint64_t *d_group,
                           uint64_t *stats);
    uint64_t dup_chunk = DUP_CHUNK_DEFAULT;  // "flat_dup_chunk": queries per range call of the self-join
    std::atomic<uint64_t> dup_calls{0}, dup_chunks{0}, dup_pairs{0};  // flat_dup_groups calls that succeeded / their range calls / non-self pairs they saw
    std::atomic<uint64_t> write_gen{0};  // bumped by add_rows / swap_remove / remove_rows: what a RowMask is checked against
    uint64_t flat_filtered_direct_max = 8192;  // allow-lists up to this many rows take the direct path ("flat_filtered_direct_max")
    std::atomic<uint64_t> filtered_queries{0}, filtered_direct_queries{0}, filtered_i8_queries{0}, filtered_fallback_queries{0};
    std::atomic<uint64_t> filtered_multi_calls{0}, filtered_grouped_queries{0};  // calls with a mask per query / queries their grouped launch answered
    uint64_t range_max_results = 0;  // ceiling on the pairs of one call ("flat_range_max_results"; 0: what the device can hold)
    std::atomic<uint64_t> range_queries{0}, range_i8_queries{0}, range_scan_queries{0}, range_hits{0}, range_results{0};
    std::atomic<uint64_t> range_hits_max{0};  // longest hit list of a query the tier answered
    std::atomic<uint64_t> range_multi_calls{0}, range_grouped_queries{0};  // range calls with a mask per query / queries their grouped launch answered

private:
    // ---- Mirror upkeep: how a row edit (add_rows, swap_remove, remove_rows, update_rows) is carried into the tiled images of d_rows.  A
    // write path asks live_mirrors() BEFORE its edit which images are in step, rewrites the 16-row tiles it touched with retile(), and
    // calls mirrors_shrunk() when the table got shorter; an image it cannot patch it invalidates.  docs/DESIGN_flat.md 4.1ac.
    struct MirrorSet {
        bool tiled = false, half = false, i8 = false;  // d_tiled | d_tiled_h | d_tiled_i8 + d_rowc_i8
    };
    MirrorSet live_mirrors() const;  // the tiled images that cover all n rows now (the only ones an edit may patch)
    // tiles [ta, tb) of the named images from the f32 view v of n_rows rows (v + r * dim = row r), with the current scale / mu / lambdas
    void retile_tiles(MirrorSet live, const float *v, uint64_t n_rows, uint64_t ta, uint64_t tb, hipStream_t s);
    // The touched tiles of the named images, for a table of n_rows rows (rows at and past n_rows become padding): the n_tiles tiles of the
    // device list d_tiles in one launch per image when there is a list and the rows are f32, else the range [t_begin, t_end) through
    // for_tile_chunks.  Enqueues on ws.stream; allocates nothing on an f32 index (u8: for_tile_chunks' ws.dense, reserved by the caller).
    void retile(Workspace &ws, MirrorSet live, uint64_t n_rows, const uint32_t *d_tiles, uint64_t n_tiles, uint64_t t_begin, uint64_t t_end);
    // the table shrank from n to n1 rows (n not yet updated) and the touched tiles were rewritten: an image that was in step follows, one
    // that was behind is rebuilt in full by its next use; the row-major images are dropped
    void mirrors_shrunk(uint64_t n1);
    void widen_norm_bounds(const float *sq, uint64_t count);  // xsq_max / xsq_min_pos over more row norms: widened, never narrowed
    // THE fp16 scale rule: false for all-zero or extreme data (no fp16 mirror); else need = the E with |x| < 2^E for every |x|^2 <= xsq_max
    static bool half_exp_needed(float xsq_max, int &need);
    void half_fold_err(hipStream_t s);  // syncs s, reads d_half_err's two maxima and folds them into half_dx_abs / half_dx_rel
    // rows[0..m) (checked, n <= 2^32) narrowed into h_ids and uploaded to ws.keys_a on ws.stream; h_ids lives until the caller's sync.
    // Reserves keys_a: call it before the first write.
    const uint32_t *upload_ids(Workspace &ws, const uint64_t *rows, uint64_t m, std::vector<uint32_t> &h_ids);
};

// what every filtered, mask-per-query and grouped k-NN entry point and search requires of the index
inline void require_f32_rows(const Index &ix) {
    VDB_REQUIRE(!ix.elem_u8, "filtered k-NN needs f32 rows: a VecSet<u8> index serves the filtered range search only");
}

struct WsLease {
    Index &ix;
    std::unique_ptr<Workspace> ws;
    explicit WsLease(Index &i) : ix(i), ws(i.acquire_ws()) {}
    ~WsLease() { ix.release_ws(std::move(ws)); }
    Workspace &operator*() { return *ws; }
    Workspace *operator->() { return ws.get(); }
};

}  // namespace vdb
