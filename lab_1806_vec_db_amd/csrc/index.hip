// index.hip -- Index object: HBM-resident VecSet + the Flat search pipeline.
#include "index.hpp"
#include "fetch_plan.hpp"
#include "multi_plan.hpp"
#include "remove_plan.hpp"
#include "update_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace vdb {

Index::Index(int dev, uint64_t d, int ds, bool u8) : device(dev), dim(d), dist(ds), elem_u8(u8) {
#ifndef VDB_HOST_SANITIZER_BUILD  // (the thread-sanitizer binary of tests/cpp/tsan_host.cpp has no device: host-side state only)
    use_device();
    hipDeviceProp_t prop;
    VDB_HIP(hipGetDeviceProperties(&prop, dev));
    num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    std::string arch = prop.gcnArchName;
    if (arch.rfind("gfx950", 0) != 0)
        throw Error(4, "libvdbhip is built for gfx950 (MI355X) only; device reports " + arch);
#endif
}

std::unique_ptr<Workspace> Index::acquire_ws() {
    use_device();
    {
        std::lock_guard<std::mutex> g(ws_mu);
        if (!ws_free.empty()) {
            auto ws = std::move(ws_free.back());
            ws_free.pop_back();
            return ws;
        }
    }
    return std::make_unique<Workspace>();
}
void Index::release_ws(std::unique_ptr<Workspace> ws) {
    if (!ws) return;
    std::lock_guard<std::mutex> g(ws_mu);
    ws_free.push_back(std::move(ws));
}

const float *Index::rows_f32_view(DevBuf &scratch, uint64_t r0, uint64_t r1, hipStream_t s) const {
    if (!elem_u8) return d_rows.as<float>();
    scratch.reserve(std::max<uint64_t>(r1 - r0, 1) * dim * sizeof(float));
    launch_widen_u8(d_rows.as<uint8_t>() + r0 * dim, (r1 - r0) * dim, scratch.as<float>(), s);
    return reinterpret_cast<const float *>(reinterpret_cast<uintptr_t>(scratch.p) - r0 * dim * sizeof(float));
}
const float *Index::host_rows() const {
    VDB_REQUIRE(!elem_u8, "this operation needs f32 rows: a VecSet<u8> index serves Flat search only");
    std::lock_guard<std::mutex> g(host_mu);
    if (!host_valid) {
        use_device();
        h_rows.resize(size_t(n) * dim);
        if (n) VDB_HIP(hipMemcpy(h_rows.data(), d_rows.p, size_t(n) * dim * sizeof(float), hipMemcpyDeviceToHost));
        host_valid = true;
    }
    return h_rows.data();
}

// ---- mirror upkeep of the row edits (index.hpp, the private section of Index; docs/DESIGN_flat.md 4.1ac) ---------------------------------
Index::MirrorSet Index::live_mirrors() const {
    const bool mfma = mfma_supported((uint32_t)dim);
    return {mfma && tiled_m.valid, mfma && half_m.covers(n), i8_m.covers(n)};
}
void Index::retile_tiles(MirrorSet live, const float *v, uint64_t n_rows, uint64_t ta, uint64_t tb, hipStream_t s) {
    const uint32_t d = (uint32_t)dim;
    if (live.tiled) launch_tile_rows(v, n_rows, d, ta, tb, d_tiled.as<float>(), s);
    if (live.half) launch_tile_rows_h(v, n_rows, d, ta, tb, half_sx(), d_tiled_h.p, s);
    if (live.i8)  // (f32 rows only) tiles, codes and constants; Cosine: the mirror of the UNIT rows, from the norms in d_sq
        launch_tile_rows_i8(v, n_rows, d, ta, tb, d_mu_i8.as<float>(), i8_l1, i8_l2, d_tiled_i8.p, d_rowc_i8.as<float>(), s,
                            dist == 1 ? d_sq.as<float>() : nullptr);
}
void Index::retile(Workspace &ws, MirrorSet live, uint64_t n_rows, const uint32_t *d_tiles, uint64_t n_tiles, uint64_t t_begin, uint64_t t_end) {
    if (!(live.tiled || live.half || live.i8)) return;
    hipStream_t s = ws.stream;
    if (d_tiles && !elem_u8) {
        const uint32_t d = (uint32_t)dim;
        const float *x = d_rows.as<float>();
        if (live.tiled) launch_tile_rows_list(x, n_rows, d, d_tiles, n_tiles, d_tiled.as<float>(), s);
        if (live.half) launch_tile_rows_h_list(x, n_rows, d, d_tiles, n_tiles, half_sx(), d_tiled_h.p, s);
        if (live.i8)
            launch_tile_rows_i8_list(x, n_rows, d, d_tiles, n_tiles, d_mu_i8.as<float>(), i8_l1, i8_l2, d_tiled_i8.p, d_rowc_i8.as<float>(), s,
                                     dist == 1 ? d_sq.as<float>() : nullptr);
    } else if (t_end > t_begin) {  // a u8 index re-tiles through widened chunks
        for_tile_chunks(ws, t_begin, t_end, n_rows,
                        [&](const float *v, uint64_t ta, uint64_t tb, uint64_t, uint64_t) { retile_tiles(live, v, n_rows, ta, tb, s); });
    }
}
void Index::mirrors_shrunk(uint64_t n1) {
    if (tiled_m.valid) tiled_m.rows = n1;
    // the fp16 scale stays and the moved rows' rounding error is already part of half_dx_*; behind the table, it was never measured
    if (half_m.rows == n)
        half_m.rows = n1;
    else
        half_m.invalidate();
    if (i8_m.covers(n))
        i8_m.rows = n1;
    else
        i8_m.invalidate();  // rows were added since the last search: rebuilt by the next one
    rows_h_m.invalidate();  // (rebuilt by the next walk / scan that uses them)
    rows_q8_m.invalidate();
}
void Index::widen_norm_bounds(const float *sq, uint64_t count) {
    for (uint64_t j = 0; j < count; j++) {
        const float v = sq[j];
        if (v > xsq_max && std::isfinite(v)) xsq_max = v;
        if (v > 0.0f && v < xsq_min_pos) xsq_min_pos = v;
    }
}
bool Index::half_exp_needed(float xsq_max, int &need) {
    if (!(xsq_max >= 0x1p-80f && xsq_max <= 0x1p80f)) return false;
    int e = 0;
    (void)std::frexp(xsq_max, &e);  // xsq_max = m * 2^e, m in [0.5, 1)  =>  |x| < 2^ceil(e/2)
    need = e >= 0 ? (e + 1) / 2 : -((-e) / 2);
    return true;
}
void Index::half_fold_err(hipStream_t s) {
    VDB_SYNC(s);
    float e2[2];  // (the f32 bits of the kernel's two maxima; read into this call's own storage, not the workspace's pinned block)
    VDB_HIP(hipMemcpy(e2, d_half_err.p, sizeof(e2), hipMemcpyDeviceToHost));
    half_dx_abs = std::max(half_dx_abs, std::sqrt(e2[0]) * 1.001f);  // the kernel's f32 sums: relative error << 1e-3
    half_dx_rel = std::max(half_dx_rel, std::sqrt(e2[1]) * 1.001f);
}
const uint32_t *Index::upload_ids(Workspace &ws, const uint64_t *rows, uint64_t m, std::vector<uint32_t> &h_ids) {
    h_ids.resize(m);
    labels_scatter_ids(rows, m, h_ids.data());
    ws.keys_a.reserve(m * sizeof(uint32_t));
    VDB_HIP(hipMemcpyAsync(ws.keys_a.p, h_ids.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice, ws.stream));
    return ws.keys_a.as<uint32_t>();
}

// VecSet::push (vec_set.rs:113-118) for `count` rows + dist_cache (hnsw_index.rs:251-254)
void Index::add_rows(const void *rows, uint64_t count, bool on_device) {
    if (count == 0) return;
    use_device();
    VDB_REQUIRE(n + count < (1ull << 32), "a shard holds at most 2^32-1 rows (ids are u32 on the device)");
    WsLease ws(*this);
    hipStream_t s = ws->stream;
    size_t row_bytes = size_t(dim) * elem_size();
    d_rows.grow((n + count) * row_bytes + 16, n * row_bytes, s);  // +16: the u8 kernels may read a 16-B word at the last row's end
    d_sq.grow((n + count + 128) * sizeof(float), n * sizeof(float), s);  // +128: kernels may read a few entries past n
    for (uint32_t c = 0; c < LABEL_COLUMNS; c++)  // (a failed allocation here leaves every buffer's contents and n as they were)
        if (label_live[c]) d_labels[c].grow((n + count) * sizeof(uint32_t), n * sizeof(uint32_t), s);
    launch_label_fill(label_cols(), n, n + count, num_cu, s);  // the new rows carry no label
    char *dst = d_rows.as<char>() + n * row_bytes;
    VDB_HIP(hipMemcpyAsync(dst, rows, count * row_bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    const uint64_t tiles_new = mirror_tiles(n + count), tiles_old = n / 16;  // (the partially filled tile is rewritten)
    const uint64_t tile_bytes = 16 * size_t(mfma_dim_pad((uint32_t)dim)) * sizeof(float);
    // a built split-bf16 mirror is extended; one that cannot grow is dropped and rebuilt (or not) by the search that wants it
    const bool mirror = mfma_supported((uint32_t)dim) && tiled_m.valid &&
                        tiled_m.attempt([&] { d_tiled.grow(tiles_new * tile_bytes, tiles_old * tile_bytes, s); });
    // row norms of the new rows and the fragment-ordered mirror of every 16-row tile that received rows (a u8 index feeds
    // these f32 build kernels widened chunks; the rows themselves stay at one byte per element)
    for_tile_chunks(*ws, tiles_old, tiles_new, n + count, [&](const float *v, uint64_t ta, uint64_t tb, uint64_t ra, uint64_t rb) {
        const uint64_t a = std::max(ra, n);
        if (rb > a) launch_row_sqnorm(v + a * dim, rb - a, (uint32_t)dim, d_sq.as<float>() + a, s);
        retile_tiles({mirror, false, false}, v, n + count, ta, tb, s);
    });
    std::vector<float> sq(count);
    VDB_HIP(hipMemcpyAsync(sq.data(), d_sq.as<float>() + n, count * sizeof(float), hipMemcpyDeviceToHost, s));
    VDB_SYNC(s);
    widen_norm_bounds(sq.data(), count);
    h_sq.insert(h_sq.end(), sq.begin(), sq.end());
    if (mirror) tiled_m.rows = n + count;
    // an fp16 mirror in step is extended (needs the new xsq_max) unless the 8-bit pass is this index's first tier: then it waits for its
    // first use, as does one already behind (ensure_half catches up); one that cannot grow is dropped (as above)
    if (half_m.rows == n && !i8_defers_half() && half_m.attempt([&] { half_refresh(*ws, n, n + count); })) half_m.rows = n + count;
    {
        std::lock_guard<std::mutex> g(host_mu);
        if (on_device || elem_u8) {
            host_valid = false;
        } else if (host_valid) {
            const float *fr = static_cast<const float *>(rows);
            h_rows.insert(h_rows.end(), fr, fr + count * dim);
        }
    }
    n += count;
    write_gen += 1;
}

// VecSet::swap_remove (vec_set.rs:131-137)
void Index::swap_remove(uint64_t i) {
    VDB_REQUIRE(i < n, "swap_remove: index out of bounds");
    use_device();
    WsLease ws(*this);
    hipStream_t s = ws->stream;
    uint64_t last = n - 1;
    const size_t row_bytes = size_t(dim) * elem_size();
    if (i < last) {
        VDB_HIP(hipMemcpyAsync(d_rows.as<char>() + i * row_bytes, d_rows.as<char>() + last * row_bytes, row_bytes, hipMemcpyDeviceToDevice, s));
        VDB_HIP(hipMemcpyAsync(d_sq.as<float>() + i, d_sq.as<float>() + last, sizeof(float), hipMemcpyDeviceToDevice, s));
        launch_label_move_one(label_cols(), (uint32_t)i, (uint32_t)last, s);
    }
    // the tiles of the moved row and of the removed last row, once each (d_sq[i] already holds the moved row's norm)
    const MirrorSet live = live_mirrors();
    retile(*ws, live, last, nullptr, 0, i / 16, i / 16 + 1);
    if (last / 16 != i / 16) retile(*ws, live, last, nullptr, 0, last / 16, last / 16 + 1);
    mirrors_shrunk(last);
    VDB_SYNC(s);
    {
        std::lock_guard<std::mutex> g(host_mu);
        if (host_valid && !elem_u8) {
            if (i < last) std::memcpy(h_rows.data() + i * dim, h_rows.data() + last * dim, dim * sizeof(float));
            h_rows.resize(last * dim);
        }
    }
    if (i < last) h_sq[i] = h_sq[last];
    h_sq.resize(last);
    n = last;
    write_gen += 1;
    // xsq_max stays an upper bound (certification only needs a bound)
}

// MetadataVecTable::delete's loop of swap_removes (metadata_vec_table.rs:170-186) as one pass
void Index::remove_rows(const uint64_t *rows, uint64_t m, std::vector<uint64_t> &dst, std::vector<uint64_t> &src) {
    dst.clear();
    src.clear();
    const char *why = remove_plan_check(n, rows, m);
    VDB_REQUIRE(!why, why);
    if (m == 0) return;
    use_device();
    WsLease ws(*this);
    hipStream_t s = ws->stream;
    const uint64_t n1 = n - m;
    const size_t row_bytes = size_t(dim) * elem_size();
    remove_plan(n, rows, m, dst, src);
    const uint64_t moves = dst.size();
    // the 16-row tiles whose rows change: those of the filled holes, and from the new end of the table to the end of a mirror of n1 rows
    // (rows at and past n1 become padding)
    const MirrorSet live = live_mirrors();
    const bool tiles_wanted = mfma_supported((uint32_t)dim) || live.i8;
    std::vector<uint32_t> h_moves(2 * moves), h_tiles;
    for (uint64_t j = 0; j < moves; j++) {
        h_moves[2 * j] = (uint32_t)dst[j];
        h_moves[2 * j + 1] = (uint32_t)src[j];
    }
    if (tiles_wanted) {
        for (uint64_t j = moves; j-- > 0;)  // (dst descends)
            if (h_tiles.empty() || h_tiles.back() != dst[j] / 16) h_tiles.push_back(uint32_t(dst[j] / 16));
        for (uint64_t t = n1 / 16; t < mirror_tiles(n1); t++)
            if (h_tiles.empty() || h_tiles.back() != t) h_tiles.push_back((uint32_t)t);
    }
    const uint64_t n_tiles = h_tiles.size();
    // a u8 index re-tiles through the widened chunks of the range path, from the first touched tile to the end
    const bool list_form = !elem_u8;
    ws->keys_a.reserve(std::max<size_t>(h_moves.size(), 1) * sizeof(uint32_t));
    ws->keys_b.reserve(std::max<size_t>(n_tiles, 1) * sizeof(uint32_t));
    if (!list_form && n_tiles) ws->dense.reserve(tile_chunk_bytes());  // (for_tile_chunks' buffer: its own reserve is then a no-op)
    // ---- nothing was changed up to here; from here on nothing allocates on the device ----
    const uint32_t *d_moves = ws->keys_a.as<uint32_t>(), *d_tiles = ws->keys_b.as<uint32_t>();
    if (moves) VDB_HIP(hipMemcpyAsync(ws->keys_a.p, h_moves.data(), h_moves.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    if (n_tiles && list_form) VDB_HIP(hipMemcpyAsync(ws->keys_b.p, h_tiles.data(), n_tiles * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    launch_rows_move(d_rows.p, row_bytes, d_sq.as<float>(), d_moves, moves, num_cu, s);
    launch_label_move(label_cols(), d_moves, moves, num_cu, s);  // (the columns only shrink here: nothing to reserve)
    retile(*ws, live, n1, d_tiles, n_tiles, n_tiles ? h_tiles.front() : mirror_tiles(n1), mirror_tiles(n1));  // (d_sq already holds the moved rows')
    mirrors_shrunk(n1);
    VDB_SYNC(s);
    {
        std::lock_guard<std::mutex> g(host_mu);
        if (host_valid && !elem_u8) {
            for (uint64_t j = 0; j < moves; j++) std::memcpy(h_rows.data() + dst[j] * dim, h_rows.data() + src[j] * dim, dim * sizeof(float));
            h_rows.resize(n1 * dim);
        }
    }
    for (uint64_t j = 0; j < moves; j++) h_sq[dst[j]] = h_sq[src[j]];
    h_sq.resize(n1);
    n = n1;
    write_gen += 1;
    // xsq_max / xsq_min_pos stay bounds
}

// New vectors for the rows `rows` (distinct, any order), in place: no row moves, n / id_offset / the label columns stay, and so does
// write_gen -- a RowMask is a set of rows and the set did not change (docs/DESIGN_flat.md 4.1r).
void Index::update_rows(const uint64_t *rows, uint64_t m, const void *vecs, bool on_device) {
    const char *why = update_plan_check(n, rows, m);
    VDB_REQUIRE(!why, why);
    if (m == 0) return;
    VDB_REQUIRE(vecs, "update_rows: null vectors");
    VDB_REQUIRE(!elem_u8, "update_rows needs f32 rows: a VecSet<u8> index is not updated in place");
    use_device();
    WsLease ws(*this);
    hipStream_t s = ws->stream;
    const uint32_t d = (uint32_t)dim;
    const size_t row_bytes = size_t(dim) * sizeof(float);
    std::vector<uint32_t> h_ids, h_tiles;
    update_plan(n, rows, m, h_tiles);
    const uint64_t n_tiles = h_tiles.size();
    const MirrorSet live = live_mirrors();  // (the fp16 mirror's touched tiles are rewritten only if the scale still fits)
    // host vectors go through a bounded staging buffer, a chunk of rows at a time; device vectors are read where they are
    const uint64_t chunk = std::min<uint64_t>(m, std::max<uint64_t>(UPDATE_STAGE_BYTES / row_bytes, 1));
    std::vector<float> sq(m);
    ws->keys_b.reserve(n_tiles * sizeof(uint32_t));
    ws->misc.reserve(m * sizeof(float));
    if (!on_device) ws->dense.reserve(chunk * row_bytes);
    if (live.half) d_half_err.reserve(2 * sizeof(uint32_t));
    const uint32_t *d_ids = upload_ids(*ws, rows, m, h_ids), *d_tiles = ws->keys_b.as<uint32_t>();  // (the last reserve: ws.keys_a)
    // ---- nothing was changed up to here; from here on nothing allocates on the device ----
    float *d_sq_new = ws->misc.as<float>();
    VDB_HIP(hipMemcpyAsync(ws->keys_b.p, h_tiles.data(), n_tiles * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    if (live.half) VDB_HIP(hipMemsetAsync(d_half_err.p, 0, 2 * sizeof(uint32_t), s));
    for (uint64_t j0 = 0; j0 < m; j0 += chunk) {
        const uint64_t nb = std::min(chunk, m - j0);
        const char *from = static_cast<const char *>(vecs) + j0 * row_bytes;
        const float *d_new = reinterpret_cast<const float *>(from);
        if (!on_device) {
            VDB_HIP(hipMemcpyAsync(ws->dense.p, from, nb * row_bytes, hipMemcpyHostToDevice, s));
            d_new = ws->dense.as<float>();
        }
        launch_row_sqnorm(d_new, nb, d, d_sq_new + j0, s);  // the strict fold of add_rows: the norms of a table built with these rows
        launch_rows_scatter(d_rows.p, row_bytes, d_sq.as<float>(), d_ids + j0, d_new, d_sq_new + j0, nb, num_cu, s);
        // the new rows' rounding error under the CURRENT fp16 scale (dropped below if that scale no longer fits)
        if (live.half) launch_row_split_err(d_new, d_sq_new + j0, 0, nb, d, half_sx(), d_half_err.as<uint32_t>(), s);
    }
    // the 8-bit mirror keeps its mu / lambdas (bounds for any row); Cosine reads d_sq: the new norms are in place
    retile(*ws, {live.tiled, false, live.i8}, n, d_tiles, n_tiles, 0, 0);
    if (!live.i8) i8_m.invalidate();  // rows were added since the last search: rebuilt by the next one
    VDB_HIP(hipMemcpyAsync(sq.data(), d_sq_new, m * sizeof(float), hipMemcpyDeviceToHost, s));
    VDB_SYNC(s);
    widen_norm_bounds(sq.data(), m);
    for (uint64_t j = 0; j < m; j++) h_sq[rows[j]] = sq[j];
    // fp16 mirror: patched when the new xsq_max still fits the scale it was built with
    int need = 0;
    if (live.half && half_exp_needed(xsq_max, need) && need <= half_exp) {
        retile(*ws, {false, true, false}, n, d_tiles, n_tiles, 0, 0);
        half_fold_err(s);
    } else {
        half_m.invalidate();  // behind the table, or the scale is too small now: rebuilt in full by its next use
    }
    rows_h_m.invalidate();
    rows_q8_m.invalidate();
    {
        std::lock_guard<std::mutex> g(host_mu);
        if (on_device) {
            host_valid = false;
        } else if (host_valid) {
            const float *fr = static_cast<const float *>(vecs);
            for (uint64_t j = 0; j < m; j++) std::memcpy(h_rows.data() + rows[j] * dim, fr + j * dim, row_bytes);
        }
    }
    rowc_gen += 1;  // the masks' copies of the row constants are stale; the masks themselves are not
    update_calls += 1;
    updated_rows += m;
}

// ---- bulk row fetch (fetch_plan.hpp, k_fetch.hip; docs/DESIGN_flat.md 4.1s) -----------------------------------------------------------
// Chunk c is gathered into staging buffer c & 1 on ws.stream and copied to the host from there on ws.copy_stream.  The gather of chunk
// c + 1 is enqueued BEFORE the copy of chunk c: a copy into pageable memory holds the calling thread until it is done, and the gather
// runs meanwhile.  The copies go straight into `out` (no pinned bounce buffer of the library's: that would add a second pass over the
// result on the host behind the runtime's own staging of pageable copies).
void Index::fetch_gathered(Workspace &ws, const uint32_t *d_ids, uint64_t m, void *out, bool widen, uint64_t chunk_rows) {
    const size_t out_row = widen ? size_t(dim) * sizeof(float) : size_t(dim) * elem_size();
    const uint64_t n_chunks = m / chunk_rows + (m % chunk_rows ? 1 : 0);
    DevBuf *stage[2] = {&ws.dense, &ws.lists};
    stage[0]->reserve(std::min(m, chunk_rows) * out_row);
    if (n_chunks > 1) {
        stage[1]->reserve(chunk_rows * out_row);
        ws.fetch_streams();
    }
    hipStream_t s = ws.stream, cs = n_chunks > 1 ? ws.copy_stream : ws.stream;
    auto gather = [&](uint64_t c) {
        const uint64_t j0 = c * chunk_rows, nb = std::min(chunk_rows, m - j0);
        const int b = int(c & 1);
        if (c >= 2) VDB_HIP(hipStreamWaitEvent(s, ws.fetch_ev[2 + b], 0));  // the copy that last read this buffer
        if (widen)
            launch_rows_gather_widen(d_rows.as<uint8_t>(), dim, d_ids + j0, false, 0, stage[b]->as<float>(), nb, num_cu, s);
        else
            launch_rows_gather(d_rows.p, out_row, d_ids + j0, false, 0, stage[b]->p, nb, num_cu, s);
        if (n_chunks > 1) VDB_HIP(hipEventRecord(ws.fetch_ev[b], s));
    };
    try {
        gather(0);
        for (uint64_t c = 0; c < n_chunks; c++) {
            if (c + 1 < n_chunks) gather(c + 1);
            const uint64_t j0 = c * chunk_rows, nb = std::min(chunk_rows, m - j0);
            const int b = int(c & 1);
            if (n_chunks > 1) VDB_HIP(hipStreamWaitEvent(cs, ws.fetch_ev[b], 0));
            VDB_HIP(hipMemcpyAsync(static_cast<char *>(out) + j0 * out_row, stage[b]->p, nb * out_row, hipMemcpyDeviceToHost, cs));
            if (n_chunks > 1) VDB_HIP(hipEventRecord(ws.fetch_ev[2 + b], cs));
        }
        if (cs != s) VDB_SYNC(cs);
        VDB_SYNC(s);
    } catch (...) {  // nothing of a failed call still writes to the caller's memory or reads the staging buffers
        if (cs != s) (void)hipStreamSynchronize(cs);
        (void)hipStreamSynchronize(s);
        throw;
    }
}

void Index::get_rows(const uint64_t *rows, uint64_t m, void *out, bool as_f32) {
    VDB_REQUIRE(as_f32 || elem_u8, "not a VecSet<u8> index");
    const bool widen = as_f32 && elem_u8;
    const uint64_t out_row = as_f32 ? dim * sizeof(float) : dim;
    const char *why = fetch_plan_check(n, rows, m, out_row);
    VDB_REQUIRE(!why, why);
    if (m == 0) return;
    VDB_REQUIRE(out, "get_rows: null out");
    VDB_REQUIRE(n <= (1ull << 32), "get_rows: a shard holds at most 2^32 rows");
    const FetchPlan plan = fetch_plan(rows, m, out_row, fetch_chunk_bytes);
    use_device();
    WsLease ws(*this);
    hipStream_t s = ws->stream;
    if (plan.route == FETCH_DIRECT && !widen) {  // a contiguous piece of the table, as it stands
        VDB_HIP(hipMemcpyAsync(out, d_rows.as<char>() + rows[0] * out_row, m * out_row, hipMemcpyDeviceToHost, s));
        VDB_SYNC(s);
        fetch_direct += 1;
    } else {
        std::vector<uint32_t> h_ids;
        fetch_gathered(*ws, upload_ids(*ws, rows, m, h_ids), m, out, widen, plan.chunk_rows);  // (synchronised: h_ids may go)
        fetch_chunks += plan.n_chunks;
    }
    fetch_calls += 1;
    fetch_rows += m;
}

void Index::get_rows_mask(const RowMask &mask, float *out) {
    const uint64_t m = mask.m, out_row = dim * sizeof(float);
    VDB_REQUIRE(m <= ~uint64_t(0) / out_row, "get_rows: the result does not fit the address space");
    if (m == 0) return;
    VDB_REQUIRE(out, "get_rows: null out");
    const FetchPlan plan = fetch_plan_chunks(m, out_row, fetch_chunk_bytes);
    use_device();
    WsLease ws(*this);
    fetch_gathered(*ws, mask.d_ids.as<uint32_t>(), m, out, elem_u8, plan.chunk_rows);
    fetch_chunks += plan.n_chunks;
    fetch_calls += 1;
    fetch_rows += m;
}

void Index::get_rows_device(Workspace &ws, const uint64_t *d_ids, uint64_t m, void *d_out, hipStream_t s) {
    ws.flags.reserve(sizeof(uint32_t));
    ids_ok(ws, s, ws.flags.as<uint32_t>(), "get_rows: the list holds an id that is no row of this index (id - id_offset must be below len)",
           [&](uint32_t *d_flag) { launch_fetch_check(d_ids, m, n, id_offset, d_flag, num_cu, s); });
    if (elem_u8)
        launch_rows_gather_widen(d_rows.as<uint8_t>(), dim, d_ids, true, id_offset, static_cast<float *>(d_out), m, num_cu, s);
    else
        launch_rows_gather(d_rows.p, dim * sizeof(float), d_ids, true, id_offset, d_out, m, num_cu, s);
    VDB_SYNC(s);
    fetch_chunks += 1;
    fetch_calls += 1;
    fetch_rows += m;
}

// ---- label columns (k_labels.hip; the masks built from them: index_masks.hip) ----------------------------------------------------------
LabelCols Index::label_cols() const {
    LabelCols lc{};
    for (uint32_t c = 0; c < LABEL_COLUMNS; c++)
        if (uint32_t *col = label_col(c)) lc.col[lc.n++] = col;
    return lc;
}

static void labels_check_range(const Index &ix, uint32_t column, uint64_t first_row, uint64_t count) {
    VDB_REQUIRE(column < LABEL_COLUMNS, "labels: column " + std::to_string(column) + ", an index has " + std::to_string(LABEL_COLUMNS));
    VDB_REQUIRE(first_row <= ix.n && count <= ix.n - first_row, "labels: rows [" + std::to_string(first_row) + ", " + std::to_string(first_row) +
                                                                    " + " + std::to_string(count) + ") pass the " + std::to_string(ix.n) +
                                                                    " rows of the index");
}

void Index::labels_set(uint32_t column, uint64_t first_row, const uint32_t *codes, uint64_t count) {
    labels_check_range(*this, column, first_row, count);
    if (count == 0) return;
    VDB_REQUIRE(codes, "null argument");
    use_device();
    WsLease ws(*this);
    hipStream_t s = ws->stream;
    if (!label_live[column]) {  // first write: the column comes to life with every row unlabelled
        d_labels[column].grow(n * sizeof(uint32_t), 0, s);
        LabelCols one{};
        one.col[0] = d_labels[column].as<uint32_t>();
        one.n = 1;
        launch_label_fill(one, 0, n, num_cu, s);
        label_live[column] = true;
    }
    VDB_HIP(hipMemcpyAsync(d_labels[column].as<uint32_t>() + first_row, codes, count * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    VDB_SYNC(s);
}

void Index::labels_get(uint32_t column, uint64_t first_row, uint64_t count, uint32_t *out) const {
    labels_check_range(*this, column, first_row, count);
    if (count == 0) return;
    VDB_REQUIRE(out, "null argument");
    if (!label_live[column]) {
        std::fill(out, out + count, LABEL_NONE);
        return;
    }
    use_device();
    VDB_HIP(hipMemcpy(out, d_labels[column].as<uint32_t>() + first_row, count * sizeof(uint32_t), hipMemcpyDeviceToHost));
}

// ---- scattered label writes (labels_scatter_plan.hpp, k_labels.hip; docs/DESIGN_flat.md 4.1t) --------------------------------------------
LabelCols Index::labels_targets(const uint32_t *columns, uint64_t n_cols, hipStream_t s) {
    LabelCols fresh{};
    for (uint64_t c = 0; c < n_cols; c++)
        if (!label_live[columns[c]]) {
            d_labels[columns[c]].grow(n * sizeof(uint32_t), 0, s);
            fresh.col[fresh.n++] = d_labels[columns[c]].as<uint32_t>();
        }
    launch_label_fill(fresh, 0, n, num_cu, s);  // first write: the columns come to life with every row unlabelled
    LabelCols target{};
    for (uint64_t c = 0; c < n_cols; c++) {  // (live only now: an allocation that failed above left no column half made)
        label_live[columns[c]] = true;
        target.col[target.n++] = d_labels[columns[c]].as<uint32_t>();
    }
    return target;
}

void Index::labels_scatter(const uint64_t *rows, uint64_t m, const uint32_t *columns, uint64_t n_cols, const uint32_t *codes) {
    const char *why = labels_scatter_check(n, rows, m, columns, n_cols);
    VDB_REQUIRE(!why, why);
    if (m == 0) return;
    VDB_REQUIRE(codes, "labels_scatter: null codes");
    VDB_REQUIRE(n <= (1ull << 32), "labels_scatter: a shard holds at most 2^32 rows");
    use_device();
    WsLease ws(*this);
    hipStream_t s = ws->stream;
    std::vector<uint32_t> h_ids;
    ws->misc.reserve(n_cols * m * sizeof(uint32_t));
    const uint32_t *d_ids = upload_ids(*ws, rows, m, h_ids);  // (into the workspace: no column is allocated or written yet)
    const LabelCols target = labels_targets(columns, n_cols, s);
    VDB_HIP(hipMemcpyAsync(ws->misc.p, codes, n_cols * m * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    prof_begin(*ws, "labels_scatter", double(m) * sizeof(uint32_t) * double(1 + 2 * n_cols));
    launch_labels_scatter(target, d_ids, false, 0, ws->misc.as<uint32_t>(), m, num_cu, labels_scatter_max_blocks, s);
    prof_end(*ws);
    VDB_SYNC(s);  // (h_ids and the caller's codes may go)
    prof_collect(*ws);
    labels_scatter_calls += 1;
    labels_scatter_rows += m;
}

void Index::labels_scatter_device(const uint64_t *d_ids, uint64_t m, const uint32_t *columns, uint64_t n_cols, const uint32_t *d_codes) {
    const char *why = labels_scatter_columns_check(m, columns, n_cols);
    VDB_REQUIRE(!why, why);
    if (m == 0) return;
    VDB_REQUIRE(d_ids && d_codes, "labels_scatter: null argument");
    VDB_REQUIRE(reinterpret_cast<uintptr_t>(d_ids) % 8 == 0 && reinterpret_cast<uintptr_t>(d_codes) % 4 == 0,
                "labels_scatter: d_ids must be 8-byte and d_codes 4-byte aligned");
    use_device();
    WsLease ws(*this);
    hipStream_t s = ws->stream;
    ws->flags.reserve(sizeof(uint32_t));
    ids_ok(*ws, s, ws->flags.as<uint32_t>(), "labels_scatter: the list holds an id that is no row of this index (id - id_offset must be below len)",
           [&](uint32_t *d_flag) { launch_fetch_check(d_ids, m, n, id_offset, d_flag, num_cu, s); });
    const LabelCols target = labels_targets(columns, n_cols, s);
    prof_begin(*ws, "labels_scatter", double(m) * (sizeof(uint64_t) + sizeof(uint32_t) * double(2 * n_cols)));
    launch_labels_scatter(target, d_ids, true, id_offset, d_codes, m, num_cu, labels_scatter_max_blocks, s);
    prof_end(*ws);
    VDB_SYNC(s);
    prof_collect(*ws);
    labels_scatter_calls += 1;
    labels_scatter_rows += m;
}

void Index::labels_set_mask(const RowMask &mask, const uint32_t *columns, const uint32_t *codes, uint64_t n_cols) {
    const uint64_t m = mask.m;
    const char *why = labels_scatter_columns_check(m, columns, n_cols);
    VDB_REQUIRE(!why, why);
    if (m == 0) return;
    VDB_REQUIRE(codes, "labels_set_mask: null codes");
    use_device();
    WsLease ws(*this);
    hipStream_t s = ws->stream;
    const LabelCols target = labels_targets(columns, n_cols, s);
    LabelSet set{};
    for (uint32_t c = 0; c < target.n; c++) {
        set.col[c] = target.col[c];
        set.code[c] = codes[c];
    }
    set.n = target.n;
    prof_begin(*ws, "labels_scatter", double(m) * sizeof(uint32_t) * double(1 + n_cols));
    launch_labels_set_mask(set, mask.d_ids.as<uint32_t>(), m, num_cu, labels_scatter_max_blocks, s);
    prof_end(*ws);
    VDB_SYNC(s);
    prof_collect(*ws);
    labels_scatter_calls += 1;
    labels_scatter_rows += m;
}

// ---- images of the rows (RowMirror): a tier whose image is missing leaves its queries to the next one (8-bit -> fp16 -> split-bf16 ->
// exact scan over the rows themselves; IVF scan: 8-bit -> fp16 -> f32 rows)
bool RowMirror::attempt(const std::function<void()> &build) {
    try {
        build();
        return true;
    } catch (const AllocError &) {  // (DevBuf::grow allocates before it frees: an old image, if any, is intact but stale)
        for (DevBuf *b : bufs) b->release();
        invalidate();
        failures += 1;
        return false;
    }
}
bool RowMirror::ensure(uint64_t n, const std::function<bool()> &current, const std::function<void()> &build) {
    std::lock_guard<std::mutex> g(mu);
    if (current()) return true;
    if (failed_n == n) return false;
    if (attempt(build)) return true;
    failed_n = n;
    return false;
}

bool Index::ensure_tiled(Workspace &ws) {
    if (n == 0) return true;
    return tiled_m.ensure(n, [&] { return tiled_m.covers(n); }, [&] {
        const uint64_t tiles = mirror_tiles(n);
        d_tiled.reserve(tiles * 16 * size_t(mfma_dim_pad((uint32_t)dim)) * sizeof(float));
        for_tile_chunks(ws, 0, tiles, n, [&](const float *v, uint64_t ta, uint64_t tb, uint64_t, uint64_t) {
            retile_tiles({true, false, false}, v, n, ta, tb, ws.stream);
        });
        VDB_SYNC(ws.stream);
        tiled_m.set(n);
    });
}

uint64_t Index::hbm_bytes_per_row() const {
    uint64_t b = dim * elem_size() + sizeof(float);  // VecSet row + dist_cache entry
    if (mfma_supported((uint32_t)dim)) {
        if (tiled_m.valid) b += uint64_t(mfma_dim_pad((uint32_t)dim)) * sizeof(float);
        if (half_m.valid) b += uint64_t(mfma_dim_pad((uint32_t)dim)) * sizeof(uint16_t);
    }
    if (i8_m.valid) b += uint64_t(mfma_dim_pad((uint32_t)dim)) + 2 * sizeof(float);
    if (rows_h_m.valid) b += dim * sizeof(uint16_t);
    if (rows_q8_m.valid) b += dim + 2 * sizeof(float);
    if (pq.present) b += pq.enc_dim * (pq.codes_t_valid ? 2 : 1);
    if (hnsw.present) b += hnsw.max_m0 * sizeof(uint32_t) + sizeof(uint32_t);
    b += uint64_t(label_columns()) * sizeof(uint32_t);
    return b;
}

// ---- scaled fp16 mirror (k_half.hip) ---------------------------------------------------------------
// Called with d_rows, d_sq and xsq_max valid for n_new rows; rows [n_old, n_new) are new.  The scale follows the
// largest row norm: when that grows past the current scale's range the whole mirror is rewritten (one extra bit of
// headroom, so this happens at most once per doubling of the largest norm).
void Index::half_refresh(Workspace &ws, uint64_t n_old, uint64_t n_new) {
    if (!gemm_f16_supported((uint32_t)dim)) return;
    int need = 0;
    if (!half_exp_needed(xsq_max, need)) {  // the split-bf16 / exact paths serve such data
        half_m.valid = false;
        return;
    }
    hipStream_t s = ws.stream;
    const bool rebuild = !half_m.valid || need > half_exp;
    const uint64_t tiles_new = mirror_tiles(n_new);
    const uint64_t tile_bytes = 16 * size_t(mfma_dim_pad((uint32_t)dim)) * sizeof(uint16_t);
    uint64_t t0 = n_old / 16, r0 = n_old;
    if (rebuild) {
        half_exp = need + 1;
        half_dx_abs = half_dx_rel = 0.0f;
        t0 = 0;
        r0 = 0;
    }
    d_tiled_h.grow(tiles_new * tile_bytes, t0 * tile_bytes, s);
    d_half_err.reserve(2 * sizeof(uint32_t));
    VDB_HIP(hipMemsetAsync(d_half_err.p, 0, 2 * sizeof(uint32_t), s));
    for_tile_chunks(ws, t0, tiles_new, n_new, [&](const float *v, uint64_t ta, uint64_t tb, uint64_t ra, uint64_t rb) {
        retile_tiles({false, true, false}, v, n_new, ta, tb, s);
        const uint64_t a = std::max(ra, r0);
        if (rb > a) launch_row_split_err(v, d_sq.as<float>(), a, rb, (uint32_t)dim, half_sx(), d_half_err.as<uint32_t>(), s);
    });
    half_fold_err(s);
    half_m.valid = true;
}

// ---- centred 8-bit mirror (k_i8.hip) ---------------------------------------------------------------
bool Index::i8_mirror_applicable() const {
    if (elem_u8 || flat_i8_mode == 1 || (dim & 3) != 0 || !gemm8_supported((uint32_t)dim) || n <= 64) return false;
    return xsq_max <= 0x1p80f;  // extreme data: the other tiers' own guards decide
}
bool Index::i8_applicable(uint32_t ksel) const {
    if (!i8_mirror_applicable() || !flat_tail_lb_supported((uint32_t)dim, flat_i8_kprime, ksel)) return false;
    const uint64_t iq = i8_queries.load(), ir = i8_redo.load();
    return flat_i8_mode == 2 || iq < 1024 || ir * 8 <= iq;
}
bool Index::ensure_i8(Workspace &ws) {
    return i8_m.ensure(n, [&] { return i8_m.covers(n); }, [&] { build_i8(ws); });
}
void Index::build_i8(Workspace &ws) {  // (under i8_m.mu)
    hipStream_t s = ws.stream;
    const uint32_t d = (uint32_t)dim;
    const uint64_t tiles = mirror_tiles(n);
    const uint64_t tile_bytes = 16 * size_t(mfma_dim_pad(d));
    const bool rebuild = !i8_m.valid || i8_m.rows > n || n >= 2 * i8_mu_rows;
    const float *xsq_cos = dist == 1 ? d_sq.as<float>() : nullptr;  // Cosine: the mirror of the UNIT rows (k_i8.hip)
    uint64_t t0 = rebuild ? 0 : i8_m.rows / 16;
    d_tiled_i8.grow(tiles * tile_bytes, t0 * tile_bytes, s);
    d_rowc_i8.grow(tiles * 16 * 2 * sizeof(float), t0 * 16 * 2 * sizeof(float), s);
    if (rebuild) {
        // mu = mean of a row sample; rho = typical |dx| / |x_c| of that sample -> l1 = rho, l2 = 1 / rho (k_i8.hip: any
        // positive pair is valid, this one is tight for queries that look like rows)
        d_mu_i8.reserve(size_t(d) * sizeof(float));
        ws.dense.reserve(size_t(I8_MEAN_CHUNKS) * d * sizeof(float) + 2 * 16384 * sizeof(float));
        launch_i8_col_mean(d_rows.as<float>(), n, d, ws.dense.as<float>(), d_mu_i8.as<float>(), s, xsq_cos);
        const uint64_t n_s = std::min<uint64_t>(n, 16384), stride = n / n_s, n_s16 = (n_s + 15) / 16 * 16;
        float *d_stats = ws.dense.as<float>() + size_t(I8_MEAN_CHUNKS) * d;
        launch_i8_row_stats(d_rows.as<float>(), n, d, d_mu_i8.as<float>(), n_s, stride, d_stats, s, xsq_cos);
        std::vector<float> st(2 * n_s16), mu(d);
        VDB_HIP(hipMemcpyAsync(st.data(), d_stats, st.size() * sizeof(float), hipMemcpyDeviceToHost, s));
        VDB_HIP(hipMemcpyAsync(mu.data(), d_mu_i8.p, d * sizeof(float), hipMemcpyDeviceToHost, s));
        VDB_SYNC(s);
        double e2 = 0, xs = 0, m2 = 0;
        for (uint64_t i = 0; i < n_s; i++)
            if (std::isfinite(st[2 * i]) && std::isfinite(st[2 * i + 1])) {
                e2 += st[2 * i];
                xs += st[2 * i + 1];
            }
        for (float v : mu) m2 += double(v) * v;
        float rho = xs > 0 ? (float)std::sqrt(e2 / xs) : 0.01f;
        if (!(rho >= 1e-4f)) rho = 1e-4f;  // exactly representable rows: keep the split finite
        if (rho > 0.5f) rho = 0.5f;
        i8_l1 = rho;
        i8_l2 = 1.0f / rho;
        i8_mu_norm = (float)std::sqrt(m2) * 1.001f;
        i8_mu_rows = n;
    }
    retile_tiles({false, false, true}, d_rows.as<float>(), n, t0, tiles, s);
    VDB_SYNC(s);
    i8_m.set(n);
}

bool Index::i8_defers_half() const {
    return !elem_u8 && flat_i8_mode != 1 && (dim & 3) == 0 && gemm8_supported((uint32_t)dim);
}
bool Index::ensure_half(Workspace &ws) {
    return half_m.ensure(n, [&] { return half_m.rows == n; }, [&] {
        half_refresh(ws, half_m.rows > n ? 0 : half_m.rows.load(), n);
        half_m.rows = n;
    }) && half_m.valid;
}

void Index::prepare_flat(bool all_tiers) {
    if (n == 0) return;
    use_device();
    WsLease ws(*this);
    if (!mfma_supported((uint32_t)dim) || elem_u8) return;  // the exact scan needs nothing beyond the rows
    bool first = false;
    if (i8_defers_half() && n > 64) first = ensure_i8(*ws);
    if (!first || all_tiers) first = ensure_half(*ws) || first;
    if (!first || all_tiers) (void)ensure_tiled(*ws);
}

// the row-major images are accelerators (pre-passes, key refinement, the IVF scan's first tier): their callers go on without them
bool Index::ensure_rows_h(Workspace &ws) {
    if (elem_u8 || dim % 64 != 0 || dim > 4096 || n == 0 || !ensure_half(ws)) return false;
    return rows_h_m.ensure(n, [&] { return rows_h_m.covers(n) && rows_h_exp == half_exp; }, [&] {
        const uint64_t r0 = rows_h_exp != half_exp || rows_h_m.rows > n ? 0 : rows_h_m.rows.load();
        d_rows_h.grow(n * dim * sizeof(uint16_t) + 16, r0 * dim * sizeof(uint16_t), ws.stream);
        launch_rows_to_half(d_rows.as<float>() + r0 * dim, (n - r0) * dim, half_sx(), d_rows_h.as<uint16_t>() + r0 * dim, ws.stream);
        VDB_SYNC(ws.stream);
        rows_h_m.set(n);
        rows_h_exp = half_exp;
    });
}

bool Index::ensure_rows_q8(Workspace &ws) {
    if (elem_u8 || dim % 64 != 0 || dim > 1024 || n == 0) return false;  // (dim * 127^2 < 2^24: the integer sums are exact as f32)
    return rows_q8_m.ensure(n, [&] { return rows_q8_m.covers(n); }, [&] {
        const uint64_t r0 = rows_q8_m.rows > n ? 0 : rows_q8_m.rows.load();
        d_rows_q8.grow(n * dim + 16, r0 * dim, ws.stream);
        d_q8_scale.grow((n + 64) * sizeof(float), r0 * sizeof(float), ws.stream);
        d_q8_err.grow((n + 64) * sizeof(float), r0 * sizeof(float), ws.stream);
        launch_rows_to_q8(d_rows.as<float>() + r0 * dim, n - r0, (uint32_t)dim, d_rows_q8.as<int8_t>() + r0 * dim,
                          d_q8_scale.as<float>() + r0, d_q8_err.as<float>() + r0, ws.stream);
        VDB_SYNC(ws.stream);
        rows_q8_m.set(n);
    });
}

// ---- timing hooks ------------------------------------------------------------------------------
void Index::prof_begin(Workspace &ws, const char *name, double bytes) {
    if (!prof_on) return;
    if (ws.ev_used == ws.ev_pool.size()) {
        hipEvent_t a, b;
        VDB_HIP(hipEventCreate(&a));
        VDB_HIP(hipEventCreate(&b));
        ws.ev_pool.emplace_back(a, b);
    }
    ws.pending.push_back({name, ws.ev_used, bytes});
    VDB_HIP(hipEventRecord(ws.ev_pool[ws.ev_used].first, ws.stream));
}
void Index::prof_end(Workspace &ws) {
    if (!prof_on) return;
    VDB_HIP(hipEventRecord(ws.ev_pool[ws.ev_used].second, ws.stream));
    ws.ev_used++;
}
void Index::prof_collect(Workspace &ws) {
    if (ws.pending.empty()) return;
    std::lock_guard<std::mutex> g(prof_mu);
    for (auto &p : ws.pending) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ws.ev_pool[p.ev].first, ws.ev_pool[p.ev].second) == hipSuccess) {
            auto &e = prof[p.name];
            e.ms += ms;
            e.launches += 1;
            e.bytes += p.bytes;
        }
    }
    ws.pending.clear();
    ws.ev_used = 0;
}

// the two search-time readers of the row-major rows, by element type
void Index::scan_rows(uint64_t nrows, uint32_t d, const float *Q, uint32_t nq, int metric, const float *xsq, const float *qsq,
                      float *out, uint64_t ld, bool use_lds, hipStream_t s) const {
    if (elem_u8)
        launch_scan_exact_u8(d_rows.as<uint8_t>(), nrows, d, Q, nq, metric, xsq, qsq, out, ld, s);
    else
        launch_scan_exact(d_rows.as<float>(), nrows, d, Q, nq, metric, xsq, qsq, out, ld, use_lds, s);
}
void Index::rerank_rows(uint32_t d, const float *Q, uint32_t nq, int metric, const float *xsq, const float *qsq, const uint64_t *cand,
                        uint64_t *out, uint32_t ncand, uint32_t ldc, hipStream_t s) const {
    if (elem_u8)
        launch_rerank_u8(d_rows.as<uint8_t>(), d, Q, nq, metric, xsq, qsq, cand, out, ncand, ldc, s);
    else
        launch_rerank(d_rows.as<float>(), d, Q, nq, metric, xsq, qsq, cand, out, ncand, ldc, s);
}

// ---- Flat: exact scan path -----------------------------------------------------------------------
// FlatIndex::knn (flat_index.rs:48-57) for nq queries: strict-order distances for every row, then the
// k smallest pairs by (distance, index).
void Index::flat_exact_device(Workspace &ws, const float *d_q, const float *d_qsq, uint64_t nq, uint32_t ksel,
                              uint64_t k, uint64_t *d_idx, float *d_dist, uint64_t *d_cnt) {
    hipStream_t s = ws.stream;
    const int metric = dist == 0 ? MET_L2_DIRECT : MET_COSINE;
    const uint64_t ld = (n + 63) & ~63ull;
    const uint32_t nl = topk_num_lists(n);
    const uint32_t cap = topk_capacity(ksel);
    constexpr uint32_t BQ = 8;
    ws.dense.reserve(size_t(BQ) * ld * sizeof(float));
    ws.lists.reserve(size_t(BQ) * nl * cap * sizeof(uint64_t));
    ws.keys_c.reserve(size_t(BQ) * cap * sizeof(uint64_t));
    // Small corpus, many queries (tables of a few thousand rows, centroid sets): one thread per (query, row) pair
    // folds in reference order and a wave per query selects -- three launches for the whole batch.  The scan kernel
    // below assigns a thread per ROW and walks 8 queries per launch: 4 workgroups for 1000 rows (measured 119 us per
    // 8 queries, i.e. launch- and latency-bound).
    if (n <= 8192 && nq >= 32) {
        constexpr uint64_t QCH = 4096;  // queries per round: QCH x ld pair keys twice
        const uint64_t qch = std::min<uint64_t>(nq, QCH);
        ws.keys_a.reserve(qch * ld * sizeof(uint64_t));
        ws.keys_b.reserve(qch * ld * sizeof(uint64_t));
        ws.keys_c.reserve(qch * cap * sizeof(uint64_t));
        for (uint64_t q0 = 0; q0 < nq; q0 += qch) {
            const uint32_t nb = (uint32_t)std::min<uint64_t>(qch, nq - q0);
            launch_iota_keys(ws.keys_a.as<uint64_t>(), nb, (uint32_t)n, (uint32_t)ld, s);
            prof_begin(ws, "flat_exact", double(n) * dim * sizeof(float));
            rerank_rows((uint32_t)dim, d_q + q0 * dim, nb, metric, d_sq.as<float>(),
                          d_qsq ? d_qsq + q0 : nullptr, ws.keys_a.as<uint64_t>(), ws.keys_b.as<uint64_t>(), (uint32_t)n,
                          (uint32_t)ld, s);
            prof_end(ws);
            launch_topk_merge(ws.keys_b.as<uint64_t>(), 1, (uint32_t)ld, nb, ksel, ws.keys_c.as<uint64_t>(), s);
            launch_finalize(ws.keys_c.as<uint64_t>(), cap, nb, ksel, (uint32_t)k, id_offset, d_idx + q0 * k, d_dist + q0 * k,
                            d_cnt + q0, s);
        }
        return;
    }
    const bool use_lds = n >= 4096;
    for (uint64_t q0 = 0; q0 < nq; q0 += BQ) {
        uint32_t nb = (uint32_t)std::min<uint64_t>(BQ, nq - q0);
        prof_begin(ws, "flat_exact", double(n) * dim * sizeof(float));
        scan_rows(n, (uint32_t)dim, d_q + q0 * dim, nb, metric, d_sq.as<float>(),
                          d_qsq ? d_qsq + q0 : nullptr, ws.dense.as<float>(), ld, use_lds, s);
        prof_end(ws);
        launch_topk_dense(ws.dense.as<float>(), ld, n, nb, ksel, ws.lists.as<uint64_t>(), s);
        launch_topk_merge(ws.lists.as<uint64_t>(), nl, cap, nb, ksel, ws.keys_c.as<uint64_t>(), s);
        launch_finalize(ws.keys_c.as<uint64_t>(), cap, nb, ksel, (uint32_t)k, id_offset, d_idx + q0 * k, d_dist + q0 * k,
                        d_cnt + q0, s);
    }
}

// ---- Flat, k > 1024: exact distances of every row, full sort of the (distance, index) pairs -------------------
void Index::flat_sorted_device(Workspace &ws, const float *d_q, uint64_t nq, uint64_t ksel, uint64_t k, uint64_t *d_idx,
                               float *d_dist, uint64_t *d_cnt) {
    hipStream_t s = ws.stream;
    VDB_REQUIRE(k < (1ull << 31), "flat knn: k too large");
    const int metric = dist == 0 ? MET_L2_DIRECT : MET_COSINE;
    const uint64_t ld = (n + 63) & ~63ull;
    constexpr uint32_t BQ = 8;
    size_t tb = sort_pairs_temp_bytes(n);
    ws.qsq.reserve(nq * sizeof(float));
    launch_row_sqnorm(d_q, nq, (uint32_t)dim, ws.qsq.as<float>(), s);
    ws.dense.reserve(size_t(BQ) * ld * sizeof(float));
    ws.keys_a.reserve(n * sizeof(uint64_t));
    ws.keys_b.reserve(n * sizeof(uint64_t));
    ws.lists.reserve(tb + 256);
    if (k > ksel) {
        VDB_HIP(hipMemsetAsync(d_idx, 0, nq * k * sizeof(uint64_t), s));
        VDB_HIP(hipMemsetAsync(d_dist, 0, nq * k * sizeof(float), s));
    }
    for (uint64_t q0 = 0; q0 < nq; q0 += BQ) {
        uint32_t nb = (uint32_t)std::min<uint64_t>(BQ, nq - q0);
        scan_rows(n, (uint32_t)dim, d_q + q0 * dim, nb, metric, d_sq.as<float>(),
                          ws.qsq.as<float>() + q0, ws.dense.as<float>(), ld, n >= 4096, s);
        for (uint32_t b = 0; b < nb; b++) {
            launch_sort_pairs(ws.dense.as<float>() + b * ld, n, ws.keys_a.as<uint64_t>(), ws.keys_b.as<uint64_t>(),
                              ws.lists.p, tb, s);
            launch_finalize(ws.keys_b.as<uint64_t>(), (uint32_t)n, 1, (uint32_t)ksel, (uint32_t)k, id_offset,
                            d_idx + (q0 + b) * k, d_dist + (q0 + b) * k, d_cnt + q0 + b, s);
        }
    }
}

// ---- Flat: small table, few queries -> one launch (k_small.hip) ------------------------------------------------------------
bool Index::flat_small_applies(uint64_t nq, uint64_t k) const {
    if (flat_small_mode == 1 || elem_u8 || n == 0 || !flat_small_supported(n, (uint32_t)dim, nq, k)) return false;
    if (flat_small_mode == 2) return true;
    if (flat_mode != 0) return false;
    if (n <= flat_small_max_rows) return nq < 32;  // below the MFMA shortlist's domain the alternative is the five-launch scan
    // Beyond it the one-launch kernel competes with the MFMA pipeline, whose cost is a fixed ~100 us of dependent launches plus
    // ~0.3 us per 1000 rows, while this kernel re-reads the rows per query: ~25 us + ~0.9 us per 1000 (row, query) pairs
    // (tools/probe_small_vs_mfma.py: one query wins up to ~125k rows of 960 columns, four queries up to ~23k).  Rows of other
    // widths scale both sides alike.
    return mfma_supported((uint32_t)dim) ? double(n) * (0.9 * double(nq) - 0.3) < 75000.0 : nq < 32 && n <= (1u << 17);
}
void Index::flat_small_device(Workspace &ws, const float *q, uint64_t nq, uint64_t k, uint64_t *o_idx, float *o_dist, uint64_t *o_cnt) {
    hipStream_t s = ws.stream;
    const uint32_t ksel = (uint32_t)std::min<uint64_t>(k, n);
    ws.small_part.reserve(flat_small_part_keys(n, nq, ksel, num_cu) * sizeof(uint64_t));
    if (ws.small_cnt.cap < 64 * sizeof(uint32_t)) {
        ws.small_cnt.reserve(64 * sizeof(uint32_t));
        VDB_HIP(hipMemsetAsync(ws.small_cnt.p, 0, 64 * sizeof(uint32_t), s));  // the kernel leaves them zero
    }
    FlatSmallArgs a{};
    a.X = d_rows.as<float>();
    a.n = n;
    a.dim = (uint32_t)dim;
    a.Q = q;
    a.metric = dist == 0 ? MET_L2_DIRECT : MET_COSINE;
    a.xsq = d_sq.as<float>();
    a.part = ws.small_part.as<uint64_t>();
    a.counter = ws.small_cnt.as<uint32_t>();
    a.ksel = ksel;
    a.kstride = (uint32_t)k;
    a.id_offset = id_offset;
    a.out_idx = o_idx;
    a.out_dist = o_dist;
    a.out_count = o_cnt;
    prof_begin(ws, "flat_small", double(nq) * double(n) * dim * sizeof(float));
    launch_flat_small(a, (uint32_t)nq, num_cu, s);
    prof_end(ws);
}

// ---- Flat: the pieces of a filter pass that k-NN, range search, filtered search and flat_debug_keys share ------------------------------
constexpr uint64_t QCH = 1024;  // queries per round of the range / filtered 8-bit tiers (8 groups of 128: 64 MB of hit lists; range: 64 MB of exact keys)

// Calls in flight on other workspaces (re-entrant readers, vdb_flat_knn_device_begin): their corpus passes take turns.
// Each pass wants every CU (one persistent workgroup per CU); two of them resident at once only wait for each other's
// workgroups, and their HIP-event durations would measure that wait.  The small kernels around the passes still overlap.
template <class F>
void Index::corpus_pass(Workspace &ws, const char *name, double bytes, F launch) {
    {
        std::lock_guard<std::mutex> g(pass_mu);
        if (pass_ev_valid) VDB_HIP(hipStreamWaitEvent(ws.stream, pass_ev, 0));
    }
    prof_begin(ws, name, bytes);
    launch();
    prof_end(ws);
    std::lock_guard<std::mutex> g(pass_mu);
    if (!pass_ev) VDB_HIP(hipEventCreateWithFlags(&pass_ev, hipEventDisableTiming));
    VDB_HIP(hipEventRecord(pass_ev, ws.stream));
    pass_ev_valid = true;
}

// The query side of an 8-bit pass over the nb queries at Q.  What k_query_prep_i8 and k_flat_gemm8 ask of these buffers: ws.misc holds
// tau | hit counters | rendezvous words in ONE allocation -- the prep kernel zeroes the nq_pad counters and the 128 words behind them, which
// the filter's cooperative sets meet on; qsq is written for q < nb only; the padding queries [nb, nq_pad) get a zero image and scale 0 (their
// tau = -inf comes from the threshold step).  Sizes are the largest any caller ever asked for (reserve never shrinks).
I8Queries Index::i8_query_prep(Workspace &ws, const float *Q, uint64_t nb) {
    I8Queries qp;
    const uint64_t gq = gemm_group();
    qp.ngroups = (nb + gq - 1) / gq;
    qp.nq_pad = qp.ngroups * gq;
    const size_t sync_words = std::max<size_t>(128, mfma_sync_words(uint32_t(qp.nq_pad / mfma_batch((uint32_t)dim)), num_cu));
    ws.qsq.reserve(qp.nq_pad * sizeof(float));
    ws.qfrag_g.reserve(qp.nq_pad * size_t(mfma_dim_pad((uint32_t)dim)) * sizeof(float));
    ws.qaux.reserve(3 * qp.nq_pad * sizeof(float));
    ws.misc.reserve(qp.nq_pad * (sizeof(float) + sizeof(uint32_t)) + sync_words * sizeof(uint32_t));
    qp.d_tau = ws.misc.as<float>();
    qp.d_hits = reinterpret_cast<uint32_t *>(qp.d_tau + qp.nq_pad);
    qp.d_qscale = ws.qaux.as<float>();
    qp.d_qoff = qp.d_qscale + qp.nq_pad;
    launch_query_prep_i8(Q, (uint32_t)nb, (uint32_t)qp.nq_pad, (uint32_t)dim, d_mu_i8.as<float>(), i8_l1, i8_l2, ws.qsq.as<float>(), qp.d_qscale,
                         qp.d_qoff, qp.d_hits, ws.qfrag_g.p, ws.stream, dist == 1 ? 1 : 0);
    return qp;
}

// The threshold sample of the 8-bit pass: planned for 64 guaranteed hits, flat_i8_hits (~1000) expected -- the exact stage takes tau itself
// as the bound of everything outside the hit list, so a list shorter than flat_i8_kprime is no failure.  With many sampled units the sample
// kernel hands the selection ONE value per (query, unit), the unit's smallest key: 48 x fewer values to write and select from (1M rows:
// 31 MB -> 0.65 MB per 1000 queries; k_gemm8.hip).
TauSample Index::i8_sample_plan() const {
    TauSample sp;
    sp.s_rank = 64;
    mfma_sample_plan(n, 64u, &sp.s_step, &sp.s_rank, flat_i8_hits);
    const uint64_t units = gemm8_sample_units(n, sp.s_step);
    sp.unit_min = flat_i8_unit_min != 1 && units >= (flat_i8_unit_min == 2 ? 2ull : 16ull) * sp.s_rank;  // (2: tests force it on short samples)
    sp.set_keys(sp.unit_min ? units : gemm8_sample_rows(n, sp.s_step));
    return sp;
}

void Index::i8_sample(Workspace &ws, const I8Queries &qp, const float *rowc, const TauSample &sp) {
    launch_flat_gemm8_sample(d_tiled_i8.p, n, (uint32_t)dim, ws.qfrag_g.p, qp.d_qscale, (uint32_t)qp.ngroups, rowc, sp.s_step, ws.dense.as<float>(),
                             sp.ld_s, num_cu, ws.stream, sp.unit_min ? 1 : 0);
}

// tau[q] = the s_rank-th smallest of the sample keys in ws.dense (scratch beyond select_tau_max_n() keys: ws.lists, ws.keys_a)
void Index::select_tau(Workspace &ws, const TauSample &sp, uint64_t nq_pad, uint64_t nq, float *d_tau) {
    hipStream_t s = ws.stream;
    if (sp.n_s <= select_tau_max_n()) {  // tau only needs the s_rank-th smallest sampled key, not a sorted sample shortlist
        launch_select_tau(ws.dense.as<float>(), sp.ld_s, (uint32_t)sp.n_s, (uint32_t)nq_pad, (uint32_t)nq, sp.s_rank, d_tau, s);
        return;
    }
    // (lists of topk_capacity(s_rank) slots -- NOT of k' slots: a thinned sample's rank is below k', and so is the 8-bit pass's)
    launch_topk_dense(ws.dense.as<float>(), sp.ld_s, sp.n_s, (uint32_t)nq_pad, sp.s_rank, ws.lists.as<uint64_t>(), s);
    launch_topk_merge(ws.lists.as<uint64_t>(), sp.nl_s, sp.cap_s, (uint32_t)nq_pad, sp.s_rank, ws.keys_a.as<uint64_t>(), s);
    launch_extract_tau(ws.keys_a.as<uint64_t>(), sp.cap_s, (uint32_t)nq_pad, sp.s_rank, d_tau, s);
    // padding queries are zero vectors: under Cosine every row ties at key 0 = tau and would flood the hit buffers of
    // the real queries that share their workgroup batch; tau = -inf lets nothing through  (k_select_tau does it itself)
    if (nq_pad > nq) VDB_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_tau + nq), (int)0xFF800000u, nq_pad - nq, s));
}

// one corpus pass of k_flat_gemm8 per 128 queries: hits (key <= tau, keys by `rowc`) -> ws.lists, FLAT_CAND_CAP slots per query
// (hits_expected per query sizes the hand-over blocks)
void Index::i8_filter(Workspace &ws, const I8Queries &qp, const float *rowc, const char *name, uint32_t hits_expected) {
    corpus_pass(ws, name, double(qp.ngroups) * double(n) * dim, [&] {
        launch_flat_gemm8_filter(d_tiled_i8.p, n, (uint32_t)dim, ws.qfrag_g.p, qp.d_qscale, (uint32_t)qp.ngroups, rowc, qp.d_tau, ws.lists.as<uint64_t>(),
                                 qp.d_hits, FLAT_CAND_CAP, flat_gemm_debug, num_cu, ws.stream, hits_expected);
    });
}

// the exact stage's arguments that come from the index and the filter pass (hit lists in ws.lists); Q, the outputs, kprime / ksel / kstride,
// flags and qstat are the caller's
FlatTailArgs Index::flat_tail_args(const Workspace &ws, const uint32_t *d_hits, const float *d_tau, const SplitErr &se) const {
    FlatTailArgs t{};
    t.cand = ws.lists.as<uint64_t>();
    t.cap = FLAT_CAND_CAP;
    t.cnt = d_hits;
    t.X = d_rows.as<float>();
    t.dim = (uint32_t)dim;
    t.cosine = dist == 1 ? 1 : 0;
    t.metric = t.cosine ? MET_COSINE : MET_L2_DIRECT;
    t.xsq = d_sq.as<float>();
    t.qsq = ws.qsq.as<float>();
    t.n_rows = n;
    t.xsq_max = xsq_max;
    t.xsq_min_pos = xsq_min_pos;
    t.se = se;
    t.id_offset = id_offset;
    t.tau = d_tau;
    return t;
}

bool Index::i8_side_tier(Workspace &ws) {
    return flat_mode != 1 && (flat_mode == 2 || n >= 16384) && flat_gemm_mode != 1 && i8_mirror_applicable() && ensure_i8(ws);
}

// Queries a tier leaves open: gathered into buffers of their own, answered elsewhere into ri / rd / rc, scattered back.  Rare: allocated on
// demand.  `rows` is pageable host memory: the caller keeps it alive until a stream sync after the constructor.
struct RedoSet {
    const uint64_t nr, k;
    DevBuf rx, rq, ri, rd, rc;
    RedoSet(const std::vector<uint64_t> &rows, const float *d_q, uint64_t dim, uint64_t k_, hipStream_t s) : nr(rows.size()), k(k_) {
        rx.reserve(nr * sizeof(uint64_t));
        rq.reserve(nr * dim * sizeof(float));
        ri.reserve(nr * k * sizeof(uint64_t));
        rd.reserve(nr * k * sizeof(float));
        rc.reserve(nr * sizeof(uint64_t));
        VDB_HIP(hipMemcpyAsync(rx.p, rows.data(), nr * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        launch_gather_rows_f32(d_q, rx.as<uint64_t>(), nr, (uint32_t)dim, rq.as<float>(), s);
        VDB_HIP(hipMemsetAsync(ri.p, 0, nr * k * sizeof(uint64_t), s));
        VDB_HIP(hipMemsetAsync(rd.p, 0, nr * k * sizeof(float), s));
    }
    void scatter(uint64_t *d_idx, float *d_dist, uint64_t *d_cnt, hipStream_t s) {
        launch_scatter_results(ri.as<uint64_t>(), rd.as<float>(), rc.as<uint64_t>(), rx.as<uint64_t>(), nr, (uint32_t)k, d_idx, d_dist, d_cnt, s);
        VDB_SYNC(s);  // (the buffers are freed with the set)
    }
};

// ---- Flat: full pipeline ---------------------------------------------------------------------------
uint64_t Index::flat_knn_device(Workspace &ws, const float *d_q, uint64_t nq, uint64_t k, uint64_t *d_idx,
                                float *d_dist, uint64_t *d_cnt, bool allow_half, uint32_t kprime_min, bool allow_i8, const float *d_dk_hint) {
    FlatPending p;
    flat_knn_enqueue(ws, d_q, nq, k, d_idx, d_dist, d_cnt, allow_half, kprime_min, p, allow_i8, d_dk_hint);
    return flat_knn_finish(ws, p);
}

// Everything of a Flat call up to (not including) the host's look at the certification flags.  p.active on return: the MFMA
// pipeline is enqueued on ws.stream and flat_knn_finish must follow (same workspace); otherwise the call took one of the
// synchronous-by-nature paths (small table, exact scan, k > 1024) and is enqueued in full -- nothing left but the stream sync.
void Index::flat_knn_enqueue(Workspace &ws, const float *d_q, uint64_t nq, uint64_t k, uint64_t *d_idx, float *d_dist,
                             uint64_t *d_cnt, bool allow_half, uint32_t kprime_min, FlatPending &p, bool allow_i8, const float *d_dk_hint) {
    hipStream_t s = ws.stream;
    p = FlatPending{};
    if (nq == 0) return;
    if (k == 0 || n == 0) {  // ResultSet::new(0) rejects everything; empty VecSet -> empty result
        VDB_HIP(hipMemsetAsync(d_cnt, 0, nq * sizeof(uint64_t), s));
        return;
    }
    if (flat_small_applies(nq, k)) {
        flat_small_device(ws, d_q, nq, k, d_idx, d_dist, d_cnt);
        return;
    }
    const uint64_t ksel64 = std::min<uint64_t>(k, n);
    if (ksel64 > 1024) {  // beyond the register-resident select: exact scan + full radix sort per query
        flat_sorted_device(ws, d_q, nq, ksel64, k, d_idx, d_dist, d_cnt);
        return;
    }
    const uint32_t ksel = (uint32_t)ksel64;
    if (k > ksel) {  // slots beyond min(k, len) are defined (zero) but not counted
        VDB_HIP(hipMemsetAsync(d_idx, 0, nq * k * sizeof(uint64_t), s));
        VDB_HIP(hipMemsetAsync(d_dist, 0, nq * k * sizeof(float), s));
    }
    ws.qsq.reserve(nq * sizeof(float));

    uint32_t kprime = std::max<uint32_t>(32, 2 * ksel);
    // a redo of queries the fp16 pass could not certify keeps that pass's (longer) shortlist: tiny margins -- clusters of
    // near-duplicates -- need rows, not precision, and the split-bf16 tier should never certify less than the tier before it
    if (kprime_min > kprime && kprime_min <= 1024 && n > kprime_min) kprime = kprime_min;
    const int cosine = dist == 1 ? 1 : 0;
    bool mfma = mfma_supported((uint32_t)dim) && kprime <= 1024 && n > kprime &&
                (flat_mode == 2 || (flat_mode == 0 && n >= 16384));
    if (flat_mode == 1) mfma = false;
    if (!mfma) {
        launch_row_sqnorm(d_q, nq, (uint32_t)dim, ws.qsq.as<float>(), s);
        flat_exact_device(ws, d_q, ws.qsq.as<float>(), nq, ksel, k, d_idx, d_dist, d_cnt);
        return;
    }

    // --- MFMA shortlist -> exact re-rank -> certification --------------------------------------
    // phase 1: keys of a strided row sample for every query -> tau[q] = r-th smallest sampled key, an upper bound of
    //          the r-th smallest key over all rows (the sample is a subset of the rows; mfma_sample_plan picks r)
    // phase 2: one corpus pass per 128 queries (k_flat_gemm; calls of at most 64 queries without an fp16 mirror: per
    //          2 x 32 queries, k_flat_mfma) that parks only the keys <= tau[q] (expected ~r * step ~ 1000 hits)
    // phase 3: shortlist = k' smallest parked pairs per query -> exact re-rank -> top-k -> certification
    const uint64_t bq = mfma_batch((uint32_t)dim);  // queries per workgroup batch (32, or 16 for 1024 < dim <= 2048)
    // First pass with fp16 operands (k_half.hip): half the HBM bytes and a third of the matrix work per row, coarser
    // keys -> a longer shortlist and a wider certification margin; what it cannot certify is redone below with the
    // split-bf16 operands.  Switched off (auto mode) once more than 1/8 of the queries had to be redone.  When it is
    // available it also serves small calls (one 128-query group, mostly padding: the pass is HBM-bound and reads half
    // the bytes of the small-batch kernel's -- 0.36 instead of 0.63 ms per pass at 1M x 960).
    const uint32_t kprime_h = std::max<uint32_t>(64, flat_half_kmul * ksel);
    const uint64_t hq = half_queries.load(), hr = half_redo.load();
    // First pass on the centred 8-bit mirror (k_gemm8.hip): half the bytes of the fp16 pass again; its keys are lower
    // bounds of the distances, its exact stage walks the hit list until the k-th distance is below the next bound
    // (k_flat_tail_lb).  What it cannot close in flat_i8_kprime rows goes through this function again (fp16 pass next).
    // Every tier falls through to the next when its mirror cannot be allocated (ensure_*: false).
    const bool i8_first = allow_i8 && allow_half && kprime_min == 0 && flat_gemm_mode != 1 && (d_dk_hint ? i8_m.valid.load() : i8_applicable(ksel));
    const bool i8 = i8_first && ensure_i8(ws);
    const bool half_wanted = !i8 && allow_half && flat_half_mode != 1 && kprime_h <= 1024 && n > kprime_h &&
                             (flat_half_mode == 2 || hq < 1024 || hr * 8 <= hq);
    const bool half_ok = half_wanted && ensure_half(ws);
    const bool gemm = i8 || flat_gemm_mode == 2 || (flat_gemm_mode == 0 && (nq > 64 || half_ok));
    const bool half = !i8 && half_ok && gemm;
    if (half) kprime = kprime_h;
    const bool i8_second = i8 && d_dk_hint != nullptr;
    if (i8) kprime = i8_second ? FLAT_CAND_CAP : flat_i8_kprime;  // (second attempt: the exact stage may walk the whole candidate list)
    if (!half && !i8) launch_row_sqnorm(d_q, nq, (uint32_t)dim, ws.qsq.as<float>(), s);  // (the fp16 / 8-bit passes: k_query_prep_*)
    if (!half && !i8 && !ensure_tiled(ws)) {  // no mirror at all: the strict-order scan over the rows themselves
        flat_exact_device(ws, d_q, ws.qsq.as<float>(), nq, ksel, k, d_idx, d_dist, d_cnt);
        return;
    }
    const uint32_t capp = topk_capacity(i8 ? 64u : kprime);  // (8-bit pass: only its sample's lists -- rank <= 64 -- use these buffers)
    const uint32_t capk = topk_capacity(ksel);
    const uint64_t gq = gemm_group();
    const uint64_t ngroups = gemm ? (nq + gq - 1) / gq : 0;
    const uint64_t nq_pad = gemm ? ngroups * gq : (nq + bq - 1) / bq * bq;
    const uint64_t nbatch = nq_pad / bq;
    // threshold sample: every s_step-th item, tau = s_rank-th smallest sampled key
    TauSample sp;
    if (i8) {
        sp = i8_sample_plan();
    } else {
        sp.s_rank = kprime;
        mfma_sample_plan(n, kprime, &sp.s_step, &sp.s_rank);
        sp.set_keys(gemm ? gemm_sample_rows(n, sp.s_step) : mfma_sample_rows(n, sp.s_step));
    }
    const size_t qf = mfma_qfrag_floats((uint32_t)dim);
    ws.qfrag.reserve(nbatch * qf * sizeof(float));
    ws.dense.reserve(nq_pad * sp.ld_s * sizeof(float));
    ws.lists.reserve(std::max<size_t>(nq_pad * sp.nl_s * capp, nq_pad * size_t(FLAT_CAND_CAP)) * sizeof(uint64_t));
    ws.keys_a.reserve(nq_pad * capp * sizeof(uint64_t));  // approximate shortlist, sorted
    ws.keys_b.reserve(nq_pad * capp * sizeof(uint64_t));  // exact keys of the shortlist, unsorted
    ws.keys_c.reserve(nq_pad * capk * sizeof(uint64_t));  // exact top-k, sorted
    const size_t sync_words = mfma_sync_words((uint32_t)nbatch, num_cu);
    I8Queries qp;  // (of the 8-bit pass; the other passes fill in the thresholds and counters they share with it)
    if (i8) {
        qp = i8_query_prep(ws, d_q, nq);
    } else {
        ws.misc.reserve(nq_pad * (sizeof(float) + sizeof(uint32_t)) + sync_words * sizeof(uint32_t));  // tau | hit counters | rendezvous
        qp.d_tau = ws.misc.as<float>();
        qp.d_hits = reinterpret_cast<uint32_t *>(qp.d_tau + nq_pad);
    }
    float *const d_tau = qp.d_tau;
    uint32_t *const d_hits = qp.d_hits;
    if (!gemm) launch_mfma_pack_queries(d_q, (uint32_t)nq, (uint32_t)nq_pad, (uint32_t)dim, ws.qfrag.as<float>(), s);
    const float *xt = half ? d_tiled_h.as<float>() : d_tiled.as<float>();
    float *d_qmul = nullptr, *d_qerr = nullptr;
    if (gemm && !i8) {
        ws.qfrag_g.reserve(nq_pad * size_t(mfma_dim_pad((uint32_t)dim)) * sizeof(float));
        if (half) {
            ws.qaux.reserve(3 * nq_pad * sizeof(float));
            float *d_qscale = ws.qaux.as<float>();
            d_qmul = d_qscale + nq_pad;
            d_qerr = d_qmul + nq_pad;
            launch_query_prep_h(d_q, (uint32_t)nq, (uint32_t)nq_pad, (uint32_t)dim, half_sx(), ws.qsq.as<float>(), d_qscale, d_qmul,
                                d_qerr, d_hits, ws.qfrag_g.p, s);  // norms, scales, rounding errors AND the packed fp16 image
        } else {
            launch_mfma_pack_queries_nh(d_q, (uint32_t)nq, (uint32_t)nq_pad, (uint32_t)dim, 8, ws.qfrag_g.as<float>(), s);
        }
    }
    if (i8_second) {
        // thresholds from the k-th exact distances the first walk left behind (k_redo.hip): no sample, no selection
        launch_i8_tau_from_dk(d_dk_hint, (uint32_t)nq, (uint32_t)nq_pad, qp.d_qoff, ws.qsq.as<float>(), xsq_max, i8_mu_norm, (uint32_t)dim, cosine,
                              d_tau, s);
    } else {
        if (i8)
            i8_sample(ws, qp, d_rowc_i8.as<float>(), sp);
        else if (gemm)  // the sample through the 128-query kernel too: same arithmetic as the filter, 4x fewer re-reads of the sample
            launch_flat_gemm_sample(xt, n, (uint32_t)dim, ws.qfrag_g.as<float>(), d_qmul, (uint32_t)ngroups,
                                    d_sq.as<float>(), cosine, sp.s_step, ws.dense.as<float>(), sp.ld_s, num_cu, s);
        else
            launch_flat_mfma_sample(d_tiled.as<float>(), n, (uint32_t)dim, ws.qfrag.as<float>(), (uint32_t)nbatch,
                                    d_sq.as<float>(), cosine, sp.s_step, ws.dense.as<float>(), sp.ld_s, num_cu, s);
        select_tau(ws, sp, nq_pad, nq, d_tau);
    }
    uint64_t *d_cand = ws.lists.as<uint64_t>();  // the sample lists are dead now
    if (i8) {
        // (expected hits per query: sizes the hand-over blocks)
        i8_filter(ws, qp, d_rowc_i8.as<float>(), "flat_i8", i8_second ? FLAT_CAND_CAP : std::max<uint32_t>(64u, sp.s_step * sp.s_rank));
    } else {
        if (!half) VDB_HIP(hipMemsetAsync(d_hits, 0, (nq_pad + sync_words) * sizeof(uint32_t), s));  // (k_query_prep_h zeroes the counters)
        // algorithmic bytes: one corpus pass (N*d*4) serves 32*share queries (bytes/query = N*d*4 / B)
        // (the fp16 pass streams N*d*2 bytes per 128 queries: its own counter, so that GB/s are the bytes really read)
        const uint64_t hbm_passes = gemm ? ngroups : (nbatch + mfma_share() - 1) / mfma_share();
        corpus_pass(ws, half ? "flat_half" : "flat_mfma", double(hbm_passes) * double(n) * dim * (half ? sizeof(uint16_t) : sizeof(float)), [&] {
            if (gemm)
                launch_flat_gemm_filter(xt, n, (uint32_t)dim, ws.qfrag_g.as<float>(), d_qmul, (uint32_t)ngroups,
                                        d_sq.as<float>(), cosine, d_tau, d_cand, d_hits, FLAT_CAND_CAP, flat_gemm_debug, num_cu, s);
            else
                launch_flat_mfma_filter(d_tiled.as<float>(), n, (uint32_t)dim, ws.qfrag.as<float>(), (uint32_t)nbatch,
                                        d_sq.as<float>(), cosine, d_tau, d_cand, d_hits, FLAT_CAND_CAP, d_hits + nq_pad, num_cu, s);
        });
    }
    SplitErr se;
    if (half) {
        se.qerr = d_qerr;
        se.dx_abs = half_dx_abs;
        se.dx_rel = half_dx_rel;
    }
    if (i8) {
        se.qoff = qp.d_qoff;
        se.mu_norm = i8_mu_norm;
    }
    if (i8 || (flat_tail_mode != 1 && !elem_u8 && flat_tail64_supported((uint32_t)dim, kprime, ksel))) {
        FlatTailArgs t = flat_tail_args(ws, d_hits, d_tau, se);
        t.kprime = kprime;
        t.ksel = ksel;
        t.kstride = (uint32_t)k;
        t.Q = d_q;
        // long walks (tight clusters): the keys of the hits are tightened from the row-major fp16 image first (k_redo.hip).  (Building the image
        // leaves the pinned block alone, and the flags block taken below stays valid until this workspace's next, larger pinned() call.)
        bool refine = false;
        if (i8 && !i8_second && nq >= 64 && flat_i8_refine != 1) {
            bool on = flat_i8_refine == 2;
            if (flat_i8_refine == 0 && i8_refine_on.load() != 0) on = (i8_refine_calls.fetch_add(1) % 32u) != 31u;  // (the 32nd: a probe without)
            refine = on && ensure_rows_h(ws);
        }
        // (flags, then -- measurement builds of a call, flat_i8_stats -- one word per query of exact-stage statistics)
        const size_t st_off = (nq + 15) & ~size_t(15);
        const bool want_stats = i8 && flat_i8_stats;
        t.flags = static_cast<uint8_t *>(ws.pinned(want_stats ? st_off + nq * sizeof(uint32_t) : nq));
        if (want_stats) t.qstat = reinterpret_cast<uint32_t *>(t.flags + st_off);
        p.stats = want_stats;
        p.refined = refine;
        if (refine) {
            launch_flat_refine_half(d_rows_h.as<uint16_t>(), (uint32_t)dim, half_sx(), half_dx_abs, half_dx_rel, cosine, d_q, d_sq.as<float>(),
                                    ws.qsq.as<float>(), qp.d_qoff, d_cand, FLAT_CAND_CAP, d_hits, (uint32_t)nq, FLAT_CAND_CAP, s);  // (a list holds up to FLAT_CAND_CAP hits; the walk selects among all of them)
            i8_refine_queries += nq;
        }
        t.out_idx = d_idx;
        t.out_dist = d_dist;
        t.out_count = d_cnt;
        if (i8 && i8_second && nq <= 96 && flat_i8_full != 1) {
            // a handful of queries on their second attempt: all their candidates at once instead of a chain of 63-row rounds (k_exact.hip)
            ws.keys_b.reserve(nq * size_t(FLAT_CAND_CAP) * sizeof(uint64_t));
            launch_flat_full_lb(t, (uint32_t)nq, ws.keys_b.as<uint64_t>(), ws.keys_c.as<uint64_t>(), s);
        } else if (i8)
            launch_flat_tail_lb(t, (uint32_t)nq, s);
        else
            launch_flat_tail64(t, (uint32_t)nq, s);
    } else {
        launch_topk_merge_counted(d_cand, FLAT_CAND_CAP, d_hits, (uint32_t)nq, kprime, ws.keys_a.as<uint64_t>(), s);
        rerank_rows((uint32_t)dim, d_q, (uint32_t)nq, cosine ? MET_COSINE : MET_L2_DIRECT, d_sq.as<float>(),
                      ws.qsq.as<float>(), ws.keys_a.as<uint64_t>(), ws.keys_b.as<uint64_t>(), kprime, capp, s);  // pads its rows
        launch_topk_merge(ws.keys_b.as<uint64_t>(), 1, capp, (uint32_t)nq, ksel, ws.keys_c.as<uint64_t>(), s);
        launch_flat_finish(ws.keys_c.as<uint64_t>(), capk, ws.keys_a.as<uint64_t>(), capp, (uint32_t)nq, ksel, (uint32_t)k, kprime,
                           n, ws.qsq.as<float>(), xsq_max, xsq_min_pos, cosine, (uint32_t)dim, se, d_hits, FLAT_CAND_CAP, id_offset,
                           static_cast<uint8_t *>(ws.pinned(nq)), d_idx, d_dist, d_cnt, s);
    }
    p.active = true;
    p.half = half;
    p.i8 = i8;
    p.i8_second = i8_second;
    p.kprime = kprime;
    p.ksel = ksel;
    p.nq = nq;
    p.k = k;
    p.d_q = d_q;
    p.d_idx = d_idx;
    p.d_dist = d_dist;
    p.d_cnt = d_cnt;
}

// the host's half of a Flat call: wait for the stream, read the certification flags, redo what was not certified
uint64_t Index::flat_knn_finish(Workspace &ws, FlatPending &p) {
    hipStream_t s = ws.stream;
    if (!p.active) return 0;
    p.active = false;
    const uint64_t nq = p.nq, k = p.k;
    // the flags go straight to pinned host memory (device-visible): no copy kernel between the last kernel and the sync
    const uint8_t *flags = static_cast<const uint8_t *>(ws.pinned(nq));
    VDB_SYNC(s);
    // uncertified queries: gather them, redo them (8-bit pass: once more with thresholds from the k-th distances the first walk found,
    // then the fp16 pass; fp16 pass: through this function again with the split-bf16 operands; split-bf16 pass: 8 per corpus pass with
    // the exact scan), scatter the results
    std::vector<uint64_t> redo;
    for (uint64_t q = 0; q < nq; q++)
        if (flags[q] & 1u) redo.push_back(q);  // (bits 1..7: rounds the 8-bit pass's exact stage walked)
    if (p.half) {
        half_queries += nq;
        half_redo += redo.size();
    }
    if (p.i8 && p.i8_second) {
        i8_second_queries += nq;
        i8_second_redo += redo.size();
    }
    const bool try_second = p.i8 && !p.i8_second && flat_i8_second != 1 && !redo.empty();
    if (p.i8 && !p.i8_second) {
        i8_queries += nq;
        if (!try_second) i8_redo += redo.size();  // (with a second attempt: what THAT passes on, counted below)
        if (flat_i8_refine == 0 && nq >= 64) {
            // auto rule of the fp16 refinement: it costs half the f32 bytes of every hit (~0.5 ms per 1000 queries), a round of the walk
            // ~0.1 ms per 1000 queries -- on when the walks average 6 rounds, off again when a probe call without it averages under 4
            // (the rounds come with the flags: bits 1..7)
            uint64_t rs = 0;
            for (uint64_t q = 0; q < nq; q++) rs += std::min<uint32_t>(flags[q] >> 1, 32u);
            const double mean_rounds = double(rs) / double(nq);
            if (!p.refined) {
                const int was = i8_refine_on.load();
                const int now = was ? (mean_rounds >= 4.0 ? 1 : 0) : (mean_rounds >= 6.0 ? 1 : 0);
                if (now != was) {
                    i8_refine_on = now;
                    i8_refine_calls = 0;
                }
            }
        }
        if (p.stats) {
            const uint32_t *qs = reinterpret_cast<const uint32_t *>(flags + ((nq + 15) & ~size_t(15)));
            uint64_t hs = 0, hm = 0;
            for (uint64_t q = 0; q < nq; q++) {
                const uint32_t r = qs[q] & 0xFFu, h = qs[q] >> 8;
                i8_rounds_hist[r < 8 ? r : 8] += 1;
                hs += h;
                hm = std::max<uint64_t>(hm, h);
            }
            i8_hits_sum += hs;
            i8_stat_queries += nq;
            uint64_t cur = i8_hits_max.load();
            while (hm > cur && !i8_hits_max.compare_exchange_weak(cur, hm)) {
            }
        }
    }
    if (redo.empty()) return 0;
    if (!p.half && !p.i8) fallback_count += redo.size();
    const uint64_t nr = redo.size();
    RedoSet r(redo, p.d_q, dim, k, s);
    DevBuf rqs, rdk;
    rqs.reserve(nr * sizeof(float));
    launch_gather_rows_f32(ws.qsq.as<float>(), r.rx.as<uint64_t>(), nr, 1, rqs.as<float>(), s);
    if (try_second) {
        rdk.reserve(nr * sizeof(float));
        launch_gather_dk(p.d_dist, p.d_cnt, r.rx.as<uint64_t>(), nr, (uint32_t)k, p.ksel, rdk.as<float>(), s);
    }
    VDB_SYNC(s);  // (`redo` is pageable host memory: the copy above must have read it before it goes out of scope in a nested call's unwinding)
    uint64_t *ri = r.ri.as<uint64_t>(), *rc = r.rc.as<uint64_t>();
    float *rq = r.rq.as<float>(), *rd = r.rd.as<float>();
    // the second 8-bit attempt: what it still cannot close goes to the fp16 tier from inside that call, and what it hands on is what the
    // auto rule counts (what left the 8-bit tier for good)
    if (try_second)
        i8_redo += flat_knn_device(ws, rq, nr, k, ri, rd, rc, true, 0, true, rdk.as<float>());
    else if (p.i8)  // next tier: the fp16 pass (or whatever this index has instead), with its own shortlist rules
        flat_knn_device(ws, rq, nr, k, ri, rd, rc, true, 0, false);
    else if (p.half)
        flat_knn_device(ws, rq, nr, k, ri, rd, rc, false, p.kprime);
    else
        flat_exact_device(ws, rq, rqs.as<float>(), nr, p.ksel, k, ri, rd, rc);
    r.scatter(p.d_idx, p.d_dist, p.d_cnt, s);
    return p.i8 ? nr : 0;
}

// ---- Flat: exact range search ----------------------------------------------------------------------------------------------------
// Every row with D(row, q) <= r_q, D the reference-order f32 distance of FlatIndex::knn, ascending by (distance, index): what
// `search(k, upper_bound = r)` (metadata_vec_table.rs:194-212) returns once k covers the whole set; limit > 0 = that call with k = limit.
//   8-bit tier (k_range.hip, docs/DESIGN_flat.md "Range search"): tau_q from r_q by the inversion of the certification bound, admission by
//     the bound itself, ONE filter pass, exact keys of every hit, cut at r_q + sort.  No sample, no selection, no rounds, no redo tier.
//   scan tier: the strict-order scan, 8 queries per corpus pass, for scan mode, small tables, u8 rows, dimensions the 8-bit pass does not
//     take, a mirror that cannot be allocated, and the queries the tier did not admit or whose hit list overflowed.
// The sorted pair keys of both tiers go to a pool in the order they are produced; the CSR arrays are gathered from it at the end
// (8 B per pair in the pool + 12 B per pair in the result).  Range calls neither read nor write the k-NN tiers' auto-off counters.
void Index::flat_range_device(Workspace &ws, const float *d_q, uint64_t nq, const float *d_radius, uint64_t limit, RangeResult &out,
                              const RowMask *mask) {
    if (mask) check_mask(*mask);
    out.device = device;
    out.nq = nq;
    out.lims.assign(nq + 1, 0);
    range_queries += nq;
    if (nq == 0) return;
    if (n == 0) {  // empty VecSet -> empty results
        range_scan_queries += nq;
        return;
    }
    std::vector<uint64_t> h_off(nq, 0), h_cnt(nq, 0);
    RangePool pool;
    flat_range_collect(ws, d_q, nq, d_radius, limit, mask, pool, h_off.data(), h_cnt.data(), nullptr);
    flat_range_assemble(ws, nq, pool, h_off, h_cnt, out);
}

// The first half of a range call: the sorted pair keys of every query's slice into `rp`, in the order they are produced; h_off[q] / h_cnt[q]
// (zero on entry) = where query q's slice lies in the pool and how many pairs it has.  n > 0, nq > 0; the mask has been checked; returns
// synchronised.  Several collects may share one pool (flat_range_masked_multi_device): the ceiling is the call's.  tally: what this
// collect added to the tier counters, for a caller that takes it back when the call fails later.
void Index::flat_range_collect(Workspace &ws, const float *d_q, uint64_t nq, const float *d_radius, uint64_t limit, const RowMask *mask, RangePool &rp,
                               uint64_t *h_off, uint64_t *h_cnt, RangeTally *tally) {
    hipStream_t s = ws.stream;
    constexpr uint32_t BQ = 8;  // queries per corpus pass of the scan
    const int cosine = dist == 1 ? 1 : 0;
    const int metric = cosine ? MET_COSINE : MET_L2_DIRECT;
    const uint64_t cap_pairs = range_max_results ? range_max_results : ~0ull;
    DevBuf &pool = rp.buf;
    uint64_t &pool_used = rp.used;
    // the pinned block of this call: [off u64 x QCH | cnt u32 x QCH | hits u32 x QCH | take u32 x QCH]; written by the kernels (cnt, hits) and
    // by the host between two stream syncs (off, take) -- never while a kernel that reads them is in flight
    char *hp = static_cast<char *>(ws.pinned(QCH * (sizeof(uint64_t) + 3 * sizeof(uint32_t))));
    uint64_t *p_off = reinterpret_cast<uint64_t *>(hp);
    uint32_t *p_cnt = reinterpret_cast<uint32_t *>(p_off + QCH), *p_hits = p_cnt + QCH, *p_take = p_hits + QCH;
    auto pool_room = [&](uint64_t add) { rp.room(add, cap_pairs, s); };
    std::vector<uint64_t> scan;  // queries the scan tier answers
    const bool tier = i8_side_tier(ws);
    // under a mask the filter pass reads the masked copy of the row constants: a disallowed row's key is +inf and passes no (finite) threshold
    const float *rowc = tier ? (mask ? masked_rowc(ws, *mask) : d_rowc_i8.as<float>()) : nullptr;
    if (!tier) {
        scan.resize(nq);
        for (uint64_t q = 0; q < nq; q++) scan[q] = q;
    }
    for (uint64_t q0 = 0; tier && q0 < nq; q0 += QCH) {
        const uint64_t nb = std::min<uint64_t>(QCH, nq - q0);
        const float *Q = d_q + q0 * dim, *R = d_radius + q0;
        const I8Queries qp = i8_query_prep(ws, Q, nb);
        ws.lists.reserve(qp.nq_pad * size_t(FLAT_CAND_CAP) * sizeof(uint64_t));
        ws.keys_b.reserve(nb * size_t(FLAT_CAND_CAP) * sizeof(uint64_t));
        uint64_t *d_keys = ws.keys_b.as<uint64_t>();
        launch_i8_tau_from_dk(R, (uint32_t)nb, (uint32_t)qp.nq_pad, qp.d_qoff, ws.qsq.as<float>(), xsq_max, i8_mu_norm, (uint32_t)dim, cosine, qp.d_tau, s);
        launch_range_admit(R, (uint32_t)nb, qp.d_qoff, ws.qsq.as<float>(), xsq_max, xsq_min_pos, i8_mu_norm, (uint32_t)dim, cosine, qp.d_tau, s);
        if (mask) launch_tau_clamp(qp.d_tau, (uint32_t)qp.nq_pad, s);
        i8_filter(ws, qp, rowc, "flat_range_i8", FLAT_CAND_CAP);
        prof_begin(ws, "flat_range_exact", 0.0);
        launch_rerank(d_rows.as<float>(), (uint32_t)dim, Q, (uint32_t)nb, metric, d_sq.as<float>(), ws.qsq.as<float>(), ws.lists.as<uint64_t>(), d_keys,
                      FLAT_CAND_CAP, FLAT_CAND_CAP, s, qp.d_hits);
        launch_range_cut(d_keys, FLAT_CAND_CAP, qp.d_hits, R, qp.d_tau, (uint32_t)nb, p_cnt, p_hits, s);
        prof_end(ws);
        VDB_SYNC(s);
        uint64_t add = 0, max_take = 0, hits = 0, served = 0, hmax = 0;
        for (uint64_t j = 0; j < nb; j++) {
            if (p_cnt[j] == RANGE_LEFT) {  // not admitted, or more hits than the list holds
                scan.push_back(q0 + j);
                p_take[j] = 0;
                p_off[j] = 0;
                continue;
            }
            const uint64_t t = limit ? std::min<uint64_t>(p_cnt[j], limit) : p_cnt[j];
            h_cnt[q0 + j] = t;
            h_off[q0 + j] = pool_used + add;
            p_off[j] = pool_used + add;
            p_take[j] = (uint32_t)t;
            add += t;
            max_take = std::max(max_take, t);
            hits += p_hits[j];
            hmax = std::max<uint64_t>(hmax, p_hits[j]);
            served++;
        }
        range_i8_queries += served;
        range_hits += hits;
        if (tally) tally->i8 += served, tally->hits += hits;
        for (uint64_t cur = range_hits_max.load(); hmax > cur && !range_hits_max.compare_exchange_weak(cur, hmax);) {
        }
        if (add) {
            pool_room(add);
            launch_range_append(d_keys, FLAT_CAND_CAP, p_off, p_take, (uint32_t)nb, max_take, pool.as<uint64_t>(), s);
            pool_used += add;
            VDB_SYNC(s);  // (the pinned block is rewritten by the next round)
        }
    }
    range_scan_queries += scan.size();
    if (tally) tally->scan += scan.size();
    if (!scan.empty()) {
        const uint64_t ns = scan.size(), ld = (n + 63) & ~63ull;
        const uint32_t nblk = range_scan_blocks(n);
        const bool all = ns == nq;  // (then scan[j] == j: the queries are used where they are)
        DevBuf rx, rq, rr, rqs, blk;  // (like flat_knn_finish's redo set: allocated on demand)
        rqs.reserve(BQ * sizeof(float));
        blk.reserve(size_t(BQ) * nblk * sizeof(uint32_t));
        if (!all) {
            rx.reserve(ns * sizeof(uint64_t));
            rq.reserve(size_t(BQ) * dim * sizeof(float));
            rr.reserve(BQ * sizeof(float));
            VDB_HIP(hipMemcpyAsync(rx.p, scan.data(), ns * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        }
        ws.dense.reserve(size_t(BQ) * ld * sizeof(float));
        for (uint64_t g0 = 0; g0 < ns; g0 += BQ) {
            const uint32_t nb = (uint32_t)std::min<uint64_t>(BQ, ns - g0);
            const float *Q = d_q + g0 * dim, *R = d_radius + g0;
            if (!all) {
                launch_gather_rows_f32(d_q, rx.as<uint64_t>() + g0, nb, (uint32_t)dim, rq.as<float>(), s);
                launch_gather_rows_f32(d_radius, rx.as<uint64_t>() + g0, nb, 1, rr.as<float>(), s);
                Q = rq.as<float>();
                R = rr.as<float>();
            }
            launch_row_sqnorm(Q, nb, (uint32_t)dim, rqs.as<float>(), s);
            prof_begin(ws, "flat_range_scan", double(n) * dim * elem_size());
            scan_rows(n, (uint32_t)dim, Q, nb, metric, d_sq.as<float>(), rqs.as<float>(), ws.dense.as<float>(), ld, n >= 4096, s);
            prof_end(ws);
            if (mask) launch_mask_dense_nan(ws.dense.as<float>(), ld, n, nb, mask->d_bits.as<uint64_t>(), s);  // (a NaN distance is never inside)
            launch_range_scan_select(ws.dense.as<float>(), ld, n, R, nb, blk.as<uint32_t>(), p_cnt, s);
            VDB_SYNC(s);
            uint64_t add = 0, max_tot = 0, max_take = 0;
            for (uint32_t j = 0; j < nb; j++) {
                const uint64_t q = scan[g0 + j], t = limit ? std::min<uint64_t>(p_cnt[j], limit) : p_cnt[j];
                h_cnt[q] = t;
                h_off[q] = pool_used + add;
                p_off[j] = pool_used + add;
                p_take[j] = (uint32_t)t;
                add += t;
                max_tot = std::max<uint64_t>(max_tot, p_cnt[j]);
                max_take = std::max(max_take, t);
            }
            if (add == 0) continue;
            pool_room(add);
            // survivors in row order -> one padded row of pair keys per query -> sorted rows -> the pool
            const uint64_t ldo = (max_tot + 63) & ~63ull;
            const size_t tb = sort_rows_temp_bytes(nb, ldo);
            ws.keys_a.reserve(size_t(nb) * ldo * sizeof(uint64_t));
            ws.keys_b.reserve(size_t(nb) * ldo * sizeof(uint64_t));
            ws.lists.reserve(tb);
            VDB_HIP(hipMemsetAsync(ws.keys_a.p, 0xFF, size_t(nb) * ldo * sizeof(uint64_t), s));  // PAIR_NONE pads sort last
            launch_range_compact(ws.dense.as<float>(), ld, n, R, nb, blk.as<uint32_t>(), ws.keys_a.as<uint64_t>(), ldo, s);
            launch_sort_rows(ws.keys_a.as<uint64_t>(), ws.keys_b.as<uint64_t>(), nb, ldo, ws.lists.p, tb, s);
            launch_range_append(ws.keys_b.as<uint64_t>(), ldo, p_off, p_take, nb, max_take, pool.as<uint64_t>(), s);
            pool_used += add;
            VDB_SYNC(s);  // (the pinned block is rewritten by the next pass)
        }
        VDB_SYNC(s);  // (`scan` and rx..blk go out of scope)
    }
}

void RangePool::room(uint64_t add, uint64_t cap_pairs, hipStream_t s) {
    if (add > cap_pairs || used > cap_pairs - add)
        throw Error(1, "range search: more than " + std::to_string(cap_pairs) + " results in one call (flat_range_max_results); use a limit, "
                       "smaller radii or fewer queries per call");
    buf.grow((used + add) * sizeof(uint64_t), used * sizeof(uint64_t), s);
}

// The second half: the CSR arrays of `out` (lims assigned to nq + 1 zeros by the caller) from the pool and every query's (offset, count).
void Index::flat_range_assemble(Workspace &ws, uint64_t nq, const RangePool &rp, const std::vector<uint64_t> &h_off, const std::vector<uint64_t> &h_cnt,
                                RangeResult &out) {
    hipStream_t s = ws.stream;
    const DevBuf &pool = rp.buf;
    uint64_t total = 0, max_take = 0;
    for (uint64_t q = 0; q < nq; q++) {
        out.lims[q] = total;
        total += h_cnt[q];
        max_take = std::max(max_take, h_cnt[q]);
    }
    out.lims[nq] = total;
    range_results += total;
    if (total == 0) return;
    out.idx.reserve(total * sizeof(uint64_t));
    out.dist.reserve(total * sizeof(float));
    DevBuf meta;  // [off nq | lims nq + 1]
    meta.reserve((2 * nq + 1) * sizeof(uint64_t));
    VDB_HIP(hipMemcpyAsync(meta.p, h_off.data(), nq * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    VDB_HIP(hipMemcpyAsync(meta.as<uint64_t>() + nq, out.lims.data(), (nq + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    launch_range_gather(pool.as<uint64_t>(), meta.as<uint64_t>(), meta.as<uint64_t>() + nq, nq, max_take, id_offset, out.idx.as<uint64_t>(),
                        out.dist.as<float>(), s);
    VDB_SYNC(s);
}

// ---- Flat: exact filtered search over a row allow-list (k_filter.hip) ----------------------------------------------------------------
// The first min(k, m) pairs of FlatIndex::knn over the m allowed rows of a RowMask, ascending by (distance, row id), distances bit-exact.
//   direct path: strict-order scan of the GATHERED rows (column j of the dense matrix = row ids[j], ids ascending, so the order of
//     (distance, column) IS the order of (distance, id)), the k-NN selections as they are, k_filter_finalize maps columns to rows.
//     For m <= flat_filtered_direct_max, for shapes the 8-bit tier does not take, and for the queries that tier hands on.
//   8-bit tier: the shared pieces of the 8-bit pass (above) per chunk of QCH queries, with the MASKED row constants in the sample and
//     the filter launch (a disallowed row's key is +inf) and the thresholds clamped to FLT_MAX in between, so that no threshold admits such
//     a key.  The hit list then holds allowed rows only and every allowed row outside it has key > tau: k_flat_tail_lb and its bound apply
//     unchanged.  One attempt: no refinement, no second pass, no fp16 / split-bf16 tier; what is still open goes to the direct path.
// Like the range search this call neither reads nor writes the k-NN tiers' auto-off counters (the tier's shape test is i8_applicable
// without its clause about them).
void Index::check_mask(const RowMask &mask) const {
    if (mask.owner != this) throw Error(1, "mask: made for another index");
    if (mask.gen != write_gen.load() || mask.n_rows != n)
        throw Error(3, "mask: stale -- rows were added to or removed from the index after the mask was made; make a new one");
}

const float *Index::masked_rowc(Workspace &ws, const RowMask &mask) {
    std::lock_guard<std::mutex> g(mask.mu);  // read-side calls are re-entrant: one of them builds, the others wait
    // (update_rows rewrites constants inside the same allocation: the generation tells, the pointer alone would not)
    const uint64_t gen = rowc_gen.load();
    if (mask.rowc_of == d_rowc_i8.p && mask.rowc_gen == gen && mask.d_rowc.p) return mask.d_rowc.as<float>();
    const uint64_t rows_pad = mirror_tiles(n) * 16;
    mask.d_rowc.reserve(rows_pad * 2 * sizeof(float));
    launch_mask_rowc(d_rowc_i8.as<float>(), mask.d_bits.as<uint64_t>(), n, rows_pad, mask.d_rowc.as<float>(), ws.stream);
    VDB_SYNC(ws.stream);
    mask.rowc_of = d_rowc_i8.p;
    mask.rowc_gen = gen;
    return mask.d_rowc.as<float>();
}

void Index::flat_masked_direct(Workspace &ws, const float *d_q, uint64_t nq, uint64_t k, const RowMask &mask, uint64_t *d_idx, float *d_dist,
                               uint64_t *d_cnt) {
    hipStream_t s = ws.stream;
    const uint64_t m = mask.m;
    if (nq == 0 || k == 0 || m == 0) return;
    VDB_REQUIRE(k < (1ull << 31), "flat knn: k too large");
    const int metric = dist == 0 ? MET_L2_DIRECT : MET_COSINE;
    const uint64_t ksel = std::min<uint64_t>(k, m), ld = (m + 63) & ~63ull;
    const uint32_t *ids = mask.d_ids.as<uint32_t>();
    const bool use_lds = m >= 4096;
    constexpr uint64_t BUDGET = 256ull << 20;  // bytes of the dense matrix (and of each key buffer) per chunk of queries
    auto chunk_of = [&](uint64_t row_bytes) { return std::max<uint64_t>(8, std::min<uint64_t>(BUDGET / row_bytes, 32768) & ~7ull); };
    ws.qsq.reserve(nq * sizeof(float));
    launch_row_sqnorm(d_q, nq, (uint32_t)dim, ws.qsq.as<float>(), s);
    if (ksel <= 1024) {
        const uint32_t nl = topk_num_lists(m), cap = topk_capacity((uint32_t)ksel);
        const uint64_t qch = std::min(nq, std::min(chunk_of(ld * sizeof(float)), chunk_of(uint64_t(nl) * cap * sizeof(uint64_t))));
        ws.dense.reserve(qch * ld * sizeof(float));  // (before the loop: a later, larger reserve would free a buffer in use)
        ws.lists.reserve(qch * nl * cap * sizeof(uint64_t));
        ws.keys_c.reserve(qch * cap * sizeof(uint64_t));
        for (uint64_t q0 = 0; q0 < nq; q0 += qch) {
            const uint32_t nb = (uint32_t)std::min<uint64_t>(qch, nq - q0);
            prof_begin(ws, "flat_filtered_scan", double((nb + 7) / 8) * double(m) * dim * sizeof(float));
            launch_scan_gather(d_rows.as<float>(), ids, m, (uint32_t)dim, d_q + q0 * dim, nb, metric, d_sq.as<float>(), ws.qsq.as<float>() + q0,
                               ws.dense.as<float>(), ld, use_lds, s);
            prof_end(ws);
            launch_topk_dense(ws.dense.as<float>(), ld, m, nb, (uint32_t)ksel, ws.lists.as<uint64_t>(), s);
            launch_topk_merge(ws.lists.as<uint64_t>(), nl, cap, nb, (uint32_t)ksel, ws.keys_c.as<uint64_t>(), s);
            launch_filter_finalize(ws.keys_c.as<uint64_t>(), cap, nb, (uint32_t)ksel, (uint32_t)k, ids, m, id_offset, d_idx + q0 * k, d_dist + q0 * k,
                                   d_cnt + q0, s);
        }
        return;
    }
    // beyond the register-resident select: every (distance, column) pair of a query sorted, the first ksel kept
    const uint64_t qch = std::min(nq, chunk_of(ld * sizeof(uint64_t)));
    const size_t tb = sort_rows_temp_bytes(qch, ld);
    ws.dense.reserve(qch * ld * sizeof(float));
    ws.keys_a.reserve(qch * ld * sizeof(uint64_t));
    ws.keys_b.reserve(qch * ld * sizeof(uint64_t));
    ws.keys_c.reserve(qch * ksel * sizeof(uint64_t));
    ws.lists.reserve(tb);
    for (uint64_t q0 = 0; q0 < nq; q0 += qch) {
        const uint32_t nb = (uint32_t)std::min<uint64_t>(qch, nq - q0);
        prof_begin(ws, "flat_filtered_scan", double((nb + 7) / 8) * double(m) * dim * sizeof(float));
        launch_scan_gather(d_rows.as<float>(), ids, m, (uint32_t)dim, d_q + q0 * dim, nb, metric, d_sq.as<float>(), ws.qsq.as<float>() + q0,
                           ws.dense.as<float>(), ld, use_lds, s);
        prof_end(ws);
        launch_pair_keys_rows(ws.dense.as<float>(), ld, m, nb, ws.keys_a.as<uint64_t>(), ld, s);
        launch_sort_rows(ws.keys_a.as<uint64_t>(), ws.keys_b.as<uint64_t>(), nb, ld, ws.lists.p, tb, s);
        launch_copy_prefix(ws.keys_b.as<uint64_t>(), ld, ws.keys_c.as<uint64_t>(), ksel, ksel, nb, s);
        launch_filter_finalize(ws.keys_c.as<uint64_t>(), ksel, nb, (uint32_t)ksel, (uint32_t)k, ids, m, id_offset, d_idx + q0 * k, d_dist + q0 * k,
                               d_cnt + q0, s);
    }
}

void Index::flat_knn_masked_device(Workspace &ws, const float *d_q, uint64_t nq, uint64_t k, const RowMask &mask, uint64_t *d_idx, float *d_dist,
                                   uint64_t *d_cnt) {
    hipStream_t s = ws.stream;
    check_mask(mask);
    require_f32_rows(*this);
    filtered_queries += nq;
    if (nq == 0) return;
    const uint64_t m = mask.m;
    const uint64_t ksel64 = std::min<uint64_t>(k, m);
    VDB_HIP(hipMemsetAsync(d_cnt, 0, nq * sizeof(uint64_t), s));
    if (k > ksel64) {  // slots beyond min(k, m) are defined (zero) but not counted
        VDB_HIP(hipMemsetAsync(d_idx, 0, nq * k * sizeof(uint64_t), s));
        VDB_HIP(hipMemsetAsync(d_dist, 0, nq * k * sizeof(float), s));
    }
    if (ksel64 == 0) {  // k == 0, or nothing is allowed: empty results
        filtered_direct_queries += nq;
        VDB_SYNC(s);
        return;
    }
    const bool tier = m > flat_filtered_direct_max && ksel64 <= 64 && flat_tail_lb_supported((uint32_t)dim, flat_i8_kprime, (uint32_t)ksel64) &&
                      i8_side_tier(ws);
    if (!tier) {
        filtered_direct_queries += nq;
        flat_masked_direct(ws, d_q, nq, k, mask, d_idx, d_dist, d_cnt);
        VDB_SYNC(s);
        return;
    }
    const float *rowc = masked_rowc(ws, mask);
    const TauSample sp = i8_sample_plan();
    std::vector<uint64_t> redo;  // queries the tier hands on
    for (uint64_t q0 = 0; q0 < nq; q0 += QCH) {
        const uint64_t nb = std::min<uint64_t>(QCH, nq - q0);
        const float *Q = d_q + q0 * dim;
        const I8Queries qp = i8_query_prep(ws, Q, nb);
        ws.dense.reserve(qp.nq_pad * sp.ld_s * sizeof(float));
        ws.lists.reserve(std::max<size_t>(qp.nq_pad * size_t(sp.nl_s) * sp.cap_s, qp.nq_pad * size_t(FLAT_CAND_CAP)) * sizeof(uint64_t));
        ws.keys_a.reserve(qp.nq_pad * size_t(sp.cap_s) * sizeof(uint64_t));
        // thresholds: the s_rank-th smallest sampled key among the ALLOWED rows (the others' keys are +inf) bounds the s_rank-th smallest
        // key over all allowed rows
        i8_sample(ws, qp, rowc, sp);
        select_tau(ws, sp, qp.nq_pad, nb, qp.d_tau);
        // a sample with fewer than s_rank allowed rows selects +inf, which every masked row's key would pass: with tau = FLT_MAX the query
        // collects every allowed row with a finite key instead -- certified if they fit the list, handed on if not
        launch_tau_clamp(qp.d_tau, (uint32_t)qp.nq_pad, s);
        i8_filter(ws, qp, rowc, "flat_filtered_i8", std::max<uint32_t>(64u, sp.s_step * sp.s_rank));  // (the sample lists are dead now)
        SplitErr se;
        se.qoff = qp.d_qoff;
        se.mu_norm = i8_mu_norm;
        FlatTailArgs t = flat_tail_args(ws, qp.d_hits, qp.d_tau, se);
        t.kprime = flat_i8_kprime;
        t.ksel = (uint32_t)ksel64;
        t.kstride = (uint32_t)k;
        t.Q = Q;
        t.flags = static_cast<uint8_t *>(ws.pinned(nb));
        t.out_idx = d_idx + q0 * k;
        t.out_dist = d_dist + q0 * k;
        t.out_count = d_cnt + q0;
        launch_flat_tail_lb(t, (uint32_t)nb, s);
        VDB_SYNC(s);  // (the flags are in pinned host memory)
        for (uint64_t q = 0; q < nb; q++)
            if (t.flags[q] & 1u) redo.push_back(q0 + q);
    }
    filtered_i8_queries += nq;
    filtered_fallback_queries += redo.size();
    if (redo.empty()) return;
    // the open queries over all m allowed rows on the direct path
    RedoSet r(redo, d_q, dim, k, s);
    VDB_HIP(hipMemsetAsync(r.rc.p, 0, r.nr * sizeof(uint64_t), s));
    flat_masked_direct(ws, r.rq.as<float>(), r.nr, k, mask, r.ri.as<uint64_t>(), r.rd.as<float>(), r.rc.as<uint64_t>());
    r.scatter(d_idx, d_dist, d_cnt, s);  // (its sync: before `redo` goes out of scope)
}

// ---- shared by the two searches with one row mask per query (k-NN and range, below) ------------------------------------------------------
// The rows of every mask, which masks take the grouped route (grouped_if(m)), and for every other mask the positions of its queries in
// the call: the buckets of the per-mask route.
namespace {
struct MaskRoutes {
    std::vector<uint64_t> m_of;
    std::vector<uint8_t> grouped;
    std::vector<std::vector<uint64_t>> bucket;
};
template <class Pred>
MaskRoutes mask_routes(const RowMask *const *masks, uint64_t n_masks, const uint32_t *mask_of, uint64_t nq, Pred grouped_if) {
    MaskRoutes r;
    r.m_of = std::vector<uint64_t>(n_masks);
    r.grouped = std::vector<uint8_t>(n_masks);
    r.bucket = std::vector<std::vector<uint64_t>>(n_masks);
    for (uint64_t g = 0; g < n_masks; g++) {
        r.m_of[g] = masks[g]->m;
        r.grouped[g] = grouped_if(r.m_of[g]);
    }
    for (uint64_t q = 0; q < nq; q++)
        if (!r.grouped[mask_of[q]]) r.bucket[mask_of[q]].push_back(q);
    return r;
}

// The device image of a MultiPlan in ws.misc, one reserve and one upload for the call: [slot_ids (8 B) | items (24 B) | slot_q | slot_m |
// slot_c], the 8-byte members first.  with_ids: the id list and m of every slot's mask (what the k-NN finalize reads); with_counters: a
// zeroed u32 per slot (what the range gather counts into).  The image owns the host arrays it uploads from -- pageable memory: keep it (and
// the plan, whose slot_query is uploaded as it stands) alive until the call's final stream sync.
struct PlanImage {
    const uint32_t *const *slot_ids = nullptr;
    const GroupedItem *items = nullptr;
    const uint32_t *slot_q = nullptr, *slot_m = nullptr;
    uint32_t *slot_c = nullptr;
    std::vector<GroupedItem> h_items;
    std::vector<const uint32_t *> h_ids;
    std::vector<uint32_t> h_m;
};
PlanImage plan_image(Workspace &ws, const MultiPlan &plan, const RowMask *const *masks, const std::vector<uint64_t> &m_of, bool with_ids,
                            bool with_counters) {
    hipStream_t s = ws.stream;
    PlanImage im;
    const uint64_t ns = plan.slot_query.size();
    im.h_items = std::vector<GroupedItem>(plan.items.size());
    for (size_t i = 0; i < im.h_items.size(); i++) {
        const MultiItem &it = plan.items[i];
        im.h_items[i] = GroupedItem{masks[it.mask]->d_ids.as<uint32_t>(), (uint32_t)m_of[it.mask], it.tile, it.slot, it.nb};
    }
    if (with_ids) {
        im.h_ids = std::vector<const uint32_t *>(ns);
        im.h_m = std::vector<uint32_t>(ns);
        for (uint64_t i = 0; i < ns; i++) {
            im.h_ids[i] = masks[plan.slot_mask[i]]->d_ids.as<uint32_t>();
            im.h_m[i] = (uint32_t)m_of[plan.slot_mask[i]];
        }
    }
    static_assert(sizeof(GroupedItem) % 8 == 0, "the items follow the pointer array");
    const size_t sb = ns * sizeof(uint32_t), off_items = with_ids ? ns * sizeof(uint32_t *) : 0, off_q = off_items + im.h_items.size() * sizeof(GroupedItem);
    const size_t off_m = off_q + sb, off_c = off_m + (with_ids ? sb : 0);
    ws.misc.reserve(off_c + (with_counters ? sb : 0));
    char *d = ws.misc.as<char>();
    if (!im.h_items.empty()) VDB_HIP(hipMemcpyAsync(d + off_items, im.h_items.data(), im.h_items.size() * sizeof(GroupedItem), hipMemcpyHostToDevice, s));
    VDB_HIP(hipMemcpyAsync(d + off_q, plan.slot_query.data(), sb, hipMemcpyHostToDevice, s));
    im.items = reinterpret_cast<const GroupedItem *>(d + off_items);
    im.slot_q = reinterpret_cast<const uint32_t *>(d + off_q);
    if (with_ids) {
        VDB_HIP(hipMemcpyAsync(d, im.h_ids.data(), ns * sizeof(uint32_t *), hipMemcpyHostToDevice, s));
        VDB_HIP(hipMemcpyAsync(d + off_m, im.h_m.data(), sb, hipMemcpyHostToDevice, s));
        im.slot_ids = reinterpret_cast<const uint32_t *const *>(d);
        im.slot_m = reinterpret_cast<const uint32_t *>(d + off_m);
    }
    if (with_counters) {
        VDB_HIP(hipMemsetAsync(d + off_c, 0, sb, s));
        im.slot_c = reinterpret_cast<uint32_t *>(d + off_c);
    }
    return im;
}
}  // namespace

// ---- Flat: exact filtered k-NN with one row mask per query (k_filter.hip, multi_plan.hpp) ------------------------------------------------
// Query q is answered as flat_knn_masked_device answers it alone under masks[mask_of[q]].  The queries are bucketed by mask on the host:
//   per-mask route: a bucket whose mask is longer than flat_filtered_direct_max (or any bucket when k > 1024) is gathered into a block of
//     its own, goes through flat_knn_masked_device as it stands -- the 8-bit tier with that mask's row constants, or the direct path --
//     and is scattered back (RedoSet).
//   grouped route: every other bucket.  multi_plan lays them out as slots and cuts the slots into chunks; a chunk is ONE launch of
//     k_scan_gather_grouped over all its (mask, query group, tile) work items into a dense matrix of leading dimension ld = the chunk's
//     largest m rounded up to 64, ONE selection over (ld, max m) and ONE finalize.  Padding: the matrix is filled with 0xFF bytes first,
//     so a slot's columns at and past its own m hold a NaN; pair_key canonicalises every NaN to one orderable image, the greatest
//     (common.hpp), so (NaN, column j >= m) sorts behind every real key of that slot -- a real NaN included, whose column is smaller --
//     and the real keys are a prefix of the slot's sorted row.  k_topk_dense / k_topk_merge compare whole u64 keys and treat only
//     PAIR_NONE (~0, which no column below 2^32 - 1 produces) specially; k_filter_finalize_grouped cuts at column < m.
// The caller has checked every mask and every mask_of entry.  Returns synchronised; touches no auto-off counter.
void Index::flat_knn_masked_multi_device(Workspace &ws, const float *d_q, uint64_t nq, uint64_t k, const RowMask *const *masks, uint64_t n_masks,
                                         const uint32_t *mask_of, uint64_t *d_idx, float *d_dist, uint64_t *d_cnt) {
    hipStream_t s = ws.stream;
    require_f32_rows(*this);
    if (nq == 0) return;
    VDB_REQUIRE(nq < (1ull << 32) && k < (1ull << 31), "flat knn: too many queries or k too large");
    if (k == 0) {
        filtered_queries += nq;
        filtered_direct_queries += nq;
        VDB_HIP(hipMemsetAsync(d_cnt, 0, nq * sizeof(uint64_t), s));
        VDB_SYNC(s);
        return;
    }
    const MaskRoutes rt = mask_routes(masks, n_masks, mask_of, nq, [&](uint64_t m) { return k <= 1024 && m <= flat_filtered_direct_max; });
    // per-mask route first: every such call returns synchronised, so the grouped route's reserves below free nothing in use
    for (uint64_t g = 0; g < n_masks; g++) {
        if (rt.bucket[g].empty()) continue;
        RedoSet r(rt.bucket[g], d_q, dim, k, s);
        VDB_HIP(hipMemsetAsync(r.rc.p, 0, r.nr * sizeof(uint64_t), s));
        flat_knn_masked_device(ws, r.rq.as<float>(), r.nr, k, *masks[g], r.ri.as<uint64_t>(), r.rd.as<float>(), r.rc.as<uint64_t>());
        r.scatter(d_idx, d_dist, d_cnt, s);
    }
    const uint64_t max_m = multi_plan_max_m(rt.m_of.data(), rt.grouped.data(), n_masks, mask_of, nq);
    const uint64_t ksel_all = std::min<uint64_t>(k, max_m);
    const uint64_t list_bytes = ksel_all ? uint64_t(topk_num_lists(max_m)) * topk_capacity((uint32_t)ksel_all) * sizeof(uint64_t) : 64;
    constexpr uint64_t BUDGET = 256ull << 20;  // bytes of the dense matrix (and of the selection's lists) per chunk, as in flat_masked_direct
    MultiPlan plan;
    multi_plan(rt.m_of.data(), rt.grouped.data(), n_masks, mask_of, nq, BUDGET, list_bytes, plan);
    const uint64_t ns = plan.slot_query.size();
    if (ns == 0) return;
    filtered_queries += ns;
    filtered_direct_queries += ns;
    filtered_grouped_queries += ns;
    const int metric = dist == 0 ? MET_L2_DIRECT : MET_COSINE;
    // every buffer of the call reserved before its first launch (a later, larger reserve would free a buffer in use); ws.misc: plan_image
    ws.qsq.reserve(nq * sizeof(float));
    const uint64_t ld_all = (max_m + 63) & ~63ull;
    const uint64_t qch = std::min(plan.qch, ns);
    if (ksel_all) {
        ws.dense.reserve(qch * ld_all * sizeof(float));
        ws.lists.reserve(qch * list_bytes);
        ws.keys_c.reserve(qch * topk_capacity((uint32_t)ksel_all) * sizeof(uint64_t));
    }
    const PlanImage im = plan_image(ws, plan, masks, rt.m_of, true, false);
    launch_row_sqnorm(d_q, nq, (uint32_t)dim, ws.qsq.as<float>(), s);
    for (const MultiChunk &c : plan.chunks) {
        const uint32_t nb = (uint32_t)c.nslots;
        const uint64_t ksel = std::min<uint64_t>(k, c.max_m);
        uint32_t cap = 0;
        if (ksel) {
            const uint32_t nl = topk_num_lists(c.max_m);
            cap = topk_capacity((uint32_t)ksel);
            VDB_HIP(hipMemsetAsync(ws.dense.p, 0xFF, uint64_t(nb) * c.ld * sizeof(float), s));  // padding columns: NaN, behind every real key
            prof_begin(ws, "flat_filtered_scan_grouped", double(c.rows) * dim * sizeof(float));
            launch_scan_gather_grouped(d_rows.as<float>(), (uint32_t)dim, im.items + c.item0, c.nitems, im.slot_q + c.slot0, d_q, metric, d_sq.as<float>(),
                                       ws.qsq.as<float>(), ws.dense.as<float>(), c.ld, s);
            prof_end(ws);
            launch_topk_dense(ws.dense.as<float>(), c.ld, c.max_m, nb, (uint32_t)ksel, ws.lists.as<uint64_t>(), s);
            launch_topk_merge(ws.lists.as<uint64_t>(), nl, cap, nb, (uint32_t)ksel, ws.keys_c.as<uint64_t>(), s);
        }
        launch_filter_finalize_grouped(ws.keys_c.as<uint64_t>(), cap, nb, (uint32_t)ksel, (uint32_t)k, im.slot_ids + c.slot0, im.slot_m + c.slot0,
                                       im.slot_q + c.slot0, id_offset, d_idx, d_dist, d_cnt, s);
    }
    VDB_SYNC(s);  // (the plan's and the image's host arrays are pageable memory: alive until here)
}

// ---- Flat: exact filtered range search with one row mask per query (k_filter.hip, multi_plan.hpp) --------------------------------------
// Query q's slice is what flat_range_device returns for it alone under masks[mask_of[q]].  The queries are bucketed by mask on the host:
//   per-mask route: a bucket whose mask is longer than flat_filtered_direct_max, and every bucket of a u8 index, is gathered (queries and
//     radii) into a block of its own and goes through flat_range_collect under its mask as it stands -- the 8-bit tier with that mask's row
//     constants, or the scan of all rows -- into the call's pool.
//   grouped route: every other bucket, in every flat mode (the path is exact and reads f32 rows only).  multi_plan lays them out as slots
//     and cuts the slots into chunks; a chunk is ONE launch of k_range_gather_grouped, which decides d <= r on the spot and appends the
//     pair keys (distance, ROW) of the pairs inside to the slot's row of a [slot][ld] matrix filled with PAIR_NONE, one read-back of the
//     slots' counters, ONE sort of the rows (ld wide: launch_sort_rows has one figure for a row's stride and its length) and ONE append of
//     every slot's first `take` keys to the pool.  No dense matrix, no selection, no finalize: the keys carry rows, not columns.
// One pool and one k_range_gather for the whole call.  The counters of the call are added when it has succeeded; what the per-mask route
// added on the way is taken back when it fails.
void Index::flat_range_masked_multi_device(Workspace &ws, const float *d_q, uint64_t nq, const float *d_radius, uint64_t limit,
                                           const RowMask *const *masks, uint64_t n_masks, const uint32_t *mask_of, RangeResult &out) {
    hipStream_t s = ws.stream;
    out.device = device;
    out.nq = nq;
    out.lims.assign(nq + 1, 0);
    if (nq == 0) return;
    VDB_REQUIRE(nq < (1ull << 32), "flat range: too many queries");
    if (n == 0) {  // empty VecSet -> empty results
        range_queries += nq;
        range_scan_queries += nq;
        return;
    }
    const MaskRoutes rt = mask_routes(masks, n_masks, mask_of, nq, [&](uint64_t m) { return !elem_u8 && m <= flat_filtered_direct_max; });
    std::vector<uint64_t> h_off(nq, 0), h_cnt(nq, 0);
    RangePool pool;
    RangeTally tally;
    const uint64_t cap_pairs = range_max_results ? range_max_results : ~0ull;
    uint64_t ns = 0;
    try {
        // per-mask route first: every collect returns synchronised, so the grouped route's reserves below free nothing in use
        {
            uint64_t longest = 0;
            for (uint64_t g = 0; g < n_masks; g++) longest = std::max<uint64_t>(longest, rt.bucket[g].size());
            DevBuf rx, rq, rr;
            if (longest) {
                rx.reserve(longest * sizeof(uint64_t));
                rq.reserve(longest * dim * sizeof(float));
                rr.reserve(longest * sizeof(float));
            }
            std::vector<uint64_t> b_off, b_cnt;
            for (uint64_t g = 0; g < n_masks; g++) {
                const std::vector<uint64_t> &bq = rt.bucket[g];
                const uint64_t nb = bq.size();
                if (nb == 0) continue;
                VDB_HIP(hipMemcpyAsync(rx.p, bq.data(), nb * sizeof(uint64_t), hipMemcpyHostToDevice, s));
                launch_gather_rows_f32(d_q, rx.as<uint64_t>(), nb, (uint32_t)dim, rq.as<float>(), s);
                launch_gather_rows_f32(d_radius, rx.as<uint64_t>(), nb, 1, rr.as<float>(), s);
                b_off.assign(nb, 0);
                b_cnt.assign(nb, 0);
                flat_range_collect(ws, rq.as<float>(), nb, rr.as<float>(), limit, masks[g], pool, b_off.data(), b_cnt.data(), &tally);
                for (uint64_t j = 0; j < nb; j++) {
                    h_off[bq[j]] = b_off[j];
                    h_cnt[bq[j]] = b_cnt[j];
                }
            }
        }
        const uint64_t max_m = multi_plan_max_m(rt.m_of.data(), rt.grouped.data(), n_masks, mask_of, nq);
        const uint64_t ld_all = (max_m + 63) & ~63ull;
        constexpr uint64_t BUDGET = 256ull << 20;  // bytes of each of the two key matrices per chunk
        MultiPlan plan;
        multi_plan(rt.m_of.data(), rt.grouped.data(), n_masks, mask_of, nq, BUDGET, std::max<uint64_t>(ld_all * sizeof(uint64_t), 64), plan);
        ns = plan.slot_query.size();
        if (ns && max_m) {
            const int metric = dist == 0 ? MET_L2_DIRECT : MET_COSINE;
            const uint64_t qch = std::min(plan.qch, ns);
            const size_t tb = sort_rows_temp_bytes(qch, ld_all);
            // every buffer of the route reserved before its first launch (a later, larger reserve would free a buffer in use); ws.misc: plan_image
            ws.qsq.reserve(nq * sizeof(float));
            ws.keys_a.reserve(qch * ld_all * sizeof(uint64_t));
            ws.keys_b.reserve(qch * ld_all * sizeof(uint64_t));
            ws.lists.reserve(tb);
            // the pinned block of the route: [off u64 x qch | cnt u32 x qch | take u32 x qch]; cnt is copied from the device, off and take are
            // written by the host between two stream syncs -- never while a kernel that reads them is in flight
            char *hp = static_cast<char *>(ws.pinned(qch * (sizeof(uint64_t) + 2 * sizeof(uint32_t))));
            uint64_t *p_off = reinterpret_cast<uint64_t *>(hp);
            uint32_t *p_cnt = reinterpret_cast<uint32_t *>(p_off + qch), *p_take = p_cnt + qch;
            const PlanImage im = plan_image(ws, plan, masks, rt.m_of, false, true);
            if (metric == MET_COSINE) launch_row_sqnorm(d_q, nq, (uint32_t)dim, ws.qsq.as<float>(), s);
            for (const MultiChunk &c : plan.chunks) {
                if (c.nitems == 0) continue;  // (only masks without rows: every count stays 0)
                const uint32_t nb = (uint32_t)c.nslots;
                VDB_HIP(hipMemsetAsync(ws.keys_a.p, 0xFF, uint64_t(nb) * c.ld * sizeof(uint64_t), s));  // PAIR_NONE pads sort last
                prof_begin(ws, "flat_range_gather_grouped", double(c.rows) * dim * sizeof(float));
                launch_range_gather_grouped(d_rows.as<float>(), (uint32_t)dim, im.items + c.item0, c.nitems, im.slot_q + c.slot0, d_q, metric,
                                            d_sq.as<float>(), ws.qsq.as<float>(), d_radius, ws.keys_a.as<uint64_t>(), c.ld, im.slot_c + c.slot0, s);
                prof_end(ws);
                VDB_HIP(hipMemcpyAsync(p_cnt, im.slot_c + c.slot0, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
                VDB_SYNC(s);
                uint64_t add = 0, max_take = 0;
                for (uint32_t j = 0; j < nb; j++) {
                    const uint64_t q = plan.slot_query[c.slot0 + j], t = limit ? std::min<uint64_t>(p_cnt[j], limit) : p_cnt[j];
                    h_cnt[q] = t;
                    h_off[q] = pool.used + add;
                    p_off[j] = pool.used + add;
                    p_take[j] = (uint32_t)t;
                    add += t;
                    max_take = std::max(max_take, t);
                }
                if (add == 0) continue;
                pool.room(add, cap_pairs, s);
                launch_sort_rows(ws.keys_a.as<uint64_t>(), ws.keys_b.as<uint64_t>(), nb, c.ld, ws.lists.p, tb, s);
                launch_range_append(ws.keys_b.as<uint64_t>(), c.ld, p_off, p_take, nb, max_take, pool.buf.as<uint64_t>(), s);
                pool.used += add;
                VDB_SYNC(s);  // (the pinned block is rewritten by the next chunk)
            }
        }
        VDB_SYNC(s);  // (the plan's host arrays are pageable memory: alive until here)
        uint64_t total = 0;
        for (uint64_t q = 0; q < nq; q++) total += h_cnt[q];
        out.idx.reserve(total * sizeof(uint64_t));  // (what can fail for want of memory fails before the assemble counts the results)
        out.dist.reserve(total * sizeof(float));
        flat_range_assemble(ws, nq, pool, h_off, h_cnt, out);
    } catch (...) {
        range_i8_queries -= tally.i8;
        range_scan_queries -= tally.scan;
        range_hits -= tally.hits;
        throw;
    }
    range_queries += nq;
    range_grouped_queries += ns;
}

// ---- the approximate keys of the Flat shortlist pass, for every row ------------------------------------------------
// What the filter kernels compare with tau, produced by the SAME kernel in its dense (sample) mode with unit_step = 1:
// L2Sqr key(r, q) = |x_r|^2 - 2 S~(r, q)  (approximate distance = key + |q|^2);  Cosine key = -S~ / |x_r|  (approximate
// distance = 1 + key / |q|).  tier 0 = fp16 operands (k_flat_gemm<GEMM_F16>), tier 1 = split-bf16 operands.  Also the
// quantities the certification bound is built from: |q|^2 (strict fold), the measured |dq| of the fp16 query image and
// the measured row rounding errors (dx_abs = max |dx_r|, dx_rel = max |dx_r| / |x_r|).  Test / measurement entry point.
void Index::flat_debug_keys(Workspace &ws, const float *d_q, uint64_t nq, int tier, float *h_keys, float *h_qsq, float *h_qerr,
                            float *h_dx) {
    hipStream_t s = ws.stream;
    VDB_REQUIRE(nq >= 1 && nq <= 1024 && n >= 1, "debug keys: 1..1024 queries on a non-empty index");
    VDB_REQUIRE(mfma_supported((uint32_t)dim), "debug keys: the dimension has no MFMA shortlist path");
    const int cosine = dist == 1 ? 1 : 0;
    const uint64_t gq = gemm_group(), ngroups = (nq + gq - 1) / gq, nq_pad = ngroups * gq;
    if (tier == 2) {  // 8-bit operands: keys are lower bounds, D >= key + qoff (h_qerr = qoff; h_dx = l1, l2, |mu|, 0)
        VDB_REQUIRE(!elem_u8 && (dim & 3) == 0 && gemm8_supported((uint32_t)dim), "debug keys: the index has no 8-bit pass");
        VDB_REQUIRE(ensure_i8(ws), "debug keys: the 8-bit mirror could not be allocated");
        TauSample sp;  // every row's key: step 1, no unit minima
        sp.set_keys(gemm8_sample_rows(n, 1));
        const I8Queries qp = i8_query_prep(ws, d_q, nq);
        ws.dense.reserve(qp.nq_pad * sp.ld_s * sizeof(float));
        i8_sample(ws, qp, d_rowc_i8.as<float>(), sp);
        VDB_HIP(hipMemcpy2DAsync(h_keys, n * sizeof(float), ws.dense.p, sp.ld_s * sizeof(float), n * sizeof(float), nq, hipMemcpyDeviceToHost, s));
        if (h_qsq) VDB_HIP(hipMemcpyAsync(h_qsq, ws.qsq.p, nq * sizeof(float), hipMemcpyDeviceToHost, s));
        if (h_qerr) VDB_HIP(hipMemcpyAsync(h_qerr, qp.d_qoff, nq * sizeof(float), hipMemcpyDeviceToHost, s));
        VDB_SYNC(s);
        if (h_dx) {
            h_dx[0] = i8_l1;
            h_dx[1] = i8_l2;
            h_dx[2] = i8_mu_norm;
            h_dx[3] = 0.0f;
        }
        return;
    }
    const bool half = tier == 0;
    VDB_REQUIRE(!half || ensure_half(ws), "debug keys: the index holds no fp16 mirror");
    if (!half) VDB_REQUIRE(ensure_tiled(ws), "debug keys: the split-bf16 mirror could not be allocated");
    const uint64_t n_s = gemm_sample_rows(n, 1), ld = (n_s + 63) & ~63ull;
    ws.qsq.reserve(nq_pad * sizeof(float));
    ws.qfrag_g.reserve(nq_pad * size_t(mfma_dim_pad((uint32_t)dim)) * sizeof(float));
    ws.dense.reserve(nq_pad * ld * sizeof(float));
    ws.qaux.reserve(3 * nq_pad * sizeof(float));
    ws.misc.reserve((nq_pad + 128) * sizeof(uint32_t));  // (the preparation kernel also zeroes the 128 rendezvous words behind the counters)
    float *d_qscale = ws.qaux.as<float>(), *d_qmul = d_qscale + nq_pad, *d_qerr = d_qmul + nq_pad;
    if (half) {
        launch_query_prep_h(d_q, (uint32_t)nq, (uint32_t)nq_pad, (uint32_t)dim, half_sx(), ws.qsq.as<float>(), d_qscale, d_qmul, d_qerr,
                            ws.misc.as<uint32_t>(), nullptr, s);  // (the stand-alone packing kernel below: the two must agree)
        launch_pack_queries_h(d_q, (uint32_t)nq, (uint32_t)nq_pad, (uint32_t)dim, 8, d_qscale, ws.qfrag_g.p, s);
    } else {
        launch_row_sqnorm(d_q, nq, (uint32_t)dim, ws.qsq.as<float>(), s);
        launch_mfma_pack_queries_nh(d_q, (uint32_t)nq, (uint32_t)nq_pad, (uint32_t)dim, 8, ws.qfrag_g.as<float>(), s);
    }
    launch_flat_gemm_sample(half ? d_tiled_h.as<float>() : d_tiled.as<float>(), n, (uint32_t)dim, ws.qfrag_g.as<float>(),
                            half ? d_qmul : nullptr, (uint32_t)ngroups, d_sq.as<float>(), cosine, 1, ws.dense.as<float>(), ld, num_cu, s);
    VDB_HIP(hipMemcpy2DAsync(h_keys, n * sizeof(float), ws.dense.p, ld * sizeof(float), n * sizeof(float), nq, hipMemcpyDeviceToHost, s));
    if (h_qsq) VDB_HIP(hipMemcpyAsync(h_qsq, ws.qsq.p, nq * sizeof(float), hipMemcpyDeviceToHost, s));
    if (h_qerr) {
        if (half)
            VDB_HIP(hipMemcpyAsync(h_qerr, d_qerr, nq * sizeof(float), hipMemcpyDeviceToHost, s));
        else
            std::memset(h_qerr, 0, nq * sizeof(float));
    }
    VDB_SYNC(s);
    if (h_dx) {
        h_dx[0] = half ? half_dx_abs : 0.0f;
        h_dx[1] = half ? half_dx_rel : 0.0f;
        h_dx[2] = xsq_max;
        h_dx[3] = xsq_min_pos;
    }
}

}  // namespace vdb
