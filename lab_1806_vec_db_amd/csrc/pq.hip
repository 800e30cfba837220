// pq.hip -- product quantisation on gfx950, host side: the PQ table of an index (attach / build / clear, k-means
// training) and the search drivers of FlatIndex::knn_pq -- the ADC shortlist, its exact re-rank, the reference-order
// re-sort, the row-sharded form.  The kernels and their launchers are in k_pq.hip (declared in kernels.hpp).
// Reference: src/distance/pq_table.rs, src/distance/k_means.rs, FlatIndex::knn_pq
// (src/index_algorithm/flat_index.rs:84-104), ResultSet::pq_resort (src/index_algorithm/candidate_pair.rs:102-108).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <thread>

#include "pq_hnsw.hpp"

#pragma clang fp contract(off)

namespace vdb {

static std::atomic<int> g_adc_fast{1};
void pq_set_adc_fast(int v) { g_adc_fast = v; }
static std::atomic<int> g_adc16_sample{0};  // threshold sample on the quantised tables (L2Sqr): 0 auto (on with the quantised scan), 1 off (f32 sample)
void pq_set_adc16_sample(int v) { g_adc16_sample = v; }
static std::atomic<int> g_adc8_sliced{0};  // 8-bit codes: 0 = sixteen queries per pass on sliced one-byte tables (k_pq_adc8x16), 1 = one query per pass on a byte table (k_pq_adc8), 2 = eight queries per pass on sliced 16-bit tables (k_pq_adc16x8)
void pq_set_adc8_sliced(int v) { g_adc8_sliced = v; }
static std::atomic<int> g_adc16{0};  // quantised first pass of the threshold-filter scan: 0 auto (4-bit, L2Sqr, 16-B code words), 1 off
void pq_set_adc16(int v) { g_adc16 = v; }

// pq_groups (pq_table.rs:38-53)
static std::vector<uint64_t> pq_groups(uint64_t dim, uint64_t m) {
    std::vector<uint64_t> g{0};
    uint64_t cur = 0;
    while (cur < dim) {
        uint64_t rem = m - (g.size() - 1);
        uint64_t gs = (dim - cur + rem - 1) / rem;
        cur += gs;
        g.push_back(cur);
    }
    return g;
}

static float host_dot(const float *a, const float *b, size_t n) {
    float acc = 0.0f;
    for (size_t i = 0; i < n; i++) {
        float p = a[i] * b[i];
        acc = acc + p;
    }
    return acc;
}
static float host_l2(const float *a, const float *b, size_t n) {
    float acc = 0.0f;
    for (size_t i = 0; i < n; i++) {
        float df = a[i] - b[i];
        float sq = df * df;
        acc = acc + sq;
    }
    return acc;
}
static float host_dist(int dist, const float *a, const float *b, size_t n) {
    if (dist == 0) return host_l2(a, b, n);
    float na = std::sqrt(host_dot(a, a, n)), nb = std::sqrt(host_dot(b, b, n));
    float den = std::fmax(na * nb, 1e-10f);
    return 1.0f - host_dot(a, b, n) / den;
}

void pq_clear(Index &ix) {
    ix.pq.present = false;
    ix.pq.n_coded = 0;
    ix.pq.codes_t_valid = false;
    ix.pq.d_codes.release();
    ix.pq.d_codes_t.release();
}

static void pq_install(Index &ix, uint64_t n_bits, uint64_t m, const float *centroids) {
    VDB_REQUIRE(n_bits == 4 || n_bits == 8, "n_bits must be 4 or 8 in PQTable.");  // pq_table.rs:142-145
    VDB_REQUIRE(m > 0 && m <= ix.dim, "m must be in 1..=dim");
    PQState &pq = ix.pq;
    pq.present = false;
    pq.n_bits = n_bits;
    pq.m = m;
    pq.kc = 1ull << n_bits;
    pq.enc_dim = n_bits == 4 ? (m + 1) / 2 : m;
    pq.gstart = pq_groups(ix.dim, m);
    VDB_REQUIRE(pq.gstart.size() == m + 1, "pq_groups produced fewer groups than m");
    pq.h_centroids.assign(centroids, centroids + pq.kc * ix.dim);
    pq.h_cent_cache.assign(m * pq.kc, 0.0f);
    // dot(c,c) is needed by the cosine ADC (pq_table.rs:160-165) and by the cosine encoder
    for (uint64_t g = 0; g < m; g++) {
        uint64_t s = pq.gstart[g], gd = pq.gstart[g + 1] - s;
        for (uint64_t c = 0; c < pq.kc; c++) {
            const float *cc = pq.h_centroids.data() + pq.kc * s + c * gd;
            pq.h_cent_cache[g * pq.kc + c] = host_dot(cc, cc, gd);
        }
    }
    ix.use_device();
    pq.d_centroids.reserve(pq.h_centroids.size() * sizeof(float));
    pq.d_cent_cache.reserve(pq.h_cent_cache.size() * sizeof(float));
    pq.d_gstart.reserve(pq.gstart.size() * sizeof(uint64_t));
    VDB_HIP(hipMemcpy(pq.d_centroids.p, pq.h_centroids.data(), pq.h_centroids.size() * sizeof(float), hipMemcpyHostToDevice));
    VDB_HIP(hipMemcpy(pq.d_cent_cache.p, pq.h_cent_cache.data(), pq.h_cent_cache.size() * sizeof(float), hipMemcpyHostToDevice));
    VDB_HIP(hipMemcpy(pq.d_gstart.p, pq.gstart.data(), pq.gstart.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    pq.d_codes.reserve(std::max<uint64_t>(ix.n, 1) * pq.enc_dim);
}

// word-major mirror of the codes for the quantised scans (rows padded to whole 16-B code words)
static void pq_tile_codes(Index &ix) {
    PQState &pq = ix.pq;
    pq.codes_t_valid = false;
    if ((pq.n_bits != 4 && pq.n_bits != 8) || ix.n == 0) return;
    const uint32_t nwords = (uint32_t)((pq.enc_dim + 15) / 16);
    // tables whose quantised image (4-bit: 16-bit entries of 8 queries; 8-bit: one-byte entries of one query) would not fit LDS never take the quantised scan
    if (size_t(nwords) * (pq.n_bits == 4 ? 32 * 256 : 16 * 256) > 150 * 1024) return;
    const uint64_t total = (ix.n + 63) / 64 * 64 * nwords;
    pq.d_codes_t.reserve(total * sizeof(uint4));
    WsLease ws(ix);
    launch_pq_tile_codes(pq.d_codes.as<uint8_t>(), ix.n, (uint32_t)pq.enc_dim, nwords, pq.d_codes_t.as<uint4>(), ws->stream);
    VDB_SYNC(ws->stream);
    pq.codes_t_valid = true;
}

static void pq_encode_all(Index &ix) {
    PQState &pq = ix.pq;
    if (ix.n == 0) return;
    WsLease ws(ix);
    launch_pq_encode(ix.d_rows.as<float>(), ix.n, (uint32_t)ix.dim, pq.d_centroids.as<float>(), pq.d_cent_cache.as<float>(),
                     pq.d_gstart.as<uint64_t>(), (uint32_t)pq.m, (uint32_t)pq.kc, (uint32_t)pq.n_bits, ix.dist == 1 ? 1 : 0,
                     (uint32_t)pq.enc_dim, pq.d_codes.as<uint8_t>(), ws->stream);
    VDB_SYNC(ws->stream);
}

void pq_attach(Index &ix, uint64_t n_bits, uint64_t m, const float *centroids, const uint8_t *codes) {
    VDB_REQUIRE(!ix.elem_u8, "PQ / HNSW / IVF are built over f32 tables (DynamicIndex, dynamic_index.rs:11-14): a VecSet<u8> index serves Flat search");
    pq_install(ix, n_bits, m, centroids);
    if (codes) {
        if (ix.n) VDB_HIP(hipMemcpy(ix.pq.d_codes.p, codes, ix.n * ix.pq.enc_dim, hipMemcpyHostToDevice));
    } else {
        pq_encode_all(ix);
    }
    pq_tile_codes(ix);
    ix.pq.n_coded = ix.n;
    ix.pq.present = true;
}

// ---- k-means (k_means.rs:61-162), host side, one RNG stream per group so groups can run in parallel ----
static uint64_t splitmix64(uint64_t &s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static float uniform01(uint64_t &s) { return (float(uint32_t(splitmix64(s) >> 40)) + 0.5f) * (1.0f / 16777216.0f); }

static size_t nearest_centroid(const float *v, const float *cents, size_t k, size_t gd, int dist) {
    size_t best = 0;
    float bd = 0;
    for (size_t c = 0; c < k; c++) {
        float d = host_dist(dist, v, cents + c * gd, gd);
        uint32_t od = f32_orderable(d), ob = f32_orderable(bd);
        if (c == 0 || od < ob) {  // equal distance keeps the smaller index
            bd = d;
            best = c;
        }
    }
    return best;
}

static void kmeans_group(const float *train, size_t nt, size_t dim, size_t c0, size_t c1, size_t k, size_t max_iter,
                         float tol, int dist, uint64_t seed, float *cent, const KMeansAssignFn &assign_fn = nullptr) {
    size_t gd = c1 - c0;
    std::vector<float> sel(nt * gd);
    for (size_t i = 0; i < nt; i++) std::memcpy(&sel[i * gd], train + i * dim + c0, gd * sizeof(float));
    uint64_t rng = seed;
    // k-means++ seeding (k_means.rs:61-87): weights are running-min distances
    size_t first = splitmix64(rng) % nt;
    std::memcpy(cent, &sel[first * gd], gd * sizeof(float));
    std::vector<float> w(nt, INFINITY);
    for (size_t idx = 1; idx < k; idx++) {
        const float *prev = cent + (idx - 1) * gd;
        bool bad = false;
        float total = 0;
        for (size_t i = 0; i < nt; i++) {
            float d = host_dist(dist, prev, &sel[i * gd], gd);
            if (std::isnan(w[i]))
                w[i] = d;
            else if (!std::isnan(d) && d < w[i])
                w[i] = d;
            if (!(w[i] >= 0.0f) || std::isinf(w[i])) bad = true;
            total += w[i];
        }
        size_t c;
        if (bad || !(total > 0.0f) || std::isinf(total)) {
            c = splitmix64(rng) % nt;  // WeightedIndex error -> uniform (k_means.rs:80-82)
        } else {
            float u = uniform01(rng) * total, cum = 0;
            c = nt - 1;
            for (size_t i = 0; i < nt; i++) {
                cum += w[i];
                if (cum > u) {
                    c = i;
                    break;
                }
            }
        }
        std::memcpy(cent + idx * gd, &sel[c * gd], gd * sizeof(float));
    }
    // Lloyd (k_means.rs:95-162)
    std::vector<float> sums(k * gd);
    std::vector<size_t> cnt(k);
    std::vector<uint32_t> asg(assign_fn ? nt : 0);
    for (size_t it = 0; it < max_iter; it++) {
        std::fill(sums.begin(), sums.end(), 0.0f);
        std::fill(cnt.begin(), cnt.end(), 0);
        // assignment step (k_means.rs:117-120): on the GPU when the caller provides it (same (distance, index) minimum,
        // same strict-order distances, so the same clusters as the host loop); the sums stay in row order
        if (assign_fn) assign_fn(cent, asg.data());
        for (size_t i = 0; i < nt; i++) {
            size_t c = assign_fn ? asg[i] : nearest_centroid(&sel[i * gd], cent, k, gd, dist);
            cnt[c]++;
            for (size_t j = 0; j < gd; j++) sums[c * gd + j] += sel[i * gd + j];
        }
        float max_diff = -INFINITY;
        for (size_t c = 0; c < k; c++) {
            if (cnt[c] == 0)
                std::memcpy(&sums[c * gd], cent + c * gd, gd * sizeof(float));
            else
                for (size_t j = 0; j < gd; j++) sums[c * gd + j] /= float(cnt[c]);
            float d = host_l2(cent + c * gd, &sums[c * gd], gd);
            if (!std::isnan(d) && d > max_diff) max_diff = d;
        }
        std::memcpy(cent, sums.data(), k * gd * sizeof(float));
        if (max_diff < tol) break;
    }
}

// PQTable::from_vec_set (pq_table.rs:141-191): sample, per-group k-means on the host, encode on the GPU
void host_kmeans(const float *train, size_t nt, size_t dim, size_t c0, size_t c1, size_t k, size_t max_iter, float tol,
                 int dist, uint64_t seed, float *cent, const KMeansAssignFn &assign_fn) {
    kmeans_group(train, nt, dim, c0, c1, k, max_iter, tol, dist, seed, cent, assign_fn);
}
uint64_t host_splitmix64(uint64_t &s) { return splitmix64(s); }

void pq_build(Index &ix, uint64_t n_bits, uint64_t m, uint64_t train_n, uint64_t max_iter, float tol,
              uint64_t seed) {
    VDB_REQUIRE(n_bits == 4 || n_bits == 8, "n_bits must be 4 or 8 in PQTable.");
    VDB_REQUIRE(!ix.elem_u8, "PQ / HNSW / IVF are built over f32 tables (DynamicIndex, dynamic_index.rs:11-14): a VecSet<u8> index serves Flat search");
    VDB_REQUIRE(m > 0 && m <= ix.dim, "m must be in 1..=dim");
    VDB_REQUIRE(ix.n > 0, "Cannot build PQ table for an empty table");  // metadata_vec_table.rs:120-122
    const float *rows = ix.host_rows();
    size_t n = ix.n, dim = ix.dim, kc = 1ull << n_bits;
    std::vector<float> sample;
    const float *train = rows;
    size_t nt = n;
    uint64_t rng = seed;
    if (train_n && train_n < n) {  // VecSet::random_sample (vec_set.rs:154-163)
        std::vector<size_t> perm(n);
        for (size_t i = 0; i < n; i++) perm[i] = i;
        sample.resize(train_n * dim);
        for (size_t i = 0; i < train_n; i++) {
            size_t j = i + splitmix64(rng) % (n - i);
            std::swap(perm[i], perm[j]);
            std::memcpy(&sample[i * dim], rows + perm[i] * dim, dim * sizeof(float));
        }
        train = sample.data();
        nt = train_n;
    }
    auto gs = pq_groups(dim, m);
    std::vector<float> cent(kc * dim);
    unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    unsigned nth = (unsigned)std::min<uint64_t>(hw, m);
    auto par_groups = [&](const std::function<void(uint64_t)> &fn) {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nth; t++)
            th.emplace_back([&, t]() {
                for (uint64_t g = t; g < m; g += nth) fn(g);
            });
        for (auto &t : th) t.join();
    };
    // (1) k-means++ seeding per group on the host (k_means.rs:61-87: a sequential weighted draw per centroid)
    par_groups([&](uint64_t g) {
        uint64_t gseed = seed ^ (0xD1B54A32D192ED03ull * (g + 1));
        kmeans_group(train, nt, dim, gs[g], gs[g + 1], kc, /*max_iter=*/0, tol, ix.dist, gseed, cent.data() + kc * gs[g]);
    });
    // (2) Lloyd (k_means.rs:95-162) for ALL groups together: the assignment step (:117-120) -- nt x m x kc strict-order
    // sub-vector distances per iteration -- is find_nearest_base of every training row against the current centroids,
    // i.e. exactly the encoder: one k_pq_encode launch on the training rows per iteration.  The update (sums in row
    // order, empty clusters keep their centroid, max shift against tol) stays on the host, per group in parallel; a
    // group that has converged is frozen, as its own loop would have stopped.
    {
        ix.use_device();
        const uint64_t enc = n_bits == 4 ? (m + 1) / 2 : m;
        DevBuf d_train, d_cent, d_csq, d_gs, d_codes;
        d_train.reserve(nt * dim * sizeof(float));
        d_cent.reserve(kc * dim * sizeof(float));
        d_csq.reserve(m * kc * sizeof(float));
        d_gs.reserve((m + 1) * sizeof(uint64_t));
        d_codes.reserve(nt * enc);
        VDB_HIP(hipMemcpy(d_train.p, train, nt * dim * sizeof(float), hipMemcpyHostToDevice));
        VDB_HIP(hipMemcpy(d_gs.p, gs.data(), (m + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
        std::vector<uint8_t> codes(nt * enc);
        std::vector<float> csq(m * kc);
        std::vector<char> active(m, 1);
        WsLease ws(ix);
        for (uint64_t it = 0; it < max_iter; it++) {
            for (uint64_t g = 0; g < m; g++)
                for (uint64_t c = 0; c < kc; c++) {
                    const float *cc = cent.data() + kc * gs[g] + c * (gs[g + 1] - gs[g]);
                    csq[g * kc + c] = host_dot(cc, cc, gs[g + 1] - gs[g]);
                }
            VDB_HIP(hipMemcpyAsync(d_cent.p, cent.data(), kc * dim * sizeof(float), hipMemcpyHostToDevice, ws->stream));
            VDB_HIP(hipMemcpyAsync(d_csq.p, csq.data(), m * kc * sizeof(float), hipMemcpyHostToDevice, ws->stream));
            launch_pq_encode(d_train.as<float>(), (uint64_t)nt, (uint32_t)dim, d_cent.as<float>(), d_csq.as<float>(), d_gs.as<uint64_t>(), (uint32_t)m,
                             (uint32_t)kc, (uint32_t)n_bits, ix.dist == 1 ? 1 : 0, (uint32_t)enc, d_codes.as<uint8_t>(), ws->stream);
            VDB_HIP(hipMemcpyAsync(codes.data(), d_codes.p, nt * enc, hipMemcpyDeviceToHost, ws->stream));
            VDB_SYNC(ws->stream);
            par_groups([&](uint64_t g) {
                if (!active[g]) return;
                const size_t c0 = gs[g], gd = gs[g + 1] - gs[g];
                float *cg = cent.data() + kc * c0;
                std::vector<float> sums(kc * gd, 0.0f);
                std::vector<size_t> cnt(kc, 0);
                for (size_t i = 0; i < nt; i++) {
                    const size_t c = n_bits == 4 ? ((codes[i * enc + g / 2] >> (4 * (g & 1))) & 0xf) : codes[i * enc + g];
                    cnt[c]++;
                    const float *v = train + i * dim + c0;
                    for (size_t j = 0; j < gd; j++) sums[c * gd + j] += v[j];
                }
                float max_diff = -INFINITY;
                for (size_t c = 0; c < kc; c++) {
                    if (cnt[c] == 0)
                        std::memcpy(&sums[c * gd], cg + c * gd, gd * sizeof(float));
                    else
                        for (size_t j = 0; j < gd; j++) sums[c * gd + j] /= float(cnt[c]);
                    const float d = host_l2(cg + c * gd, &sums[c * gd], gd);
                    if (!std::isnan(d) && d > max_diff) max_diff = d;
                }
                std::memcpy(cg, sums.data(), kc * gd * sizeof(float));
                if (max_diff < tol) active[g] = 0;
            });
            if (std::none_of(active.begin(), active.end(), [](char a) { return a != 0; })) break;
        }
    }
    pq_install(ix, n_bits, m, cent.data());
    pq_encode_all(ix);
    pq_tile_codes(ix);
    ix.pq.n_coded = ix.n;
    ix.pq.present = true;
}
// ---- FlatIndex::knn_pq (flat_index.rs:84-104) --------------------------------------------------------
void pq_make_luts(Index &ix, Workspace &ws, const float *d_q, uint64_t nq) {
    PQState &pq = ix.pq;
    ws.lut.reserve(nq * pq.m * pq.kc * sizeof(float));
    launch_pq_lut(d_q, (uint32_t)ix.dim, pq.d_centroids.as<float>(), pq.d_gstart.as<uint64_t>(), (uint32_t)pq.m, (uint32_t)pq.kc,
                  ix.dist == 1 ? 1 : 0, (uint32_t)nq, ws.lut.as<float>(), ws.stream);
}

void pq_resort_launch(const uint64_t *exact_keys, uint32_t ncand, uint32_t ldc, uint32_t nq, uint32_t k,
                      uint64_t *out, hipStream_t s) {
    launch_pq_resort(exact_keys, ncand, ldc, nq, k, out, s);
}

// row stride of the per-query shortlists: the register-resident select writes topk_capacity(efk) entries (efk <= 1024);
// beyond that the any-size path writes efk rounded up to 64
static uint32_t pq_list_ld(uint32_t efk) { return efk <= 1024 ? topk_capacity(efk) : ((efk + 63) & ~63u); }

// the query norms and lookup tables every ADC scan of a call starts from: ws.qsq [nq], ws.lut [nq][m * kc]
static void pq_prepare_queries(Index &ix, Workspace &ws, const float *d_q, uint64_t nq) {
    ws.qsq.reserve(nq * sizeof(float));
    launch_row_sqnorm(d_q, nq, (uint32_t)ix.dim, ws.qsq.as<float>(), ws.stream);
    pq_make_luts(ix, ws, d_q, nq);
}

// queries per pass and rows per row block of the f32 scan over this index's tables (the launcher decides by the same rule)
static AdcPlan pq_f32_plan(const Index &ix) { return pq_adc_plan(ix.pq.m * ix.pq.kc * sizeof(float), ix.dist == 1); }
// row stride of a dense ADC matrix over all rows: the rows padded to whole row blocks, then to 64
static uint64_t pq_dense_ld(const Index &ix) { return (ix.n + pq_f32_plan(ix).nt + 63) & ~63ull; }

// f32 scan arguments for queries [g0, g0 + gn) of the call (after pq_prepare_queries): every row, no output yet
static AdcArgs pq_f32_args(Index &ix, Workspace &ws, uint64_t g0, uint64_t gn) {
    PQState &pq = ix.pq;
    AdcArgs a{};
    a.codes = pq.d_codes.as<uint8_t>();
    a.n = ix.n;
    a.enc_dim = (uint32_t)pq.enc_dim;
    a.m = (uint32_t)pq.m;
    a.cent_cache = pq.d_cent_cache.as<float>();
    a.cosine = ix.dist == 1 ? 1 : 0;
    a.blk_step = 1;
    a.fast = g_adc_fast;
    a.nq_total = (uint32_t)gn;
    a.lut = ws.lut.as<float>() + g0 * pq.m * pq.kc;
    a.qsq = ws.qsq.as<float>() + g0;
    return a;
}

static void pq_prof_begin(Index &ix, Workspace &ws, uint64_t passes) { ix.prof_begin(ws, "pq_adc", double(passes) * double(ix.n) * ix.pq.enc_dim); }

// dense ADC of queries [g0, g0 + gn) into ws.dense [gn][ld] (reserved by the caller): every blk_step-th row block (1: every row)
static void pq_dense_adc(Index &ix, Workspace &ws, uint64_t g0, uint64_t gn, uint64_t ld, uint32_t blk_step, bool prof) {
    AdcArgs a = pq_f32_args(ix, ws, g0, gn);
    a.blk_step = blk_step;
    a.out = ws.dense.as<float>();
    a.ld = ld;
    const uint32_t BQ = pq_f32_plan(ix).BQ;
    if (prof) pq_prof_begin(ix, ws, (gn + BQ - 1) / BQ);
    launch_pq_adc(a, (uint32_t)ix.pq.n_bits, 0, ix.num_cu, ws.stream);
    if (prof) ix.prof_end(ws);
}

// any ef: every ADC value of every row, a full (adc, idx) sort per query, the first efk pairs (flat_index.rs:96-100
// with ResultSet::new(ef.max(k)) of any size) -> ws.keys_a [nq][pq_list_ld(efk)]
static void pq_adc_shortlist_sorted(Index &ix, Workspace &ws, const float *d_q, uint64_t nq, uint32_t efk) {
    hipStream_t s = ws.stream;
    const uint64_t n = ix.n;
    pq_prepare_queries(ix, ws, d_q, nq);
    const uint32_t BQ = pq_f32_plan(ix).BQ;
    const uint64_t ld = pq_dense_ld(ix);
    const uint32_t ldo = pq_list_ld(efk);
    const uint64_t GQ = std::max<uint64_t>(BQ, std::min<uint64_t>(64, (size_t(1) << 30) / (ld * 20)) / BQ * BQ);
    const size_t tb = sort_rows_temp_bytes(GQ, ld);
    ws.keys_a.reserve(nq * ldo * sizeof(uint64_t));
    ws.keys_b.reserve(nq * ldo * sizeof(uint64_t));
    ws.dense.reserve(GQ * ld * sizeof(float));
    ws.lists.reserve(2 * GQ * ld * sizeof(uint64_t) + tb);
    uint64_t *k_in = ws.lists.as<uint64_t>(), *k_out = k_in + GQ * ld;
    void *temp = k_out + GQ * ld;
    for (uint64_t g0 = 0; g0 < nq; g0 += GQ) {
        const uint64_t gn = std::min<uint64_t>(GQ, nq - g0);
        pq_dense_adc(ix, ws, g0, gn, ld, 1, true);
        launch_pair_keys_rows(ws.dense.as<float>(), ld, n, (uint32_t)gn, k_in, ld, s);
        launch_sort_rows(k_in, k_out, gn, ld, temp, tb, s);
        launch_copy_prefix(k_out, ld, ws.keys_a.as<uint64_t>() + g0 * ldo, ldo, efk, (uint32_t)gn, s);
    }
}

// dense path for one group of queries: every ADC distance, then the wave select (also the fallback of the filtered scans)
static void pq_dense_group(Index &ix, Workspace &ws, uint64_t g0, uint64_t gn, uint32_t efk) {
    const uint64_t n = ix.n, ld = pq_dense_ld(ix);
    const uint32_t nl = topk_num_lists(n), cape = topk_capacity(efk);
    ws.dense.reserve(gn * ld * sizeof(float));
    ws.lists.reserve(gn * nl * cape * sizeof(uint64_t));
    pq_dense_adc(ix, ws, g0, gn, ld, 1, true);
    launch_topk_dense(ws.dense.as<float>(), ld, n, (uint32_t)gn, efk, ws.lists.as<uint64_t>(), ws.stream);
    launch_topk_merge(ws.lists.as<uint64_t>(), nl, cape, (uint32_t)gn, efk, ws.keys_a.as<uint64_t>() + g0 * cape, ws.stream);
}

// ---- the threshold-filter shortlist ---------------------------------------------------------------------
// tau[q] from a strided row-block sample, ONE filtered scan of all rows that parks the rows at or below tau[q] in a candidate
// list, exact f32 sums for the candidates where the scan ran on quantised tables, a counted merge -- in rounds of GQ queries --,
// then the counts read back once per call and the queries whose list overflowed or came out short redone densely.  What differs
// between the code widths is the scan (Scan8 / Scan4 below: query image, sample, filter, exact stage, books); the rounds
// (pq_filter_rounds), the threshold (pq_tau_from_sample) and the read-back (pq_read_back) are shared.

// Threshold sample: every step-th row block, tau = the rank-th smallest sampled ADC value.  rank = efk guarantees
// >= efk hits (the sample is a subset) at efk * step expected ones; when the shard is large enough a thinner rank
// r = max(8, efk / 8) with step ~ max(1024, 4 efk) / r gives ~1000 hits instead of ~6400 (every hit costs the scan's
// epilogue an LDS append and the counted merge an insertion) and the hit count is CHECKED: hits / step is
// Gamma(r)-distributed, the rule below keeps P[hits < efk] under ~1e-5.  (mfma_sample_plan is a different rule.)
struct PqSamplePlan {
    uint32_t step, rank;
};
static PqSamplePlan pq_sample_plan(uint64_t nblk, uint32_t efk) {
    PqSamplePlan p{(uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(64, nblk / 16)), efk};
    const uint32_t r = efk / 8 < 8 ? 8 : efk / 8;
    const uint64_t target = std::max<uint64_t>(1024, 4ull * efk);
    const uint64_t st = std::min<uint64_t>(nblk / 16, target / r);
    const double thr = r < 16 ? r / 8.0 : (r < 32 ? r / 4.0 : r / 3.0);
    if (r < efk && st >= p.step && double(efk) <= thr * double(st) * 1.1) {
        p.rank = r;
        p.step = (uint32_t)st;
    }
    return p;
}

// One call of the threshold-filter shortlist: its sample, its rounds and the buffers every round shares.
struct FilterCall {
    Index &ix;
    Workspace &ws;
    uint64_t nq;
    uint32_t efk, cape;
    uint32_t step = 1, rank = 0;         // the sample plan over row blocks of `blk` rows
    uint64_t n_sb = 0, n_s = 0, ld_s = 0;  // sampled blocks, sampled rows (incl. padding past n), row stride of the sample matrix
    uint32_t cap = 0;                    // slots of a query's candidate list
    uint64_t GQ = 0;                     // queries per round: bounded by the sample matrix (GQ x ld_s floats) and the candidate lists
    float *d_tau = nullptr;              // [nq]
    uint32_t *d_hits = nullptr, *d_valid = nullptr;  // [nq] rows the scan parked | pairs the exact stage kept

    // the sample over row blocks of blk rows (8-bit scans: 1024; else the f32 scan's row block); false: too small to pay
    bool plan_sample(uint32_t blk) {
        const uint64_t nblk = (ix.n + blk - 1) / blk;
        const PqSamplePlan p = pq_sample_plan(nblk, efk);
        step = p.step, rank = p.rank;
        n_sb = (nblk + step - 1) / step, n_s = n_sb * blk, ld_s = (n_s + 63) & ~63ull;
        return n_s >= 2 * uint64_t(efk) && ix.n >= 65536 && n_s >= 64ull * rank;
    }
    void reserve() {
        const uint64_t gq_max = std::min<uint64_t>(GQ, nq);
        ws.dense.reserve(gq_max * ld_s * sizeof(float));
        // ws.lists serves a round twice: first the level-1 lists of a large sample (pq_tau_from_sample), then -- those are dead once
        // tau is known -- the candidate lists of the scan
        ws.lists.reserve(std::max<size_t>(gq_max * topk_num_lists(n_s) * cape, gq_max * size_t(cap)) * sizeof(uint64_t));
        ws.misc.reserve(nq * (sizeof(float) + 2 * sizeof(uint32_t)));
        d_tau = ws.misc.as<float>();
        d_hits = reinterpret_cast<uint32_t *>(d_tau + nq);
        d_valid = d_hits + nq;
        VDB_HIP(hipMemsetAsync(d_hits, 0, 2 * nq * sizeof(uint32_t), ws.stream));
    }
    uint64_t *cand() const { return ws.lists.as<uint64_t>(); }
};

// offset / step / flag of the quantisation a sample's sums are in (per query of the round); all null: the sample holds f32 ADC values
struct SampleQuant {
    const double *qM = nullptr, *qD = nullptr;
    const uint32_t *qflag = nullptr;
};

// tau of the round's queries from the sample matrix ws.dense [gn][ld_s]: the rank-th smallest of n_s values is a selection up to
// select_tau_max_n(), beyond it the two-level top-k; quantised sums are turned into thresholds of the f32 sums (k_pq_tau_from16)
static void pq_tau_from_sample(const FilterCall &c, uint64_t g0, uint64_t gn, const SampleQuant &sq) {
    Workspace &ws = c.ws;
    hipStream_t s = ws.stream;
    if (c.n_s <= select_tau_max_n()) {
        launch_select_tau(ws.dense.as<float>(), c.ld_s, (uint32_t)c.n_s, (uint32_t)gn, (uint32_t)gn, c.rank, c.d_tau + g0, s);
    } else {
        uint64_t *top = ws.keys_a.as<uint64_t>() + g0 * c.cape;  // (overwritten by the round's merge)
        launch_topk_dense(ws.dense.as<float>(), c.ld_s, c.n_s, (uint32_t)gn, c.rank, ws.lists.as<uint64_t>(), s);
        launch_topk_merge(ws.lists.as<uint64_t>(), topk_num_lists(c.n_s), c.cape, (uint32_t)gn, c.rank, top, s);
        launch_extract_tau(top, c.cape, (uint32_t)gn, c.rank, c.d_tau + g0, s);
    }
    if (sq.qM) launch_pq_tau_from16(c.d_tau + g0, sq.qM, sq.qD, sq.qflag, (uint32_t)c.ix.pq.m, (uint32_t)gn, s);
}

template <class Scan>
static std::vector<uint64_t> pq_filter_rounds(FilterCall &c) {
    Scan scan(c);
    c.reserve();
    scan.prepare();
    for (uint64_t g0 = 0; g0 < c.nq; g0 += c.GQ) {
        const uint64_t gn = std::min<uint64_t>(c.GQ, c.nq - g0);
        pq_tau_from_sample(c, g0, gn, scan.sample(g0, gn));
        scan.filter(g0, gn);
        scan.exact(g0, gn);
        launch_topk_merge_counted(c.cand(), c.cap, c.d_hits + g0, (uint32_t)gn, c.efk, c.ws.keys_a.as<uint64_t>() + g0 * c.cape, c.ws.stream);
    }
    return scan.books();  // the counts read back (the one sync of the call): the queries the f32 scan has to answer
}

// The counts of every query of the call, read back once: hv[q] = rows the scan parked, hv[nq + q] = pairs the exact stage kept
// (pinned memory, valid until the workspace's next read-back).  Returns the queries the f32 scan has to answer: overflowed lists
// (hv[q] > cap) and short ones -- fewer than min(efk, n) rows at or below tau (thinned sample), counted AFTER the exact stage where
// there is one (by_valid).  A table that cannot be quantised ends up in one of the two: tau = +inf overflows the list, or the
// scan parks nothing for the flagged query.
// The books differ per scan and are the callers': bench.py and the full-size tests read them.
//   Scan4, quantised: short by hv[nq + q]; pq_adc16_redo += the queries returned; nothing else.
//   Scan4, f32 filter: short by hv[q] (no exact stage: d_valid stays zero); nothing is counted.
//   Scan8: short by hv[nq + q]; pq_q8_overflow / pq_q8_short count the two reasons apart, pq_q8_hits_sum / _max cover the lists
//          that did not overflow; pq_adc16_redo is left alone.
static std::vector<uint64_t> pq_read_back(const FilterCall &c, bool by_valid, const uint32_t **hv_out = nullptr) {
    const uint64_t nq = c.nq;
    uint32_t *hv = static_cast<uint32_t *>(c.ws.pinned(2 * nq * sizeof(uint32_t)));
    VDB_HIP(hipMemcpyAsync(hv, c.d_hits, 2 * nq * sizeof(uint32_t), hipMemcpyDeviceToHost, c.ws.stream));
    VDB_SYNC(c.ws.stream);
    const uint64_t need = std::min<uint64_t>(c.efk, c.ix.n);
    std::vector<uint64_t> redo;
    for (uint64_t q = 0; q < nq; q++)
        if (hv[q] > c.cap || (by_valid ? hv[nq + q] : hv[q]) < need) redo.push_back(q);
    if (hv_out) *hv_out = hv;
    return redo;
}

struct ScanBase {  // the call a scan works for, and its index
    FilterCall &c;
    Index &ix;
    Workspace &ws;
    PQState &pq;
    explicit ScanBase(FilterCall &call) : c(call), ix(call.ix), ws(call.ws), pq(call.ix.pq) {}
};

// ---- 8-bit codes (L2Sqr): sixteen queries per pass on one-byte table entries (k_pq_adc8x16, sample included); pq_adc8_sliced = 1 / 2:
// the earlier forms -- sample and scan of one query per pass on a byte table (k_pq_adc8) | that sample, then eight per pass on sliced
// 16-bit tables (k_pq_adc16x8)
struct Scan8 : ScanBase {
    enum Form { X16, BYTE, X8 };
    const uint32_t nw8 = (uint32_t)((pq.enc_dim + 15) / 16), m8 = 16 * nw8;  // 16-B code words per row, groups of the one-byte image
    Form form;
    double *d_qM = nullptr, *d_qD = nullptr;  // BYTE / X8: the one-byte quantisation of every query of the call
    uint32_t *d_qflag = nullptr;
    Adc16x8Args b16{};  // X16: the round's arguments, sample and scan

    explicit Scan8(FilterCall &call) : ScanBase(call) {
        const int v = g_adc8_sliced;
        form = v == 0 && pq_adc8x16_lds_bytes() <= 158 * 1024 ? X16 : (v != 1 && pq_adc16x8_lds_bytes() <= 158 * 1024 ? X8 : BYTE);
    }
    static bool plan(FilterCall &c) {
        const PQState &pq = c.ix.pq;
        if (!(g_adc16 != 1 && pq.codes_t_valid && pq.n_bits == 8 && c.ix.dist == 0 && pq.m <= 1024 &&
              pq_adc8_lds_bytes((uint32_t)((pq.enc_dim + 15) / 16)) <= 150 * 1024 && c.plan_sample(1024)))
            return false;
        // (lists of ~1000 expected candidates reach 4000 on a query in a thousand: 8192 entries keep those off the f32 scan)
        c.cap = (uint32_t)std::min<uint64_t>(65536, std::max<uint64_t>(8192, 4ull * c.rank * c.step));
        c.GQ = std::max<uint64_t>(64, std::min<uint64_t>(2048, (size_t(256) << 20) / (c.ld_s * sizeof(float))));
        return true;
    }
    void prepare() {
        if (form == X16) return;  // its image is made per round
        const uint64_t nq = c.nq;
        ws.qfrag_g.reserve(nq * size_t(m8) * 256);
        ws.qaux.reserve(nq * (2 * sizeof(double) + sizeof(uint32_t)));
        d_qM = ws.qaux.as<double>(), d_qD = d_qM + nq;
        d_qflag = reinterpret_cast<uint32_t *>(d_qD + nq);
        launch_pq_quant8(ws.lut.as<float>(), (uint32_t)pq.m, m8, (uint32_t)nq, ws.qfrag_g.as<uint8_t>(), d_qM, d_qD, d_qflag, ws.stream);
    }
    Adc8Args byte_args(uint64_t g0, uint64_t gn) const {
        Adc8Args a{};
        a.codes_t = pq.d_codes_t.as<uint4>();
        a.n = ix.n;
        a.nwords = nw8;
        a.m = (uint32_t)pq.m;
        a.img = ws.qfrag_g.as<uint8_t>() + g0 * size_t(m8) * 256;
        a.qM = d_qM + g0;
        a.qD = d_qD + g0;
        a.qflag = d_qflag + g0;
        a.tau = c.d_tau + g0;
        a.nq = (uint32_t)gn;
        a.cand = c.cand();
        a.cnt = c.d_hits + g0;
        a.cap = c.cap;
        a.blk_step = c.step;
        a.s8_out = ws.dense.as<float>();
        a.ld_s = c.ld_s;
        return a;
    }
    // the sliced image of the round's queries (ws.pq_img16; statistics in ws.pq_aux16) and the scan arguments over it
    Adc16x8Args sliced_round(uint64_t g0, uint64_t gn, bool sixteen) {
        const uint32_t gs = sixteen ? ADC8X16_GS : ADC16X8_GS, rpt = sixteen ? ADC8X16_RPT : ADC16X8_RPT, per = sixteen ? 16 : 8;
        const uint32_t nsl = (uint32_t)((pq.m + gs - 1) / gs), m_pad = nsl * gs, ngrp = (uint32_t)((gn + per - 1) / per);
        ws.pq_img16.reserve(size_t(ngrp) * m_pad * 256 * sizeof(uint4));
        ws.pq_aux16.reserve(gn * pq.m * sizeof(float) + gn * (2 * sizeof(double) + sizeof(uint32_t)) + 64);
        double *qM = ws.pq_aux16.as<double>(), *qD = qM + gn;
        uint32_t *qf = reinterpret_cast<uint32_t *>(qD + gn);
        float *mn = reinterpret_cast<float *>(qf + ((gn + 3) & ~uint64_t(3)));
        launch_pq_quant_sliced(sixteen, ws.lut.as<float>() + g0 * pq.m * pq.kc, (uint32_t)pq.m, m_pad, (uint32_t)gn,
                               sixteen ? std::min(65000.0, 512.0 * double(pq.m)) : 65000.0, mn, qM, qD, qf, ws.pq_img16.as<uint4>(), ws.stream);
        Adc16x8Args b{};
        b.codes_t = pq.d_codes_t.as<uint4>();
        b.n = ix.n;
        b.nwords = nw8;
        b.m = (uint32_t)pq.m;
        b.nslices = nsl;
        b.img = ws.pq_img16.as<uint4>();
        b.qM = qM;
        b.qD = qD;
        b.qflag = qf;
        b.tau = c.d_tau + g0;
        b.nq = (uint32_t)gn;
        b.rows_per_wg = uint64_t(rpt) * 1024;  // one block of rows per workgroup: every slice of the image is loaded once
        b.cand = c.cand();
        b.cnt = c.d_hits + g0;
        b.cap = c.cap;
        if (sixteen) {  // its sample runs on the same image
            b.blk_step = c.step;
            b.n_sb = c.n_sb;
            b.s8_out = ws.dense.as<float>();
            b.ld_s = c.ld_s;
        }
        return b;
    }
    SampleQuant sample(uint64_t g0, uint64_t gn) {
        if (form == X16) {
            b16 = sliced_round(g0, gn, true);
            launch_pq_adc8x16(b16, true, ws.stream);
            return {b16.qM, b16.qD, b16.qflag};  // (the sample's sums are in the scan's own quantisation)
        }
        launch_pq_adc8(byte_args(g0, gn), true, ix.num_cu, ws.stream);
        return {d_qM + g0, d_qD + g0, d_qflag + g0};
    }
    void filter(uint64_t g0, uint64_t gn) {
        if (form == X16) {
            pq_prof_begin(ix, ws, (gn + 15) / 16);
            launch_pq_adc8x16(b16, false, ws.stream);
        } else if (form == X8) {
            const Adc16x8Args b = sliced_round(g0, gn, false);
            pq_prof_begin(ix, ws, (gn + 7) / 8);
            launch_pq_adc16x8(b, ws.stream);
        } else {
            Adc8Args a = byte_args(g0, gn);
            const uint32_t nwg = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(ix.num_cu, (4ull * ix.num_cu + gn - 1) / gn));
            a.rows_per_wg = ((ix.n + nwg - 1) / nwg + 63) / 64 * 64;
            pq_prof_begin(ix, ws, gn);
            launch_pq_adc8(a, false, ix.num_cu, ws.stream);
        }
        ix.prof_end(ws);
        pq.adc16_queries += gn;
    }
    void exact(uint64_t g0, uint64_t gn) {
        launch_pq_adc_exact8(pq.d_codes.as<uint8_t>(), (uint32_t)pq.enc_dim, pq.d_codes_t.as<uint4>(), nw8, (uint32_t)pq.m,
                             ws.lut.as<float>() + g0 * pq.m * pq.kc, c.d_tau + g0, c.cand(), c.d_hits + g0, c.cap, c.d_valid + g0, (uint32_t)gn, ws.stream);
    }
    std::vector<uint64_t> books() {  // (see pq_read_back)
        const uint32_t *hv = nullptr;
        std::vector<uint64_t> redo = pq_read_back(c, true, &hv);
        uint64_t hsum = 0, hmax = 0, n_over = 0;
        for (uint64_t q = 0; q < c.nq; q++) {
            if (hv[q] > c.cap) n_over++;
            else hsum += hv[q], hmax = std::max<uint64_t>(hmax, hv[q]);
        }
        pq.q8_overflow += n_over;
        pq.q8_short += redo.size() - n_over;
        pq.q8_hits_sum += hsum;
        if (hmax > pq.q8_hits_max) pq.q8_hits_max = hmax;
        return redo;
    }
};

// ---- 4-bit codes and tables of any width on the f32 scan.  q16: the scan runs on the 16-bit quantised tables, 8 queries per pass
// (k_pq_adc16; Cosine: 7, slot 7 of an entry is the |centroid|^2 table), and the exact f32 sums are computed for its candidates only
// (k_pq_adc_exact); otherwise the f32 scan itself filters (k_pq_adc MODE 1) and its values are exact already.
struct Scan4 : ScanBase {
    const bool q16 = quantised(ix), cos16 = q16 && ix.dist == 1;
    const uint32_t NQ16 = cos16 ? 7 : 8;                                         // queries per image group
    const uint32_t nw16 = (uint32_t)((pq.enc_dim + 15) / 16), m16 = 32 * nw16;  // code words per (padded) row, groups of the image
    double *d_qM = nullptr, *d_qD = nullptr, *d_qMC = nullptr, *d_qDC = nullptr;
    uint32_t *d_qflag = nullptr;

    static bool quantised(const Index &ix) {
        const PQState &pq = ix.pq;
        const AdcPlan tp = pq_f32_plan(ix);
        return g_adc16 != 1 && pq.codes_t_valid && pq.n_bits == 4 && pq_adc16_lds_bytes((uint32_t)((pq.enc_dim + 15) / 16)) <= 150 * 1024 &&
               tp.nt == 1024 && (ix.dist == 0 ? tp.BQ == 4 : true);
    }
    static bool plan(FilterCall &c) {
        if (!c.plan_sample(pq_f32_plan(c.ix).nt)) return false;
        c.cap = (uint32_t)std::min<uint64_t>(65536, std::max<uint64_t>(4096, 4ull * c.rank * c.step));
        // (q16: a multiple of 448 = 7 * 64, so that a round starts on a whole image group for either metric)
        c.GQ = quantised(c.ix) ? std::max<uint64_t>(448, std::min<uint64_t>(1792, (size_t(256) << 20) / (c.ld_s * sizeof(float))) / 448 * 448) : 64;
        return true;
    }
    using ScanBase::ScanBase;
    void prepare() {
        if (!q16) return;
        const uint64_t nq = c.nq, ngrp = (nq + NQ16 - 1) / NQ16;
        ws.qfrag_g.reserve(ngrp * size_t(m16) * 256);
        ws.qaux.reserve(nq * (4 * sizeof(double) + sizeof(uint32_t)));
        d_qM = ws.qaux.as<double>(), d_qD = d_qM + nq, d_qMC = d_qD + nq, d_qDC = d_qMC + nq;
        d_qflag = reinterpret_cast<uint32_t *>(d_qDC + nq);
        // slots of the last image group beyond nq keep whatever the buffer held: their thresholds never hit
        launch_pq_quant16(ws.lut.as<float>(), pq.d_cent_cache.as<float>(), (uint32_t)pq.m, m16, (uint32_t)nq, cos16 ? 1 : 0, ws.qfrag_g.as<uint16_t>(),
                          d_qM, d_qD, d_qMC, d_qDC, d_qflag, ws.stream);
    }
    Adc16Args image_args(uint64_t g0, uint64_t gn) const {  // what sample and scan share; a round starts on a whole image group (GQ % 56 == 0)
        Adc16Args a{};
        a.codes_t = pq.d_codes_t.as<uint4>();
        a.n = ix.n;
        a.enc_dim = (uint32_t)pq.enc_dim;
        a.m = m16;
        a.img = reinterpret_cast<const uint4 *>(ws.qfrag_g.as<uint8_t>() + (g0 / NQ16) * size_t(m16) * 256);
        a.nq = (uint32_t)gn;
        return a;
    }
    SampleQuant sample(uint64_t g0, uint64_t gn) {
        if (q16 && !cos16 && g_adc16_sample != 1) {  // the sample at the scan's rate, on the scan's tables: quantised sums
            Adc16Args a = image_args(g0, gn);
            a.blk_step = c.step;
            a.s16_out = ws.dense.as<float>();
            a.ld_s = c.ld_s;
            launch_pq_adc16(a, false, true, nw16, ix.num_cu, ws.stream);
            return {d_qM + g0, d_qD + g0, d_qflag + g0};
        }
        pq_dense_adc(ix, ws, g0, gn, c.ld_s, c.step, false);  // exact f32 ADC values
        return {};
    }
    void filter(uint64_t g0, uint64_t gn) {
        if (q16) {
            Adc16Args a = image_args(g0, gn);
            a.qM = d_qM + g0;
            a.qD = d_qD + g0;
            a.qMC = d_qMC + g0;
            a.qDC = d_qDC + g0;
            a.qsq = ws.qsq.as<float>() + g0;
            a.qflag = d_qflag + g0;
            a.tau = c.d_tau + g0;
            a.rows_per_wg = ((ix.n + ix.num_cu - 1) / ix.num_cu + 63) / 64 * 64;
            a.cand = c.cand();
            a.cnt = c.d_hits + g0;
            a.cap = c.cap;
            pq_prof_begin(ix, ws, (gn + NQ16 - 1) / NQ16);
            launch_pq_adc16(a, cos16, false, nw16, ix.num_cu, ws.stream);
            pq.adc16_queries += gn;
        } else {
            AdcArgs a = pq_f32_args(ix, ws, g0, gn);
            a.tau = c.d_tau + g0;
            a.cand = c.cand();
            a.cnt = c.d_hits + g0;
            a.cap = c.cap;
            const uint32_t BQ = pq_f32_plan(ix).BQ;
            pq_prof_begin(ix, ws, (gn + BQ - 1) / BQ);
            launch_pq_adc(a, (uint32_t)pq.n_bits, 1, ix.num_cu, ws.stream);
        }
        ix.prof_end(ws);
    }
    void exact(uint64_t g0, uint64_t gn) {
        if (!q16) return;
        launch_pq_adc_exact(cos16, pq.d_codes.as<uint8_t>(), (uint32_t)pq.enc_dim, (uint32_t)pq.m, ws.lut.as<float>() + g0 * pq.m * pq.kc,
                            pq.d_cent_cache.as<float>(), ws.qsq.as<float>() + g0, c.d_tau + g0, c.cand(), c.d_hits + g0, c.cap, c.d_valid + g0,
                            (uint32_t)gn, ws.stream);
    }
    std::vector<uint64_t> books() {  // (see pq_read_back)
        std::vector<uint64_t> redo = pq_read_back(c, q16);
        if (q16) pq.adc16_redo += redo.size();
        return redo;
    }
};

// ADC scan of the whole code table (pq_table.rs:239-301 through flat_index.rs:96-100): per query the efk smallest
// (ADC distance, row) pairs, sorted by the CandidatePair order, land in ws.keys_a [nq][topk_capacity(efk)];
// ws.qsq holds the query norms afterwards.
static void pq_adc_shortlist(Index &ix, Workspace &ws, const float *d_q, uint64_t nq, uint32_t efk) {
    PQState &pq = ix.pq;
    VDB_REQUIRE(pq.present && pq.n_coded == ix.n, "PQ table does not cover the rows of the index (rebuild it after add)");
    if (efk > 1024) {  // beyond the register-resident select
        pq_adc_shortlist_sorted(ix, ws, d_q, nq, efk);
        return;
    }
    pq_prepare_queries(ix, ws, d_q, nq);
    const uint32_t cape = topk_capacity(efk);
    ws.keys_a.reserve(nq * cape * sizeof(uint64_t));
    ws.keys_b.reserve(nq * cape * sizeof(uint64_t));

    FilterCall c{ix, ws, nq, efk, cape};
    std::vector<uint64_t> redo;
    if (Scan8::plan(c)) {
        redo = pq_filter_rounds<Scan8>(c);
    } else if (Scan4::plan(c)) {
        redo = pq_filter_rounds<Scan4>(c);
    } else {  // a sample that would not pay: the dense path for every query
        const AdcPlan tp = pq_f32_plan(ix);
        const uint64_t GQ = std::max<uint64_t>(tp.BQ, std::min<uint64_t>(64, (size_t(512) << 20) / ((ix.n + tp.nt + 64) * sizeof(float))) / tp.BQ * tp.BQ);
        for (uint64_t g0 = 0; g0 < nq; g0 += GQ) pq_dense_group(ix, ws, g0, std::min<uint64_t>(GQ, nq - g0), efk);
        return;
    }
    for (uint64_t q : redo) pq_dense_group(ix, ws, q, 1, efk);  // overflowed / short / unquantisable: the f32 scan answers
}

// PQTable::create_lookup (pq_table.rs:195-224) and the ADC adapter (pq_table.rs:239-301) over every code row, exported
// as they are computed by the search kernels (k_pq_lut, k_pq_adc dense mode): lut [nq][m*kc], qcache [nq] (0 for L2Sqr,
// |q| for Cosine: PQLookupTable::dist_cache), adc [nq][n].  Host outputs; used by the direct parity tests of a11 / a12.
void pq_export_lookup(Index &ix, Workspace &ws, const float *d_q, uint64_t nq, float *h_lut, float *h_qcache) {
    hipStream_t s = ws.stream;
    PQState &pq = ix.pq;
    VDB_REQUIRE(pq.present, "no PQ table");
    if (nq == 0) return;
    const uint64_t lsz = pq.m * pq.kc;
    pq_prepare_queries(ix, ws, d_q, nq);
    if (h_lut) VDB_HIP(hipMemcpyAsync(h_lut, ws.lut.p, nq * lsz * sizeof(float), hipMemcpyDeviceToHost, s));
    std::vector<float> qs(nq);
    VDB_HIP(hipMemcpyAsync(qs.data(), ws.qsq.p, nq * sizeof(float), hipMemcpyDeviceToHost, s));
    VDB_SYNC(s);
    if (h_qcache)
        for (uint64_t q = 0; q < nq; q++) h_qcache[q] = ix.dist == 1 ? std::sqrt(qs[q]) : 0.0f;
}

void pq_export_adc_all(Index &ix, Workspace &ws, const float *d_q, uint64_t nq, float *h_out) {
    hipStream_t s = ws.stream;
    PQState &pq = ix.pq;
    VDB_REQUIRE(pq.present && pq.n_coded == ix.n, "PQ table does not cover the rows of the index (rebuild it after add)");
    const uint64_t n = ix.n;
    if (nq == 0 || n == 0) return;
    pq_prepare_queries(ix, ws, d_q, nq);
    const uint32_t BQ = pq_f32_plan(ix).BQ;
    const uint64_t ld = pq_dense_ld(ix);
    const uint64_t GQ = std::max<uint64_t>(BQ, std::min<uint64_t>(64, (size_t(512) << 20) / (ld * sizeof(float))) / BQ * BQ);
    ws.dense.reserve(GQ * ld * sizeof(float));
    for (uint64_t g0 = 0; g0 < nq; g0 += GQ) {
        const uint64_t gn = std::min<uint64_t>(GQ, nq - g0);
        pq_dense_adc(ix, ws, g0, gn, ld, 1, false);
        VDB_HIP(hipMemcpy2DAsync(h_out + g0 * n, n * sizeof(float), ws.dense.p, ld * sizeof(float), n * sizeof(float), gn,
                                 hipMemcpyDeviceToHost, s));
        VDB_SYNC(s);
    }
}

// exact distances of the ADC shortlist, in ADC order (the operand order of pq_resort, candidate_pair.rs:102-108):
// ws.keys_a -> ws.keys_b
static void pq_exact_of_shortlist(Index &ix, Workspace &ws, const float *d_q, uint64_t nq, uint32_t efk) {
    hipStream_t s = ws.stream;
    const uint32_t cape = pq_list_ld(efk);
    VDB_HIP(hipMemsetAsync(ws.keys_b.p, 0xff, nq * cape * sizeof(uint64_t), s));
    launch_rerank(ix.d_rows.as<float>(), (uint32_t)ix.dim, d_q, (uint32_t)nq, ix.dist == 0 ? MET_L2_DIRECT : MET_COSINE,
                  ix.d_sq.as<float>(), ws.qsq.as<float>(), ws.keys_a.as<uint64_t>(), ws.keys_b.as<uint64_t>(), efk,
                  cape, s);
}

// ResultSet::pq_resort (candidate_pair.rs:102-108) of the exact keys [nq][ldc] (ADC order, first ncand per row) with set
// capacity ksel, then the outputs.  ksel <= 1024: the wave-resident replay; beyond: the heap replay + a row sort.
void pq_resort_finalize(Index &ix, Workspace &ws, const uint64_t *exact_keys, uint32_t ncand, uint32_t ldc, uint64_t nq,
                               uint32_t ksel, uint64_t k, uint64_t id_offset, uint64_t *d_idx, float *d_dist, uint64_t *d_cnt) {
    hipStream_t s = ws.stream;
    if (ksel <= 1024) {
        const uint32_t capk = topk_capacity(ksel);
        ws.keys_c.reserve(nq * capk * sizeof(uint64_t));
        pq_resort_launch(exact_keys, ncand, ldc, (uint32_t)nq, ksel, ws.keys_c.as<uint64_t>(), s);
        launch_finalize(ws.keys_c.as<uint64_t>(), capk, (uint32_t)nq, ksel, (uint32_t)k, id_offset, d_idx, d_dist, d_cnt, s);
        return;
    }
    const uint32_t ldk = (ksel + 63) & ~63u;
    const size_t tb = sort_rows_temp_bytes(nq, ldk);
    ws.keys_c.reserve(nq * ldk * sizeof(uint64_t));
    ws.lists.reserve(nq * ldk * sizeof(uint64_t) + tb);
    uint64_t *heap = ws.lists.as<uint64_t>();
    launch_resort_big(exact_keys, ncand, ldc, (uint32_t)nq, ksel, heap, ldk, s);
    launch_sort_rows(heap, ws.keys_c.as<uint64_t>(), nq, ldk, heap + nq * ldk, tb, s);
    launch_finalize(ws.keys_c.as<uint64_t>(), ldk, (uint32_t)nq, ksel, (uint32_t)k, id_offset, d_idx, d_dist, d_cnt, s);
}

void flat_knn_pq_device(Index &ix, Workspace &ws, const float *d_q, uint64_t nq, uint64_t k, uint64_t ef,
                        uint64_t *d_idx, float *d_dist, uint64_t *d_cnt) {
    hipStream_t s = ws.stream;
    if (nq == 0) return;
    if (k == 0 || ix.n == 0) {
        VDB_HIP(hipMemsetAsync(d_cnt, 0, nq * sizeof(uint64_t), s));
        return;
    }
    const uint64_t n = ix.n;
    const uint64_t efk64 = std::min<uint64_t>(std::max(ef, k), n);  // ResultSet::new(ef.max(k)) flat_index.rs:96
    const uint64_t ksel64 = std::min<uint64_t>(k, n);
    VDB_REQUIRE(efk64 < (1ull << 31), "knn_pq: ef too large");
    const uint32_t efk = (uint32_t)efk64, ksel = (uint32_t)ksel64;
    if (efk > 1024) {  // any-size path: bound the per-call buffers (efk keys per query, three times)
        const uint64_t qs = std::max<uint64_t>(1, (size_t(1) << 30) / (uint64_t(pq_list_ld(efk)) * 32));
        if (nq > qs) {
            for (uint64_t q0 = 0; q0 < nq; q0 += qs)
                flat_knn_pq_device(ix, ws, d_q + q0 * ix.dim, std::min(qs, nq - q0), k, ef, d_idx + q0 * k, d_dist + q0 * k, d_cnt + q0);
            return;
        }
    }
    if (k > ksel) {
        VDB_HIP(hipMemsetAsync(d_idx, 0, nq * k * sizeof(uint64_t), s));
        VDB_HIP(hipMemsetAsync(d_dist, 0, nq * k * sizeof(float), s));
    }
    pq_adc_shortlist(ix, ws, d_q, nq, efk);
    pq_exact_of_shortlist(ix, ws, d_q, nq, efk);
    pq_resort_finalize(ix, ws, ws.keys_b.as<uint64_t>(), efk, pq_list_ld(efk), nq, ksel, k, ix.id_offset, d_idx, d_dist, d_cnt);
}

// Row-sharded PQ-Flat (the scheme is described at k_pq_export_keys, k_pq.hip): a shard's ADC top-max(ef,k) as two key
// rows per query with GLOBAL row ids
void flat_knn_pq_shard_device(Index &ix, Workspace &ws, const float *d_q, uint64_t nq, uint64_t k, uint64_t ef,
                              uint64_t *d_adc_keys, uint64_t *d_exact_keys) {
    hipStream_t s = ws.stream;
    if (nq == 0) return;
    const uint64_t efg = std::max(ef, k);
    VDB_REQUIRE(efg >= 1 && efg < (1ull << 31), "knn_pq shard: max(ef, k) must be in 1..2^31");
    VDB_REQUIRE(ix.id_offset <= (1ull << 32) && ix.n <= (1ull << 32) - ix.id_offset, "knn_pq shard: global row ids must fit 32 bits");
    if (ix.n == 0) {
        VDB_HIP(hipMemsetAsync(d_adc_keys, 0xff, nq * efg * sizeof(uint64_t), s));
        VDB_HIP(hipMemsetAsync(d_exact_keys, 0xff, nq * efg * sizeof(uint64_t), s));
        return;
    }
    const uint32_t efk = (uint32_t)std::min<uint64_t>(efg, ix.n);
    pq_adc_shortlist(ix, ws, d_q, nq, efk);
    pq_exact_of_shortlist(ix, ws, d_q, nq, efk);
    launch_pq_export_keys(ws.keys_a.as<uint64_t>(), ws.keys_b.as<uint64_t>(), pq_list_ld(efk), efk, (uint32_t)efg, ix.id_offset, d_adc_keys,
                          d_exact_keys, (uint32_t)nq, s);
}

void pq_merge_resort_device(Index &ix, Workspace &ws, const uint64_t *d_adc, const uint64_t *d_exact,
                            uint64_t n_shards, uint64_t nq, uint64_t efg, uint64_t k, uint64_t *d_idx, float *d_dist,
                            uint64_t *d_cnt) {
    hipStream_t s = ws.stream;
    if (nq == 0) return;
    if (k == 0) {
        VDB_HIP(hipMemsetAsync(d_cnt, 0, nq * sizeof(uint64_t), s));
        return;
    }
    VDB_REQUIRE(efg >= k && efg < (1ull << 31), "pq merge: need k <= max(ef, k) < 2^31");
    ws.keys_b.reserve(nq * efg * sizeof(uint64_t));
    launch_pq_shard_merge(d_adc, d_exact, (uint32_t)n_shards, (uint32_t)nq, (uint32_t)efg, ws.keys_b.as<uint64_t>(), s);
    VDB_HIP(hipMemsetAsync(d_idx, 0, nq * k * sizeof(uint64_t), s));
    VDB_HIP(hipMemsetAsync(d_dist, 0, nq * k * sizeof(float), s));
    pq_resort_finalize(ix, ws, ws.keys_b.as<uint64_t>(), (uint32_t)efg, (uint32_t)efg, nq, (uint32_t)k, k, 0, d_idx, d_dist, d_cnt);
}

}  // namespace vdb
