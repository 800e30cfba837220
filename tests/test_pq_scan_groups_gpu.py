"""The threshold-filter ADC shortlist (FlatIndex::knn_pq, flat_index.rs:84-104) past its first ROUND of queries, and its books.

The quantised scans take their queries in rounds of GQ (4-bit codes: 1792, 8-bit codes: 2048 at this table size), and every
buffer of a round is addressed from the round's first query g0: thresholds, hit counts, the query images (g0 / 8 or g0 / 7 image
groups), the lookup tables.  No other test sends a call more than GQ queries, so g0 > 0 runs only here.  One table shape for all
cases -- 66 000 rows, dim 32, m = 8, ef = 100, k = 10: 65 row blocks of 1024, every 4th sampled (17 blocks, 17 408 sampled rows),
threshold = the 100th smallest sampled value; n >= 65 536 puts both code widths on their quantised scans.

The second half pins which counters each path keeps when it hands queries to the f32 scan: the 4-bit path counts them in
pq_adc16_redo alone, the 8-bit path in pq_q8_overflow / pq_q8_short alone (and leaves overflowed lists out of pq_q8_hits_sum / _max).
"""
import numpy as np
import pytest

from conftest import gist_like

pytestmark = pytest.mark.gpu

N, DIM, M, K, EF = 66000, 32, 8, 10, 100
STATS = ("pq_adc16_queries", "pq_adc16_redo", "pq_q8_overflow", "pq_q8_short", "pq_q8_hits_sum", "pq_q8_hits_max")


@pytest.fixture(scope="module")
def mods():
    import lab_1806_vec_db_amd as vdb
    from oracle import oracle as O
    return vdb, O


@pytest.fixture(scope="module")
def base():
    b = gist_like(N, dim=DIM, seed=51)
    b[N // 2:N // 2 + 20] = b[:20]  # equal code rows: ADC ties that the (value, id) order breaks
    return b


@pytest.fixture(scope="module")
def queries():
    return gist_like(2052, dim=DIM, seed=52)


@pytest.fixture(scope="module")
def tables(mods, base):
    """(index, oracle table) per (metric, code width), built once for the module."""
    vdb, O = mods
    made = {}

    def get(dist, kind, n_bits):
        if (dist, n_bits) not in made:
            ix = vdb.GpuIndex(DIM, dist)
            ix.batch_add(base)
            ix.pq_build(n_bits=n_bits, m=M, train_n=400, max_iter=4, seed=5)
            pq = ix.pq_export()
            opq = O.PQ.from_centroids(DIM, M, n_bits, kind, pq["centroids"])
            opq.set_codes(pq["codes"])
            made[(dist, n_bits)] = (ix, opq)
        return made[(dist, n_bits)]

    yield get
    for ix, _ in made.values():
        ix.close()


def _stats(ix):
    return {s: ix.get_stat(s) for s in STATS}


def _f32_scan(ix, qs):
    ix.set_param("pq_adc16", 1)
    try:
        return ix.knn_pq(qs, K, EF)
    finally:
        ix.set_param("pq_adc16", 0)


def _check_oracle(O, base, opq, kind, qs, res, rows):
    for q in rows:
        oi, od = O.flat_knn_pq(base, opq, qs[q], K, EF, kind)
        assert res[0][q, :len(oi)].tolist() == oi.tolist(), q
        assert np.array_equal(res[1][q, :len(od)], od), q


@pytest.mark.parametrize("dist,kind,sample16", [("l2sqr", 0, 0), ("l2sqr", 0, 1), ("cosine", 1, 0)])
def test_4_bit_scan_second_round(mods, base, queries, tables, dist, kind, sample16):
    """1800 queries = one round of 1792 and one of 8 on the 16-bit tables (k_pq_adc16, 8 queries per image group under L2Sqr, 7
    under Cosine): the same three arrays as the f32 scan (pq_adc16 = 1, rounds of 64), the oracle's answers on both sides of the
    round boundary, and all 1800 counted as scanned on the quantised tables.  L2Sqr with the sample on the quantised tables
    (pq_sample16 = 0) and on the f32 tables (1); Cosine always samples in f32."""
    vdb, O = mods
    ix, opq = tables(dist, kind, 4)
    qs = queries[:1800]
    ix.set_param("pq_sample16", sample16)
    try:
        s0 = _stats(ix)
        a = ix.knn_pq(qs, K, EF)
        s1 = _stats(ix)
    finally:
        ix.set_param("pq_sample16", 0)
    b = _f32_scan(ix, qs)
    s2 = _stats(ix)
    assert s1["pq_adc16_queries"] - s0["pq_adc16_queries"] == 1800
    assert s2["pq_adc16_queries"] == s1["pq_adc16_queries"]
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    _check_oracle(O, base, opq, kind, qs, a, (0, 1791, 1792, 1799))


def test_8_bit_scan_second_round(mods, base, queries, tables):
    """2052 queries = one round of 2048 and one of 4, on each of the three 8-bit scans (pq_adc8_sliced = 0: k_pq_adc8x16, 1:
    k_pq_adc8, 2: k_pq_adc16x8): identical answers, identical to the f32 scan, the oracle's on both sides of the boundary, 2052
    counted per quantised call."""
    vdb, O = mods
    ix, opq = tables("l2sqr", 0, 8)
    qs = queries[:2052]
    res = []
    try:
        for variant in (0, 1, 2):
            ix.set_param("pq_adc8_sliced", variant)
            ran = ix.get_stat("pq_adc16_queries")
            res.append(ix.knn_pq(qs, K, EF))
            assert ix.get_stat("pq_adc16_queries") - ran == 2052, variant
    finally:
        ix.set_param("pq_adc8_sliced", 0)
    ran = ix.get_stat("pq_adc16_queries")
    b = _f32_scan(ix, qs)
    assert ix.get_stat("pq_adc16_queries") == ran
    for variant in (0, 1, 2):
        assert all(np.array_equal(x, y) for x, y in zip(res[variant], b)), variant
    _check_oracle(O, base, opq, 0, qs, res[0], (0, 2047, 2048, 2051))


def _degenerate_queries(base):
    """the 12 queries of test_quantised_scan_fallbacks_on_degenerate_queries at this dim"""
    qs = gist_like(12, dim=DIM, seed=42)
    qs[1, 5] = np.nan
    qs[2, :] = 0.0
    qs[3, 7] = 3.0e19
    qs[4, :] = 1.0e-30
    qs[5] = base[123]
    qs[6, 9] = -np.inf
    qs[8] = -base[77]
    qs[9] = base[5] * 1e-25
    return qs


def test_4_bit_scan_books(mods, base, tables):
    """Queries 1, 3 and 6 have a NaN / +inf in their tables: flagged, threshold +inf, all 66 000 rows hit, the list (cap <= 65 536)
    overflows, the f32 scan answers (this table: exactly those 3).  The 4-bit path counts what it hands on in pq_adc16_redo and
    touches none of the 8-bit counters."""
    vdb, O = mods
    ix, _ = tables("l2sqr", 0, 4)
    qs = _degenerate_queries(base)
    s0 = _stats(ix)
    ix.knn_pq(qs, K, EF)
    s1 = _stats(ix)
    d = {s: s1[s] - s0[s] for s in STATS}
    print("4-bit books:", d)
    assert d["pq_adc16_queries"] == 12
    assert 3 <= d["pq_adc16_redo"] <= 12
    assert all(s1[s] == s0[s] for s in ("pq_q8_overflow", "pq_q8_short", "pq_q8_hits_sum", "pq_q8_hits_max"))


def test_8_bit_scan_books(mods, base, tables):
    """The same queries on 8-bit codes: handed on as overflowed or short lists, counted in pq_q8_overflow + pq_q8_short (this table:
    0 + 3 -- the sixteen-query scan parks nothing for a flagged query, so its list comes out short); pq_adc16_redo is the 4-bit
    path's and stays."""
    vdb, O = mods
    ix, _ = tables("l2sqr", 0, 8)
    qs = _degenerate_queries(base)
    s0 = _stats(ix)
    ix.knn_pq(qs, K, EF)
    s1 = _stats(ix)
    d = {s: s1[s] - s0[s] for s in STATS}
    print("8-bit books:", d)
    assert d["pq_adc16_queries"] == 12
    assert 3 <= d["pq_q8_overflow"] + d["pq_q8_short"] <= 12
    assert d["pq_adc16_redo"] == 0
