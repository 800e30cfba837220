"""GPU: the 8-bit filter kernel (k_flat_gemm8) after its per-unit vector ALU work was cut (profiles/gemm8_unit_valu_ab.txt): the X-ring
refills are addressed scalar base + 32-bit lane offset.  Two more cuts were built and held to these tests as well, then taken out because
they did not show in the kernel time (a unit's accumulators started from a zero C operand in a peeled first chunk; the stage's query number
made behind the hit branch): the dimensions below are those at which the peel or the addressing takes another path.  None of it touches a
key's arithmetic, so every bit must stay:

* the dense keys of every (row, query) pair hash to what the PARENT commit's library wrote (tests/golden/flat_i8_dense_key_sha256.json,
  recorded by tools/record_flat_i8_dense_keys.py), at every dimension where the peel or the addressing takes another path;
* the filter's answers are the oracle's bit for bit and both epilogue forms park the same hits, without and with cooperative sets.

The switches are process-wide: every test puts them back.
"""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, gist_like

pytestmark = pytest.mark.gpu

N_ROWS, N_QUERIES = 6011, 140  # 125 units + 11 rows: a ragged, padded last unit; the second query group has 12 real queries
# (dim, the flat_gemm8_kc values to force): k-blocks / ring -- 128: 2 / ring 2, 192: 3 / ring 3, 320: 5 / ring 5 (one chunk each: the
# peeled chunk is also the last), 256: 4 / two chunks, 960: 15 / rings 5 and 3, 2048: 32 / the image does not fit LDS (chunked, 16 chunks)
DENSE_DIMS = ((128, (0,)), (192, (0,)), (320, (0,)), (256, (0,)), (960, (5, 3)), (2048, (0,)))
METRICS = ("l2sqr", "cosine")
HASH_FILE = os.path.join(GOLDEN, "flat_i8_dense_key_sha256.json")
SWITCHES = ("flat_gemm8_epi", "flat_gemm8_res", "flat_gemm8_kc", "flat_gemm8_burst", "flat_gemm8_nt", "flat_gemm8_coop")


def dense_inputs(dim):
    if dim == 960:
        return gist_like(N_ROWS, dim=dim, seed=3), gist_like(N_QUERIES, dim=dim, seed=4)
    rng = np.random.Generator(np.random.PCG64(1000 + dim))
    base = rng.standard_normal((N_ROWS, dim), dtype=np.float32)
    base *= np.exp(rng.uniform(np.log(0.1), np.log(10.0), size=(N_ROWS, 1))).astype(np.float32)  # row norms over two decades
    return base, rng.standard_normal((N_QUERIES, dim), dtype=np.float32)


def dense_key_hashes(vdb, dim, metric, kcs):
    """{case name: sha256 of the dense keys' bits} for one index: every forced ring, resident and chunked, both epilogue forms"""
    base, qs = dense_inputs(dim)
    ix = vdb.GpuIndex(dim, metric)
    ix.batch_add(base)
    out = {}
    try:
        for kc in kcs:
            for res in (0, 1):
                for epi in (0, 1):
                    ix.set_param("flat_gemm8_kc", kc)
                    ix.set_param("flat_gemm8_res", res)
                    ix.set_param("flat_gemm8_epi", epi)
                    keys = ix.flat_shortlist_keys(qs, 2)[0]
                    assert keys.shape == (N_QUERIES, N_ROWS) and keys.dtype == np.float32
                    out[f"dim{dim}_{metric}_kc{kc}_res{res}_epi{epi}"] = hashlib.sha256(np.ascontiguousarray(keys).view(np.uint32).tobytes()).hexdigest()
    finally:
        for name in SWITCHES:
            ix.set_param(name, 0)
        ix.close()
    return out


@pytest.fixture(scope="module")
def mods():
    import lab_1806_vec_db_amd as vdb
    from oracle import oracle as O
    return vdb, O


@pytest.fixture(scope="module")
def recorded():
    with open(HASH_FILE) as f:
        return json.load(f)["sha256"]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim,kcs", DENSE_DIMS)
def test_dense_keys_are_the_parents(mods, recorded, dim, kcs, metric):
    vdb, _ = mods
    got = dense_key_hashes(vdb, dim, metric, kcs)
    assert len(got) == 4 * len(kcs)
    for name, h in got.items():
        assert recorded[name] == h, name


def test_every_dense_case_is_recorded(recorded):
    names = {f"dim{d}_{m}_kc{kc}_res{res}_epi{epi}" for d, kcs in DENSE_DIMS for m in METRICS for kc in kcs for res in (0, 1) for epi in (0, 1)}
    assert set(recorded) == names and len(names) == 56


def _both_forms(ix, qs, k):
    """one search per epilogue form: the answers and the hits-per-query counters must be the same; returns the answers"""
    out = []
    for epi in (0, 1):
        ix.set_param("flat_gemm8_epi", epi)
        ix.set_param("flat_i8_stats", 1)  # (resets the counters)
        r = ix.flat_knn(qs, k)
        out.append((r, ix.get_stat("flat_i8_hits_sum"), ix.get_stat("flat_i8_hits_max")))
    ix.set_param("flat_gemm8_epi", 0)
    for x, y in zip(out[0][0], out[1][0]):
        np.testing.assert_array_equal(x, y)
    assert out[0][1:] == out[1][1:] and out[0][1] > 0, (out[0][1:], out[1][1:])
    return out[0][0]


def _check(got, oi, od, oc):
    idx, d, cnt = got
    assert cnt.tolist() == oc.tolist()
    assert np.array_equal(idx.astype(np.uint64), oi.astype(np.uint64))
    assert np.array_equal(d.view(np.uint32), od.view(np.uint32))


@pytest.mark.parametrize("dim", [192, 256, 960])
def test_filter_answers_without_sets(mods, dim):
    """two query groups over 20 011 rows (417 units on 256 workgroups: most waves one unit, a ragged last one; too few units for sets),
    resident and chunked forms"""
    vdb, O = mods
    n, nq = 20011, 140
    if dim == 960:
        base, qs = gist_like(n, seed=51), gist_like(nq, seed=52)
    else:
        rng = np.random.Generator(np.random.PCG64(2000 + dim))
        base, qs = rng.standard_normal((n, dim), dtype=np.float32), rng.standard_normal((nq, dim), dtype=np.float32)
    oi, od, oc = O.flat_knn_batch(base, qs, 10, O.L2SQR, nthreads=8)
    ix = vdb.GpuIndex(dim, "l2sqr")
    ix.batch_add(base)
    ix.set_flat_mode(2)
    ix.set_param("flat_i8", 2)
    try:
        for res in (0, 1):
            ix.set_param("flat_gemm8_res", res)
            _check(_both_forms(ix, qs, 10), oi, od, oc)
            assert ix.get_stat("flat_gemm8_coop_sets") <= 1
        assert ix.get_stat("flat_i8_queries") == 4 * nq
    finally:
        for name in SWITCHES:
            ix.set_param(name, 0)
        ix.close()


def test_filter_answers_with_cooperative_sets(mods):
    """eight query groups over 99 001 rows at dim 192 (2063 units: sets of 8, the hit buffer handed over in blocks of units)"""
    vdb, O = mods
    n, nq, dim = 99001, 1024, 192
    rng = np.random.Generator(np.random.PCG64(77))
    base, qs = rng.standard_normal((n, dim), dtype=np.float32), rng.standard_normal((nq, dim), dtype=np.float32)
    ix = vdb.GpuIndex(dim, "l2sqr")
    ix.batch_add(base)
    ix.set_flat_mode(2)
    try:
        got = _both_forms(ix, qs, 10)
        assert ix.get_stat("flat_gemm8_coop_sets") == 8
        sel = np.arange(5, nq, 21)  # 49 queries, every group
        oi, od, oc = O.flat_knn_batch(base, qs[sel], 10, O.L2SQR, nthreads=8)
        _check(tuple(x[sel] for x in got), oi, od, oc)
    finally:
        for name in SWITCHES:
            ix.set_param(name, 0)
        ix.close()
