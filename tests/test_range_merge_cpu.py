"""CPU: the host merge of range results (range_merge / vdb_range_merge) against a Python sort of the union.

Every shard hands in a CSR result (lims from 0, pairs per query ascending by (distance, id)); the merged list of a query is the
union in the same order -- f32_orderable(distance) (-0.0 == +0.0), then the 64-bit id -- cut after `limit` pairs.  Bit-exact:
offsets, ids and the distances' bit patterns (a pair keeps the distance it came with)."""
import numpy as np
import pytest


def _orderable(d):
    u = (np.asarray(d, dtype=np.float32) + np.float32(0)).view(np.uint32).astype(np.uint64)  # -0 -> +0
    return np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)


def _sorted_pairs(ids, ds):
    order = sorted(range(len(ids)), key=lambda j: (int(_orderable(ds[j:j + 1])[0]), int(ids[j])))
    return np.asarray(ids, dtype=np.uint64)[order], np.asarray(ds, dtype=np.float32)[order]


def _pack(lists, nq):
    """lists[s][q] = (ids, dists) sorted -> (lims [S][nq + 1], ids [S][stride], dists [S][stride])"""
    S = len(lists)
    lims = np.zeros((S, nq + 1), dtype=np.uint64)
    for s in range(S):
        for q in range(nq):
            lims[s, q + 1] = lims[s, q] + len(lists[s][q][0])
    stride = max(int(lims[:, nq].max()), 1)
    ids = np.zeros((S, stride), dtype=np.uint64)
    ds = np.zeros((S, stride), dtype=np.float32)
    for s in range(S):
        for q in range(nq):
            ids[s, int(lims[s, q]):int(lims[s, q + 1])] = lists[s][q][0]
            ds[s, int(lims[s, q]):int(lims[s, q + 1])] = lists[s][q][1]
    return lims, ids, ds


def _expect(lists, nq, limit):
    lims, oi, od = [0], [], []
    for q in range(nq):
        ids = np.concatenate([l[q][0] for l in lists])
        ds = np.concatenate([l[q][1] for l in lists])
        i, d = _sorted_pairs(ids, ds)
        cut = len(i) if limit is None else min(limit, len(i))
        oi.append(i[:cut])
        od.append(d[:cut])
        lims.append(lims[-1] + cut)
    return np.array(lims, dtype=np.uint64), np.concatenate(oi), np.concatenate(od)


def _same(got, exp, what):
    assert np.array_equal(got[0], exp[0]), (what, got[0], exp[0])
    assert got[1].dtype == np.uint64 and np.array_equal(got[1], exp[1]), what
    assert got[2].dtype == np.float32 and np.array_equal(got[2].view(np.uint32), exp[2].view(np.uint32)), what


def _random_lists(S, nq, seed):
    """few distinct distances (ties within and across shards, -0.0 and 0.0 among them), ids unique over all shards and mostly above 2^32;
    shard 1 (if any) is entirely empty, query 4 is empty on every shard"""
    rng = np.random.default_rng(seed)
    values = np.array([-0.0, 0.0, 0.25, 0.5, 0.5000001, 1.0, 3.5, np.inf], dtype=np.float32)
    lists = []
    for s in range(S):
        per_q = []
        for q in range(nq):
            n = 0 if (q == 4 or (s == 1 and S > 1)) else int(rng.integers(0, 40))
            ids = (rng.permutation(1000)[:n].astype(np.uint64) * np.uint64(S) + np.uint64(s)) + (np.uint64((s + 1) % 3) << np.uint64(33))
            per_q.append(_sorted_pairs(ids, values[rng.integers(0, len(values), n)]))
        lists.append(per_q)
    return lists


@pytest.mark.parametrize("S", [1, 2, 3, 8])
def test_range_merge_equals_sorted_union(S):
    from lab_1806_vec_db_amd import range_merge

    nq = 9
    lists = _random_lists(S, nq, 100 + S)
    lims, ids, ds = _pack(lists, nq)
    assert S == 1 or lims[1, nq] == 0
    assert ids.max() > (1 << 32)
    full = _expect(lists, nq, None)
    union0 = int(full[0][1])
    assert union0 > 0 and int(full[0][5]) == int(full[0][4])  # query 4 is empty everywhere
    longest = int(np.diff(full[0].astype(np.int64)).max())
    for limit in (None, 1, max(union0 - 1, 1), union0, union0 + 1, longest, longest + 7):
        _same(range_merge(lims, ids, ds, limit), _expect(lists, nq, limit), (S, limit))
    # the same shards as a sequence of per-shard arrays
    seq_i = [ids[s, :int(lims[s, nq])] for s in range(S)]
    seq_d = [ds[s, :int(lims[s, nq])] for s in range(S)]
    _same(range_merge(lims, seq_i, seq_d, 5), _expect(lists, nq, 5), (S, "sequence"))


def test_equal_distances_across_shards_smaller_id_first():
    from lab_1806_vec_db_amd import range_merge

    big = np.uint64(1) << np.uint64(40)
    a = (np.array([7, big + np.uint64(1)], dtype=np.uint64), np.array([1.5, 1.5], dtype=np.float32))
    b = (np.array([3, big], dtype=np.uint64), np.array([1.5, 1.5], dtype=np.float32))
    lims, ids, ds = _pack([[a], [b]], 1)
    ol, oi, od = range_merge(lims, ids, ds)
    assert ol.tolist() == [0, 4] and oi.tolist() == [3, 7, int(big), int(big) + 1] and od.tolist() == [1.5] * 4
    ol, oi, od = range_merge(lims, ids, ds, 3)
    assert ol.tolist() == [0, 3] and oi.tolist() == [3, 7, int(big)]


def test_negative_zero_orders_like_zero_and_keeps_its_bits():
    from lab_1806_vec_db_amd import range_merge

    a = (np.array([5, 9], dtype=np.uint64), np.array([-0.0, 0.0], dtype=np.float32))
    b = (np.array([2, 7], dtype=np.uint64), np.array([0.0, -0.0], dtype=np.float32))
    c = (np.array([1], dtype=np.uint64), np.array([-1.0], dtype=np.float32))
    lims, ids, ds = _pack([[a], [b], [c]], 1)
    ol, oi, od = range_merge(lims, ids, ds)
    assert oi.tolist() == [1, 2, 5, 7, 9]
    assert od.view(np.uint32).tolist() == [0xBF800000, 0, 0x80000000, 0x80000000, 0]


def test_all_empty_and_no_queries():
    from lab_1806_vec_db_amd import range_merge

    ol, oi, od = range_merge(np.zeros((3, 5), dtype=np.uint64), np.zeros((3, 1), dtype=np.uint64), np.zeros((3, 1), dtype=np.float32))
    assert ol.tolist() == [0] * 5 and len(oi) == 0 and len(od) == 0
    ol, oi, od = range_merge(np.zeros((2, 1), dtype=np.uint64), np.zeros((2, 1), dtype=np.uint64), np.zeros((2, 1), dtype=np.float32))
    assert ol.tolist() == [0] and len(oi) == 0


def test_inconsistent_lims_are_errors():
    import lab_1806_vec_db_amd as vdb

    ids = np.arange(8, dtype=np.uint64).reshape(2, 4)
    ds = np.zeros((2, 4), dtype=np.float32)
    good = np.array([[0, 2, 4], [0, 1, 3]], dtype=np.uint64)
    assert vdb.range_merge(good, ids, ds)[0].tolist() == [0, 3, 7]
    for bad in ([[1, 2, 4], [0, 1, 3]],      # does not start at 0
                [[0, 3, 2], [0, 1, 3]],      # decreases
                [[0, 2, 4], [0, 1, 5]],      # more pairs than the shard's block holds
                [[0, 2, 2 ** 63], [0, 1, 3]]):
        with pytest.raises(vdb.VdbError, match="range merge"):
            vdb.range_merge(np.array(bad, dtype=np.uint64), ids, ds)
    for limit in (0, -1):
        with pytest.raises(ValueError):
            vdb.range_merge(good, ids, ds, limit)
    # one shard: its lims must fit its block like any other's
    one_i, one_d = np.arange(4, dtype=np.uint64).reshape(1, 4), np.zeros((1, 4), dtype=np.float32)
    assert vdb.range_merge(np.array([[0, 2, 4]], dtype=np.uint64), one_i, one_d)[0].tolist() == [0, 2, 4]
    for bad in ([[0, 2, 6]], [[0, 2, 3_000_000]], [[1, 2, 4]], [[0, 3, 2]]):
        with pytest.raises(vdb.VdbError, match="range merge"):
            vdb.range_merge(np.array(bad, dtype=np.uint64), one_i, one_d)
