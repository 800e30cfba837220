"""CPU: the plain references of merge_ref.py against the library's host merges (merge_topk / vdb_merge_topk, pq_merge_resort /
vdb_pq_merge_resort) on the constructed inputs the GPU tests feed to the device merges -- the references and the inputs are checked
here before a GPU is involved.  Bit-exact: ids, counts, distance bit patterns.  The host merge carries 64-bit ids; the device merges
do not (test_merge_topk_gpu.py)."""
import numpy as np
import pytest

import merge_ref as M

FLAT_CASES = ([(S, k, nq) for S, k in M.SHAPES_K64 + M.SHAPES_LISTS for nq in M.NQS] + [M.SHAPE_LARGEST + (2,), (4, 3, 5)])


def test_order_image_is_the_documented_order():
    bits = np.array([0xFF800000, 0xBFC00000, 0x80000001, 0x80000000, 0x00000000, 0x00000001, 0x3F800000, 0x7F7FFFFF, 0x7F800000,
                     0x7FC00000, 0xFFC00123, 0x7F800001], dtype=np.uint32)  # -inf, -1.5, -subnormal, -0, +0, subnormal, 1, FLT_MAX, inf, NaNs
    img = M.order_image(bits.view(np.float32)).tolist()
    assert img[3] == img[4] == 0x80000000  # -0 is +0
    assert img[9] == img[10] == img[11] == 0xFFC00000  # one NaN, and it is not the distance word of PAIR_NONE
    assert img[:3] == sorted(img[:3]) and img[2] < img[3] and img[4:10] == sorted(img[4:10]) and img[8] < img[9]
    assert len(set(img)) == len(img) - 3
    back = M.image_to_f32(np.array(img, dtype=np.uint64)).view(np.uint32).tolist()
    assert back[:3] == bits[:3].tolist() and back[3] == 0 and back[4:9] == bits[4:9].tolist() and back[9:] == [0x7FC00000] * 3


def test_constructed_lists_hold_what_they_promise():
    S, nq, k = 7, 33, 9
    d, ids, counts = M.flat_case(S, nq, k, seed=5)
    img = M.order_image(d)
    seen_bits, tie_across, not_id_order = set(), False, False
    for q in range(nq):
        c = np.minimum(counts[:, q], k).astype(int)
        used = np.concatenate([ids[s, q, :c[s]] for s in range(S)])
        assert len(set(used.tolist())) == len(used) and (used <= M.ID_TOP).all()
        for s in range(S):
            key = [(int(a), int(b)) for a, b in zip(img[s, q, :c[s]], ids[s, q, :c[s]])]
            assert key == sorted(key)  # ascending by (distance, id)
            assert (d[s, q, c[s]:].view(np.uint32) == M.NEG_INF_BITS).all()  # poison past the count ...
            assert not set(ids[s, q, c[s]:].tolist()) & set(used.tolist())  # ... under ids no list uses
            seen_bits |= set(d[s, q, :c[s]].view(np.uint32).tolist())
        if len(used):
            at = [(s, j) for s in range(S) for j in range(c[s]) if ids[s, q, j] == M.ID_TOP]
            assert len(at) == 1 and np.isnan(d[at[0][0], q, at[0][1]])  # the pair (NaN, 2^32 - 1)
        firsts = [(int(img[s, q, 0]), s) for s in range(S) if c[s]]
        tie_across |= len(firsts) > len({f[0] for f in firsts})
        heads = [int(ids[s, q, 0]) for s in range(S) if c[s]]
        not_id_order |= heads != sorted(heads)
    assert seen_bits == set(M.VALUE_BITS.tolist())
    assert tie_across and not_id_order
    totals = np.minimum(counts, k).sum(axis=0)
    assert (totals == 0).any() and ((totals > 0) & (totals < k)).any() and (counts > k).any()
    assert set(np.minimum(counts, k).reshape(-1).tolist()) == {0, 1, k - 1, k}
    # kind 0: the highest shard holds the smallest pairs
    q = 0
    last = max(s for s in range(S) if counts[s, q])
    assert (int(img[last, q, 0]), int(ids[last, q, 0])) == min((int(img[s, q, 0]), int(ids[s, q, 0])) for s in range(S) if counts[s, q])
    # the expected answer returns the pair (NaN, 2^32 - 1) as an entry where fewer than k pairs exist
    ei, ed, ec = M.merge_topk_ref(d, ids, counts, k)
    q = 2
    assert 0 < ec[q] < k and ei[q, int(ec[q]) - 1] == M.ID_TOP and ed[q, int(ec[q]) - 1:int(ec[q])].view(np.uint32)[0] == 0x7FC00000
    assert not ei[q, int(ec[q]):].any() and not ed[q, int(ec[q]):].view(np.uint32).any()  # pads: id 0, +0.0
    assert not (ed.view(np.uint32) == M.NEG_INF_BITS).any()  # no poison


@pytest.mark.parametrize("id_base", [0, 1 << 40])
@pytest.mark.parametrize("S,k,nq", FLAT_CASES)
def test_reference_equals_host_merge(S, k, nq, id_base):
    from lab_1806_vec_db_amd import merge_topk

    d, ids, counts = M.flat_case(S, nq, k, seed=1000 * S + k, id_base=id_base)
    exp = M.merge_topk_ref(d, ids, counts, k)
    M.same(merge_topk(d, ids, counts, k), exp, (S, k, nq, id_base))
    if id_base:  # the host merge carries 64-bit ids: every returned id lies above 2^40
        assert all((exp[0][q, :int(c)] >= id_base).all() for q, c in enumerate(exp[2]))


def test_host_merge_keeps_64_bit_ids():
    from lab_1806_vec_db_amd import merge_topk

    big = (1 << 32) + 5
    d = np.array([[[0.5, 0.5]], [[0.5, 1.0]]], dtype=np.float32)
    ids = np.array([[[big, big + 2]], [[5, (1 << 63) + 1]]], dtype=np.uint64)
    oi, od, oc = merge_topk(d, ids, np.array([[2], [2]], dtype=np.uint64), 2)
    assert oi.tolist() == [[5, big]] and od.tolist() == [[0.5, 0.5]] and oc.tolist() == [2]
    oi, _, _ = merge_topk(d, ids, np.array([[0], [2]], dtype=np.uint64), 2)
    assert oi.tolist() == [[5, (1 << 63) + 1]]


def test_host_merge_of_zero_shards_writes_empty_results():
    from lab_1806_vec_db_amd import merge_topk

    oi, od, oc = merge_topk(np.zeros((0, 3, 4), dtype=np.float32), np.zeros((0, 3, 4), dtype=np.uint64), np.zeros((0, 3), dtype=np.uint64), 4)
    assert not oi.any() and not od.view(np.uint32).any() and not oc.any()


def test_constructed_pq_rows_hold_what_they_promise():
    S, nq, efk, k = 4, 7, 100, 10
    adc, ex = M.pq_case(S, nq, efk, k, seed=3)
    none = np.uint64(M.PAIR_NONE)
    lengths = set()
    for q in range(nq):
        valid = adc[:, q, :] != none
        assert np.array_equal(valid, ex[:, q, :] != none)
        for s in range(S):
            n = int(valid[s].sum())
            lengths.add(n)
            assert valid[s, :n].all() and (np.diff(adc[s, q, :n].astype(object)) > 0).all()  # ascending, the tail is PAIR_NONE
        low = (adc[:, q, :][valid] & np.uint64(0xFFFFFFFF))
        assert len(set(low.tolist())) == len(low)  # ids unique over the shards
        assert np.array_equal(low, ex[:, q, :][valid] & np.uint64(0xFFFFFFFF))
        if q % 3 == 2:
            assert valid.sum() < k
        if q % 3 == 1:
            assert (valid.sum(axis=1) == 0).sum() == 1  # a shard that is entirely PAIR_NONE
            words = [set((adc[s, q, :] >> np.uint64(32)).tolist()) for s in range(S) if valid[s].any()]
            assert set.intersection(*words)  # ADC distances tied across shards
    assert len(lengths) >= 4
    assert len(set((ex[ex != none] >> np.uint64(32)).tolist())) == 4


@pytest.mark.parametrize("nq", M.PQ_NQS)
@pytest.mark.parametrize("S,efk,k", M.PQ_SHAPES)
def test_pq_reference_equals_host_merge(S, efk, k, nq):
    from lab_1806_vec_db_amd.index import pq_merge_resort

    adc, ex = M.pq_case(S, nq, efk, k, seed=100 * S + efk + k)
    M.same(pq_merge_resort(adc, ex, k), M.pq_merge_resort_ref(adc, ex, k), (S, efk, k, nq))


def test_pq_replay_depends_on_the_merged_order():
    """two shards, capacity 1, equal exact distances: the pair that comes first in the merged ADC order stays (strict <), whichever
    shard holds it -- an answer that only the merged order can give"""
    from lab_1806_vec_db_amd.index import pq_merge_resort

    one = int(M.order_image(np.array([1.0], dtype=np.float32))[0]) << 32
    for first, second in ((7, 3), (3, 7)):
        adc = np.array([[[one | first, M.PAIR_NONE]], [[(one + (1 << 32)) | second, M.PAIR_NONE]]], dtype=np.uint64)
        ex = np.array([[[one | first, M.PAIR_NONE]], [[one | second, M.PAIR_NONE]]], dtype=np.uint64)
        for a, e in ((adc, ex), (adc[::-1].copy(), ex[::-1].copy())):
            exp = M.pq_merge_resort_ref(a, e, 1)
            assert exp[0].tolist() == [[first]] and exp[2].tolist() == [1]
            M.same(pq_merge_resort(a, e, 1), exp)


def test_host_pq_merge_refuses_efk_below_k():
    from lab_1806_vec_db_amd import VdbError
    from lab_1806_vec_db_amd.index import pq_merge_resort

    adc, ex = M.pq_case(2, 1, 4, 4, seed=1)
    with pytest.raises(VdbError, match="efk"):
        pq_merge_resort(adc, ex, 5)
