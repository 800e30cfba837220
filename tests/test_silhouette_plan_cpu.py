"""CPU: vdb_silhouette_plan (csrc/silhouette_plan.hpp) -- the layout of a silhouette call against hand-written numbers, and every refusal
text the calls share with it.  No GPU."""
import numpy as np
import pytest


def _plan(*a, **kw):
    import lab_1806_vec_db_amd as vdb

    return vdb.GpuIndex.silhouette_plan(*a, **kw)


def test_layout_against_hand_written_numbers():
    # sizes 1 / 63 / 64 fill one tile of 64 each, 65 two, 129 three: 8 tiles, 512 slots; dim 130 = 9 slices of 16; 512 / 256 = 2 slots per
    # mean segment; scratch = 322 candidates x 12 B + 512 slots x 40 B + 8 tiles x 4 B + 5 clusters x 4 B
    padded, tiles, slices, mean_slots, scratch, first = _plan(400, 130, [1, 63, 64, 65, 129], m_allowed=322)
    assert (padded, tiles, slices, mean_slots) == (512, 8, 9, 2)
    assert first.tolist() == [0, 1, 2, 3, 5, 8]
    assert scratch == 322 * 12 + 512 * 40 + 8 * 4 + 5 * 4
    # one dimension is one slice; 256 slots are one per mean segment; no mask: every row is a candidate
    assert _plan(193, 1, [64, 129])[:4] == (256, 4, 1, 1)
    assert _plan(193, 16, [64, 129])[2] == 1 and _plan(193, 17, [64, 129])[2] == 2 and _plan(193, 2048, [64, 129])[2] == 128
    assert _plan(70000, 8, [64 * 257, 2])[:2] == (64 * 258, 258) and _plan(70000, 8, [64 * 257, 2])[3] == 65


@pytest.mark.parametrize("kw, word", [
    (dict(elem_u8=True), "needs f32 rows"),
    (dict(dim=0), "dim must be in 1 .. 2048"),
    (dict(dim=2049), "dim must be in 1 .. 2048"),
    (dict(n_rows=2 ** 32, sizes=[2, 2]), "2\\^32 rows or more"),
    (dict(flags=2), "unknown flags 2"),
    (dict(cosine=True, flags=1), "VDB_SIL_EUCLIDEAN on a Cosine table"),
    (dict(col=16), "label column 16, the columns are 0 .. 15"),
    (dict(col=3, col_live=False), "label column 3 was never written"),
    (dict(m_allowed=11), "11 allowed rows, the index holds 10"),
    (dict(sizes=[0, 5]), "a cluster size must be in 1"),
    (dict(sizes=[6, 5]), "a cluster size must be in 1"),
    (dict(sizes=[10]), "1 clusters among 10 scored rows, need 2 .. rows - 1"),
    (dict(sizes=[]), "0 clusters among 0 scored rows"),
    (dict(sizes=[1] * 10), "10 clusters among 10 scored rows"),
])
def test_refusal_texts(kw, word):
    import lab_1806_vec_db_amd as vdb

    a = dict(n_rows=10, dim=8, sizes=[5, 5])
    a.update(kw)
    with pytest.raises(vdb.VdbError, match=word):
        _plan(a.pop("n_rows"), a.pop("dim"), a.pop("sizes"), **a)
    assert _plan(10, 8, [2] + [1] * 8)[1] == 9 and _plan(10, 8, [8, 1], cosine=True)[1] == 2  # the edges that are accepted
