"""CPU: tests/dbscan_ref.py, the reference of the density clustering, on its hand cases, whose answers are written down by hand."""
import pytest

import dbscan_ref as R


@pytest.mark.parametrize("name,n,min_samples,edges,label,kind", R.HAND_CASES, ids=[c[0] for c in R.HAND_CASES])
def test_hand_cases(name, n, min_samples, edges, label, kind):
    src, lists = R.lists_of_edges(n, edges)
    got = R.dbscan_ref(n, src, *R.csr(lists), min_samples, id_offset=100)
    assert got[0].tolist() == [v if v >= R.ROW_NOISE else v + 100 for v in label] and got[1].tolist() == kind
    assert got[2] == {"clusters": len({v for v in label if v < R.ROW_NOISE}), "core": kind.count(3), "border": kind.count(2), "noise": kind.count(1), "pairs": 2 * len(edges)}
