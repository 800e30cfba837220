"""GPU: the two score stages alone (GpuIndex.lof_lists_device; k_lof_lrd / k_lof_score of k_outlier.hip) over hand-made graphs against
tests/lof_ref.py: kdist bit for bit, lrd and lof at relative 1e-6 (lof_ref.RTOL says why)."""
import numpy as np
import pytest
import torch

import lab_1806_vec_db_amd as vdb
import lof_ref as R
from test_flat_dups_gpu import _index

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(-7.5)


@pytest.fixture(scope="module")
def ix():
    made = _index("l2sqr", np.ones((3, 4), dtype=np.float32))  # (lends its device and stream: the rows are never looked at)
    yield made
    made.close()


def _run(ix, nbr, nd, cnt, k=None):
    """-> (kdist, lrd, lof) f32 [m]; sentinel-filled outputs kept in _run.last even when the call raises"""
    m, k = len(cnt), nd.shape[1] if k is None else k
    t = [torch.from_numpy(np.concatenate([np.asarray(a).ravel(), np.zeros(1, dtype=a.dtype)])).cuda()  # (never an empty tensor)
         for a in (nbr.astype(np.int64).astype(np.uint32).view(np.int32), nd.astype(np.float32), np.asarray(cnt).astype(np.int64).astype(np.uint32).view(np.int32))]
    out = [torch.full((m + 1,), float(SENTINEL), dtype=torch.float32, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    try:
        ix.lof_lists_device(*(x.data_ptr() for x in t), m, k, *(o.data_ptr() for o in out))
    finally:
        _run.last = [o.cpu().numpy() for o in out]
    assert all(o[m] == SENTINEL for o in _run.last)  # nothing behind the m-th item
    return [o[:m] for o in _run.last]


@pytest.mark.parametrize("m", (1, 2, 65, 5000))
@pytest.mark.parametrize("k", (1, 2, 3, 20, 32, 33, 63, 64, 65, 200))  # every lane-group width, the wave boundary, the strided form
def test_ragged_graph_against_the_reference(ix, k, m):
    rng = np.random.default_rng(1000 * k + m)
    nd = rng.random((m, k), dtype=np.float32) + np.float32(0.01)
    if m < 65:
        nbr, cnt = rng.integers(0, m, (m, k)), rng.integers(0, k + 1, m)
    else:  # NaN spreads to whoever lists it: items 0 .. 2 carry one and only items 2 .. 4 list them, so that most scores stay numbers
        nbr, cnt = rng.integers(3, m, (m, k)), rng.integers(1, k + 1, m)  # ragged: short lists ..
        cnt[0], nd[1, 0], nbr[2, 0], nbr[3, 0], nbr[4, 0] = 0, np.nan, 0, 2, 1  # .. an empty one, a NaN distance, their listers
        cnt[7], nd[7, k // 2], nd[m // 3, :] = k, np.inf, 0.0  # a +inf distance in a full list, a list at distance 0
    cnt[-1] = k  # .. and a full one
    want = R.of_lists(nbr, nd, cnt)
    got = _run(ix, nbr, nd, cnt)
    assert np.array_equal(got[0].view(np.uint32)[cnt > 0], want[0].view(np.uint32)[cnt > 0]) and np.isnan(got[0][cnt == 0]).all()  # bit for bit
    R.close(got[1], want[1]), R.close(got[2], want[2])
    assert m < 65 or (5 <= np.isnan(want[2]).sum() <= m // 4 and want[1][7] == 0 and np.isinf(want[2]).any())  # (a condition on the input)
    again = _run(ix, nbr, nd, cnt)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, again))  # two calls: the same bits
    zero = _run(ix, nbr, np.zeros_like(nd), np.full(m, k))  # all-zero distances: every reach is 0
    assert (zero[0] == 0).all() and (zero[1] == np.float32(1e10)).all() and (zero[2] == 1).all()


@pytest.mark.parametrize("k", (3, 65))
@pytest.mark.parametrize("what", ("id", "count", "k"))
def test_a_bad_graph_is_refused_with_the_outputs_untouched(ix, k, what):
    m = 70
    nbr, nd, cnt = np.arange(m * k).reshape(m, k) % m, np.ones((m, k), dtype=np.float32), np.full(m, k)
    _run(ix, nbr, nd, cnt)  # (accepted as it stands)
    if what == "id":
        nbr[m - 1, k - 1] = m  # the last counted slot of the last list names item m
    elif what == "count":
        cnt[m // 2] = k + 1
    with pytest.raises(vdb.VdbError, match="k must be" if what == "k" else "lof lists"):
        _run(ix, nbr, nd, cnt, k=1024 if what == "k" else None)
    assert all((o == SENTINEL).all() for o in _run.last)
    nbr[m - 1, k - 1], cnt[m - 1], cnt[m // 2] = m, k - 1, k  # the same id behind the count is not looked at
    _run(ix, nbr, nd, cnt)
