"""GPU: the driver the four Flat list re-rankers share (csrc/flat_rerank.hip: grouped, diversified, by-example and fused search) -- a call of
several queries answers every query as the same call made with that query alone, bit for bit, without masks and with two masks of
which one is empty.  300 rows x dim 8, 5 queries.

What decides the sub-chunks of a call is LIST_BUDGET (csrc/list_plan.hpp), and no form has a parameter that lowers it, so sub-chunks of
1 and of 2 queries cannot be asked for.  At this size the grouped, diversified and by-example calls are ONE sub-chunk: their lists would
have to pass 256 MiB (22 million list entries) before a second one exists, which no quick test reaches, and their test files hold no such
shape either.  The fused call is cut by a second rule, at most 16384 sub-queries per list call / the most sub-queries of one fused query,
and that one is reachable: one fused query of 32 sub-queries caps a sub-chunk at 512 fused queries, so 1025 fused queries run as
sub-chunks of 512, 512 and a remainder of 1 -- a smaller shape than the 9000 x 2 of test_flat_fused_gpu.py, the only one with more
than one sub-chunk before this file."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, DIM, NQ, K = 300, 8, 5, 4


@pytest.fixture(scope="module")
def env():
    import lab_1806_vec_db_amd as vdb

    rng = np.random.default_rng(2024)
    ix = vdb.GpuIndex(DIM, "l2sqr", device=0)
    ix.batch_add(rng.standard_normal((N, DIM)).astype(np.float32))
    ix.set_labels(0, (np.arange(N) % 7).astype(np.uint32))
    masks = [ix.make_mask(rng.random(N) < 0.4), ix.make_mask(np.zeros(N, dtype=bool))]  # the second one allows nothing
    yield ix, masks, rng
    for m in masks:
        m.close()
    ix.close()


def _same(got, exp, what):
    assert np.array_equal(got[2], exp[2]), (what, got[2], exp[2])
    assert np.array_equal(got[0], exp[0]), what
    assert np.array_equal(got[1].view(np.uint32), exp[1].view(np.uint32)), what


def _one_by_one(call, nq):
    """call(q, q + 1) for every query, stacked"""
    parts = [call(q, q + 1) for q in range(nq)]
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


def _mask_args(masks, mask_of, lo, hi):
    return dict(masks=masks, mask_of=mask_of[lo:hi]) if masks else {}


@pytest.mark.parametrize("filtered", (False, True), ids=("all_rows", "two_masks"))
def test_a_batch_is_its_queries_one_at_a_time(env, filtered):
    ix, masks, rng = env
    masks = masks if filtered else None
    mask_of = np.array([0, 1, 0, 0, 1], dtype=np.uint32)
    qs = rng.standard_normal((NQ, DIM)).astype(np.float32)
    pos = [[int(r) for r in rng.choice(N, size=n, replace=False)] for n in (1, 3, 2, 5, 1)]
    neg = [[int(r) for r in rng.choice(N, size=n, replace=False)] for n in (0, 2, 0, 1, 4)]
    forms = {
        "grouped": lambda lo, hi: ix.flat_knn_grouped(qs[lo:hi], K, 0, 1, **_mask_args(masks, mask_of, lo, hi)),
        "mmr": lambda lo, hi: ix.flat_knn_mmr(qs[lo:hi], K, 20, 0.5, **_mask_args(masks, mask_of, lo, hi)),
        "like": lambda lo, hi: ix.flat_knn_like(pos[lo:hi], K, negatives=neg[lo:hi], **_mask_args(masks, mask_of, lo, hi)),
    }
    for name, call in forms.items():
        got = call(0, NQ)
        _same(got, _one_by_one(call, NQ), (name, filtered))
        if filtered:
            assert got[2][1] == 0 and got[2][4] == 0 and got[2][0] == K  # (the empty mask; the other one allows about 120 rows)
        else:
            assert (got[2] == K).all()


@pytest.mark.parametrize("filtered", (False, True), ids=("all_rows", "two_masks"))
def test_fused_sub_chunks_with_a_remainder(env, filtered):
    """5 fused queries, and 1025 of which the first has 32 sub-queries: sub-chunks of 512, 512 and 1 fused queries"""
    ix, masks, rng = env
    masks = masks if filtered else None
    for sizes in ((2, 1, 3, 1, 2), (32,) + (1,) * 1024):
        lims = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        nq, nsub = len(sizes), int(lims[-1])
        qs = rng.standard_normal((nsub, DIM)).astype(np.float32)
        w = (0.5 + rng.random(nsub)).astype(np.float32)
        mask_of = (np.arange(nsub) % 3 == 1).astype(np.uint32)  # every third sub-query under the empty mask

        def call(lo, hi):
            j0, j1 = int(lims[lo]), int(lims[hi])
            return ix.flat_knn_fused(qs[j0:j1], lims[lo:hi + 1] - lims[lo], K, 8, "rrf", w[j0:j1], **_mask_args(masks, mask_of, j0, j1))

        before = ix.get_stat("flat_filtered_multi_calls")
        got = call(0, nq)
        assert ix.get_stat("flat_filtered_multi_calls") - before == (1 if filtered else 0)  # one call, however many sub-chunks
        _same(got, _one_by_one(call, nq), (nq, filtered))
        assert (got[2][1:] > 0).sum() >= nq // 2
