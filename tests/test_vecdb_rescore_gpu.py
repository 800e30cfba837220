"""GPU: VecDB.batch_search_fused(group_by=, fusion=, rescore=) -- the fused call's candidate documents rescored over all their chunks.
2100 x 24 rows, a document's 7 chunks spread over 3 of 20 clusters: a list cut at fetch_k sees some chunks of a document and not others,
so the first stage's lower bounds misorder documents (asserted on the CPU reference first).  The expected answers come from a test-local
model over the metadata: the CPU oracle's distance of every vector to every row, the true MaxSim score of every document, and the first
stage restated by tests/fuse_groups_ref.py."""
import numpy as np
import pytest

import fuse_groups_ref as R

pytestmark = pytest.mark.gpu

N, DIM, K, FETCH = 2100, 24, 5, 24
SMALL = {"sum": 8, "min": 24}  # a rescore at which the reference certifies some questions of the batch and not others
SIZES = (3, 1, 4, 2, 4, 3)  # (at most 4 vectors: 4 x 4096 list entries is the fused call's limit, and one call fetches the whole table)


def _table():
    rng = np.random.default_rng(7300)
    centres = rng.random((20, DIM)).astype(np.float32)
    doc = np.arange(N) // 7
    cl = (doc * 7 + (np.arange(N) % 7) % 3 * 5) % 20
    vecs = (centres[cl] + rng.standard_normal((N, DIM)).astype(np.float32) * np.float32(0.02)).astype(np.float32)
    metas = [{"id": str(i), **({"doc": "d%d" % doc[i]} if i % 41 else {})} for i in range(N)]
    groups = [(centres[rng.integers(0, 20, s)] + rng.standard_normal((s, DIM)).astype(np.float32) * np.float32(0.02)).astype(np.float32) for s in SIZES]
    return vecs, metas, groups


class Model:
    def __init__(self, kind):
        from oracle import oracle as O

        self.vecs, self.metas, self.groups = _table()
        self.dm = []  # per question the dense distance table [S][N], computed once
        for g in self.groups:
            oi, od, oc = O.flat_knn_batch(self.vecs, g, N, kind, nthreads=16)
            d = np.zeros((len(g), N), np.float32)
            np.put_along_axis(d, oi.astype(np.int64), od, axis=1)
            self.dm.append((oi.astype(np.int64), od, d))
        self.members = {}
        for i in range(N):
            self.members.setdefault(self.group_of(i), []).append(i)

    def group_of(self, i):
        v = self.metas[int(i)].get("doc")
        return ("r", int(i)) if v is None else ("l", v)

    def true(self, q, fusion, only=None):
        """the documents (all, or the groups `only`) by true score: [(order key, representative row, score)] ascending"""
        d = self.dm[q][2]
        out = []
        for g in (self.members if only is None else only):
            rows = self.members[g]
            best = [min((R.order_key(d[s, r]), r) for r in rows) for s in range(len(d))]
            acc = np.float32(0.0)
            for s, (_, r) in enumerate(best):
                acc = np.float32(acc + d[s, r])
            s_min = min(range(len(d)), key=lambda s: (best[s][0], s))
            score = acc if fusion == "sum" else d[s_min, best[s_min][1]]
            out.append((R.order_key(score), best[s_min][1], score))
        return sorted(out)

    def first_stage(self, q, fusion, kc):
        oi, od, _ = self.dm[q]
        return R.fuse_groups([(oi[s, :FETCH], od[s, :FETCH]) for s in range(len(oi))], self.group_of, kc, fusion, trunc_len=FETCH)

    def expect(self, q, fusion, r):
        """-> ([(tag, score)], exact) of rescore=r at k = K, fetch_k = FETCH"""
        kc = min(r, FETCH)
        ids, sc, ex = self.first_stage(q, fusion, kc)
        ans = self.true(q, fusion, only=list(dict.fromkeys(self.group_of(i) for i in ids)))[:K]
        cert = len(ids) == kc and len(ans) == K and ans[K - 1][0] < R.order_key(sc[kc - 1])
        return [(self.metas[rep]["id"], float(s)) for _, rep, s in ans], bool(ex) or cert


@pytest.fixture(scope="module")
def models():
    return {0: Model(0), 1: Model(1)}


_tags = lambda res: [(e[0]["id"], e[1]) for e in res]  # noqa: E731


@pytest.mark.parametrize("fusion", ("sum", "min"))
def test_the_reference_tells_the_two_stages_apart(models, fusion):
    md = models[0]  # (otherwise the comparisons of the next test would show nothing)
    nq = len(SIZES)
    top = [[(md.metas[rep]["id"], float(s)) for _, rep, s in md.true(q, fusion)[:K]] for q in range(nq)]
    first = [[md.metas[int(i)]["id"] for i in md.first_stage(q, fusion, K)[0]] for q in range(nq)]
    if fusion == "sum":
        assert any([t for t, _ in top[q]] != first[q] for q in range(nq))  # the lower bounds misorder documents
    small = [md.expect(q, fusion, SMALL[fusion]) for q in range(nq)]
    assert {e[1] for e in small} == {True, False}  # a small rescore certifies some questions and not others
    assert all(e[0] == top[q] for q, e in enumerate(small) if e[1])  # ... and a certified answer is the true top k


@pytest.mark.parametrize("dist,kind", (("l2sqr", 0), ("cosine", 1)))
def test_rescore_against_the_model(models, dist, kind):
    from lab_1806_vec_db_amd.vecdb import VecDB

    md = models[kind]
    db = VecDB()
    db.create_table_if_not_exists("t", DIM, dist)
    db.batch_add("t", md.vecs, md.metas)
    ix = db._t("t").index
    nq = len(SIZES)
    for fusion in ("sum", "min"):
        top = [[(md.metas[rep]["id"], float(s)) for _, rep, s in md.true(q, fusion)[:K]] for q in range(nq)]
        # rescore at least the number of documents, fetch_k the whole table: every document is a candidate
        s0 = ix.get_stat("flat_rescore_calls")
        got, exact = db.batch_search_fused("t", md.groups, K, fusion, fetch_k=4096, group_by="doc", return_exact=True, rescore=4096)
        assert ix.get_stat("flat_rescore_calls") == s0 + 1  # the whole ragged batch: ONE call
        assert [_tags(r) for r in got] == top and exact == [True] * nq, fusion
        for r in (8, 5, 24, 1000):
            got, exact = db.batch_search_fused("t", md.groups, K, fusion, fetch_k=FETCH, group_by="doc", return_exact=True, rescore=r)
            exp = [md.expect(q, fusion, r) for q in range(nq)]
            assert [_tags(x) for x in got] == [e[0] for e in exp] and exact == [e[1] for e in exp], (fusion, r)
            assert all(_tags(x) == top[q] for q, x in enumerate(got) if exact[q])  # every certified answer is the true top k
            if r == SMALL[fusion]:
                assert set(exact) == {True, False}
        got, ex = db.search_fused("t", md.groups[2], K, fusion, fetch_k=FETCH, group_by="doc", return_exact=True, rescore=8)
        assert (_tags(got), ex) == md.expect(2, fusion, 8)
        assert [_tags(x) for x in db.batch_search_fused("t", md.groups, K, fusion, fetch_k=FETCH, group_by="doc", rescore=8)] == \
            [md.expect(q, fusion, 8)[0] for q in range(nq)]  # the default return shape
    for kw in (dict(fusion="sum"), dict(fusion="rrf", group_by="doc"), dict(fusion="sum", group_by="doc", rescore=K - 1)):
        with pytest.raises(ValueError, match="rescore"):
            db.batch_search_fused("t", md.groups, K, **{"rescore": 8, **kw})
    with pytest.raises(ValueError, match="no usable label column.*'tags'|'tags'.*no usable label column"):
        db.add("t", md.vecs[0], {"id": "x", "tags": ["a"]})
        db.search_fused("t", md.groups[0], K, "sum", group_by="tags", rescore=8)
