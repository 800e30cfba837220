"""GPU: no poison, real leftovers -- every entry point behind other calls on the SAME index and thread, hence in the same workspace.

The case table, the baselines and the CPU references are those of tests/scratch_cases.py.  Before each entry E a polluter runs on the
shared index:
  1. the kind's largest calls (_larger): more queries, larger k and longer lists than any row uses, so the buffers of the k-NN tiers, the
     range and filtered passes and the list re-rankers hold a longer call's data past E's own sizes.  This is per TABLE KIND, not per
     feature: masks, labels, get_rows and most analytics rows (covariance, project, silhouette, kmeans, dup_groups, dbscan) have no larger
     version of themselves here;
  2. a row of another feature on the same index -- the next row of another family in the table, not one picked from the code for sharing
     E's buffers; the random orders below make up for part of that;
  3. two refused calls.  One is refused AFTER it has put work on the device and left its mark in the scratch: a device id list with an id
     that is no row (ids_ok reads the flag back and leaves it set in ws.flags -- get_rows_device, every kind -- or in ws.grp_aux --
     fuse_lists_device, the f32 kinds), or a range search past flat_range_max_results (refused once its passes have run, every kind).  The
     other, by turns, is refused on the host before the workspace is taken (a foreign mask, a list length over its limit, an unwritten
     label column, a dimension mismatch): it must leave the counters alone.
E's answer and counter deltas must equal its baseline.  Then two seeded random orders of the whole table, and the contract of small_cnt
(k_flat_small's arrival counters stay zero between launches).  The one-launch kernel itself has no refusal after device work: its
arguments are checked on the host before the route is chosen, so "after a refused small-kernel search" can only be a host refusal.

The shared indexes live in scratch_cases (both files use them) and are closed by this module's finaliser; the baselines stay cached."""
import numpy as np
import pytest

import scratch_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vdb():
    import lab_1806_vec_db_amd as vdb
    yield vdb
    sc.close_shared()


def _vdb_error():
    from lab_1806_vec_db_amd._lib import VdbError
    return VdbError


def _larger(env):
    """the same features at larger shapes than any row of the table"""
    ix, q = env.ix, env.q
    if env.kind in ("big_l2", "big_cos"):
        env.route(2, flat_i8=2)
        ix.flat_knn(q[:150], 64)
        ix.flat_knn_fused(q[:96], np.arange(0, 97, 4), 32, 64, "rrf")
        ix.flat_knn_vote(q[:150], 64, 1, 8)
        ix.range_search(q[8:72], env.D.radii(env.kind, 8, 72, 200) if env.kind == "big_l2" else np.full(64, 0.05, np.float32))
        env.route(2, flat_filtered_direct_max=0)
        ix.flat_knn_filtered(q[:150], 64, env.mask("a"))
    elif env.kind == "u8":
        env.route(0, flat_u8=2)
        ix.flat_knn(q[:150], 64)
    else:
        env.route(0)
        ix.flat_knn(q[:150], 100)
        ix.knn_graph(20)
        ix.range_search(q[:150], np.full(150, 200.0, np.float32), limit=300)


def _refused_after_device_work(env, turn):
    """a call that is refused once its check has run on the device and left its flag, or its passes' data, in the workspace"""
    ix, E = env.ix, _vdb_error()
    before = env.snap()
    ids = np.array([3, env.n, 7], dtype=np.uint64)  # (env.n: the first id that is no row)
    turns = ["rows", "range"] + (["lists"] if env.kind != "u8" else [])
    what = turns[turn % len(turns)]
    if what == "rows":
        with pytest.raises(E, match="no row of this index"):
            sc.get_rows_device(env, ids)
    elif what == "lists":
        bad = np.full((8, 12), 5, dtype=np.uint64)
        bad[7, 11] = env.n
        with pytest.raises(E, match="no row of this index"):
            sc.fuse_lists_device(env, bad)
    else:
        ix.set_param("flat_range_max_results", 10)
        try:
            with pytest.raises(E, match="flat_range_max_results"):
                ix.range_search(env.q[8:40], np.full(32, 1e9, np.float32))  # (every row of every query: far past 10 pairs)
        finally:
            ix.set_param("flat_range_max_results", 0)
    if what != "range":  # (flat_range_device counts its queries, and a tier's hits, as it goes: only the id checks promise untouched counters)
        assert env.snap() == before, "an id check that fails moves no counter"


def _refused_on_the_host(vdb, env, turn):
    """one call that the library refuses before it takes the workspace, by turns"""
    ix, q, E = env.ix, env.q, _vdb_error()
    foreign = sc.shared_env(vdb, "small" if env.kind != "small" else "ann").mask("a")
    if env.kind == "u8":
        calls = [lambda: ix.flat_knn_filtered(q[:8], 10, foreign), lambda: ix.flat_knn(q[:8, :64], 10)]
    else:
        calls = [lambda: ix.flat_knn_filtered(q[:8], 10, foreign),           # a mask of another index
                 lambda: ix.flat_knn_fused(q[:8], [0, 2, 5, 8], 5, 5000),    # fetch_k over its limit
                 lambda: ix.silhouette(7),                                   # a label column never written
                 lambda: ix.flat_knn_mmr(q[:8], 8, 4, 0.5),                  # k over fetch_k
                 lambda: ix.flat_knn(q[:8, :64], 10)]                        # dimension mismatch
    before = env.snap()
    with pytest.raises(E):
        calls[turn % len(calls)]()
    assert env.snap() == before, "a call refused on the host moves no counter"


@pytest.mark.parametrize("name", [c.name for c in sc.CASES if c.kind != "edit"])
def test_behind_a_polluter(vdb, name):
    case = sc.BY_NAME[name]
    sc.baseline(vdb, case)
    env = sc.shared_env(vdb, case.kind)
    at = sc.CASES.index(case)
    _larger(env)
    peers = [c for c in sc.CASES[at + 1:] + sc.CASES[:at] if c.kind == case.kind]
    other = next((c for c in peers if c.family != case.family), peers[0])  # (the ANN indexes hold ANN rows only: the other structure's walk)
    sc.check(vdb, other, what=f"as the polluter of {name}")
    _refused_on_the_host(vdb, env, at)
    _refused_after_device_work(env, at)
    sc.check(vdb, case, what="behind larger calls, another feature and refused calls")


@pytest.mark.parametrize("kind", ["big_l2", "small", "u8"])
def test_every_refusal_after_device_work_then_its_own_entry(vdb, kind):
    """the entry point whose flag word the refusal left set runs right behind it: get_rows_device after a bad id (ws.flags), the list
    fusion after a bad list id (ws.grp_aux), a range search after one past its ceiling"""
    env = sc.shared_env(vdb, kind)
    follow = {"big_l2": ["get_rows_device", "range-i8", "fuse_lists_device"], "small": ["range-small", "range-small", "dbscan"],
              "u8": ["range-u8", "range-u8"]}[kind]
    for turn, name in enumerate(follow):
        sc.baseline(vdb, sc.BY_NAME[name])
        _refused_after_device_work(env, turn)
        sc.check(vdb, sc.BY_NAME[name], what=f"right behind refusal {turn}")


@pytest.mark.parametrize("seed", [1806, 4711])
def test_random_order_of_the_whole_table(vdb, seed):
    order = np.random.default_rng(seed).permutation(len(sc.CASES))[:60]
    for step, at in enumerate(order.tolist()):
        sc.check(vdb, sc.CASES[at], what=f"seed {seed} step {step}: {[sc.CASES[j].name for j in order[max(0, step - 3):step]]} before it")


def test_small_kernel_counters_stay_zero_between_launches(vdb):
    """Workspace::small_cnt is zeroed once, when it is allocated, and k_flat_small leaves it zero: a search of another nq after one that
    ran, and after a refused one (on the host: the kernel's calls have no later refusal), answers as the oracle does"""
    D, E = sc.data(), _vdb_error()
    ix = vdb.GpuIndex(sc.DIM, "l2sqr")
    try:
        ix.batch_add(D.small)
        ix.set_param("flat_small", 2)
        ix.prof_enable(True)
        with pytest.raises(E, match="dimension"):
            ix.flat_knn(D.q_small[:4, :64], 10)
        shapes = ((3, 5), (7, 10), (1, 1), (64, 10), (2, 3))
        for nq, k in shapes:
            got = ix.flat_knn(D.q_small[8:8 + nq], k)
            oi, od, _ = sc.O().flat_knn_batch(D.small, D.q_small[8:8 + nq], k)
            assert np.array_equal(got[0], oi) and sc.same(got[1], od) and (got[2] == k).all(), (nq, k)
            with pytest.raises(E, match="dimension"):
                ix.flat_knn(D.q_small[:4, :64], 10)
        assert ix.prof_get("flat_small")["launches"] == len(shapes) and ix.prof_get("flat_exact")["launches"] == 0
    finally:
        ix.close()
