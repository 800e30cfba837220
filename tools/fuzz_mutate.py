"""Randomised WRITE / READ sequences on one index against the host model of the row edits (tests/edit_model.py) and the oracle: the steps
of edit_model.draw_steps -- batch_add of 1 / 3 / 200 / 2500 rows, swap_remove, remove_rows of a block / a random share / the last tile,
update_rows, label writes -- with one of the model's checks after every write (k-NN in a random flat mode with a random number of
queries aimed at what the write touched, filtered k-NN under a host-made or a label mask, range search, the touched rows and the label
columns read back), so that the one-launch kernel, the many-queries path, the exact scan and the MFMA pipeline with its mirrors --
extended by add, patched by the removes and the update -- all see tables that grew and shrank across their thresholds; an IVF or HNSW
search on the current rows now and then (their lazily built images must follow the rows too).  The seeded sequences of the suite
(tests/test_edit_sequences_gpu.py) run the same engine; this is the tool for soaks.
usage: python tools/fuzz_mutate.py [seconds] [seed]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import lab_1806_vec_db_amd as vdb
from oracle import oracle as O
import edit_model as em

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 240.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1806)
t_end = time.time() + budget
runs = ops = bad = 0


def ivf_search(ix, m, qs, k):
    kc = int(rng.integers(2, 30))
    ix.ivf_build(kc, train_n=min(len(m), 500), max_iter=3, seed=runs)
    ex = ix.ivf_export()
    iv = O.IVF(m.rows, ex["centroids"], m.kind, assign=ex["assign"])
    npb = int(rng.choice([1, 4, 30]))
    idx, d, cnt = ix.ivf_knn(qs[:8], k, npb)
    ix.ivf_clear()  # (the row edits refuse to run under IVF clusters; add would leave them stale)
    for q in range(min(len(qs), 8)):
        oi, od = iv.knn(qs[q], k, npb)
        c = int(cnt[q])
        assert c == len(oi) and idx[q, :c].tolist() == oi.tolist() and np.array_equal(d[q, :c], od), (f"ivf {kc} clusters {npb} probes", q, m.log)


def hnsw_search(ix, m, qs, k):
    ix.hnsw_build(M=8, ef_construction=40, seed=runs, batch=1, nthreads=4)
    oh = O.HNSW.from_graph(m.rows, m.kind, 8, 40, ix.hnsw_export())
    ix.set_param("hnsw_half", int(rng.choice([1, 2, 0])))
    idx, d, cnt = ix.knn_with_ef(qs[:8], k, 50)
    ix.set_param("hnsw_half", 1)
    ix.hnsw_clear()
    for q in range(min(len(qs), 8)):
        oi, od = oh.knn(qs[q], k, 50)
        c = int(cnt[q])
        assert c == len(oi) and idx[q, :c].tolist() == oi.tolist() and np.array_equal(d[q, :c], od), ("hnsw", q, m.log)


while time.time() < t_end:
    runs += 1
    dim = int(rng.choice([16, 64, 96, 128, 192, 320, 960]))
    dist, kind = (("l2sqr", 0), ("cosine", 1))[int(rng.integers(0, 2))]
    scale = float(rng.choice([0.05, 1.0, 30.0]))
    n0 = int(rng.choice([300, 3000, 9000, 15000, 17000, 40000]))
    m = em.EditModel(dim, kind, scale=scale, seed=int(rng.integers(1 << 30)))
    ix = vdb.GpuIndex(dim, dist)
    first = ("add", m.vectors(n0, 0))
    em.apply_to_index(ix, first)
    m.apply(first, note=f"dim {dim} {dist} scale {scale} seed {m.seed} start {n0}")
    steps = em.draw_steps(rng, m, int(rng.integers(6, 16)), min_rows=64)
    m.log.append(f"steps = {steps!r}")
    try:
        for st in steps:
            op = m.expand(st)
            em.apply_to_index(ix, op)
            touch = m.apply(op, note=repr(st))
            nq = int(rng.choice([1, 2, 8, 31, 40, 130]))
            qs, _ = m.queries(rng, touch, nq)
            mode = int(rng.choice([0, 0, 0, 2]))
            ix.set_flat_mode(mode)
            which = rng.random()
            ops += 1
            if which < 0.4:
                em.check_knn(ix, m, qs, int(rng.choice([1, 10, 33])), what=(st, "knn", mode, nq))
            elif which < 0.55:
                allow = rng.random(len(m)) < float(rng.choice([0.5, 0.9, 0.02]))
                allow[:64] = True
                mk = ix.make_mask(allow)
                em.check_filtered(ix, m, qs, mk, allow, em.K, what=(st, "filtered", mode, nq))
                mk.close()
            elif which < 0.7:
                em.check_range(ix, m, qs, em.K, what=(st, "range", mode, nq))
            elif which < 0.85:
                em.check_rows(ix, m, np.unique(np.concatenate([touch.new_at, touch.moved_to, [0, len(m) - 1]])), what=(st, "rows"))
                em.check_labels(ix, m, what=(st, "labels"))
            elif which < 0.95 and len(m) >= 600:
                ivf_search(ix, m, qs, int(rng.choice([1, 10, 33])))
            elif len(m) <= 3000:  # (the host builder on a prefix would not match the index: build on all rows when small)
                hnsw_search(ix, m, qs, int(rng.choice([1, 10, 33])))
            ix.set_flat_mode(0)
    except AssertionError as e:
        bad += 1
        print("MISMATCH in run", runs, "|", e, flush=True)
    print(f"run {runs}: {m.log[0]} -> {len(m)} rows after {len(steps)} writes", flush=True)
    ix.close()
print(f"done: {runs} runs, {ops} checked writes, {bad} mismatches")
sys.exit(1 if bad else 0)
